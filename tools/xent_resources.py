"""Per-kernel resources of the loss-head sources, two trees side by side (profiles/xent_refactor_resources.txt).

    python tools/xent_resources.py PARENT_TREE [THIS_TREE]

Compiles srfrd_xent.hip and srfrd_sxent.hip of both trees to gfx950 ISA with the library's own flags (no GPU needed) and
prints, per kernel instantiation, what the compiler reports: scratch bytes, occupancy, LDS bytes, VGPRs, SGPRs.  For the six
streaming kernels at KS = 13 (d_item 50) it also counts the MFMA, LDS, global-memory and barrier instructions in the ISA.
"""
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
from __graft_entry__ import FLAGS  # noqa: E402

FILES = ["srfrd_xent.hip", "srfrd_sxent.hip"]
INFO = [("scratch", r"; ScratchSize: (\d+)"), ("occ", r"; Occupancy: (\d+)"), ("lds", r"; LDSByteSize: (\d+)"),
        ("vgpr", r"; TotalNumVgprs: (\d+)"), ("sgpr", r"; TotalNumSgprs: (\d+)")]
INSTS = [("v_mfma", r"^\s+v_mfma"), ("ds_read", r"^\s+ds_read"), ("ds_write", r"^\s+ds_write"),
         ("global_load", r"^\s+global_load"), ("global_store", r"^\s+global_store"), ("s_barrier", r"^\s+s_barrier")]
C2 = re.compile(r"s?xent_(fwd|dh|de)_kernel<13")


def kernels(tree):
    """{demangled kernel name: ({resource: value}, {instruction: count})} of one tree's loss-head sources"""
    out = {}
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        for f in FILES:
            asm = os.path.join(tmp, f + ".s")
            src = os.path.join(tree, "srfrd_amd", "csrc", f)
            subprocess.run([hipcc] + FLAGS + ["--cuda-device-only", "-S", src, "-o", asm], check=True, stderr=subprocess.DEVNULL)
            text = open(asm).read()
            # a kernel's code runs from its label to its "; Kernel info:" block
            for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^; Kernel info:\n(.*?)^; COMPUTE_PGM", text, re.S | re.M):
                name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout
                name = re.sub(r"^(void )?srfrd::\(anonymous namespace\)::|\(.*$", "", name.strip(), flags=re.S)
                res = {k: int(re.search(p, m.group(3)).group(1)) for k, p in INFO}
                ins = {k: len(re.findall(p, m.group(2), re.M)) for k, p in INSTS}
                out[name] = (res, ins)
    return out


def main():
    parent = kernels(sys.argv[1])
    branch = kernels(sys.argv[2] if len(sys.argv) > 2 else HERE)
    cols = [k for k, _ in INFO]
    print(f"{'kernel':42s} " + " ".join(f"{c + ' p/b':>13s}" for c in cols))
    for name in sorted(set(parent) | set(branch)):
        p, b = parent.get(name), branch.get(name)
        cell = lambda c: (str(p[0][c]) if p else "-") + "/" + (str(b[0][c]) if b else "-")
        print(f"{name:42s} " + " ".join(f"{cell(c):>13s}" for c in cols))
    print()
    cols = [k for k, _ in INSTS]
    print(f"{'instructions in the ISA, KS = 13':42s} " + " ".join(f"{c + ' p/b':>16s}" for c in cols))
    for name in sorted(n for n in set(parent) & set(branch) if C2.search(n)):
        print(f"{name:42s} " + " ".join(f"{str(parent[name][1][c]) + '/' + str(branch[name][1][c]):>16s}" for c in cols))


if __name__ == "__main__":
    main()
