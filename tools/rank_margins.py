"""Reduce the RANK_MARGIN lines of the ranking width / shape tests to profiles/rank_width_margins.txt:

    python -m pytest -m gpu -s -q tests/test_gpu_rank_widths.py tests/test_gpu_rank_shapes.py | python tools/rank_margins.py > profiles/rank_width_margins.txt

Per table route and op: the largest |value - s64| / (max(E32, 2^-23) A) any case printed (the tests allow 4), and that case."""
import re
import sys

worst = {}
for line in sys.stdin:
    for m in re.finditer(r"RANK_MARGIN (.*?) ratio ([0-9.]+)", line):
        tag, ratio = m.group(1), float(m.group(2))
        route = "fp32 forced" if "fp32_forced" in tag else "bf16 shadow" if "bf16" in tag else "fp32"
        op = "predict_logits" if tag.startswith("predict") else "top-k / target rank"
        if ratio > worst.get((op, route), (-1.0, ""))[0]:
            worst[(op, route)] = (ratio, tag)
print("Largest |value - s64| / (max(E32, 2^-23) A) seen by the ranking width and shape tests on an MI355X (allowed: 4).")
print("E32 is the error of a plain fp32 matmul of the same operands on the CPU, A = sum_k |h_k| |e_k| (tests/rank_refs.py).\n")
print(f"{'route':<13} {'op':<21} {'ratio':>6}   case")
for (op, route), (ratio, tag) in sorted(worst.items(), reverse=True):
    print(f"{route:<13} {op:<21} {ratio:6.3f}   {tag}")
