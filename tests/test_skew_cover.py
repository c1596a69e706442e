"""CPU-only: what tests/test_gpu_skew_bits.py can and cannot see, checked on the sources and the kernel plans.

For every workgroup width the product launches, some library assigned to that kernel's exercisers delays some but not all
of the workgroup's waves; for the kernels of the seven translation units compiled under the two new masks, a second library
delays exactly the complement.  (The encoder units are the 0x0f0f objects in all three skewed libraries - the build links
them as they are - so an encoder workgroup is split one way only; tools/race_skew.py builds the other masks.)  Widths come
from the threads srfrd_rank_plan reports, from the table of encoder families in tests/skew_cases.py (held to the sources
here), and from the ``__launch_bounds__`` of the seven non-encoder sources with their named constants resolved: a new kernel
with a new width, or a new source, fails until an exerciser is assigned.  Mask 0x0f0f alone fails for width 256: the negative
control.  Every C entry point that launches a kernel is named by an exerciser or exempted with a reason.
"""
import os
import re

import pytest

from tests import skew_cases as S


def _masks(libs, encoder):
    table = S.libraries()
    return {name: table[name][1 if encoder else 2] for name in libs}


def _split_both_ways(masks, width):
    split = [m for m in masks.values() if S.splits(m, width)]
    both = any(S.complementary(a, b, width) for a in split for b in split)
    return bool(split), both


def test_the_libraries_are_what_the_build_links():
    import __graft_entry__ as g
    libs = S.libraries()
    assert set(libs) == {"product", "skew", "even", "odd"}
    assert libs["product"][1:] == (0, 0) and libs["skew"][1:] == (0x0f0f, 0x0f0f)
    assert libs["even"][1:] == (0x0f0f, 0x5555) and libs["odd"][1:] == (0x0f0f, 0xaaaa)
    assert libs["even"][2] ^ libs["odd"][2] == 0xffff
    assert sorted(g.SPLIT_SOURCES) == sorted(["srfrd_optim.hip", "srfrd_rank.hip", "srfrd_xent.hip", "srfrd_sxent.hip",
                                              "srfrd_negs.hip", "srfrd_tneg.hip", "srfrd_tneg_sample.hip"])
    assert len(g.SOURCES) - len(g.SPLIT_SOURCES) == 10 and all(s.startswith("srfrd_encoder_") for s in g.SOURCES if s not in g.SPLIT_SOURCES)
    assert os.path.basename(libs["skew"][0]) == "libsrfrd_hip_skew.so"


@pytest.mark.parametrize("src", S.non_encoder_sources())
def test_every_width_of_a_non_encoder_source_is_split_both_ways(src):
    widths = S.launch_widths(src)
    assert widths, src
    users = [e for e in S.EXERCISERS.values() if src in e.sources]
    assert users, f"no exerciser of tests/skew_cases.py launches the kernels of {src}"
    libs = sorted({lib for e in users for lib in e.libs})
    for w in sorted(widths):
        if w <= 64:                       # one wave: nobody to run ahead of
            continue
        split, both = _split_both_ways(_masks(libs, encoder=False), w)
        assert split and both, (src, w, libs)


def test_the_sources_have_the_widths_the_issue_counted():
    """the resolution of the named constants, pinned on the widths known today"""
    assert S.launch_widths("srfrd_optim.hip") == {64, 256, 512}
    assert S.launch_widths("srfrd_tneg_sample.hip") == {256} and S.launch_widths("srfrd_negs.hip") == {256}
    assert S.launch_widths("srfrd_tneg.hip") == {256, 1024}          # (1024: the counting kernels of srfrd_xent_common.h it includes)
    assert S.launch_widths("srfrd_xent.hip") == {256, 1024} and S.launch_widths("srfrd_sxent.hip") == {256, 1024}
    assert S.launch_widths("srfrd_rank.hip") == {64, 256, 512, 1024}


def test_mask_0f0f_alone_cannot_skew_a_256_thread_workgroup():
    """the negative control: under libsrfrd_hip_skew.so every wave of a four-wave workgroup sleeps alike"""
    assert not S.splits(0x0f0f, 256) and not S.splits(0x0f0f, 128)
    assert _split_both_ways({"skew": 0x0f0f}, 256) == (False, False)
    assert S.splits(0x0f0f, 512) and S.splits(0x0f0f, 1024)
    for w in (128, 256, 512, 1024):
        assert _split_both_ways({"even": 0x5555, "odd": 0xaaaa}, w) == (True, True)
    for e in S.EXERCISERS.values():
        if not e.families:                # no encoder kernel in it: 0x0f0f would test nothing
            assert "skew" not in e.libs and set(e.libs) == {"even", "odd"}, e.name


def _rank_layout(d_item, bf16):
    from tests import rank_refs as RR
    return RR.plan_layout(d_item, 0, S.RANK_ITEMS, bf16)


def test_every_width_the_rank_plan_reports_is_split_both_ways():
    from srfrd_amd import _lib
    libs = sorted({lib for e in S.EXERCISERS.values() if e.name.startswith("ranking-") for lib in e.libs})
    masks = _masks(libs, encoder=False)
    seen = set()
    for route, (d_item, bf16) in S.ROUTES.items():
        lay = _rank_layout(d_item, bf16)
        for B in (1, 37):
            for op, k, excl in [(_lib.RANK_TOPK, k, x) for k in (1, 10, 64) for x in (False, True)] + \
                               [(_lib.RANK_TARGET, 1, False), (_lib.RANK_TARGET, 1, True), (_lib.RANK_TARGET_METRIC, 1, False)]:
                plan = _lib.rank_plan(lay, op, B, k, 0, S.RANK_ITEMS + 1, excl)
                assert isinstance(plan, list) and plan, (route, B, op, k, excl, plan)
                for name, _, threads, _ in plan:
                    seen.add((name.split("<")[0], threads))
                    if threads > 64:
                        assert _split_both_ways(masks, threads) == (True, True), (name, threads)
    print(sorted(seen))
    assert {t for _, t in seen} - S.launch_widths("srfrd_rank.hip") == set()      # the plan launches what the source declares
    assert len({n for n, _ in seen}) >= 6                                        # more than one route's kernels were asked for


def test_encoder_widths_match_the_sources_and_0f0f_splits_them():
    consts = S.constants(open(os.path.join(S.CSRC, "srfrd_enc_common.h")).read())
    widths = {}
    for fam, w in S.ENCODER_WIDTHS.items():
        widths[fam] = consts[w[0]] * w[1] if isinstance(w, tuple) else w
    assert set(widths.values()) == {512, 1024}
    # the sources' own words for these widths
    text = {f: open(os.path.join(S.CSRC, f)).read() for f in os.listdir(S.CSRC)}
    assert "__launch_bounds__(NW_ > 0 ? NW_ * 64 : 512" in text["srfrd_encoder_fwd_kernel.inc"]
    assert "__launch_bounds__(NW_ > 0 ? NW_ * 64 : 512)" in text["srfrd_encoder_bwd_kernel.inc"]
    for f in ("srfrd_encoder_fwd_ragged_kernel.inc", "srfrd_encoder_bwd_ragged_kernel.inc", "srfrd_encoder_train_ragged.hip"):
        assert "__launch_bounds__(512, 4)" in text[f], f
    assert "__launch_bounds__(kRowWaves * 64)" in text["srfrd_encoder_fwd_rows_kernel.inc"]
    assert "__launch_bounds__(kSlotWaves * 64" in text["srfrd_encoder_bwd_slots_kernel.inc"]
    assert "__launch_bounds__(kCkWaves * 64)" in text["srfrd_encoder_bwd_chunks_kernel.inc"]
    # every other __launch_bounds__ of an encoder unit is one of the two barrier-free 256-thread kernels
    import __graft_entry__ as g
    others = []
    for f, t in text.items():
        if f.startswith("srfrd_encoder_") and (f in g.SOURCES or f.endswith(".inc")):
            for m in re.finditer(r"__launch_bounds__\(([^)]*)\)\s*(\w+)\(", t):
                if m.group(1).strip() == "256":
                    others.append((m.group(2), f))
    assert sorted(others) == sorted(S.BARRIER_FREE.items()), others
    for kernel, f in S.BARRIER_FREE.items():
        body = text[f].split(kernel + "(", 1)[1].split("\n}\n", 1)[0]
        assert "__syncthreads" not in body and "s_barrier" not in body, kernel
    # 0x0f0f splits every encoder family's workgroup, in each of the three libraries the encoder exercisers run under
    enc = [e for e in S.EXERCISERS.values() if e.families]
    assert set().union(*[e.families for e in enc]) == set(S.ENCODER_WIDTHS)
    for e in enc:
        assert e.libs == S.ENCODER_LIBS, e.name
        for fam in e.families:
            for lib, mask in _masks(e.libs, encoder=True).items():
                assert S.splits(mask, widths[fam]), (e.name, fam, lib)


def test_encoder_exercisers_are_the_complete_case_list():
    from tests import grad_refs as G
    names = {e.name for e in S.EXERCISERS.values() if e.name.startswith("encoder-")}
    assert names == {"encoder-" + cid for cid in G.case_ids()} and len(names) == len(G.ALL_CASES)
    assert {c.blocks for c in G.ALL_CASES} >= {1, 2, 3, 8}
    for kind in ("SASRec", "SRFRN"):
        for entry in ("sched", "ranked"):
            assert f"train_kernel-{kind}-{entry}" in S.EXERCISERS


def _header_decls():
    txt = open(os.path.join(S.ROOT, "include", "srfrd_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(srfrd_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", txt, flags=re.S)}


def test_every_launching_entry_point_is_named_or_exempt():
    from srfrd_amd import _lib
    decls = _header_decls()
    assert set(decls) == set(_lib.SIGNATURES)
    # an entry point launches on a stream it is given: the host-only ones take none
    takes_stream = {name for name, args in decls.items() if re.search(r"void\s*\*\s*stream", args)}
    assert takes_stream == set(decls) - set(S.HOST_ONLY), sorted(takes_stream ^ (set(decls) - set(S.HOST_ONLY)))
    named = set().union(*[e.entries for e in S.EXERCISERS.values()])
    assert named <= takes_stream, sorted(named - takes_stream)
    assert not (named & set(S.EXEMPT)), sorted(named & set(S.EXEMPT))
    left = takes_stream - named - set(S.EXEMPT)
    assert not left, f"launching entry points no exerciser names: {sorted(left)}"
    assert set(S.EXEMPT) <= takes_stream and all(len(reason) > 20 for reason in S.EXEMPT.values())
    assert len(S.EXEMPT) <= 3


def test_the_not_reproduced_list_holds_item_table_gradients_only():
    names = [n for ns in S.NOT_REPRODUCED.values() for n in ns]
    assert names and all(n.startswith("autograd.grad.") and n.endswith(("item_emb.weight", "item_embed.weight")) for n in names)
    assert all(n.endswith("metric_acc") for ns in S.ATOMIC_SUMS.values() for n in ns)
    assert S.listed("encoder-a-SASRec-L50-SRFRD_NO_RAGGED", "autograd.grad.item_emb.weight")
    assert not S.listed("encoder-a-SASRec-L50-SRFRD_NO_RAGGED", "autograd.grad.pos_emb.weight")
    assert not S.listed("optimizer", "autograd.grad.item_emb.weight")
    assert S.listed("ranking-bf16", "B37.eval_rank.metric_acc") and not S.listed("ranking-bf16", "B37.eval_rank")
