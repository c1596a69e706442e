"""-m gpu: every kernel held to its own bits under skewed barriers, in this process (tests/skew_cases.py: the libraries, the
swap, the exercisers, the two limits).

``build()`` links the product and three schedule-skew builds; all four are loaded side by side with ctypes, and
``srfrd_skew_mask`` - host code and a one-thread kernel - proves that a swapped handle runs its own host code and launches
its own code objects.  Each test is one exerciser under one skewed library:

  * the exerciser runs under the product twice (kept for the exerciser's other libraries).  An output the two runs do not
    reproduce bit for bit must be named in skew_cases.NOT_REPRODUCED / ATOMIC_SUMS - item-table gradients scattered by float
    atomics, sums by double atomics - and is held, under every library, by the check the exerciser gives for it (the fp64
    bar of tests/grad_refs.py; the sum recomputed on the host from the bit-compared ranks), never by its bits;
  * every other output must come out of the skewed library with the product's bits; a mismatch reports the count and the
    first indices.  A differing bit is a race in product code: two waves of one workgroup met in one barrier interval;
  * an exerciser without a bit-compared output fails, and so does one that did not call an entry point it names.

Encoder exercisers run under 0x0f0f ("skew"), "even" and "odd" (the encoder kernels themselves are the 0x0f0f objects in all
three; the reductions and the optimizer around them change); the others under "even" and "odd": 0x0f0f delays all four waves
of a 256-thread workgroup alike, which tests/test_skew_cover.py asserts as its negative control.
"""
import os

import pytest

from tests import skew_cases as S

pytestmark = pytest.mark.gpu

PAIRS = [(e.name, lib) for e in S.EXERCISERS.values() for lib in e.libs]
_product = {}        # the last exerciser's two product runs: (name, outputs, reproduced names)


def _no_substitute():
    if os.environ.get("SRFRD_LIB_PATH"):
        pytest.skip("already running against a substituted library (tools/race_skew.py)")


def test_every_library_runs_its_own_code():
    """all four handles loaded first, then asked one after the other: host mask == device mask == the mask the name promises"""
    _no_substitute()
    libs = S.libraries()
    for name in libs:
        S.load(name)
    for name, (path, _, mask) in libs.items():
        host, device = S.probe(name)
        print(f"{name}: {os.path.basename(path)} host {host:#06x} device {device:#06x}")
        assert host == mask and device == mask, (name, hex(host), hex(device), hex(mask))
    from srfrd_amd import _lib
    assert _lib.lib().srfrd_skew_mask(None, None) == 0          # ... and the process is back on the product


def _run(ex, lib):
    with S.use(lib) as rec:
        out, checks = ex.run(S.SEED)
    missing = sorted(set(ex.entries) - rec.called)
    assert not missing, f"{ex.name} under {lib} never asked the library for {missing}"
    assert out and all(t.device.type == "cpu" for t in out.values())
    for name, check in checks.items():       # what the product does not reproduce: its own bar, under every library
        assert S.listed(ex.name, name), f"{ex.name}: {name} has a check but is not in the lists of tests/skew_cases.py"
        check(out[name])
    return out, checks


def _product_runs(ex):
    if _product.get("name") != ex.name:
        _product.clear()
        a, checks = _run(ex, "product")
        b, _ = _run(ex, "product")
        assert set(a) == set(b)
        moved = sorted(n for n in a if a[n].shape != b[n].shape or bool((S.bits(a[n]) != S.bits(b[n])).any()))
        unlisted = [n for n in moved if not S.listed(ex.name, n)]
        assert not unlisted, (f"{ex.name}: the product itself does not reproduce {unlisted}: a race no mask is needed for, "
                              "or an output that belongs in tests/skew_cases.NOT_REPRODUCED with its reason")
        exact = sorted(n for n in a if not S.listed(ex.name, n))
        assert set(checks) == set(a) - set(exact), (sorted(checks), sorted(set(a) - set(exact)))
        assert exact, f"{ex.name} has no bit-compared output"
        if moved:
            print(f"{ex.name}: not reproduced by the product (held by their own checks): {moved}")
        _product.update(name=ex.name, out=a, exact=exact)
    return _product["out"], _product["exact"]


@pytest.mark.parametrize("exerciser, lib", PAIRS, ids=[f"{e}-{lib}" for e, lib in PAIRS])
def test_same_bits_under_skewed_barriers(exerciser, lib):
    _no_substitute()
    ex = S.EXERCISERS[exerciser]
    want, exact = _product_runs(ex)
    got, _ = _run(ex, lib)
    assert set(got) == set(want)
    for name in exact:
        S.assert_bitwise(name, want[name], got[name], f"{exerciser} under {lib}")
