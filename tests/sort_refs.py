"""What tests/test_key_sort_abi.py (CPU) and tests/test_gpu_key_sort.py (-m gpu) share; no test functions.

The reference of srfrd_sort_keys (include/srfrd_hip_sort.h) in numpy, and the case lists as data: the CPU file audits their cover
and holds the reference to ``torch.sort(stable=True)``, the GPU file runs them."""
import functools

import numpy as np

TILE = 2048                      # kSortTile of srfrd_amd/csrc/srfrd_keysort.h (tests/test_key_sort_abi.py holds it to the source)
SENTINEL = -(1 << 50) - 12345    # what the outputs hold before a call; no case has it as a key
KM_TOP = 2 ** 31 - 3             # the largest key_max the entry point takes


def u(keys, key_max):
    """the sort key of include/srfrd_hip_sort.h -> int64 array"""
    keys = np.asarray(keys, dtype=np.int64)
    return np.where(keys < 0, 0, np.where(keys > key_max, key_max + 2, keys + 1)).astype(np.int64)


def reference(keys, key_max):
    """-> (sorted_keys, order): numpy's stable argsort of u, and the original values in that order"""
    keys = np.asarray(keys, dtype=np.int64)
    order = np.argsort(u(keys, key_max), kind="stable").astype(np.int64)
    return keys[order], order


N_LIST = (1, 2, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 3 * TILE + 17, 1_050_000)
KEY_MAX_LIST = (0, 1, 5, 253, 254, 255, 65_533, 65_534, 50_000, 1_000_000, KM_TOP)
CONTENTS = ("zeros", "all_max", "half_pad", "descending", "ascending", "alternating", "hot", "once")

# (n, key_max, content): not the product - every n and every key_max with at least two contents (the CPU file counts)
CASES = (
    (1, 0, "zeros"), (1, 5, "all_max"),
    (2, 1, "descending"), (2, 1, "alternating"),
    (63, 253, "once"), (63, 5, "hot"),
    (64, 254, "descending"), (64, 0, "zeros"),
    (65, 255, "ascending"), (65, 65_533, "once"),
    (255, 254, "once"), (255, 253, "alternating"),
    (256, 255, "descending"), (256, 65_534, "half_pad"),
    (257, 65_533, "descending"), (257, 255, "hot"),
    (TILE - 1, 65_534, "once"), (TILE - 1, 5, "half_pad"),
    (TILE, 50_000, "descending"), (TILE, 0, "all_max"),
    (TILE + 1, 1_000_000, "ascending"), (TILE + 1, KM_TOP, "descending"),
    (3 * TILE + 17, 50_000, "once"), (3 * TILE + 17, 1_000_000, "alternating"), (3 * TILE + 17, KM_TOP, "hot"),
    (3 * TILE + 17, 254, "half_pad"),
    (1_050_000, 50_000, "half_pad"), (1_050_000, 1_000_000, "hot"), (1_050_000, KM_TOP, "once"), (1_050_000, 65_534, "ascending"),
)
# lists with invalid ids mixed in at 10 %: below one tile, two tiles and a tail, a pass count of 1, 2 and 3
OUT_OF_RANGE_CASES = ((257, 0), (TILE + 1, 253), (3 * TILE + 17, 50_000), (3 * TILE + 17, 1_000_000))
# the three smallest shapes of more than one tile: what the skewed libraries run
SKEW_CASES = tuple(sorted((c for c in CASES if c[0] > TILE), key=lambda c: c[0])[:3])


def case_id(case):
    return "-".join(str(x) for x in case)


def make(n, key_max, content, seed=0):
    """the keys of one case -> int64 (n,), every key in [0, key_max]"""
    rng = np.random.RandomState(1000 + seed + n % 977 + key_max % 991)
    i = np.arange(n, dtype=np.int64)
    if content == "zeros":
        keys = np.zeros(n, dtype=np.int64)
    elif content == "all_max":
        keys = np.full(n, key_max, dtype=np.int64)
    elif content == "half_pad":                      # the token list's shape: half pad key 0, half uniform
        keys = np.where(rng.rand(n) < 0.5, 0, rng.randint(0, key_max + 1, n)).astype(np.int64)
    elif content == "descending":                    # strictly descending, distinct
        assert n <= key_max + 1, (n, key_max)
        keys = key_max - i
    elif content == "ascending":                     # non-decreasing, with runs
        keys = np.sort(rng.randint(0, key_max + 1, n)).astype(np.int64)
    elif content == "alternating":                   # two values
        assert key_max >= 1
        keys = np.where(i % 2 == 0, key_max, key_max // 2).astype(np.int64)
    elif content == "hot":                           # one item in 90 % of the slots
        keys = np.where(rng.rand(n) < 0.9, key_max // 3 + 1 if key_max > 1 else key_max, rng.randint(0, key_max + 1, n)).astype(np.int64)
    elif content == "once":                          # every key exactly once: n distinct values, shuffled
        assert n <= key_max + 1, (n, key_max)
        stride = (key_max + 1) // n
        keys = rng.permutation(n).astype(np.int64) * stride + (key_max + 1 - stride * n)
    else:
        raise KeyError(content)
    assert keys.shape == (n,) and keys.min() >= 0 and keys.max() <= key_max
    return np.ascontiguousarray(keys)


def make_out_of_range(n, key_max, seed=0):
    """uniform keys with -1, -2^40, key_max + 1 and 2^62 mixed in at 10 %"""
    rng = np.random.RandomState(77 + seed + n % 977)
    keys = rng.randint(0, key_max + 1, n).astype(np.int64)
    bad = np.array([-1, -(1 << 40), key_max + 1, 1 << 62], dtype=np.int64)
    hit = rng.rand(n) < 0.1
    keys[hit] = bad[rng.randint(0, 4, int(hit.sum()))]
    return np.ascontiguousarray(keys)


@functools.lru_cache(maxsize=None)
def case(n, key_max, content, seed=0):
    """-> (keys, reference sorted keys, reference order) of one case: made once, shared, read-only"""
    keys = make(n, key_max, content, seed) if content != "out_of_range" else make_out_of_range(n, key_max, seed)
    skeys, order = reference(keys, key_max)
    for a in (keys, skeys, order):
        a.setflags(write=False)
    return keys, skeys, order
