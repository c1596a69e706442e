"""numpy restatement, uint32-exact, of srfrd_token_negatives (the stream and the rejection loop stated in
include/srfrd_hip.h), and builders of the small CSR histories its tests run on.  Nothing here touches the library."""
import math

import numpy as np

GOLDEN = 0x9E3779B9
SITE_TNEG = 0x4E470002
TRIES = 32
M32 = np.uint64(0xFFFFFFFF)


def fmix32(h):
    """srfrd_rng.h fmix32 on uint32 values held in uint64 arrays (no overflow warnings, the wrap is explicit)"""
    h = np.asarray(h, dtype=np.uint64) & M32
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & M32
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & M32
    h ^= h >> np.uint64(16)
    return h


def csr(histories):
    """histories[u]: the time-ordered training items of user u, u = 0..usernum -> (user_ptr int64 (usernum + 2), items int32,
    usernum)"""
    usernum = len(histories) - 1
    ptr = np.zeros(usernum + 2, np.int64)
    np.cumsum([len(h) for h in histories], out=ptr[1:])
    items = np.concatenate([np.asarray(h, np.int32) for h in histories]) if ptr[-1] else np.zeros(0, np.int32)
    return ptr, items.astype(np.int32), usernum


def token_negatives_ref(user_ptr, items, usernum, n_items, max_hist, users, targets, K, seed, batch_index, state2=None,
                        alias_prob=None, alias_idx=None, item_log_q=None, user_log_keep=None, exclude_history=True):
    """-> (ids (B, L, K) int64, log_q (B, L, K) float32, tries (B, L, K) int: draws made (0 at dead positions, TRIES + 1 where
    every draw clashed))"""
    targets = np.asarray(targets, np.int64)
    B, L = targets.shape
    s0 = fmix32((seed & 0xFFFFFFFF) ^ ((batch_index * GOLDEN) & 0xFFFFFFFF))
    s1 = fmix32(int(s0) + SITE_TNEG * GOLDEN + (0 if state2 is None else int(state2) & 0xFFFFFFFF))
    ids = np.zeros((B, L, K), np.int64)
    tries = np.zeros((B, L, K), np.int64)
    log_q = np.zeros((B, L, K), np.float32)
    uniform = np.float32(math.log(K / n_items))
    c = np.arange(L * K, dtype=np.uint64)
    live_slot = np.repeat(targets != 0, K, axis=1)                      # (B, L K)
    for b in range(B):
        u = int(min(max(int(users[b]), 0), usernum))
        n = int(min(max(int(user_ptr[u + 1] - user_ptr[u]), 0), max_hist))
        hist = np.asarray(items[user_ptr[u]:user_ptr[u] + n], np.int64)
        e = fmix32(fmix32(int(s1) + b) ^ c)
        row = np.zeros(L * K, np.int64)
        used = np.zeros(L * K, np.int64)
        open_ = live_slot[b].copy()
        for r in range(TRIES):
            if not open_.any():
                break
            h1 = fmix32(e + np.uint64(2 * r))
            bucket = ((h1 * np.uint64(n_items)) >> np.uint64(32)).astype(np.int64)
            if alias_prob is not None:
                h2 = fmix32(e + np.uint64(2 * r + 1))
                uu = (h2 >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
                keep = uu < np.asarray(alias_prob, np.float32)[bucket]
                bucket = np.where(keep, bucket, np.clip(np.asarray(alias_idx, np.int64)[bucket], 0, n_items - 1))
            cand = bucket + 1
            ok = open_ & (~np.isin(cand, hist) if exclude_history else True)
            row[ok] = cand[ok]
            used[open_] = r + 1
            open_ &= ~ok
        used[open_] = TRIES + 1
        ids[b] = row.reshape(L, K)
        tries[b] = used.reshape(L, K)
        base = uniform if item_log_q is None else np.asarray(item_log_q, np.float32)[row]
        keep_u = np.float32(0.0) if user_log_keep is None else np.asarray(user_log_keep, np.float32)[u]
        with np.errstate(invalid="ignore"):
            lq = (np.broadcast_to(base, row.shape).astype(np.float32) - keep_u).astype(np.float32)
        log_q[b] = np.where(row != 0, lq, np.float32(0.0)).reshape(L, K)
    return ids, log_q, tries


def distinct_fraction(histories, n_items):
    return max(len(set(h)) for h in histories) / n_items


def users_short(n_items=200, seed=11):
    """user 0 .. 5 in a 200-item catalog, the longest history 33 items: lengths 2 (users 0 and 1), 10 with duplicates, 32 and
    33 distinct (the set's capacity edge: 2 * 32 = 64 slots exactly, 33 takes 128), 25 with duplicates"""
    rng = np.random.RandomState(seed)
    p = rng.permutation(n_items) + 1
    return [[3, 4], [17, 5], [5, 5, 7, 9, 7, 5, 11, 9, 5, 7], list(p[:32]), list(p[40:73]),
            list(rng.choice(p[80:95], 25, replace=True))]


def users_long(n_items=200, seed=12):
    """users_short plus histories longer than any L used: 60 distinct items (30 % of the catalog), 512 and 600 draws with
    repetition from 60 and 50 items"""
    rng = np.random.RandomState(seed)
    p = rng.permutation(n_items) + 1
    return users_short(n_items) + [list(p[:60]), list(rng.choice(p[60:120], 512, replace=True)),
                                   list(rng.choice(p[100:150], 600, replace=True))]


def users_tiny():
    """8-item catalog: user 1 holds 7 of the 8 items (every live slot is 8 or 0), user 2 all 8 (every slot 0), user 3 two"""
    return [[], [1, 2, 3, 4, 5, 6, 7, 3, 1], [8, 7, 6, 5, 4, 3, 2, 1], [2, 6]]


def make_targets(histories, usernum, users, L, seed, dead_row=None):
    """(B, L) int64 next-item targets, left-padded with 0: row b walks its (clamped) user's history; row `dead_row` is all 0"""
    rng = np.random.RandomState(seed)
    B = len(users)
    tg = np.zeros((B, L), np.int64)
    for b, u in enumerate(users):
        h = histories[min(max(int(u), 0), usernum)] or [1]
        pad = int(rng.randint(0, L)) if L > 1 else 0
        for t in range(pad, L):
            tg[b, t] = h[(t - pad) % len(h)]
    if dead_row is not None and dead_row < B:
        tg[dead_row] = 0
    return tg


def counts_with_zeros(n_items, seed=5):
    """(n_items + 1,) popularity counts for the alias path: every third item has weight 0 (never drawn), the rest 1..9"""
    rng = np.random.RandomState(seed)
    c = rng.randint(1, 10, n_items + 1).astype(np.float64)
    c[3::3] = 0.0
    c[0] = 1e9                                                          # the padding id: ignored
    return c


def interaction_data(histories, n_items):
    """the histories as a srfrd_amd.InteractionData (every review real, no held-out items)"""
    from srfrd_amd import InteractionData
    ptr, items, usernum = csr(histories)
    z = np.zeros(usernum + 1, np.int32)
    return InteractionData(usernum, n_items, ptr, items, np.full(items.size, 2, np.int32), z, z.copy())


def standard_case(L=20, seed=20240611):
    """the inputs of the property tests, on the CPU and on the GPU: users_long() in a 200-item catalog (histories of at most
    30 % of it), ten rows over every user, id 99 clamped to the last one, row 2 without a target"""
    hist = users_long()
    ptr, items, usernum = csr(hist)
    users = np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 99], np.int64)
    targets = make_targets(hist, usernum, users, L, seed, dead_row=2)
    return hist, ptr, items, usernum, users, targets
