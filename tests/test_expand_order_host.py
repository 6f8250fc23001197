"""The keyed expansion's visit order (key_order, csrc/rt_math.h -- the one
definition the primary mesh kernels and the host-only rtx_expand_order share)
against a numpy restatement of sort8 and expand_sorted's packing, without a GPU.

Where key_order flags no tie, its list, count and first-child t bits equal the
network's; every input with two entered t equal in the top 29 bits is flagged,
and nothing else is. (Where it is flagged the kernel runs sort8 itself, the
shipped code, which needs no restatement here.)
"""
import ctypes as C
import itertools

import numpy as np
import pytest

import rtamd

NET = ((0, 1), (2, 3), (4, 5), (6, 7), (0, 2), (1, 3), (4, 6), (5, 7), (1, 2), (5, 6), (0, 4), (3, 7), (1, 5), (2, 6),
       (1, 4), (3, 6), (2, 4), (3, 5), (3, 4))
MISS = np.float32(-1.0)
TNEAR = np.float32(0.01)


@pytest.fixture(scope="module")
def L(rt):
    lib = rtamd.lib()
    lib.rtx_expand_order.restype = C.c_int
    lib.rtx_expand_order.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


def keyed(L, t):
    t = np.ascontiguousarray(t, np.float32)
    n = len(t)
    lst, cnt, tf = (np.empty(n, np.uint32) for _ in range(3))
    tie = np.empty(n, np.uint8)
    rtamd._lib.check(L.rtx_expand_order(t.ctypes.data, n, lst.ctypes.data, cnt.ctypes.data, tf.ctypes.data,
                                        tie.ctypes.data))
    return lst, cnt, tf, tie.astype(bool)


def network(t):
    """sort8 (swap iff t[a] > t[b]) on every row, then the list built from the
    back over the entries with t >= 0: -> list, count, first-child t bits."""
    t = np.array(t, np.float32)
    ids = np.tile(np.arange(8, dtype=np.uint32), (len(t), 1))
    for a, b in NET:
        s = t[:, a] > t[:, b]
        t[s, a], t[s, b] = t[s, b], t[s, a]
        ids[s, a], ids[s, b] = ids[s, b], ids[s, a]
    lst = np.zeros(len(t), np.uint32)
    cnt = np.zeros(len(t), np.uint32)
    tf = np.zeros(len(t), np.float32)
    for i in range(7, -1, -1):
        e = ~(t[:, i] < 0)
        lst[e] = (lst[e] << np.uint32(3)) | ids[e, i]
        cnt[e] += 1
        tf[e] = t[e, i]
    return lst, cnt, tf.view(np.uint32)


def ties29(t):
    """Rows with two entered t equal in the top 29 bits."""
    t = np.asarray(t, np.float32)
    k = (t.view(np.uint32) >> np.uint32(3)).astype(np.int64)
    k[t < 0] = -1 - np.broadcast_to(np.arange(8), t.shape)[t < 0]  # misses: distinct, never a tie
    s = np.sort(k, axis=1)
    return (s[:, 1:] == s[:, :-1]).any(axis=1)


def check(L, t):
    t = np.ascontiguousarray(t, np.float32)
    lst, cnt, tf, tie = keyed(L, t)
    want = ties29(t)
    assert np.array_equal(tie, want), f"tie flag differs in {int((tie != want).sum())} of {len(t)} rows"
    rl, rc, rtf = network(t)
    ok = ~tie
    assert np.array_equal(cnt[ok], rc[ok])
    assert np.array_equal(lst[ok], rl[ok])
    assert np.array_equal(tf[ok], rtf[ok])
    return int(tie.sum())


def test_all_permutations_of_distinct_t(L):
    vals = np.array([0.01, 0.0100001, 0.5, 0.75, 1.0, 3.0, 99.0, 100.0], np.float32)
    assert len(set((vals.view(np.uint32) >> 3).tolist())) == 8
    t = vals[np.array(list(itertools.permutations(range(8))))]
    assert t.shape == (40320, 8)
    assert check(L, t) == 0


VALUE_SETS = (
    np.array([0.01, 0.02, 0.3, 0.7, 1.5, 2.5, 50.0, 100.0], np.float32),
    np.array([100.0, 50.0, 2.5, 1.5, 0.7, 0.3, 0.02, 0.01], np.float32),
    np.array([1.0, 0.01, 3.0, 0.5, 7.0, 0.25, 2.0, 0.125], np.float32),
    np.full(8, 0.01, np.float32),  # every pair of entered children ties
    np.nextafter(np.float32(1.0), np.float32(2.0)) * np.ones(8, np.float32) + np.arange(8, dtype=np.float32) * np.float32(2.0 ** -20),
)


@pytest.mark.parametrize("k", range(len(VALUE_SETS)))
def test_every_miss_mask(L, k):
    v = VALUE_SETS[k]
    m = (np.arange(256)[:, None] >> np.arange(8)[None, :]) & 1
    t = np.where(m == 1, MISS, v[None, :]).astype(np.float32)
    ties = check(L, t)
    if k == 3:
        assert ties == 256 - 1 - 8  # every mask that leaves two or more children
    else:
        assert ties == 0
    lst, cnt, tf, _ = keyed(L, t)
    assert np.array_equal(cnt, 8 - m.sum(1))
    assert cnt[255] == 0 and lst[255] == 0 and tf[255] == 0


def test_random_draws_with_near_ties(L):
    rng = np.random.default_rng(21)
    n = 1_000_000
    base = np.float32(0.7313)
    near = (base.view(np.uint32) + np.array([0, 1, 2, 4, 7, 8, 9, 16], np.uint32)).view(np.float32)
    pool = np.concatenate([[MISS, TNEAR], near]).astype(np.float32)
    pick = rng.integers(0, len(pool) + 6, size=(n, 8))  # 6 of 16 draws: a random t
    rnd = rng.uniform(0.01, 100.0, size=(n, 8)).astype(np.float32)
    t = np.where(pick < len(pool), pool[np.minimum(pick, len(pool) - 1)], rnd).astype(np.float32)
    ties = check(L, t)
    assert 0 < ties < n  # both outcomes are exercised
    # 1 to 7 ulp apart across an 8-ulp boundary is no tie, 1 ulp inside one is
    lo = base.view(np.uint32) & ~np.uint32(7)
    a = np.array([lo + 7, lo + 8], np.uint32).view(np.float32)
    b = np.array([lo + 6, lo + 7], np.uint32).view(np.float32)
    row = np.full((2, 8), MISS, np.float32)
    row[0, 2], row[0, 5] = a
    row[1, 2], row[1, 5] = b
    assert keyed(L, row)[3].tolist() == [False, True]
