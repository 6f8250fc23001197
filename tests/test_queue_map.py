"""The work queue's item order (csrc/rt_queue.h, the one mapping that
render_persist_kernel, the ray pump and the host share), reached through the
host-only rtx_queue_item / rtx_queue_cap, without a GPU: for every item count
0..300 and every head count the queue takes, the slots below each head's cap
hold every item exactly once, and the slot at the cap is past the end.
"""
import ctypes as C

import numpy as np
import pytest

import rtamd

HEADS = (8, 16, 32, 64)
PAST = 0xFFFFFFFF


@pytest.fixture(scope="module")
def L(rt):
    lib = rtamd.lib()
    lib.rtx_queue_item.restype = C.c_int
    lib.rtx_queue_item.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]
    lib.rtx_queue_cap.restype = C.c_int64
    lib.rtx_queue_cap.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]
    return lib


def item(L, items, heads, head, k):
    out = C.c_uint32(12345)
    rtamd._lib.check(L.rtx_queue_item(items, heads, head, k, C.byref(out)))
    return out.value


@pytest.mark.parametrize("heads", HEADS)
def test_every_item_once(L, heads):
    for items in range(301):
        seen = np.zeros(items, np.int32)
        for head in range(heads):
            cap = L.rtx_queue_cap(items, heads, head)
            assert 0 <= cap <= items
            for k in range(cap):
                i = item(L, items, heads, head, k)
                assert i < items, (items, heads, head, k, i)
                seen[i] += 1
            # the first slot past the cap, and one further on, are past the end
            assert item(L, items, heads, head, cap) == PAST, (items, heads, head)
            assert item(L, items, heads, head, cap + 1) == PAST, (items, heads, head)
        assert (seen == 1).all(), (items, heads, np.flatnonzero(seen != 1)[:8])


def test_item_belongs_to_head_i_mod_heads(L):
    for heads in HEADS:
        for i in (0, 1, heads - 1, heads, 3 * heads + 5, 299):
            assert item(L, 300, heads, i % heads, i // heads) == i


def test_bad_head_counts_are_rejected(L):
    out = C.c_uint32(0)
    for heads in (0, 1, 4, 12, 24, 128):
        assert L.rtx_queue_cap(100, heads, 0) == -1
        assert L.rtx_queue_item(100, heads, 0, 0, C.byref(out)) != 0
    for heads in HEADS:  # a head past the count
        assert L.rtx_queue_cap(100, heads, heads) == -1
        assert L.rtx_queue_item(100, heads, heads, 0, C.byref(out)) != 0
