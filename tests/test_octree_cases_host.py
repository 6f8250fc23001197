"""The hand-built octrees of octree_cases.py, on the host alone: the oracle
shows that every tree and ray set does what test_octree_cases_gpu.py relies
on, and rth::flatten_octree (through the host-only rtx_octree_flatten) gives
the words, depth and verdict the rules ask for. No GPU.

The minimum counts here are conditions on the inputs, checked on the oracle
alone, so that a GPU test cannot pass by comparing nothing.
"""
import ctypes as C

import numpy as np
import pytest

import octree_cases as OC
import rtamd
from rtamd import _lib

RT_E_INVALID = -1
NEVER_WORD = 0xFFFFFFFF


def flatten(nodes, count=None):
    """rtx_octree_flatten -> (status, message, max_depth, maxd, child uint32 [n], masks uint32 [n])."""
    nodes = np.ascontiguousarray(nodes).view(np.uint8)
    n = nodes.nbytes // 36 if count is None else count
    dp, md = C.c_int32(-7), C.c_int32(-7)
    words = np.full(2 * max(n, 1), 0x5A5A5A5A, np.uint32)
    buf = nodes if nodes.nbytes else np.zeros(36, np.uint8)
    rc = rtamd.lib().rtx_octree_flatten(buf.ctypes.data, n, C.byref(dp), C.byref(md), words.ctypes.data)
    msg = rtamd.lib().rt_last_error() if rc else b""
    return rc, msg, dp.value, md.value, words[0::2], words[1::2]


def probe(maxd):
    out = np.full(3, -7, np.int32)
    assert rtamd.lib().rtx_dispatch_probe(_lib.RT_SCENE_OCTREE, maxd, 0, out.ctypes.data) == 0
    return int(out[1]), int(out[2])


# ------------------------------------------------- 1. the inputs do their job --
@pytest.mark.parametrize("tn,tf", OC.INTERVALS)
@pytest.mark.parametrize("key", OC.SPINE_KEYS + ["shared-spine"])
def test_spine_rays_do_what_they_claim(key, tn, tf):
    """On the oracle alone, per tree and interval: at least 128 hits, hits in
    the last block, hits at surface leaves of at least min(depth - 1, 3)
    distinct levels above the last, every t of a hit finite, and at least 16
    rays that hold depth - 1 frames (octree_cases.full_stack) and end in the
    last block.

    A tree of depth D has surface leaves above the last level on levels 1 ..
    D - 1 only, so for the depth-1 tree, whose only block is the last one, the
    third count is 0 by construction; from depth 4 on the bound is 3."""
    nodes, desc, o, d = OC.case(key)
    hit, t, _, prim = OC.oracle(key, tn, tf)
    h = hit.astype(bool)
    full, ends, passes = OC.spine_outcome((nodes, desc), o, d, tn, tf, hit, prim)
    lv, kd = desc.level[prim[h]], desc.kind[prim[h]]
    above = np.unique(lv[(kd == OC.SURFACE) & (lv < desc.depth)])
    print(f"{key} [{tn:g}, {tf:g}]: {int(h.sum())} hits, {int((lv == desc.depth).sum())} in the last block, surface "
          f"levels above the last {len(above)}, leaf levels {len(np.unique(lv))}, full stack {int(full.sum())}: "
          f"{int(ends.sum())} end in the last block, {int(passes.sum())} go on")
    assert np.isin(kd, (OC.SURFACE, OC.DECOY)).all(), "a hit in a node that is no hittable leaf"
    assert int(h.sum()) >= 128
    assert int((lv == desc.depth).sum()) >= 1
    assert len(above) >= min(desc.depth - 1, 3)
    assert np.isfinite(t[h]).all()
    assert int(ends.sum()) >= 16


@pytest.mark.parametrize("tn,tf", OC.INTERVALS)
@pytest.mark.parametrize("key", OC.SPINE_KEYS + ["shared-spine"])
def test_rays_go_on_from_a_full_stack(key, tn, tf):
    """At least 16 rays that hold depth - 1 frames below the last block and then
    go on, to a miss or to a hit the walk reaches later: pops run from a full
    stack, the multi-level ones after tail calls among them."""
    nodes, desc, o, d = OC.case(key)
    hit, _, _, prim = OC.oracle(key, tn, tf)
    _, _, passes = OC.spine_outcome((nodes, desc), o, d, tn, tf, hit, prim)
    assert int(passes.sum()) >= 16, f"{key} [{tn:g}, {tf:g}]: {int(passes.sum())}"


@pytest.mark.parametrize("key", OC.SPINE_KEYS + ["shared-spine"])
def test_spine_trees_hold_what_they_claim(key):
    """Each never-hits rule on at least one level, with and without its edge
    value (from depth 3 on; a depth-1 tree has no block above the last, so no
    such leaf); four surface leaves and four decoys in the last block; under
    300 nodes; the shuffled layout's properties."""
    nodes, desc, o, d = OC.case(key)
    vals, off = OC.unpack(nodes)
    assert desc.count < 300 and len(off) == desc.count
    last = desc.offset[-1]
    assert sorted(desc.kind[last:last + 8].tolist()) == [OC.SURFACE] * 4 + [OC.DECOY] * 4
    if desc.depth >= 2:
        for rule in OC.NEVER:
            assert (desc.kind == rule).sum() == desc.depth - 1
        v10, v0, va = (vals[desc.kind == r] for r in OC.NEVER)
        assert (v10 == 10.0).any() and (v0 == 0).all() and np.signbit(v0).any() and (~np.signbit(v0)).any()
        assert (va == OC.THRESH).any()
        if desc.depth >= 3:
            assert (v10 > 10.0).all(1).any() and (~np.signbit(v0)).all(1).any() and (va > OC.THRESH).all(1).any()
    for l in range(desc.depth - 1):  # the face neighbour across the axis is a decoy
        assert desc.kind[desc.offset[l] + (int(desc.path[l]) ^ (1 << (2 - desc.axis)))] == OC.DECOY
    assert ((desc.path >> (2 - desc.axis)) & 1 == desc.bit).all()
    if desc.layout == "shuffled":
        assert off.max() == desc.count - 8 and (desc.offset % 8 != 1).any() and (desc.kind == OC.UNREF).any()
        assert desc.depth == 1 or (desc.offset[1:] < desc.spine[1:]).any()
    else:
        assert (desc.offset % 8 == 1).all() and not (desc.kind == OC.UNREF).any()
    assert o.dtype == d.dtype == np.float32 and o.shape == d.shape == (OC.N, 3)
    assert (d != 0).all() and np.isfinite(d).all() and np.isfinite(o).all()
    assert np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1).max() < 1e-6


@pytest.mark.parametrize("tn,tf", OC.INTERVALS)
@pytest.mark.parametrize("key", OC.SMALL_KEYS)
def test_small_trees_are_hit(key, tn, tf):
    """A hittable root leaf and the shared blocks: at least 128 hits, all in
    surface leaves, every t finite; the never-hitting root: none."""
    _, desc, _, _ = OC.case(key)
    hit, t, _, prim = OC.oracle(key, tn, tf)
    h = hit.astype(bool)
    if key == "root-never":
        assert not h.any()
        return
    assert int(h.sum()) >= 128 and np.isfinite(t[h]).all()
    assert (desc.kind[prim[h]] == OC.SURFACE).all()
    if key.startswith("shared"):
        assert len(np.unique(prim[h])) == 8, "every leaf of the shared block is hit"


@pytest.mark.parametrize("mode", list(OC.FRAME_MODES))
@pytest.mark.parametrize("cam", [0, 1, 2])
@pytest.mark.parametrize("key", OC.KEYS)
def test_frames_show_something(key, cam, mode):
    """At least 200 pixels with a finite t in every oracle frame. The
    never-hitting root has nothing to show without the plane: its primary
    frames must be empty."""
    _, t = OC.oracle_frame(key, cam, mode)
    n = int(np.isfinite(t).sum())
    if key == "root-never" and mode == "primary":
        assert n == 0
    else:
        assert n >= 200, f"{key} camera {cam} {mode}: {n} finite t"


# --------------------------------------------------------- 2. flatten_octree --
@pytest.mark.parametrize("key", OC.KEYS)
def test_words_follow_the_rules(key):
    """child and masks of every node against octree_cases.expected_words, the
    numpy restatement (the reference's isEmpty plus all >= 1e-4 define "never
    hits"); nodes that the root does not reach keep masks 0."""
    nodes, desc, _, _ = OC.case(key)
    rc, msg, _, _, child, masks = flatten(nodes)
    assert rc == 0, msg
    want_child, want_masks, reach = OC.expected_words(nodes)
    assert np.array_equal(child, want_child)
    assert np.array_equal(masks, want_masks)
    assert np.array_equal(reach, desc.kind != OC.UNREF)
    leaf = OC.unpack(nodes)[1] == 0
    assert np.array_equal(child[leaf] == NEVER_WORD, np.isin(desc.kind[leaf], OC.NEVER) |
                          ((desc.kind[leaf] == OC.UNREF) & (want_child[leaf] == NEVER_WORD)))
    assert (child[np.isin(desc.kind, (OC.SURFACE, OC.DECOY))] == 0).all()


SLOTS = {0: (4, 1), 1: (4, 1), 2: (4, 1), 5: (4, 1), 6: (7, 1), 8: (7, 1), 9: (15, 0), 16: (15, 0), 17: (31, 0), 24: (31, 0)}


@pytest.mark.parametrize("key", OC.KEYS)
def test_depth_and_dispatch(key):
    """max_depth is the tree's depth; the slot count pick_maxd grants, fed
    through the dispatch probe, gives the kernels' slots and PACK."""
    nodes, desc, _, _ = OC.case(key)
    rc, msg, depth, maxd, _, _ = flatten(nodes)
    assert rc == 0, msg
    assert depth == desc.depth == OC.DEPTH[key]
    assert probe(maxd) == SLOTS[depth]


def test_every_depth_of_the_table_is_used():
    assert {OC.DEPTH[k] for k in OC.KEYS} >= {0, 1, 5, 6, 8, 9, 16, 17, 24}


# ------------------------------------------------------------- 3. validation --
@pytest.mark.parametrize("k", range(1, 9))
def test_shared_blocks_are_accepted(k):
    """k parents of one children block: acyclic, depth 2. (A cycle guard that
    counts visits per path refuses this from k = 2 on.)"""
    nodes, desc = OC.shared_blocks(k)
    rc, msg, depth, maxd, child, masks = flatten(nodes)
    assert rc == 0, msg
    assert depth == 2 and maxd == 4
    assert (child[1:9] == 9).sum() == k
    assert (masks[1:9][child[1:9] == 9] == 0xFFFF).all()


def test_deep_shared_blocks_are_accepted():
    """The last block of a 9-level spine with three parents on three levels:
    max_depth is the longest path."""
    nodes, desc, _, _ = OC.case("shared-spine")
    off = OC.unpack(nodes)[1]
    assert (off == desc.offset[-1]).sum() == 3
    rc, msg, depth, _, _, _ = flatten(nodes)
    assert rc == 0, msg
    assert depth == 9


def test_linear_in_heavily_shared_trees():
    """24 levels, every node of every block the parent of the next block: 8^24
    root-to-leaf paths over 193 nodes. Accepted, depth 24, at once."""
    vals = np.ones((1 + 8 * 24, 8))
    off = np.zeros(len(vals), np.uint32)
    off[0] = 1
    for l in range(23):
        off[1 + 8 * l:9 + 8 * l] = 9 + 8 * l
    rc, msg, depth, maxd, child, masks = flatten(OC.records(vals, off))
    assert rc == 0, msg
    assert depth == 24 and maxd == 31
    assert (masks == 0).all() and (child[-8:] == NEVER_WORD).all()  # all leaves are all >= 1e-4
    # one leaf of the last block made the parent of one more block: 25 levels
    vals2 = np.concatenate([vals, np.ones((8, 8))])
    off2 = np.concatenate([off, np.zeros(8, np.uint32)])
    off2[len(off) - 1] = len(off)
    rc, msg, *_ = flatten(OC.records(vals2, off2))
    assert rc == RT_E_INVALID and b"24" in msg


def test_last_legal_offset_is_accepted_and_the_next_refused():
    nodes, desc = OC.spine_tree(5, 0, "shuffled", 1, 1)
    off = OC.unpack(nodes)[1]
    node = int(np.flatnonzero(off == desc.count - 8)[0])
    assert desc.kind[node] == OC.INNER
    assert flatten(nodes)[0] == 0
    for bad in (desc.count - 7, desc.count, 0xFFFFFFFF, 0xFFFFFFF9):
        rc, msg, *_ = flatten(OC.with_offset(nodes, node, bad))
        assert rc == RT_E_INVALID and msg, hex(bad)
    # an unreachable node's offset is validated too
    unref = int(np.flatnonzero(desc.kind == OC.UNREF)[0])
    rc, msg, *_ = flatten(OC.with_offset(nodes, unref, desc.count - 7))
    assert rc == RT_E_INVALID and msg


def test_empty_file_is_refused():
    rc, msg, *_ = flatten(np.zeros(0, np.uint8), count=0)
    assert rc == RT_E_INVALID and msg


@pytest.mark.parametrize("make", [OC.cyclic_self, OC.cyclic_pair])
def test_cycles_are_refused(make):
    """To the hook only: the oracle's recursion would not end on these."""
    rc, msg, *_ = flatten(make())
    assert rc == RT_E_INVALID and b"cyclic" in msg


def test_deepest_tree():
    """24 levels are accepted, 25 refused."""
    assert flatten(OC.spine_tree(24, 1, "bfs", 0, 1)[0])[:3:2] == (0, 24)
    rc, msg, *_ = flatten(OC.spine_tree(25, 0, "bfs", 0, 0)[0])
    assert rc == RT_E_INVALID and b"24" in msg


# ------------------------------------------------------ 4. the instanced scene --
def test_every_instance_wins_rays(rt):
    """The instanced scene of test_octree_cases_gpu.py (a packed tree, a 15-slot
    and a 31-slot tree, the cube): in the oracle's composition each of the four
    instances wins at least 64 rays, flat list and top-level tree."""
    for tlas in (False, True):
        hit, t, nrm, prim = OC.instance_host_oracle(rt, tlas, 0.01, 100.0)
        won = np.bincount((prim[hit != 0] >> 32).astype(np.int64), minlength=4)
        print("wins per instance:", won.tolist())
        assert (won >= 64).all(), won.tolist()
