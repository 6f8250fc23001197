"""Shared by test_sdf_scenes_host.py, test_sdf_octree_device_gpu.py and
test_sdf_grid_update_gpu.py: the meshes of the device octree build's cases, the
oracle's octrees of them (computed once per session, read-only), their level
sizes, and rth::flatten_octree's words of a node array.
"""
import ctypes as C
import functools

import numpy as np

import cpuref
import points_ref as R

F = np.float32

# (mesh key, depth) -> (node count, level sizes or None where only the count /
# the last level is pinned): the oracle's figures the GPU cases rest on
CASES = {
    ("cube", 0): (1, [1]),
    ("cube", 1): (9, [1, 8]),
    ("cube", 2): (73, [1, 8, 64]),
    ("cube", 4): (2249, [1, 8, 64, 512, 1664]),
    ("cube", 5): (6153, [1, 8, 64, 512, 1664, 3904]),
    ("cube", 6): (37385, None),
    ("spot", 3): (281, None),
    ("spot", 4): (1097, [1, 8, 64, 208, 816]),
    ("bunny", 3): (353, None),
    ("far_cube", 3): (1, [1]),
    ("corner_cube", 4): (33, [1, 8, 8, 8, 8]),
}
LAST_LEVEL = {("cube", 5): 3904, ("cube", 6): 31232}


def _moved_cube(offset):
    """cube.obj scaled by 0.05 about the origin and moved to `offset`"""
    v, i = R.mesh("cube.obj")
    p = (v[:, :3] / v[:, 3:4]).astype(F)
    w = np.ones_like(v, dtype=F)
    w[:, :3] = p * F(0.05) + np.asarray(offset, F)
    return w, np.ascontiguousarray(i, np.uint32)


@functools.lru_cache(maxsize=None)
def mesh(key):
    """(vPos4f, indices) by name; the arrays are shared and read-only."""
    if key == "far_cube":
        v, i = _moved_cube((1.2, 1.2, 1.2))
    elif key == "corner_cube":
        v, i = _moved_cube((0.9, 0.9, 0.9))
    else:
        v, i = R.mesh({"cube": "cube.obj", "spot": "spot.obj", "bunny": "stanford-bunny.obj"}[key])
        v, i = np.ascontiguousarray(v, F), np.ascontiguousarray(i, np.uint32)
    v.setflags(write=False)
    i.setflags(write=False)
    return v, i


@functools.lru_cache(maxsize=None)
def oracle_nodes(key, depth):
    """cpuref.sdf_octree of mesh(key): uint8 [count * 36], read-only."""
    v, i = mesh(key)
    n = np.ascontiguousarray(cpuref.sdf_octree(v, i, depth, 16)).view(np.uint8).reshape(-1)
    n.setflags(write=False)
    return n


def offsets(nodes):
    return nodes.reshape(-1, 36)[:, 32:].copy().view(np.uint32).ravel()


def values(nodes):
    return nodes.reshape(-1, 36)[:, :32].copy().view(np.uint32).reshape(-1, 8)


def level_sizes(nodes):
    """Sizes of the BFS levels of a node array whose children blocks follow in
    the order of their parents."""
    off = offsets(nodes)
    sizes, first, n = [], 0, 1
    while n:
        sizes.append(n)
        inner = int(np.count_nonzero(off[first:first + n]))
        first += n
        n = 8 * inner
    assert first == len(off)
    return sizes


def leaf_corners(nodes, depth):
    """The level-`depth` leaves of a node array in node order and their corner
    points as the builders compute them -> (node indices [L], float32 [L, 8, 3])."""
    off = offsets(nodes)
    xyz = np.zeros((len(off), 3), np.int64)
    lvl = np.zeros(len(off), np.int64)
    ids = np.array([[(k >> 2) & 1, (k >> 1) & 1, k & 1] for k in range(8)], np.int64)
    for node in np.flatnonzero(off):  # BFS order: parents first
        c = int(off[node])
        xyz[c:c + 8] = 2 * xyz[node] + ids
        lvl[c:c + 8] = lvl[node] + 1
    leaves = np.flatnonzero(lvl == depth) if depth else np.array([0])
    size = F(2.0) ** F(1 - depth)
    p = (xyz[leaves][:, None, :] + ids[None]).astype(F) * size - F(1.0)
    return leaves, p.astype(F)


def flatten(rt, nodes):
    """rtx_octree_flatten -> (max_depth, maxd, words uint32 [n, 2]); raises on a refused tree."""
    from rtamd._lib import check
    buf = np.ascontiguousarray(nodes).view(np.uint8).reshape(-1)
    n = buf.size // 36
    words = np.zeros((n, 2), np.uint32)
    dp, md = C.c_int32(-1), C.c_int32(-1)
    check(rt.lib().rtx_octree_flatten(buf.ctypes.data, n, C.byref(dp), C.byref(md), words.ctypes.data))
    return dp.value, md.value, words


def scene_words(rt, scene, count):
    """rtx_scene_octree_words: the {child, masks} pairs the device holds, uint32 [count, 2]."""
    from rtamd._lib import check
    words = np.zeros((count, 2), np.uint32)
    check(rt.lib().rtx_scene_octree_words(scene._handle(), words.ctypes.data, count))
    return words
