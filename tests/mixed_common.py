"""Shared by test_mixed_host.py and test_mixed_gpu.py: the bottom-level scenes,
the instanced scenes and the rays of the mixed-kind tests
(rt_scene_create_instanced_any, include/rtamd.h), and the header's loop with a
record of which kind a ray's hit was taken from.

The oracle of a mixed scene is instances_common.compose (flat list) and
tlas_common.compose_tlas (top-level tree) over cpuref.RefScene objects of all
three kinds: both only call intersect_rays, which every kind has.
"""
import functools

import numpy as np

import cpuref
import instances_common as IC
import scenes as S
import tlas_common as TC

F = np.float32
MESH, GRID, OCT = 1, 2, 3  # enum rt_scene_kind
UNIT_CUBE = np.array([-1, -1, -1, 1, 1, 1], F)  # the object box of both SDF kinds

# the BLAS set, in the order every scene below indexes it
BLAS = ("cube", "bunny", "grid17", "example_grid", "oct2", "sdf_5")
KIND = {"cube": MESH, "bunny": MESH, "grid17": GRID, "example_grid": GRID, "oct2": OCT, "sdf_5": OCT}
GRID17 = (17, 9, 13)  # non-cubic on purpose


@functools.lru_cache(maxsize=None)
def payload(name):
    """What both implementations are created from. mesh: (vPos4f, indices);
    grid: (size uint32[3], values float32); octree: 36-byte node records."""
    if name in ("cube", "bunny"):
        return IC.mesh(name)
    if name == "grid17":
        # a sphere of radius 0.6 minus a smaller one, sampled on the lattice in float32
        p = cpuref.lattice_points(GRID17).astype(F)
        c = F([0.35, 0.2, 0.1])
        big = np.sqrt((p * p).sum(1, dtype=F)).astype(F) - F(0.6)
        q = (p - c).astype(F)
        small = np.sqrt((q * q).sum(1, dtype=F)).astype(F) - F(0.35)
        vals = np.maximum(big, -small).astype(F)
        vals.setflags(write=False)
        return np.array(GRID17, np.uint32), vals
    if name == "example_grid":
        return S.inputs("example_grid.grid")[1]
    if name == "oct2":
        v, i = IC.mesh("cube")
        nodes = cpuref.sdf_octree(v, i, 2)
        nodes.setflags(write=False)
        return nodes
    return S.inputs("sdf_5.octree")[1]


@functools.lru_cache(maxsize=None)
def ref_blas(name):
    k, p = KIND[name], payload(name)
    if k == MESH:
        return IC.ref_mesh(name)
    return cpuref.RefScene.grid(*p) if k == GRID else cpuref.RefScene.octree(p)


def refs(names=BLAS):
    return {j: ref_blas(m) for j, m in enumerate(names)}


def gpu_blas(rtamd, name, dynamic=False):
    """A new GPU scene of BLAS `name` (the caller caches)."""
    k, p = KIND[name], payload(name)
    if k == MESH:
        return rtamd.BVHBuilder(rtamd.SimpleMesh(*p), dynamic=dynamic)
    return rtamd.SDFGrid(*p) if k == GRID else rtamd.SDFOctree(p)


def rigid(seed, b):
    """A rotation (det +1) with a translation."""
    q = IC.rot(seed)
    if np.linalg.det(q) < 0:
        q = q * np.array([1.0, 1.0, -1.0])
    return IC.affine(q, b)


def _defs():
    """name -> (BLAS names, [(blas, xform, flags)])."""
    d = {}
    # m1: one SDF instance under the identity, per kind (both BLAS of each kind)
    for m in ("grid17", "example_grid", "oct2", "sdf_5"):
        d[f"m1-{m}"] = ((m,), [(0, IC.IDENTITY, 0)])
    # m3: a mesh, a grid and an octree with overlapping world boxes, all rigid
    d["m3"] = (("bunny", "grid17", "sdf_5"), [(0, rigid(41, (0.0, 0.05, -0.1)), 0), (1, rigid(42, (-0.75, 0.1, 0.2)), 0),
                                              (2, rigid(43, (0.8, -0.1, 0.1)), 0)])
    # m9: all six BLAS, two instances disabled, one pose with scale (for the definition's sake)
    pos = [(-0.9, 0.85, 0.7), (0.0, 0.85, -0.6), (0.9, 0.85, 0.6), (-0.9, 0.0, -0.7), (0.0, 0.0, 0.8), (0.9, 0.0, -0.6),
           (-0.9, -0.85, 0.5), (0.0, -0.85, -0.7), (0.9, -0.85, 0.6)]
    order = [4, 2, 0, 5, 1, 3, 2, 5, 1]  # BLAS of instance i: neighbours in the list differ in kind
    inst = []
    for i, (b, c) in enumerate(zip(order, pos)):
        x = rigid(50 + i, c)
        if i == 7:  # the scaled pose: an octree at 0.8 x 0.7 x 0.75
            x = IC.affine(IC.rot(57) @ np.diag([0.8, 0.7, 0.75]), c)
        if BLAS[b] == "cube":
            x = IC.affine(IC.rot(50 + i) @ np.diag([0.55, 0.55, 0.55]), c)
        inst.append((b, x, IC.DISABLED if i in (6, 8) else 0))
    d["m9"] = (BLAS, inst)
    # m130: 130 instances on a 6 x 6 x 4 lattice, BLAS (7 k) mod 6: an index order
    # that is not spatially sorted; SDF instances rigid, the cube scaled down
    inst = []
    for k in range(130):
        c = np.float64([k % 6, (k // 6) % 6, k // 36]) * 1.6 - [4.0, 4.0, 2.4]
        b = (7 * k + k // 6) % 6
        x = rigid(600 + k, c)
        if BLAS[b] == "cube":
            x = IC.affine(IC.rot(600 + k) @ np.diag([0.5, 0.6, 0.55]), c)
        inst.append((b, x, 0))
    d["m130"] = (BLAS, inst)
    return d


DEFS = _defs()
EYE_POS = {"m3": (0.3, 0.4, 3.6), "m9": (0.3, 0.4, 5.0), "m130": (0.3, 0.4, 9.0)}
N = 4096


@functools.lru_cache(maxsize=None)
def rays(name, kind="random"):
    """random: instances_common.random_rays at N = 4096; eye: 64 x 64 eye rays
    (tlas_common.eye_rays) from a camera that sees the scene."""
    if kind == "eye":
        o, d = TC.eye_rays(pos=EYE_POS.get(name, (0.3, 0.4, 3.6)))
    else:
        o, d = IC.random_rays(N, 20261022)
    o, d = np.ascontiguousarray(o, F), np.ascontiguousarray(d, F)
    o.setflags(write=False)
    d.setflags(write=False)
    return o, d


def object_boxes(names):
    """root_boxes for tlas_common.leaf_boxes from host data: a mesh's vertex box
    (the BVH root box is the exact min / max of the vertices), the cube for SDF kinds."""
    return [TC.vertex_box(payload(m)[0]) if KIND[m] == MESH else UNIT_CUBE for m in names]


def host_scene(rt, name):
    """(refs, blas, flags, M, wbox) of a scene from host data alone."""
    names, inst = DEFS[name]
    blas = [t[0] for t in inst]
    flags = [t[2] for t in inst]
    M = np.stack([rt.affine_inverse(t[1]) for t in inst])
    wbox = TC.leaf_boxes([t[1] for t in inst], blas, flags, object_boxes(names))
    return refs(names), blas, flags, M, wbox


def compose_events(refs_, kinds, blas, flags, M, o, d, tn, tf, wbox=None):
    """instances_common.compose's loop (with wbox: compose_tlas's) that also
    records, per ray, whether a hit of one kind was replaced by a later instance
    of another kind -> (hit, best, winner instance, replaced bool)."""
    n = len(o)
    tn = np.ascontiguousarray(np.broadcast_to(F(tn), (n,)))
    tf = np.ascontiguousarray(np.broadcast_to(F(tf), (n,)))
    best = np.full(n, np.inf, F)
    win = np.full(n, -1, np.int64)
    replaced = np.zeros(n, bool)
    for i in range(len(blas)):
        if flags[i] & IC.DISABLED:
            continue
        tfi = np.where(best < tf, best, tf).astype(F)
        idx = np.arange(n) if wbox is None else np.flatnonzero(TC.box_pass(wbox[i], o, d, tn, tfi))
        if not len(idx):
            continue
        oo, dd = IC.to_object(M[i], np.ascontiguousarray(o[idx]), np.ascontiguousarray(d[idx]))
        h, t, _, _ = IC.oracle_classes(refs_[blas[i]], oo, dd, np.ascontiguousarray(tn[idx]), np.ascontiguousarray(tfi[idx]))
        up = (h != 0) & (t < best[idx])
        j = idx[up]
        prev = win[j]
        was = np.array([kinds[blas[p]] if p >= 0 else 0 for p in prev], np.int64)
        replaced[j] |= (prev >= 0) & (was != kinds[blas[i]])
        best[j], win[j] = t[up], i
    return (win >= 0).astype(np.int32), best, win, replaced
