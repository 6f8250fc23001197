"""Shared by test_sdf_refit_host.py and test_sdf_refit_gpu.py: the meshes, the
position-only deformation, the weld classes in numpy, the host restatement
(rtx_sdf_mesh_refit_host) and the sign rule of the signed distance.

Trees are refit_common's uint32 views: nodes [n_inner, 56]; tri [n_tri, 12] is
a.xyz, id | b.xyz, 0 | c.xyz, 0 of the SDF handle (not the scene's v0, e1, e2);
pn is float32 [T, 7, 4].
"""
import ctypes as C
import functools

import numpy as np

import points_ref as R
import refit_common as RC

F = np.float32
_p = RC._p


def shear(v):
    """x += 0.15 sin(4 y) in float32: a function of position only, so welded
    duplicates stay together (refit_common.deform's jitter would split them)."""
    w = np.array(v, F)
    w[:, 0] += (F(0.15) * np.sin(F(4.0) * w[:, 1])).astype(F)
    return w


def shear_back(v):
    """another position-only map, for the A -> B -> A round trip's B"""
    w = np.array(v, F)
    w[:, 2] += (F(0.1) * np.cos(F(3.0) * w[:, 0])).astype(F)
    return w


def weld_classes(v):
    """Class id per vertex of the divided positions' bits, ids in order of first appearance."""
    p = np.ascontiguousarray((v[:, :3] / v[:, 3:4]).astype(F)).view(np.uint32)
    _, first, inv = np.unique(p, axis=0, return_index=True, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    rank = np.empty(len(first), np.int64)
    rank[np.argsort(first)] = np.arange(len(first))
    return rank[inv]


def same_classes(v, w):
    return np.array_equal(weld_classes(v), weld_classes(w))


def welded_counts(v, i):
    """(welded vertices, welded edges) of a mesh, as the handle counts them."""
    cls = weld_classes(v)
    c = cls[np.asarray(i, np.int64).reshape(-1, 3)]
    e = np.concatenate([c[:, [0, 1]], c[:, [0, 2]], c[:, [1, 2]]])
    e.sort(axis=1)
    return int(cls.max()) + 1, len(np.unique(e, axis=0))


def _mesh(pos, tris):
    v = np.concatenate([np.asarray(pos, F), np.ones((len(pos), 1), F)], axis=1)
    i = np.asarray(tris, np.uint32).reshape(-1)
    v.setflags(write=False)
    i.setflags(write=False)
    return v, i


@functools.lru_cache(maxsize=None)
def mesh(key):
    """(vPos4f, indices) by name; the arrays are shared and read-only."""
    if key == "one":
        return RC.edge("rand", 1)
    if key == "nine":
        return RC.edge("rand", 9)
    if key in ("cube", "spot", "bunny"):
        v, i = R.mesh({"cube": "cube.obj", "spot": "spot.obj", "bunny": "stanford-bunny.obj"}[key])
        v, i = np.ascontiguousarray(v, F), np.ascontiguousarray(i, np.uint32)
        v.setflags(write=False)
        i.setflags(write=False)
        return v, i
    if key.startswith("grid") or key.startswith("rand"):
        return RC.edge(key[:4], int(key[4:]))
    if key == "zero_area":
        # triangle 1 is collinear along x with equal y, z: the shear keeps it so
        # (cross product exactly 0); triangle 2 is a single point three times
        return _mesh([(0, 0, 0), (0.5, 0, 0), (0, 0.5, 0.1), (0.1, 0.2, 0.3), (0.3, 0.2, 0.3), (0.7, 0.2, 0.3),
                      (-0.2, -0.3, 0.4), (-0.2, -0.3, 0.4), (-0.2, -0.3, 0.4), (-0.3, 0.2, 0.5)],
                     [0, 1, 2, 3, 4, 5, 6, 7, 8, 0, 2, 9])
    if key == "welded_corner":
        # triangle 1 names one vertex twice, triangle 2 has two vertices on one
        # position: an edge of zero length, two of its edges on one welded edge
        return _mesh([(0, 0, 0), (0.5, 0, 0), (0, 0.5, 0), (0.5, 0.5, 0.2), (0.5, 0.5, 0.2), (-0.3, 0.1, 0.2)],
                     [0, 1, 2, 1, 1, 2, 3, 4, 5, 2, 3, 5, 0, 2, 5])
    if key == "three_fan":
        # edge (0, 1) is shared by three triangles (non-manifold), each with its own copy of the edge's vertices
        return _mesh([(0, -0.5, 0), (0, 0.5, 0), (0.5, 0, 0), (0, -0.5, 0), (0, 0.5, 0), (-0.4, 0, 0.3),
                      (0, -0.5, 0), (0, 0.5, 0), (-0.1, 0, -0.5)],
                     [0, 1, 2, 4, 3, 5, 6, 7, 8])
    if key == "boundary":
        # an open strip: one inner edge, four boundary edges
        return _mesh([(0, 0, 0), (0.5, 0, 0.1), (0, 0.5, 0), (0.5, 0.5, -0.1)], [0, 1, 2, 2, 1, 3])
    raise KeyError(key)


HAND_MADE = ("zero_area", "welded_corner", "three_fan", "boundary")


def host_refit(rt, v, i, new_v=None):
    """rtx_sdf_mesh_refit_host: prep_sdf_mesh of (v, i) moved to new_v (or as
    built when new_v is None) -> (nodes, tri, pn)."""
    from rtamd._lib import check
    L = rt.lib()
    v = np.ascontiguousarray(v, F)
    i = np.ascontiguousarray(i, np.uint32)
    nv = None if new_v is None else np.ascontiguousarray(new_v, F)
    ni, nt = C.c_int64(0), C.c_int64(0)
    check(L.rtx_sdf_mesh_refit_host(_p(v), len(v), _p(i), len(i), _p(nv), None, C.byref(ni), None, C.byref(nt), None))
    nodes = np.zeros((ni.value, 56), np.uint32)
    tri = np.zeros((nt.value, 12), np.uint32)
    pn = np.zeros((len(i) // 3, 7, 4), F)
    check(L.rtx_sdf_mesh_refit_host(_p(v), len(v), _p(i), len(i), _p(nv), _p(nodes), C.byref(ni), _p(tri),
                                    C.byref(nt), _p(pn)))
    return nodes, tri, pn


def download(rt, m):
    """rtx_sdf_mesh_download: the handle's device tree now -> (nodes, tri)."""
    from rtamd._lib import check
    L = rt.lib()
    ni, nt = C.c_int64(0), C.c_int64(0)
    check(L.rtx_sdf_mesh_download(m._h, None, C.byref(ni), None, C.byref(nt)))
    nodes = np.zeros((ni.value, 56), np.uint32)
    tri = np.zeros((nt.value, 12), np.uint32)
    check(L.rtx_sdf_mesh_download(m._h, _p(nodes), C.byref(ni), _p(tri), C.byref(nt)))
    return nodes, tri


def by_id(tri):
    """Triangle records sorted by their original id (word 3)."""
    return tri[np.argsort(tri[:, 3], kind="stable")]


def signed(ref, p, pn):
    """The signed distance of the header from a brute-force result (points_ref)
    and pseudonormals pn [T, 7, 4]: sqrt(d2), negated where dot(p - q, N) < 0,
    f32, x*x + y*y + z*z left to right."""
    n = pn[ref["prim"], ref["feature"]]
    e = (p - ref["closest"]).astype(F)
    s = (e[:, 0] * n[:, 0] + e[:, 1] * n[:, 1]) + e[:, 2] * n[:, 2]
    d = np.sqrt(ref["d2"])
    return np.where(s < 0, -d, d).astype(F)
