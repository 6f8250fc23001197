"""Shared by test_instances_host.py and test_instances_gpu.py: the reference of
an instanced scene composed from the oracle alone (include/rtamd.h, "the order
is the definition"), the meshes, the poses and the rays.

The composition runs cpuref.RefScene.mesh(...).intersect_rays once per instance
and per distinct (tNear, tf_i) class, on rays transformed in numpy float32 with
the exact expressions of the header, and applies the header's normal formula to
the winner.
"""
import functools

import numpy as np

import cpuref
import scenes as S

DISABLED = 1


def to_object(M, o, d):
    """o', d' of the header for one world-to-object matrix M (float32 [3, 4]):
    ((M[r,0]*x + M[r,1]*y) + M[r,2]*z) + M[r,3], every operation in float32."""
    M = np.asarray(M, np.float32)
    oo = np.empty_like(o)
    dd = np.empty_like(d)
    for r in range(3):
        oo[:, r] = ((M[r, 0] * o[:, 0] + M[r, 1] * o[:, 1]) + M[r, 2] * o[:, 2]) + M[r, 3]
        dd[:, r] = (M[r, 0] * d[:, 0] + M[r, 1] * d[:, 1]) + M[r, 2] * d[:, 2]
    assert oo.dtype == np.float32 and dd.dtype == np.float32
    return oo, dd


def oracle_classes(rs, o, d, tn, tf):
    """The oracle on rays with per-ray intervals: one call per distinct
    (tNear, tFar) pair (tests/test_rays_device.py's _oracle_classes, grouped by
    a sort instead of one mask per class)."""
    n = len(o)
    hit, t = np.zeros(n, np.int32), np.full(n, np.inf, np.float32)
    nrm, prim = np.zeros((n, 3), np.float32), np.full(n, -1, np.int64)
    key = (tn.view(np.uint32).astype(np.uint64) << np.uint64(32)) | tf.view(np.uint32).astype(np.uint64)
    order = np.argsort(key, kind="stable")
    cuts = np.flatnonzero(np.diff(key[order])) + 1
    for idx in np.split(order, cuts):
        h, tt, nn, pp = rs.intersect_rays(o[idx], d[idx], float(tn[idx[0]]), float(tf[idx[0]]))
        hit[idx], t[idx], nrm[idx], prim[idx] = h, tt, nn, pp
    return hit, t, nrm, prim


def compose(refs, blas, flags, M, o, d, tn, tf, skipped=None):
    """The header's loop. refs: oracle mesh scenes (plane off); blas, flags:
    per instance; M: float32 [K, 3, 4] as the library stores it; tn, tf:
    float32 [n]. -> (hit int32, t, normal, prim int64), a miss being
    (0, +inf, (0, 1, 0), -1)."""
    n = len(o)
    tn = np.ascontiguousarray(np.broadcast_to(np.float32(tn), (n,)))
    tf = np.ascontiguousarray(np.broadcast_to(np.float32(tf), (n,)))
    best = np.full(n, np.inf, np.float32)
    win = np.full(n, -1, np.int64)
    tri = np.zeros(n, np.int64)
    nobj = np.zeros((n, 3), np.float32)
    for i in range(len(blas)):
        if flags[i] & DISABLED or (skipped is not None and skipped[i]):
            continue
        oo, dd = to_object(M[i], o, d)
        tfi = np.where(best < tf, best, tf).astype(np.float32)
        h, t, nn, pp = oracle_classes(refs[blas[i]], oo, dd, tn, tfi)
        up = (h != 0) & (t < best)  # ties keep the lower index
        best[up], win[up], tri[up], nobj[up] = t[up], i, pp[up], nn[up]
    hit = (win >= 0).astype(np.int32)
    nrm = np.tile(np.float32([0, 1, 0]), (n, 1))
    prim = np.full(n, -1, np.int64)
    k = np.flatnonzero(win >= 0)
    if len(k):
        Mw = np.asarray(M, np.float32)[win[k]]  # [m, 3, 4]
        nx, ny, nz = nobj[k, 0], nobj[k, 1], nobj[k, 2]
        w = np.stack([(Mw[:, 0, c] * nx + Mw[:, 1, c] * ny) + Mw[:, 2, c] * nz for c in range(3)], axis=1)
        ln = np.sqrt((w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2])
        assert w.dtype == np.float32 and ln.dtype == np.float32
        nrm[k] = w / ln[:, None]
        prim[k] = (win[k] << 32) | tri[k]
    return hit, best, nrm, prim


@functools.lru_cache(maxsize=None)
def plane_only():
    """An oracle scene that answers for the plane alone: one zero-area
    triangle (its determinant is 0, every ray misses it) under the plane."""
    v = np.float32([[50, 50, 50, 1]] * 3)
    return cpuref.RefScene.mesh(v, np.arange(3, dtype=np.uint32))


def with_plane(res, o, d, tn, tf, offset, normal=(0.0, 1.0, 0.0)):
    """SceneUnion::intersect of a composed result with the plane: the smaller t
    wins, ties go to the plane (raytracing.hpp:87-93)."""
    n = len(o)
    rs = plane_only()
    rs.set_plane(True, normal, offset)
    tn = np.ascontiguousarray(np.broadcast_to(np.float32(tn), (n,)))
    tf = np.ascontiguousarray(np.broadcast_to(np.float32(tf), (n,)))
    ph, pt, pn, pp = oracle_classes(rs, o, d, tn, tf)
    assert set(np.unique(pp).tolist()) <= {-1, -2}
    hit, t, nrm, prim = (a.copy() for a in res)
    lim = np.where(ph != 0, pt, np.float32(np.inf))
    lose = ~(t < lim)
    hit[lose], t[lose], nrm[lose], prim[lose] = ph[lose], pt[lose], pn[lose], pp[lose]
    return hit, t, nrm, prim


# ------------------------------------------------------------------ meshes --
@functools.lru_cache(maxsize=None)
def mesh(name):
    """(vPos4f, indices) of the BLAS set: "cube", "bunny", "grid" (the tie-heavy
    integer lattice soup, 1,500 triangles) and "tri" (one triangle: a leaf root)."""
    if name == "cube":
        v, i = S.inputs("cube.obj")[1]
    elif name == "bunny":
        v, i = S.inputs("stanford-bunny.obj")[1]
    elif name == "grid":
        v = S.edge_mesh(20261, 1500, "grid")
        i = np.arange(len(v), dtype=np.uint32)
    else:
        v = np.float32([[-0.5, -0.4, 0.1, 1], [0.6, -0.3, 0.0, 1], [0.0, 0.7, -0.1, 1]])
        i = np.arange(3, dtype=np.uint32)
    v = np.ascontiguousarray(v, np.float32)
    i = np.ascontiguousarray(i, np.uint32)
    v.setflags(write=False)
    i.setflags(write=False)
    return v, i


@functools.lru_cache(maxsize=None)
def ref_mesh(name):
    return cpuref.RefScene.mesh(*mesh(name))


def rot(seed):
    """A rotation (or reflection) from the QR of a normal matrix, float64."""
    q, r = np.linalg.qr(np.random.default_rng(seed).normal(size=(3, 3)))
    return q * np.sign(np.diag(r))


def affine(A, b):
    """[3, 4] float32 from a 3x3 and a translation."""
    return np.concatenate([np.asarray(A, np.float64), np.asarray(b, np.float64)[:, None]], axis=1).astype(np.float32)


IDENTITY = affine(np.eye(3), np.zeros(3))


def flatten(v, xform):
    """The vertices under the object-to-world map, evaluated in float64 on the
    divided positions and rounded once (w = 1)."""
    x = np.asarray(xform, np.float64).reshape(3, 4)
    p = v[:, :3].astype(np.float64) / v[:, 3:4].astype(np.float64)
    w = p @ x[:, :3].T + x[:, 3]
    return np.concatenate([w, np.ones((len(w), 1))], axis=1).astype(np.float32)


def random_rays(n, seed, inside_frac=0.5):
    """tests/test_rays_device.py's recipe (a copy): half the origins inside the
    model box, an eighth of the directions axis-aligned."""
    rng = np.random.default_rng(seed)
    o = rng.uniform(-3, 3, (n, 3)).astype(np.float32)
    m = rng.random(n) < inside_frac
    o[m] = rng.uniform(-0.9, 0.9, (int(m.sum()), 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    k = n // 8
    axis = rng.integers(0, 3, k)
    d[:k] = 0.0
    d[np.arange(k), axis] = rng.choice([-1.0, 1.0], k).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True).astype(np.float32)
    return o, d.astype(np.float32)


# ------------------------------------------- convention under rotation -----
ROT_SEEDS = (1, 2, 3)
ROT_N = 4096


def rotation_case(name, seed):
    """One mesh under A = Q diag(s), s in [0.5, 2], b in [-1, 1], and rays from
    the radius-4 sphere aimed into b +- 1.5 -> (xform, o, d)."""
    rng = np.random.default_rng(1000 + seed)
    A = rot(seed) @ np.diag(rng.uniform(0.5, 2.0, 3))
    b = rng.uniform(-1, 1, 3)
    u = rng.normal(size=(ROT_N, 3))
    o = 4.0 * u / np.linalg.norm(u, axis=1, keepdims=True)
    target = b + rng.uniform(-1.5, 1.5, (ROT_N, 3))
    d = target - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return affine(A, b), o.astype(np.float32), d.astype(np.float32)


def assert_rotation_bounds(flat, got_hit, got_t, what):
    """At most 4 of 4096 hit flags differ; |dt| <= 1e-4 max(1, t) on common hits."""
    fh, ft = flat[0], flat[1]
    differ = int((fh != got_hit).sum())
    both = (fh != 0) & (got_hit != 0)
    rel = np.abs(ft[both].astype(np.float64) - got_t[both].astype(np.float64)) / np.maximum(1.0, ft[both])
    worst = float(rel.max()) if both.any() else 0.0
    print(f"{what}: {differ} flags differ, largest relative dt {worst:.3g}, {int(both.sum())} common hits")
    assert int(both.sum()) > 200, what
    assert differ <= 4, f"{what}: {differ} hit flags differ"
    assert worst <= 1e-4, f"{what}: relative dt {worst}"
