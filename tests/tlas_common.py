"""Shared by test_tlas_host.py and test_tlas_gpu.py: the definition of an
instanced scene with a top-level tree (RT_INSTANCED_TLAS, include/rtamd.h)
restated in numpy float32 -- world_box, box_pass, the tree's union -- and
compose_tlas, which is instances_common.compose plus the one new line.

Every operation is a float32 numpy operation in the header's order (numpy never
fuses), so the results are compared bitwise with the library's.
"""
import numpy as np

import instances_common as IC

F = np.float32
INF = F(np.inf)
PAD = F(2.0 ** -16)
EMPTY = np.array([INF, INF, INF, -INF, -INF, -INF], F)
UNBOUNDED = np.array([-INF, -INF, -INF, INF, INF, INF], F)


def _mn(a, b):  # a < b ? a : b
    return np.where(a < b, a, b).astype(F)


def _mx(a, b):  # a > b ? a : b
    return np.where(a > b, a, b).astype(F)


def leaf_count(k):
    p = 1
    while p < k:
        p *= 2
    return p


def world_box(xform, obox):
    """rt_instance_world_box: xform float32 [12] or [3, 4], obox lo.xyz hi.xyz."""
    x = np.asarray(xform, F).reshape(12)
    ob = np.asarray(obox, F).reshape(6)
    lo = hi = None
    with np.errstate(all="ignore"):
        for c in range(8):
            cx, cy, cz = ob[3 if c & 1 else 0], ob[4 if c & 2 else 1], ob[5 if c & 4 else 2]
            p = np.array([((x[4 * r] * cx + x[4 * r + 1] * cy) + x[4 * r + 2] * cz) + x[4 * r + 3] for r in range(3)], F)
            lo, hi = (p, p) if c == 0 else (_mn(lo, p), _mx(hi, p))
        a = _mx(np.abs(lo), np.abs(hi))
        w = (hi - lo).astype(F)
        mag, ext = a[0], w[0]
        for r in (1, 2):
            mag, ext = _mx(mag, a[r]), _mx(ext, w[r])
        e = F(PAD * F(mag + ext))
        out = np.concatenate([lo - e, hi + e]).astype(F)
    assert out.dtype == F
    return out


def box_pass(b, o, d, tn, tf):
    """box_pass of ONE box b[6] for rays o, d [n, 3] and tn, tf (scalars or
    [n]) -> bool [n]."""
    b = np.asarray(b, F)
    n = len(o)
    tn = np.broadcast_to(F(tn), (n,))
    tf = np.broadcast_to(F(tf), (n,))
    if b[0] > b[3]:
        return np.zeros(n, bool)
    with np.errstate(all="ignore"):
        inv = (F(1.0) / d).astype(F)
        t1 = ((b[None, :3] - o) * inv).astype(F)
        t2 = ((b[None, 3:] - o) * inv).astype(F)
        lo, hi = _mn(t1, t2), _mx(t1, t2)
        tmin = _mx(lo[:, 0], _mx(lo[:, 1], lo[:, 2]))
        tmax = _mn(hi[:, 0], _mn(hi[:, 1], hi[:, 2]))
        tmin = _mx(tmin, tn)
        tmax = _mn(tmax, tf)
        miss = (tmax < 0) | (tmin > tmax)
    return ~np.isfinite(inv).all(axis=1) | ~miss


def tree(leaves):
    """The implicit tree over leaf boxes [K, 6] -> node boxes float32 [2P, 6]
    (node 0 unused: zeros; leaves past K empty; inner = exact min / max)."""
    leaves = np.asarray(leaves, F).reshape(-1, 6)
    k = len(leaves)
    P = leaf_count(k)
    nodes = np.zeros((2 * P, 6), F)
    nodes[P:] = EMPTY
    nodes[P:P + k] = leaves
    for n in range(P - 1, 0, -1):
        a, c = nodes[2 * n], nodes[2 * n + 1]
        nodes[n, :3] = _mn(a[:3], c[:3])
        nodes[n, 3:] = _mx(a[3:], c[3:])
    return nodes


def leaf_boxes(xforms, blas, flags, root_boxes, skipped=None):
    """wbox_i of the definition. root_boxes[b]: float32 [6], None for a BLAS
    that is one leaf (unbounded), "empty" for an empty BLAS."""
    out = np.tile(EMPTY, (len(blas), 1))
    for i in range(len(blas)):
        if flags[i] & IC.DISABLED or (skipped is not None and skipped[i]):
            continue
        rb = root_boxes[blas[i]]
        if isinstance(rb, str):
            continue
        out[i] = UNBOUNDED if rb is None else world_box(xforms[i], rb)
    return out


def compose_tlas(refs, blas, flags, M, wbox, o, d, tn, tf, skipped=None):
    """instances_common.compose with the one new line of the header: instance i
    is tried by the rays with box_pass(wbox[i], o, d, tNear, tf_i) only.
    -> (hit int32, t, normal, prim int64, BLAS traversals per ray int32)."""
    n = len(o)
    tn = np.ascontiguousarray(np.broadcast_to(F(tn), (n,)))
    tf = np.ascontiguousarray(np.broadcast_to(F(tf), (n,)))
    best = np.full(n, np.inf, F)
    win = np.full(n, -1, np.int64)
    tri = np.zeros(n, np.int64)
    nobj = np.zeros((n, 3), F)
    trav = np.zeros(n, np.int32)
    for i in range(len(blas)):
        if flags[i] & IC.DISABLED or (skipped is not None and skipped[i]):
            continue
        tfi = np.where(best < tf, best, tf).astype(F)
        idx = np.flatnonzero(box_pass(wbox[i], o, d, tn, tfi))  # <- new, on the WORLD ray
        if not len(idx):
            continue
        trav[idx] += 1
        oo, dd = IC.to_object(M[i], np.ascontiguousarray(o[idx]), np.ascontiguousarray(d[idx]))
        h, t, nn, pp = IC.oracle_classes(refs[blas[i]], oo, dd, np.ascontiguousarray(tn[idx]), np.ascontiguousarray(tfi[idx]))
        up = (h != 0) & (t < best[idx])  # ties keep the lower index
        j = idx[up]
        best[j], win[j], tri[j], nobj[j] = t[up], i, pp[up], nn[up]
    hit = (win >= 0).astype(np.int32)
    nrm = np.tile(F([0, 1, 0]), (n, 1))
    prim = np.full(n, -1, np.int64)
    k = np.flatnonzero(win >= 0)
    if len(k):
        Mw = np.asarray(M, F)[win[k]]
        nx, ny, nz = nobj[k, 0], nobj[k, 1], nobj[k, 2]
        w = np.stack([(Mw[:, 0, c] * nx + Mw[:, 1, c] * ny) + Mw[:, 2, c] * nz for c in range(3)], axis=1)
        ln = np.sqrt((w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2])
        assert w.dtype == F and ln.dtype == F
        nrm[k] = w / ln[:, None]
        prim[k] = (win[k] << 32) | tri[k]
    return hit, best, nrm, prim, trav


def any_hit_tlas(refs, blas, flags, M, wbox, o, d, tn, tf, skipped=None):
    """RT_RAYS_ANY_HIT of the definition, literally: the OR over the instances
    with box_pass(wbox_i, o, d, tNear, tFar) of the BLAS hit flag under the full
    tFar (the closest-hit oracle's flag is its any-hit flag) -> int32 [n]."""
    n = len(o)
    tn = np.ascontiguousarray(np.broadcast_to(F(tn), (n,)))
    tf = np.ascontiguousarray(np.broadcast_to(F(tf), (n,)))
    occ = np.zeros(n, bool)
    for i in range(len(blas)):
        if flags[i] & IC.DISABLED or (skipped is not None and skipped[i]):
            continue
        idx = np.flatnonzero(box_pass(wbox[i], o, d, tn, tf) & ~occ)
        if not len(idx):
            continue
        oo, dd = IC.to_object(M[i], np.ascontiguousarray(o[idx]), np.ascontiguousarray(d[idx]))
        h = IC.oracle_classes(refs[blas[i]], oo, dd, np.ascontiguousarray(tn[idx]), np.ascontiguousarray(tf[idx]))[0]
        occ[idx[h != 0]] = True
    return occ.astype(np.int32)


def vertex_box(v):
    """lo.xyz hi.xyz of a vPos4f array (w = 1)."""
    p = np.asarray(v, F)[:, :3]
    return np.concatenate([p.min(0), p.max(0)]).astype(F)


def scene130():
    """130 instances alternating over two BLAS ("cube", "grid"): neighbouring
    lanes hold different meshes, K exceeds two waves of lanes, P = 256 with 126
    empty leaves -> (mesh names, [(blas, xform, flags)])."""
    rng = np.random.default_rng(130)
    inst = []
    for k in range(130):
        c = np.float64([k % 6, (k // 6) % 6, k // 36]) * 0.8 - [2.0, 2.0, 1.2]
        if k % 2 == 0:
            x = IC.affine(IC.rot(300 + k) @ np.diag(rng.uniform(0.15, 0.3, 3)), c)
        else:  # the lattice soup spans 0 .. 7: scaled down to about the same size
            x = IC.affine(IC.rot(300 + k) @ np.diag(rng.uniform(0.04, 0.07, 3)), c)
        inst.append((k % 2, x, 0))
    return ("cube", "grid"), inst


def eye_rays(w=64, h=64, pos=(0.3, 0.4, 6.0)):
    """w x h pinhole eye rays from pos towards the origin (coherent waves)."""
    import cpuref
    vi, pi = cpuref.camera_matrices(pos, (0, 0, 0), (0, 1, 0), 45.0, w / h, 0.01, 100.0)
    d = np.ascontiguousarray(cpuref.primary_rays(cpuref.make_params(pos, vi, pi), w, h).reshape(-1, 3), F)
    return np.tile(F(pos), (len(d), 1)), d
