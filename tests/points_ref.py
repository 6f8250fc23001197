"""The closest-point query's definition for everything the oracle does not
export (include/rtamd.h, rt_sdf_mesh_points_device): a numpy float32
restatement of oracle/cpuref.cpp's sdfref::closest and of the brute-force
lexicographic minimum over all triangles, vectorised over points x triangles.

Every operation is one f32 numpy operation in the oracle's order (numpy never
fuses a*b+c); the six region tests of Ericson's ClosestPtPointTriangle are all
evaluated and then selected in Ericson's order. test_points_host.py pins
sqrt(d2) to |cpuref.sdf_points| bit for bit, which keeps this yardstick honest.
"""
import numpy as np

import scenes as S

F = np.float32
TRI_SLICE = 12288   # triangles per slice: bounds the temporaries (points x slice f32 arrays)
POINT_SLICE = 256


def mesh(name):
    kind, (v, i), _ = S.inputs(name)
    assert kind == "mesh"
    return v, i


def corners(v, i):
    """(a, b, c): float32 [T,3] corners in original triangle order, after v /= v.w."""
    p = (v[:, :3] / v[:, 3:4]).astype(F)
    t = np.asarray(i, np.int64).reshape(-1, 3)
    return p[t[:, 0]], p[t[:, 1]], p[t[:, 2]]


def points(name, n, seed):
    """tests/test_sdfgen.py's _points: n uniform points in [-1,1]^3, n points
    0.01-normal around random vertices, and those n vertices themselves."""
    v, _ = mesh(name)
    rng = np.random.default_rng(seed)
    u = rng.uniform(-1, 1, (n, 3)).astype(F)
    pv = (v[:, :3] / v[:, 3:4])[rng.integers(0, len(v), n)]
    near = (pv + rng.normal(0, 0.01, (n, 3))).astype(F)
    return np.ascontiguousarray(np.concatenate([u, near, pv.astype(F)]))


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def closest_all(p, a, b, c):
    """sdfref::closest for points p [N,3] against triangles a, b, c [T,3]:
    (q [3][N,T], feat [N,T] int8, d2 [N,T]); d2 = dot(p - q, p - q)."""
    P = [p[:, None, k] for k in range(3)]
    A = [a[None, :, k] for k in range(3)]
    B = [b[None, :, k] for k in range(3)]
    Cc = [c[None, :, k] for k in range(3)]
    with np.errstate(all="ignore"):
        ab = [B[k] - A[k] for k in range(3)]
        ac = [Cc[k] - A[k] for k in range(3)]
        ap = [P[k] - A[k] for k in range(3)]
        d1, d2 = _dot(ab, ap), _dot(ac, ap)
        bp = [P[k] - B[k] for k in range(3)]
        d3, d4 = _dot(ab, bp), _dot(ac, bp)
        vc = d1 * d4 - d3 * d2
        cp = [P[k] - Cc[k] for k in range(3)]
        d5, d6 = _dot(ab, cp), _dot(ac, cp)
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        zero = F(0)
        in_a = (d1 <= zero) & (d2 <= zero)
        in_b = (d3 >= zero) & (d4 <= d3)
        in_ab = (vc <= zero) & (d1 >= zero) & (d3 <= zero)
        in_c = (d6 >= zero) & (d5 <= d6)
        in_ac = (vb <= zero) & (d2 >= zero) & (d6 <= zero)
        e43, e56 = d4 - d3, d5 - d6
        in_bc = (va <= zero) & (e43 >= zero) & (e56 >= zero)
        v_ab = d1 / (d1 - d3)
        w_ac = d2 / (d2 - d6)
        w_bc = e43 / (e43 + e56)
        denom = F(1) / ((va + vb) + vc)
        v_f, w_f = vb * denom, vc * denom
        # Ericson's order: a, b, ab, c, ac, bc, face (the first test that holds wins)
        conds = [in_a, in_b, in_ab, in_c, in_ac, in_bc]
        feats = [0, 1, 3, 2, 4, 5]
        feat = np.full(in_a.shape, 6, np.int8)
        for cond, f in zip(reversed(conds), reversed(feats)):
            feat = np.where(cond, np.int8(f), feat)
        q = []
        for k in range(3):
            shape = feat.shape
            cand = {0: np.broadcast_to(A[k], shape), 1: np.broadcast_to(B[k], shape), 2: np.broadcast_to(Cc[k], shape),
                    3: A[k] + ab[k] * v_ab, 4: A[k] + ac[k] * w_ac, 5: B[k] + (Cc[k] - B[k]) * w_bc,
                    6: (A[k] + ab[k] * v_f) + ac[k] * w_f}
            qk = cand[6]
            for f in (5, 4, 2, 3, 1, 0):
                qk = np.where(feat == f, cand[f], qk)
            q.append(qk.astype(F, copy=False))
        e = [P[k] - q[k] for k in range(3)]
        dd = _dot(e, e)
    return q, feat, dd.astype(F, copy=False)


def brute_force(v, i, p, radius=np.inf):
    """The definition: for every point the lexicographic minimum of
    (d2, triangle id) over the triangles with r >= 0 && d2 <= r*r.
    radius: a scalar or [N]. -> dict of d2 (f32, +inf without a winner),
    closest [N,3] (p itself, bit for bit, without a winner), prim int64 (-1)
    and feature int32 (-1)."""
    p = np.ascontiguousarray(p, F)
    n = len(p)
    a, b, c = corners(v, i)
    r = np.broadcast_to(np.asarray(radius, F), (n,))
    with np.errstate(all="ignore"):
        r2 = r * r
    out_d2 = np.full(n, np.inf, F)
    out_q = p.copy()
    out_prim = np.full(n, -1, np.int64)
    out_feat = np.full(n, -1, np.int32)
    for p0 in range(0, n, POINT_SLICE):
        ps = slice(p0, min(p0 + POINT_SLICE, n))
        pp = p[ps]
        k = len(pp)
        rows = np.arange(k)
        best = np.full(k, np.inf, F)
        won = np.zeros(k, bool)
        for t0 in range(0, len(a), TRI_SLICE):
            ts = slice(t0, t0 + TRI_SLICE)
            q, feat, d2 = closest_all(pp, a[ts], b[ts], c[ts])
            ok = (r[ps, None] >= F(0)) & (d2 <= r2[ps, None])  # (NaN d2 or NaN r: no candidate)
            key = np.where(ok, d2, F(np.inf))
            j = np.argmin(key, axis=1)  # the first minimum: the lowest id of this slice
            cand = ok[rows, j]
            kd = key[rows, j]
            # an earlier slice holds lower ids, so a later one must be strictly closer
            take = cand & (~won | (kd < best))
            best = np.where(take, kd, best)
            won |= take
            sel = np.flatnonzero(take)
            if sel.size:
                g = p0 + sel
                out_d2[g] = kd[sel]
                out_prim[g] = t0 + j[sel]
                out_feat[g] = feat[sel, j[sel]]
                for x in range(3):
                    out_q[g, x] = q[x][sel, j[sel]]
    return {"d2": out_d2, "closest": out_q, "prim": out_prim, "feature": out_feat}


def brute_force_near(v, i, p, dist, cells=8):
    """brute_force(v, i, p) for a mesh too large to pair every point with
    every triangle (the bunny: 69k triangles), given each point's distance to
    the mesh `dist` (|cpuref.sdf_points|, the oracle's own brute force).

    A triangle whose bounding box is farther from the point than
    dist * (1 + 1e-4) + 1e-5 cannot hold the minimum: its exact distance is at
    least the box's, and the f32 evaluation of either differs from the exact
    value by far less than that margin for data in [-1,1]^3. Leaving such
    triangles out therefore does not change the lexicographic minimum of
    (d2, id). The triangles are grouped by the cell of a cells^3 grid their
    centroid falls in; a group (split at TRI_SLICE triangles) whose own box is
    out of reach of a point is skipped for that point, every other
    (point, group) pair is evaluated in full, and groups are merged by
    (d2, id). Every point is answered; none is sampled."""
    p = np.ascontiguousarray(p, F)
    n = len(p)
    a, b, c = corners(v, i)
    reach = np.abs(dist).astype(np.float64) * (1 + 1e-4) + 1e-5
    lo = np.minimum(np.minimum(a, b), c).astype(np.float64)
    hi = np.maximum(np.maximum(a, b), c).astype(np.float64)
    cen = (lo + hi) / 2
    g0, g1 = cen.min(0), cen.max(0)
    cell = np.minimum((cells * (cen - g0) / np.maximum(g1 - g0, 1e-30)).astype(np.int64), cells - 1)
    key = (cell[:, 0] * cells + cell[:, 1]) * cells + cell[:, 2]
    order = np.argsort(key, kind="stable")  # ids ascending inside a group
    cuts = np.flatnonzero(np.diff(key[order])) + 1
    groups = []
    for g in np.split(order, cuts):
        groups += [g[k:k + TRI_SLICE] for k in range(0, len(g), TRI_SLICE)]
    out_d2 = np.full(n, np.inf, F)
    out_q = p.copy()
    out_prim = np.full(n, -1, np.int64)
    out_feat = np.full(n, -1, np.int32)
    p64 = p.astype(np.float64)
    for g in groups:
        glo, ghi = lo[g].min(0), hi[g].max(0)
        d = np.maximum(np.maximum(glo - p64, p64 - ghi), 0.0)
        sel = np.flatnonzero(np.sqrt((d * d).sum(1)) <= reach)
        for s0 in range(0, len(sel), POINT_SLICE):
            ps = sel[s0:s0 + POINT_SLICE]
            q, feat, d2 = closest_all(p[ps], a[g], b[g], c[g])
            rows = np.arange(len(ps))
            j = np.argmin(d2, axis=1)
            kd, ids = d2[rows, j], g[j]
            take = (kd < out_d2[ps]) | ((kd == out_d2[ps]) & ((out_prim[ps] < 0) | (ids < out_prim[ps])))
            t = ps[take]
            out_d2[t] = kd[take]
            out_prim[t] = ids[take]
            out_feat[t] = feat[rows[take], j[take]]
            for x in range(3):
                out_q[t, x] = q[x][rows[take], j[take]]
    return {"d2": out_d2, "closest": out_q, "prim": out_prim, "feature": out_feat}


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize])
