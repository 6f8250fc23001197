"""Shared by test_shade_host.py and test_shade_gpu.py: the shading oracle of
rt_shade_rays_device (include/rtamd.h) for every scene kind.

shading_ref.intersection_color takes arbitrary rays and asks its scene for two
things only, set_plane and intersect_rays. For a mesh, a grid or an octree that
scene is the cpuref one; for an instanced scene it is InstOracle below, whose
intersect_rays is the header's loop composed from the oracle alone
(instances_common.compose, or tlas_common.compose_tlas for a scene with a
top-level tree). Everything above the geometry -- the plane, the union,
Lambert, the shadow and reflection rays, the packing, the store rule -- is
shading_ref's float32 restatement, so every comparison is on bits.
"""
import types

import numpy as np

import cpuref
import instances_common as IC
import shading_ref as SR
import tlas_common as TC

F = np.float32
INF = F(np.inf)

# ------------------------------------------------------------ the test scene --
# (BLAS mesh names, [(blas, xform, flags)]): two bunnies and a cube above the
# base plane, one triangle (a leaf-root BLAS) behind them, one disabled bunny
SCENE5 = (("bunny", "cube", "tri"), [
    (0, IC.affine(IC.rot(5) @ np.diag([0.8, 0.8, 0.8]), (-0.9, -0.2, 0.0)), 0),
    (1, IC.affine(IC.rot(6) @ np.diag([0.35, 0.5, 0.35]), (0.9, -0.5, 0.3)), 0),
    (0, IC.affine(IC.rot(7) @ np.diag([0.5, 0.5, 0.5]), (0.4, 0.9, 0.4)), 0),
    (2, IC.affine(np.eye(3), (0.0, 0.0, 1.0)), 0),
    (0, IC.IDENTITY, IC.DISABLED),
])
PLANE = SR.PLANES["base"]
FRAMES = [((97, 50), (0.6, 0.9, 3.2)), ((50, 37), (0.5, 0.8, 2.8))]  # (W, H), camera
# the per-ray intervals of the random-ray tests: (tNear, tFar) classes
CLASSES = [(0.01, 100.0), (-5.0, 100.0), (0.5, 3.0)]
N_RANDOM = 4096
# (light name, mode, shadows, reflections): Lambert with the four switch
# settings under two lights, Color and Normal once
SHADINGS = [(ln, SR.LAMBERT, sh, rf) for ln in ("std", "inside") for sh, rf in SR.LAMBERT_SWITCHES] + \
           [("std", SR.COLOR, True, True), ("std", SR.NORMAL, True, True)]


class InstOracle:
    """An instanced scene as shading_ref.Scene's base: intersect_rays is the
    header's loop on the oracle's meshes. wbox (leaf boxes [K, 6]) given: the
    loop with its box_pass line (RT_INSTANCED_TLAS)."""

    def __init__(self, refs, blas, flags, M, wbox=None, skipped=None):
        self.refs, self.blas, self.flags, self.M, self.wbox, self.skipped = refs, blas, flags, M, wbox, skipped

    def set_plane(self, *_):
        pass  # the plane is shading_ref's own

    def intersect_rays(self, o, d, tn, tf):
        o, d = np.ascontiguousarray(o, F), np.ascontiguousarray(d, F)
        if self.wbox is None:
            return IC.compose(self.refs, self.blas, self.flags, self.M, o, d, tn, tf, self.skipped)
        return TC.compose_tlas(self.refs, self.blas, self.flags, self.M, self.wbox, o, d, tn, tf, self.skipped)[:4]


def host_oracles(rt, scene=SCENE5):
    """(flat, tree) InstOracle of a scene definition from host data alone: M by
    rt_affine_inverse, a BLAS's root box taken as its vertex box (the
    one-triangle mesh is a leaf root: unbounded)."""
    names, inst = scene
    refs = {k: IC.ref_mesh(m) for k, m in enumerate(names)}
    boxes = [None if m == "tri" else TC.vertex_box(IC.mesh(m)[0]) for m in names]
    blas, flags = [t[0] for t in inst], [t[2] for t in inst]
    M = np.stack([rt.affine_inverse(t[1]) for t in inst])
    wbox = TC.leaf_boxes([t[1] for t in inst], blas, flags, boxes)
    return InstOracle(refs, blas, flags, M), InstOracle(refs, blas, flags, M, wbox)


def device_oracle(gs, names):
    """The InstOracle of a live rtamd.InstancedScene: M (and, for a scene with a
    tree, the leaf boxes) as the device holds them."""
    tab = gs.instances()
    refs = {k: IC.ref_mesh(m) if isinstance(m, str) else m for k, m in enumerate(names)}
    wbox = gs.tlas()[0] if gs.has_tlas else None
    return InstOracle(refs, tab.blas, tab.flags, tab.inv, wbox, tab.skipped)


def params(W, H, light, mode, shadows, reflections, pos, module=cpuref):
    return SR.params(W, H, SR.LIGHTS[light] if isinstance(light, str) else light, mode, shadows, reflections, pos=pos,
                     module=module)


def eye_rays(W, H, pos):
    """(origins, dirs) float32 [W*H, 3]: cpuref.primary_rays, ray y*W + x = pixel (x, y)."""
    P = params(W, H, "std", SR.LAMBERT, True, True, pos)
    d = np.ascontiguousarray(cpuref.primary_rays(P, W, H).reshape(-1, 3), F)
    return np.tile(F(pos), (len(d), 1)), d


def shade(base, plane, o, d, tn, tf, light, mode, shadows, reflections):
    """The oracle of rt_shade_rays_device with RT_SHADE_CLEAR. base: a cpuref
    scene or an InstOracle; plane: (normal, offset) or None; tn, tf: floats or
    float32 [n] (rays are independent: one intersection_color call per
    distinct (tNear, tFar) pair). -> namespace with color (uint32), t, hit
    (int32), prim (int64), rgba [n, 4], ok (bool [n]: every channel of the ray
    is defined, so its colour word is), ties (union ties of the first
    intersection)."""
    n = len(d)
    scene = SR.Scene(base, SR.Plane(*plane) if plane is not None else None)
    tn = np.ascontiguousarray(np.broadcast_to(F(tn), (n,)))
    tf = np.ascontiguousarray(np.broadcast_to(F(tf), (n,)))
    light = SR.LIGHTS[light] if isinstance(light, str) else light
    r = types.SimpleNamespace(rgba=np.zeros((n, 4), F), t=np.full(n, INF, F), prim=np.full(n, -1, np.int64), ties=0)
    key = (tn.view(np.uint32).astype(np.uint64) << np.uint64(32)) | tf.view(np.uint32).astype(np.uint64)
    order = np.argsort(key, kind="stable")
    for idx in np.split(order, np.flatnonzero(np.diff(key[order])) + 1):
        rgba, t, h = SR.intersection_color(scene, np.ascontiguousarray(o[idx]), np.ascontiguousarray(d[idx]),
                                           tn[idx[0]], tf[idx[0]], light, mode, shadows, reflections)
        r.rgba[idx], r.t[idx], r.prim[idx] = rgba, t, np.where(h.hit, h.prim, -1)
        r.ties += int(h.tie.sum())
    store = ~np.isinf(r.t)
    r.hit = store.astype(np.int32)
    r.ok = np.all((r.rgba >= 0) & (r.rgba <= 1), axis=1)
    with np.errstate(invalid="ignore"):
        r.color = np.where(store, SR.color_pack_rgba(r.rgba), 0).astype(np.uint32)
    return r
