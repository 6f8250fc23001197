"""Independent float32 restatement of the reference's shading path -- TEST HELPER.

What sits above IScene::intersect of the base scene, written from the
reference text (raytracing.hpp:83-97, 119-186; raytracing.cpp:8-102) and the
shim formulas of SURVEY.md 8(c), vectorised in numpy: Plane, SceneUnion,
Renderer::intersectionColor, color_pack_rgba and draw's store rule. Geometry
comes only from cpuref.primary_rays and RefScene.intersect_rays with the
oracle's plane switched off, one call each for the primary, shadow, reflection
and reflection-shadow rays. Every operation is a float32 operation in the
reference's order: dot = (x*x + y*y) + z*z, normalize = a / sqrt(dot).

The module also holds the parameter space the shading tests share (planes,
lights, switches, the camera) and the non-vacuity floors of its cases.
"""
import functools
import types
import zlib

import numpy as np

import cpuref

F = np.float32
INF = F(np.inf)

# ------------------------------------------------------------ parameter space --
PLANES = {
    # name: (normal, offset)
    "base": ((0.0, 1.0, 0.0), -1.0),
    "xdom": ((0.8, 0.36, 0.48), -1.1),       # unit, recalcBasis' x-dominant branch
    "away": ((0.0, -0.6, 0.8), -1.2),        # the other branch, pointing away
    "axis": ((1.0, 0.0, 0.0), -1.0),
    "nonunit": ((0.3, 2.0, -0.5), -2.0),
    "xeqy": ((0.6, 0.6, 0.5), -1.0),         # |x| == |y|: the strict >
    "negzero": ((-0.0, 1.0, 0.0), -1.0),
    "through": ((0.0, 1.0, 0.0), 0.0),       # shadow / reflection origins inside the model
    "never": ((0.0, 0.0, 0.0), 0.0),         # enabled, never hit
}
LIGHTS = {
    "std": (2.0, 2.0, 2.0),
    "side": (-1.5, 0.5, 3.0),
    "inside": (0.0, 0.0, 0.0),
    "below": (0.5, -3.0, 0.5),
    "far": (50.0, 80.0, -30.0),
}
NORMAL, LAMBERT, COLOR = 0, 1, 2
LAMBERT_SWITCHES = [(True, True), (True, False), (False, True), (False, False)]  # (shadows, reflections)
CAMERA = (0.9, 0.7, 2.3)
SIZES = [(96, 72), (97, 50)]

# the coplanar union: test_gpu_edge's "flat" soup lies in this plane
FLAT_PLANE = ((0.0, 1.0, 0.0), -0.25)
FLAT_CAMERAS = [(0.0, 0.3, 2.5), (1.7, 1.2, -1.1), (0.0, 2.0, 0.0001)]
# one multi-frame launch: (camera, light name, mode, shadows, reflections) per frame
BATCH_PLANE = "xdom"
BATCH_FRAMES = [
    ((0.9, 0.7, 2.3), "std", LAMBERT, True, True),
    ((0.0, 0.0, 2.5), "side", LAMBERT, True, False),
    ((1.7, 1.2, -1.1), "inside", LAMBERT, False, True),
    ((-1.2, 0.4, 2.0), "below", LAMBERT, False, False),
    ((0.3, 2.0, 1.2), "far", COLOR, True, True),
    ((0.9, 0.7, 2.3), "side", NORMAL, True, True),
]


def batch_params(W, H, module=cpuref):
    return [params(W, H, LIGHTS[ln], mode, sh, rf, pos=pos, module=module) for pos, ln, mode, sh, rf in BATCH_FRAMES]


def params(W, H, light, mode, shadows, reflections, pos=CAMERA, module=cpuref):
    vi, pi = cpuref.camera_matrices(pos, (0, 0, 0), (0, 1, 0), 45.0, W / H, 0.01, 100.0)
    if module is cpuref:
        return cpuref.make_params(pos, vi, pi, light, mode, shadows, reflections)
    return module.render_params(pos, vi, pi, light, mode, shadows, reflections)


def cases(planes=None, lights=None):
    """(plane name, light name, mode, shadows, reflections): Lambert with all
    four switch combinations under every light; Color and Normal (which read
    neither the light nor the switches) once per plane."""
    out = []
    for pn in planes or PLANES:
        for ln in lights or LIGHTS:
            out += [(pn, ln, LAMBERT, sh, rf) for sh, rf in LAMBERT_SWITCHES]
        out.append((pn, "std", COLOR, True, True))
        if pn != "nonunit":
            # Normal mode stores (n + 1) / 2 of the plane's normal as given: 1.5 or -0.5
            # for the non-unit (0.3, 2, -0.5), outside [0, 1], where the packing's
            # float -> uint32 cast is not defined on the CPU and not part of parity
            out.append((pn, "std", NORMAL, True, True))
    return out


# ----------------------------------------------------------------- float32 math --
def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def normalize(a):
    return a / np.sqrt(dot(a, a))[..., None]


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


class Hits:
    """HitInfo for a batch: a miss has t = +inf; prim is -1 for a miss, -2 for
    the plane. albedo is one value per ray (the reference's albedos are grey)."""

    def __init__(self, hit, t, normal, albedo, refl, prim):
        self.hit, self.t, self.normal, self.albedo, self.refl, self.prim = hit, t, normal, albedo, refl, prim
        self.tie = np.zeros(len(hit), bool)  # the union's two operands hit at the same t


class Plane:
    """Plane(normal, offset) (raytracing.hpp:119-186): the normal is stored as
    given, not normalised."""

    def __init__(self, normal, offset):
        self.n = np.asarray(normal, F)
        self.off = F(offset)
        n = self.n
        a = np.abs(n)
        with np.errstate(all="ignore"):  # the (0, 0, 0) normal: a NaN basis that no hit ever reads
            if a[0] > a[1] and a[0] > a[2]:
                self.b1 = normalize(np.array([n[1], -n[0], 0], F))
            else:
                self.b1 = normalize(np.array([0, n[2], -n[1]], F))
            self.b2 = normalize(cross(self.b1, n))

    def intersect(self, o, d, tnear, tfar):
        n = len(d)
        div = dot(d, self.n)
        ok = ~(np.abs(div) < F(1e-8))
        with np.errstate(all="ignore"):
            t = (self.off - dot(o, self.n)) / div
        hit = ok & ~((t < F(tnear)) | (t > F(tfar)))
        ts = np.where(hit, t, F(0))
        p = o + ts[:, None] * d
        with np.errstate(all="ignore"):
            x = np.where(hit, np.ceil(dot(p, self.b1)), F(0)).astype(np.int64)
            y = np.where(hit, np.ceil(dot(p, self.b2)), F(0)).astype(np.int64)
        albedo = np.where(np.fmod(x + y, 2) == 0, F(0), F(1)).astype(F)  # C's %: -1 for a negative odd sum
        return Hits(hit, np.where(hit, t, INF).astype(F), np.broadcast_to(self.n, (n, 3)).copy(),
                    np.where(hit, albedo, F(1)), np.where(hit, F(0.3), F(0)).astype(F),
                    np.where(hit, -2, -1).astype(np.int64))


class Scene:
    """The base scene (oracle geometry, its plane switched off) or, with a
    plane, SceneUnion(base, plane): (h1.t < h2.t) ? h1 : h2."""

    def __init__(self, base, plane=None):
        self.base, self.plane = base, plane

    def intersect(self, o, d, tnear, tfar):
        o = np.ascontiguousarray(np.broadcast_to(np.asarray(o, F), d.shape))
        self.base.set_plane(False, (0, 1, 0), 0.0)
        bh, bt, bn, bp = self.base.intersect_rays(o, d, F(tnear), F(tfar))
        bh = bh.astype(bool)
        h1 = Hits(bh, np.where(bh, bt, INF).astype(F), bn, np.ones(len(d), F), np.zeros(len(d), F),
                  np.where(bh, bp, -1))
        if self.plane is None:
            return h1
        h2 = self.plane.intersect(o, d, tnear, tfar)
        first = h1.t < h2.t
        pick = lambda a, b: np.where(first[:, None] if a.ndim == 2 else first, a, b)
        u = Hits(pick(h1.hit, h2.hit), pick(h1.t, h2.t), pick(h1.normal, h2.normal), pick(h1.albedo, h2.albedo),
                 pick(h1.refl, h2.refl), pick(h1.prim, h2.prim))
        u.tie = h1.hit & h2.hit & (h1.t == h2.t)
        return u


def intersection_color(scene, o, d, tnear, tfar, light, mode, shadows, reflections, depth=2):
    """Renderer::intersectionColor (raytracing.cpp:13-65) for a batch of rays
    -> (rgba float32 [n, 4], t [n], Hits of the first intersection); the caller
    has folded tPrev into tfar."""
    n = len(d)
    o = np.broadcast_to(np.asarray(o, F), d.shape)
    light = np.asarray(light, F)
    h = scene.intersect(o, d, tnear, tfar)
    rgba = np.zeros((n, 4), F)
    rgba[:, 3] = F(1)
    t = np.where(h.hit, h.t, INF).astype(F)
    k = np.flatnonzero(h.hit)
    if len(k) == 0:
        return rgba, t, h
    o, d = o[k], d[k]
    nrm, alb, refl, th = h.normal[k], h.albedo[k], h.refl[k], h.t[k]
    nrm = np.where((dot(nrm, d) > 0)[:, None], nrm * F(-1), nrm)
    if mode == NORMAL:
        c = (np.concatenate([nrm, np.ones((len(k), 1), F)], 1) + F(1)) / F(2)
    elif mode == COLOR:
        c = np.stack([alb, alb, alb, np.ones(len(k), F)], 1)
    else:
        point = o + th[:, None] * d
        visible = np.ones(len(k), bool)
        if shadows:
            sd = normalize(light - point)
            visible = ~scene.intersect(point + F(0.3) * sd, sd, 0.01, 100.0).hit
        amb = alb * F(0.1)
        lam = dot(-normalize(point - light), nrm)
        lam = np.where(lam < 0, F(0), lam) * alb  # std::max(x, 0.0f) * albedo
        lit = amb + lam
        lit = np.where(F(1) < lit, F(1), lit)    # min(x, 1)
        g = np.where(visible, lit, amb)
        c = np.stack([g, g, g, np.ones(len(k), F)], 1)
        m = np.flatnonzero(refl > 0) if (reflections and depth > 1) else []
        if len(m):
            R = normalize(nrm[m] * dot(d[m], nrm[m])[:, None] * F(-2) + d[m])
            rc, _, _ = intersection_color(scene, point[m] + F(0.02) * R, R, 0.01, 100.0, light, mode, shadows,
                                          reflections, depth - 1)
            r = refl[m][:, None]
            c[m] = c[m] * (F(1) - r) + r * rc
    rgba[k] = c
    return rgba, t, h


def color_pack_rgba(rgba):
    w = (rgba * F(255)).astype(np.uint32)  # (uint32_t)(c * 255.0f): truncation
    return (w[:, 3] << 24) | (w[:, 2] << 16) | (w[:, 1] << 8) | w[:, 0]


def defined(rgba):
    """No shaded channel is NaN or outside [0, 1]: the packing is defined."""
    return bool(np.all((rgba >= 0) & (rgba <= 1)))


def render(base, plane, P, W, H, color=None, t=None):
    """Renderer::draw (raytracing.cpp:67-102). color / t given: a uniform tPrev,
    passed as tfar = min(100, tPrev); unhit pixels keep what the buffers hold."""
    scene = Scene(base, Plane(*plane) if plane is not None else None)
    d = cpuref.primary_rays(P, W, H).reshape(-1, 3)
    tprev = INF
    if t is not None:
        tprev = F(t.flat[0])
        assert np.all(t == tprev), "the restatement takes a uniform tPrev only"
    light = tuple(P.light_pos)
    rgba, tn, h = intersection_color(scene, np.array(tuple(P.camera_pos), F), d, 0.01, min(F(100.0), tprev), light,
                                     int(P.shading_mode), bool(P.enable_shadows), bool(P.enable_reflections))
    fr = types.SimpleNamespace()
    fr.ties = int(h.tie.sum())
    fr.rgba, fr.prim = rgba.reshape(H, W, 4), h.prim.reshape(H, W)
    fr.defined = defined(rgba)
    fr.color = np.zeros((H, W), np.uint32) if color is None else color.copy()
    fr.t = np.full((H, W), np.inf, np.float32) if t is None else t.copy()
    store = ~np.isinf(tn).reshape(H, W)
    with np.errstate(invalid="ignore"):
        fr.color[store] = color_pack_rgba(rgba).reshape(H, W)[store]
    fr.t[store] = tn.reshape(H, W)[store]
    return fr


# --------------------------------------------------------- oracle-side checks --
SOUPS = {"rand": (4, 300, "rand"), "flat": (7, 120, "flat")}  # test_gpu_edge.tri_mesh arguments


def soup_mesh(key):
    from test_gpu_edge import tri_mesh
    return tri_mesh(*SOUPS[key])


@functools.lru_cache(maxsize=None)
def base_scene(key):
    """Oracle scene by name: a shipped file, or "rand" / "flat" (test_gpu_edge's
    300-triangle soup and its 120 coplanar triangles at y = -0.25)."""
    if key in SOUPS:
        return cpuref.RefScene.mesh(*soup_mesh(key))
    import scenes
    return scenes.ref_scene(key)


def plane_for(key, plane_name):
    """The plane of the parameter space for scene `key`. The octrees fill more
    of the frame than the bunny: under the non-unit plane at offset -2 the
    reflection switch changes only 934-980 of their pixels (floor 1000), so for
    them that plane moves to offset -1.6 (1019-1178 pixels)."""
    n, off = PLANES[plane_name]
    if plane_name == "nonunit" and key.endswith(".octree"):
        off = -1.6
    return n, off


def oracle_frame(base, plane, P, W, H, color=None, t=None):
    """The oracle's frame for the same inputs -> (color, t, prim)."""
    if plane is None:
        base.set_plane(False, (0, 1, 0), 0.0)
    else:
        base.set_plane(True, plane[0], plane[1])
    c, tt, prim, _ = base.render(P, W, H, None if color is None else color.copy(),
                                 None if t is None else t.copy(), prim=True)
    return c, tt, prim


@functools.lru_cache(maxsize=512)  # one scene's cases at both frame sizes
def oracle_case(key, W, H, case):
    """The oracle's (color, t, prim) of one case of cases(), computed once and
    shared; callers must not write into the arrays."""
    pn, ln, mode, sh, rf = case
    return oracle_frame(base_scene(key), plane_for(key, pn), params(W, H, LIGHTS[ln], mode, sh, rf), W, H)


def random_rays(key, plane, tn):
    """20 000 of test_gpu_parity's random rays, four in five of the origins
    inside the model's box: with half of them there, fewer than 1000 rays end
    on the bunny once tNear = -5 lets the plane catch rays behind their origin."""
    from test_gpu_parity import _random_rays
    return _random_rays(20000, zlib.crc32(f"{key}{plane}{tn}".encode()), inside_frac=0.8)


FLOORS = dict(plane_px=1000, model_px=300, shadow_px=100, refl_px=1000)
FLOOR_SIZE = (96, 72)
# Lights under which the shadow switch changes fewer than 100 pixels of the
# 96x72 oracle frame (figures in the comments, measured on the oracle). Parity
# is asserted for them like for every other case; the shadow floor is asserted
# for the other lights of the plane. The through-model plane hides the lower
# half of the model, so little of it is left to cast a shadow; with the
# never-hit plane only self-shadowing is left, none at all on the convex cube.
SHADOW_FLOOR_EXEMPT = {
    ("cube.obj", "through"): {"std", "inside", "below", "far"},        # 22, 0, 0, 66 (side: 310)
    ("cube.obj", "never"): {"std", "side", "inside", "below", "far"},  # 0: a convex model
    ("stanford-bunny.obj", "through"): {"std", "far"},                 # 14, 5
    ("stanford-bunny.obj", "never"): {"std", "side", "far"},           # 13, 2, 57
    ("example_grid.grid", "nonunit"): {"far"},                         # 99
    ("example_grid.grid", "through"): {"far"},                         # 28
    ("example_grid.grid", "never"): {"std", "side", "far"},            # 18, 88, 49
    ("sdf_5.octree", "through"): {"std", "far"},                       # 27, 33
    ("sdf_5.octree", "never"): {"std", "side"},                        # 59, 17
    ("sdf_6.octree", "through"): {"std", "far"},                       # 31, 37
    ("sdf_6.octree", "never"): {"std", "side"},                        # 59, 23
}


def floor_figures(key, plane_name, light_name):
    """Non-vacuity figures of one (plane, light) Lambert case on the oracle's
    96x72 frames: plane and model pixels (prim), pixels the shadow switch
    changes, pixels the reflection switch changes."""
    W, H = FLOOR_SIZE
    fr = {sw: oracle_case(key, W, H, (plane_name, light_name, LAMBERT) + sw) for sw in LAMBERT_SWITCHES}
    c, _, prim = fr[(True, True)]
    return dict(plane_px=int((prim == -2).sum()), model_px=int((prim >= 0).sum()),
                shadow_px=int((c != fr[(False, True)][0]).sum()),
                refl_px=int((c != fr[(True, False)][0]).sum()))


def assert_floors(key):
    """Every Lambert (plane, light) case of scene `key` is not vacuous."""
    for pn in PLANES:
        for ln in LIGHTS:
            fig = floor_figures(key, pn, ln)
            for name, floor in FLOORS.items():
                if pn == "never" and name in ("plane_px", "refl_px"):
                    continue
                if name == "shadow_px" and ln in SHADOW_FLOOR_EXEMPT.get((key, pn), ()):
                    continue
                assert fig[name] >= floor, f"{key} plane {pn} light {ln}: {name} = {fig[name]} < {floor}"
