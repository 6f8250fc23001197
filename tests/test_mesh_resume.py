"""Resuming and unwinding mesh traversal frames (the choose-next tail of
mesh_run and mesh_run_coop, csrc/rt_scenes.h: a resumed frame reloads its next
child's box and word; builds that kept the second child's entry distance with
the frame, or hoisted the resume's loads above the leaf test, were measured
and deleted), against the oracle, bit for bit: colour,
coverage and t bits of frames, hit / t / normal / id of rays.

The meshes are the overlapping, tie-heavy ones of test_gpu_edge.py at sizes
whose trees take the 4-, 7- and 15-slot kernels: `rand` prunes at second and
at later children and visits many third-or-later children (the reload path),
`grid` and `flat` tie and have zero-thickness boxes, `same` ties every sibling
(a second child is never pruned: !(fbest < t) at equality) and is deep. Each
goes through the one-frame kernel (render) and the multi-frame launch the
bench times (render_device_frames, 3 frames), with the cooperative tail on
and off, so that 8-lane groups take over frames stacked by the per-lane loop
and the per-lane loop alone unwinds them.
"""
import functools

import numpy as np
import pytest

import cpuref
import rtamd
from test_gpu_edge import same, tri_mesh

pytestmark = pytest.mark.gpu

CAMS = ((0.0, 0.3, 2.5), (1.7, 1.2, -1.1), (-2.0, 0.4, 1.0))
SM = {"primary": (0, False), "default": (1, True)}
PLANE_Y = -1.0
# (seed, triangles, kind): frame size, shading modes
MESHES = {
    (12, 3000, "rand"): ((96, 72), ("primary", "default")),
    (11, 2000, "grid"): ((96, 72), ("primary", "default")),
    (14, 2500, "flat"): ((96, 72), ("primary", "default")),
    (13, 1500, "same"): ((96, 72), ("primary", "default")),
    (15, 6000, "same"): ((64, 48), ("primary",)),  # 15 stack slots: always 3-word frames
}
CASES = [(m, mode) for m, (_, modes) in MESHES.items() for mode in modes]
IDS = [f"{m[2]}{m[1]}-{mode}" for m, mode in CASES]


@functools.lru_cache(maxsize=None)
def scenes(mesh):
    v, i = tri_mesh(*mesh)
    return cpuref.RefScene.mesh(v, i), rtamd.BVHBuilder(rtamd.SimpleMesh(v, i))


def params(pos, W, H, mode, side):
    vi, pi = cpuref.camera_matrices(pos, (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 45.0, W / H, 0.01, 100.0)
    make = cpuref.make_params if side == "ref" else rtamd.render_params
    return make(pos, vi, pi, (2, 2, 2), SM[mode][0], True, True)


def set_plane(rs, gs, mode):
    plane = SM[mode][1]
    rs.set_plane(plane, (0.0, 1.0, 0.0), PLANE_Y)
    gs.set_plane(rtamd.Plane((0.0, 1.0, 0.0), PLANE_Y) if plane else None)


@functools.lru_cache(maxsize=None)
def oracle_frames(mesh, W, H, mode):
    """The oracle's frames of CAMS, computed once per case and shared."""
    rs, gs = scenes(mesh)
    set_plane(rs, gs, mode)
    out = []
    for pos in CAMS:
        c, t, _, _ = rs.render(params(pos, W, H, mode, "ref"), W, H)
        c.setflags(write=False)
        t.setflags(write=False)
        out.append((c, t))
    return tuple(out)


def set_coop(gs, on):
    rtamd._lib.check(rtamd.lib().rtx_set_coop(gs._handle(), int(on)))


def one_frame(gs, pos, W, H, mode):
    gc = np.zeros((H, W), np.uint32)
    gt = np.full((H, W), np.inf, np.float32)
    gs.render(params(pos, W, H, mode, "gpu"), gc, gt, clear=True)
    return gc, gt


def batch(gs, W, H, mode):
    import torch
    P = [params(pos, W, H, mode, "gpu") for pos in CAMS]
    cs = [torch.empty((H, W), dtype=torch.int32, device="cuda") for _ in P]
    ts = [torch.empty((H, W), dtype=torch.float32, device="cuda") for _ in P]
    st = torch.cuda.current_stream()
    gs.render_device_frames(P, [c.data_ptr() for c in cs], [t.data_ptr() for t in ts], W, H,
                            rtamd.RT_FLAG_CLEAR, stream=st.cuda_stream)
    torch.cuda.synchronize()
    return [(c.cpu().numpy().view(np.uint32), t.cpu().numpy()) for c, t in zip(cs, ts)]


@pytest.mark.parametrize("coop", [True, False], ids=["coop", "lanes"])
@pytest.mark.parametrize("mesh,mode", CASES, ids=IDS)
def test_one_frame_kernel(gpu, mesh, mode, coop):
    (W, H), _ = MESHES[mesh]
    _, gs = scenes(mesh)
    ref = oracle_frames(mesh, W, H, mode)
    set_plane(*scenes(mesh), mode)
    set_coop(gs, coop)
    try:
        for pos, r in zip(CAMS[:2], ref):
            same(r, one_frame(gs, pos, W, H, mode), f"{mesh} {mode} coop={coop} render {pos}")
    finally:
        set_coop(gs, True)


@pytest.mark.parametrize("coop", [True, False], ids=["coop", "lanes"])
@pytest.mark.parametrize("mesh,mode", CASES, ids=IDS)
def test_multi_frame_launch(gpu, mesh, mode, coop):
    (W, H), _ = MESHES[mesh]
    _, gs = scenes(mesh)
    ref = oracle_frames(mesh, W, H, mode)
    set_plane(*scenes(mesh), mode)
    set_coop(gs, coop)
    try:
        got = batch(gs, W, H, mode)
    finally:
        set_coop(gs, True)
    for pos, r, g in zip(CAMS, ref, got):
        same(r, g, f"{mesh} {mode} coop={coop} 3-frame launch {pos}")


@pytest.mark.parametrize("W,H", [(7, 5), (17, 13)])
@pytest.mark.parametrize("mode", ["primary", "default"])
def test_small_frames(gpu, W, H, mode):
    """Waves that start at or below the hand-over threshold of the cooperative tail."""
    mesh = (12, 3000, "rand")
    _, gs = scenes(mesh)
    ref = oracle_frames(mesh, W, H, mode)
    set_plane(*scenes(mesh), mode)
    for pos, r in zip(CAMS[:2], ref):
        same(r, one_frame(gs, pos, W, H, mode), f"rand {W}x{H} {mode} render {pos}")
    for pos, r, g in zip(CAMS, ref, batch(gs, W, H, mode)):
        same(r, g, f"rand {W}x{H} {mode} 3-frame launch {pos}")


@pytest.mark.parametrize("mesh", [(14, 2500, "flat"), (11, 2000, "grid")], ids=["flat", "grid"])
def test_rays_nonfinite_inverse_direction(gpu, mesh):
    """IScene::intersect on 4,096 rays of the exact slab path (a 1/d component
    infinite): rays inside the flat mesh's plane (y = -0.25, d.y = 0: 0 * inf =
    NaN entry distances, which are kept and visited) and axis-parallel rays
    from lattice coordinates (origins on box faces of the grid mesh)."""
    rs, gs = scenes(mesh)
    rng = np.random.default_rng(mesh[0])
    n = 2048
    o1 = rng.uniform(-1.5, 1.5, (n, 3)).astype(np.float32)
    o1[:, 1] = np.float32(-0.25)
    a = rng.uniform(0.0, 2.0 * np.pi, n)
    d1 = np.stack([np.cos(a), np.zeros(n), np.sin(a)], axis=1).astype(np.float32)
    o2 = (rng.integers(-8, 9, (n, 3)).astype(np.float32) * np.float32(0.25))
    d2 = np.zeros((n, 3), np.float32)
    d2[np.arange(n), rng.integers(0, 3, n)] = rng.choice(np.float32([-1.0, 1.0]), n)
    o = np.ascontiguousarray(np.concatenate([o1, o2]))
    d = np.ascontiguousarray(np.concatenate([d1, d2]))
    assert len(o) == 4096 and (d == 0.0).any(axis=1).all()
    rh, rt_, rn, rp = rs.intersect_rays(o, d, 0.01, 100.0)
    g = gs.intersect(o, d, 0.01, 100.0)
    assert int(rh.sum()) > 100
    assert np.array_equal(rh.astype(bool), g.hitten), "hit mask"
    assert np.array_equal(rp, g.prim), "primitive ids"
    h = g.hitten
    assert np.array_equal(rt_[h].view(np.uint32), g.t[h].view(np.uint32)), "t"
    assert np.array_equal(rn[h].view(np.uint32), g.normal[h].view(np.uint32)), "normal"
