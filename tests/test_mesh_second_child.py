"""A mesh frame's second child: the resume that reloads the child's box and
word (csrc/rt_scenes.h, mesh_run and mesh_run_coop). A second-child record in
LDS beside the frame stack once served it without the reload; it was measured
slower and deleted. Everything is compared with the
oracle bit for bit, so the file holds on any build.

What it adds to test_mesh_resume.py:
  * trees of an exact depth (asserted on the host through rt_bvh_export before
    anything is rendered): 5 levels, where the deepest top frame of the 4-slot
    kernels sits one level beyond the stack's slots, and 8
    levels, the same for the 7-slot kernels. The `same` meshes (every triangle
    identical: all siblings tie, none is pruned) walk every root-to-leaf path,
    so the deepest level is reached;
  * the cooperative hand-over on small frames (7x5, 17x13, 96x72) with the tail
    on and off: waves that start at or below the threshold, so an 8-lane group
    resumes frames the per-lane loop created;
  * every path: the one-frame kernel, a 3-frame persistent launch and
    rt_intersect_rays on 4,096 rays with a non-finite 1/d component (NaN entry
    distances, which are kept and visited);
  * the same stream state rendered twice with different cameras: nothing a
    tile left in LDS may reach a later tile.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import cpuref
import rtamd
from test_gpu_edge import same, tri_mesh

pytestmark = pytest.mark.gpu

CAMS = ((0.0, 0.3, 2.5), (1.7, 1.2, -1.1), (-2.0, 0.4, 1.0))
CAMS_B = ((0.4, -0.2, 2.2), (-1.1, 1.6, 1.3), (2.1, 0.1, -0.9))
SIZES = ((7, 5), (17, 13), (96, 72))
# (seed, triangles, kind) -> depth of its tree in inner levels (exact, or a range for the 15-slot mesh)
MESHES = {
    (13, 200, "same"): (5, 5),     # 4 slots, the deepest top frame at level 4 = SLOTS
    (11, 3000, "grid"): (5, 5),    # 4 slots, ties and zero-thickness boxes
    (12, 3000, "rand"): (4, 4),    # prunes at second and later children
    (14, 2500, "flat"): (4, 4),
    (13, 1500, "same"): (8, 8),    # 7 slots, the deepest top frame at level 7 = SLOTS
    (15, 6000, "same"): (9, 16),   # 15 slots: the path without records
}
IDS = [f"{m[2]}{m[1]}" for m in MESHES]


def host_depth(v, i):
    """max_depth of the tree the host builder makes of (v, i)."""
    L = rtamd.lib()
    rtamd._lib.check(L.rt_set_bvh_builder(1))
    try:
        nn, md = C.c_int64(0), C.c_int32(0)
        rtamd._lib.check(L.rt_bvh_export(v.ctypes.data, len(v), i.ctypes.data, len(i), None, C.byref(nn), None,
                                         C.byref(md)))
        return md.value
    finally:
        rtamd._lib.check(L.rt_set_bvh_builder(0))


@functools.lru_cache(maxsize=None)
def scenes(mesh):
    v, i = tri_mesh(*mesh)
    lo, hi = MESHES[mesh]
    d = host_depth(v, i)
    assert lo <= d <= hi, f"{mesh}: tree of {d} levels, the test needs {lo}..{hi}"
    gs = rtamd.BVHBuilder(rtamd.SimpleMesh(v, i))
    assert gs.tree_stats()[2] == d, f"{mesh}: the scene's tree has {gs.tree_stats()[2]} levels, the host's {d}"
    return cpuref.RefScene.mesh(v, i), gs


def params(pos, W, H, side):
    vi, pi = cpuref.camera_matrices(pos, (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 45.0, W / H, 0.01, 100.0)
    make = cpuref.make_params if side == "ref" else rtamd.render_params
    return make(pos, vi, pi, (2, 2, 2), 0, True, True)


@functools.lru_cache(maxsize=None)
def oracle_frames(mesh, W, H, cams=CAMS):
    """The oracle's primary-ray frames of `cams`, computed once and shared."""
    rs, _ = scenes(mesh)
    rs.set_plane(False, (0.0, 1.0, 0.0), -1.0)
    out = []
    for pos in cams:
        c, t, _, _ = rs.render(params(pos, W, H, "ref"), W, H)
        c.setflags(write=False)
        t.setflags(write=False)
        out.append((c, t))
    return tuple(out)


def set_coop(gs, on):
    rtamd._lib.check(rtamd.lib().rtx_set_coop(gs._handle(), int(on)))


def one_frame(gs, pos, W, H):
    gc = np.zeros((H, W), np.uint32)
    gt = np.full((H, W), np.inf, np.float32)
    gs.render(params(pos, W, H, "gpu"), gc, gt, clear=True)
    return gc, gt


class Launch:
    """3-frame launches into one set of device buffers on one stream."""

    def __init__(self, W, H):
        import torch
        self.torch, self.W, self.H = torch, W, H
        self.cs = [torch.empty((H, W), dtype=torch.int32, device="cuda") for _ in range(3)]
        self.ts = [torch.empty((H, W), dtype=torch.float32, device="cuda") for _ in range(3)]

    def run(self, gs, cams):
        P = [params(pos, self.W, self.H, "gpu") for pos in cams]
        st = self.torch.cuda.current_stream()
        gs.render_device_frames(P, [c.data_ptr() for c in self.cs], [t.data_ptr() for t in self.ts], self.W, self.H,
                                rtamd.RT_FLAG_CLEAR, stream=st.cuda_stream)
        self.torch.cuda.synchronize()
        return [(c.cpu().numpy().view(np.uint32), t.cpu().numpy()) for c, t in zip(self.cs, self.ts)]


@pytest.mark.parametrize("coop", [True, False], ids=["coop", "lanes"])
@pytest.mark.parametrize("W,H", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
@pytest.mark.parametrize("mesh", list(MESHES), ids=IDS)
def test_frames(gpu, mesh, W, H, coop):
    """One-frame kernel and 3-frame persistent launch, tail on and off."""
    _, gs = scenes(mesh)
    gs.set_plane(None)
    ref = oracle_frames(mesh, W, H, CAMS)
    set_coop(gs, coop)
    try:
        for pos, r in zip(CAMS[:2], ref):
            same(r, one_frame(gs, pos, W, H), f"{mesh} {W}x{H} coop={coop} render {pos}")
        got = Launch(W, H).run(gs, CAMS)
    finally:
        set_coop(gs, True)
    for pos, r, g in zip(CAMS, ref, got):
        same(r, g, f"{mesh} {W}x{H} coop={coop} 3-frame launch {pos}")


@pytest.mark.parametrize("mesh", [(13, 200, "same"), (12, 3000, "rand"), (13, 1500, "same")],
                         ids=["same200", "rand3000", "same1500"])
def test_same_stream_state_twice(gpu, mesh):
    """Two 3-frame launches with different cameras into the same buffers on the
    same stream: the second must be its own frames, whatever the first left."""
    W, H = 96, 72
    _, gs = scenes(mesh)
    gs.set_plane(None)
    la = Launch(W, H)
    for cams in (CAMS, CAMS_B, CAMS):
        ref = oracle_frames(mesh, W, H, cams)
        for pos, r, g in zip(cams, ref, la.run(gs, cams)):
            same(r, g, f"{mesh} launch {cams[0]} frame {pos}")


@pytest.mark.parametrize("mesh", list(MESHES), ids=IDS)
def test_rays_nonfinite_inverse_direction(gpu, mesh):
    """rt_intersect_rays on 4,096 rays whose direction has a zero component (1/d
    infinite: the exact slab path): rays inside the plane y = -0.25 (the flat
    mesh's: 0 * inf = NaN entry distances, kept and visited wherever they are
    met, a recorded second child included) and axis-parallel rays from lattice
    origins (on box faces of the grid mesh)."""
    rs, gs = scenes(mesh)
    rs.set_plane(False, (0.0, 1.0, 0.0), -1.0)
    gs.set_plane(None)
    rng = np.random.default_rng(mesh[0] + mesh[1])
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
    assert np.array_equal(rh.astype(bool), g.hitten), "hit mask"
    assert np.array_equal(rp, g.prim), "primitive ids"
    h = g.hitten
    assert np.array_equal(rt_[h].view(np.uint32), g.t[h].view(np.uint32)), "t"
    assert np.array_equal(rn[h].view(np.uint32), g.normal[h].view(np.uint32)), "normal"
