"""Tile cull of the mesh primary path (render_pixels / cull_rect in
csrc/rt_device.hip): with the switch on and off the kernels store the same
bits, and both equal the oracle's, through every launch path and store mode:
the one-frame kernel, the multi-frame launch (three cameras, one looking
away), row-band tiles of two ranks, RT_FLAG_CLEAR, CLEAR | HITS_ONLY into a
cleared frame, and no flag into a frame that holds a pattern and a finite
tPrev (culled pixels keep the pattern).

Frames are 96x72 and 98x50 (a partial last tile, W % 4 != 0); the meshes are
the cube and the 3,000-triangle `rand` soup of test_mesh_resume.py.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import cpuref
import rtamd
import scenes as S
from rtamd import tiles
from test_mesh_resume import CAMS, scenes as soup_scenes

pytestmark = pytest.mark.gpu

RAND = (12, 3000, "rand")
SIZES = [(96, 72), (98, 50)]
AWAY = ((0.3, 0.2, 3.0), (0.3, 0.2, 6.0))  # position, target: the scene is behind the camera
# the multi-frame launch's cameras: position, target
VIEWS = ((CAMS[0], (0.0, 0.0, 0.0)), AWAY, (CAMS[1], (0.0, 0.0, 0.0)))
CLEAR, HITS_ONLY = rtamd.RT_FLAG_CLEAR, rtamd._lib.RT_FLAG_HITS_ONLY
MODES = {"clear": CLEAR, "hits_only": CLEAR | HITS_ONLY, "tprev": 0}
T_PREV = np.float32(2.4)


def scene_pair(name):
    """-> (oracle scene, GPU scene), no plane"""
    if name == "cube":
        rs, gs = S.ref_scene("cube.obj"), S.gpu_scene("cube.obj")
    else:
        rs, gs = soup_scenes(RAND)
    rs.set_plane(False, (0.0, 1.0, 0.0), -1.0)
    gs.set_plane(None)
    return rs, gs


def matrices(view, W, H):
    pos, tgt = view
    return cpuref.camera_matrices(pos, tgt, (0.0, 1.0, 0.0), 45.0, W / H, 0.01, 100.0)


def gpu_params(view, W, H, sm=0):
    vi, pi = matrices(view, W, H)
    return rtamd.render_params(view[0], vi, pi, (2, 2, 2), sm, True, True)


def start_frame(W, H, mode):
    """what the buffers hold before the frame is rendered"""
    if mode == "tprev":
        c = (np.arange(W * H, dtype=np.uint32).reshape(H, W) * np.uint32(2654435761)) | np.uint32(1)
        return c, np.full((H, W), T_PREV, np.float32)
    if mode == "hits_only":
        return np.zeros((H, W), np.uint32), np.full((H, W), np.inf, np.float32)
    # RT_FLAG_CLEAR overwrites whatever is there
    return np.full((H, W), 0xABABABAB, np.uint32), np.full((H, W), -5.0, np.float32)


@functools.lru_cache(maxsize=None)
def oracle(name, W, H, view, mode):
    rs, _ = scene_pair(name)
    vi, pi = matrices(view, W, H)
    P = cpuref.make_params(view[0], vi, pi, (2, 2, 2), 0, True, True)
    if mode == "tprev":
        c, t = start_frame(W, H, mode)
        c, t = c.copy(), t.copy()
        rs.render(P, W, H, color=c, t=t)
    else:
        c, t, _, _ = rs.render(P, W, H)
    c.setflags(write=False)
    t.setflags(write=False)
    return c, t


class cull:
    """the switch for the frames filled inside the block"""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        rtamd._lib.check(rtamd.lib().rtx_set_tile_cull(int(self.on)))

    def __exit__(self, *a):
        rtamd._lib.check(rtamd.lib().rtx_set_tile_cull(-1))


def same(a, b, what):
    (ac, at), (bc, bt) = a, b
    assert np.array_equal(ac, bc), f"{what}: {int((ac != bc).sum())} colour words differ"
    assert np.array_equal(at.view(np.uint32), bt.view(np.uint32)), f"{what}: t bits differ"


def device_frames(gs, name, W, H, views, mode, tile=None):
    """the views through rt_render_device (one) or rt_render_device_frames, on
    device buffers that start as start_frame(); -> [(colour, t)] on the host"""
    import torch
    c0, t0 = start_frame(W, H, mode)
    cs = [torch.from_numpy(c0.view(np.int32).copy()).cuda() for _ in views]
    ts = [torch.from_numpy(t0.copy()).cuda() for _ in views]
    P = [gpu_params(v, W, H) for v in views]
    st = torch.cuda.current_stream().cuda_stream
    if len(views) == 1:
        gs.render_device(P[0], cs[0].data_ptr(), ts[0].data_ptr(), W, H, clear=False, tile=tile, stream=st,
                         flags=MODES[mode])
    else:
        gs.render_device_frames(P, [c.data_ptr() for c in cs], [t.data_ptr() for t in ts], W, H, MODES[mode],
                                tile=tile, stream=st)
    torch.cuda.synchronize()
    return [(c.cpu().numpy().view(np.uint32), t.cpu().numpy()) for c, t in zip(cs, ts)]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("name", ["cube", "rand"])
def test_one_frame_kernel(gpu, name, W, H, mode):
    _, gs = scene_pair(name)
    for view in VIEWS:
        got = {}
        for on in (1, 0):
            with cull(on):
                got[on] = device_frames(gs, name, W, H, [view], mode)[0]
        same(got[1], got[0], f"{name} {W}x{H} {mode} {view}: cull on / off")
        same(oracle(name, W, H, view, mode), got[1], f"{name} {W}x{H} {mode} {view}: oracle / cull on")


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("name", ["cube", "rand"])
def test_multi_frame_launch(gpu, name, W, H, mode):
    _, gs = scene_pair(name)
    got = {}
    for on in (1, 0):
        with cull(on):
            got[on] = device_frames(gs, name, W, H, VIEWS, mode)
    for view, a, b in zip(VIEWS, got[1], got[0]):
        same(a, b, f"{name} {W}x{H} {mode} {view}: cull on / off")
        same(oracle(name, W, H, view, mode), a, f"{name} {W}x{H} {mode} {view}: oracle / cull on")
    if mode == "tprev":  # the frame looking away kept every word of the pattern
        same(start_frame(W, H, mode), got[1][1], f"{name} {W}x{H}: pattern of the frame looking away")


@pytest.mark.parametrize("band_rows", [8, 12])
@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("name", ["cube", "rand"])
def test_row_band_tiles(gpu, name, W, H, band_rows):
    """Two ranks' packed row bands (12-row bands: wave tiles straddle two bands,
    whose image rows are 12 rows apart), one frame and three per launch."""
    _, gs = scene_pair(name)
    for mode in ("clear", "tprev"):
        for rank in (0, 1):
            tile = rtamd.Tile(band_rows, rank, 2, 0)
            rows = tiles.rank_rows(H, band_rows, rank, 2)
            for views in ([VIEWS[0]], list(VIEWS)):
                got = {}
                for on in (1, 0):
                    with cull(on):
                        got[on] = device_frames(gs, name, W, H, views, mode, tile)
                for view, a, b in zip(views, got[1], got[0]):
                    what = f"{name} {W}x{H} {mode} bands of {band_rows} rank {rank} x{len(views)} {view}"
                    same(a, b, what + ": cull on / off")
                    rc, rt_ = oracle(name, W, H, view, mode)
                    n = len(rows)
                    if mode == "tprev":
                        # packed rows start from the pattern's first rows, not the image rows'
                        c0, _ = start_frame(W, H, mode)
                        hit = rt_[rows] != T_PREV
                        assert np.array_equal(a[1][:n] != T_PREV, hit), what + ": coverage"
                        assert np.array_equal(a[0][:n][hit], rc[rows][hit]), what + ": colour of the hits"
                        assert np.array_equal(a[0][:n][~hit], c0[:n][~hit]), what + ": pattern kept"
                        assert np.array_equal(a[1][:n].view(np.uint32), rt_[rows].view(np.uint32)), what + ": t"
                    else:
                        same((rc[rows], rt_[rows]), (a[0][:n], a[1][:n]), what + ": oracle / cull on")
                    # nothing past the rank's rows is touched
                    c0, t0 = start_frame(W, H, mode)
                    same((c0[n:], t0[n:]), (a[0][n:], a[1][n:]), what + ": rows past the band")


def test_default_mode_is_not_culled(gpu):
    """Plane + Lambert shading: the shading kernels render every pixel; the
    switch changes nothing and the frame is the oracle's."""
    import torch
    W, H = 96, 72
    rs, gs = soup_scenes(RAND)
    rs.set_plane(True, (0.0, 1.0, 0.0), -1.0)
    gs.set_plane(rtamd.Plane((0.0, 1.0, 0.0), -1.0))
    try:
        view = VIEWS[0]
        vi, pi = matrices(view, W, H)
        rc, rt_, _, _ = rs.render(cpuref.make_params(view[0], vi, pi, (2, 2, 2), 1, True, True), W, H)
        assert np.isfinite(rt_).mean() > 0.4  # the plane: far more than the mesh's rectangle
        got = {}
        for on in (1, 0):
            with cull(on):
                c = torch.zeros((H, W), dtype=torch.int32, device="cuda")
                t = torch.zeros((H, W), dtype=torch.float32, device="cuda")
                gs.render_device(gpu_params(view, W, H, sm=1), c.data_ptr(), t.data_ptr(), W, H, clear=True,
                                 stream=torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                got[on] = (c.cpu().numpy().view(np.uint32), t.cpu().numpy())
        same(got[1], got[0], "default mode: cull on / off")
        same((rc, rt_), got[1], "default mode: oracle / cull on")
    finally:
        rs.set_plane(False, (0.0, 1.0, 0.0), -1.0)
        gs.set_plane(None)


@pytest.mark.parametrize("pinned", [True, False], ids=["pinned", "pageable"])
def test_rt_render_cleared_host_frame(gpu, pinned):
    """rt_render on host buffers that hold a cleared frame (the zero-copy
    frames and the pair flush of the one-frame kernel)."""
    L = rtamd.lib()
    for name, (W, H) in (("rand", (96, 72)), ("cube", (98, 50)), ("rand", (320, 180))):
        _, gs = scene_pair(name)
        for view in VIEWS[:2]:
            got = {}
            for on in (1, 0):
                c = np.zeros((H, W), np.uint32)
                t = np.full((H, W), np.inf, np.float32)
                if pinned:
                    rtamd._lib.check(L.rt_host_pin(C.c_void_p(c.ctypes.data), c.nbytes))
                    rtamd._lib.check(L.rt_host_pin(C.c_void_p(t.ctypes.data), t.nbytes))
                try:
                    with cull(on):
                        gs.render(gpu_params(view, W, H), c, t, cleared=True)
                finally:
                    if pinned:
                        rtamd._lib.check(L.rt_host_unpin(C.c_void_p(c.ctypes.data)))
                        rtamd._lib.check(L.rt_host_unpin(C.c_void_p(t.ctypes.data)))
                got[on] = (c, t)
            same(got[1], got[0], f"rt_render {name} {W}x{H} {view}: cull on / off")
            same(oracle(name, W, H, view, "clear"), got[1], f"rt_render {name} {W}x{H} {view}: oracle / cull on")


def test_count_work_is_unchanged(gpu):
    for name in ("cube", "rand"):
        _, gs = scene_pair(name)
        P = [gpu_params(v, 96, 72) for v in VIEWS]
        got = {}
        for on in (1, 0):
            with cull(on):
                got[on] = gs.count_work(P, 96, 72)
        assert got[1] == got[0], name
        assert sum(got[1].values()) > 3 * 96 * 72  # (at least the rays are counted)
