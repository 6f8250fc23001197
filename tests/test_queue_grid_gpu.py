"""Persistent launches whose items cover the launch's item rectangle only
(make_queue / rtq::grid, clear_outside_kernel in csrc/rt_device.hip): with the
switch on and off the frames hold the same bits, and both equal the oracle's.

Cube and spot at 200x120 and 250x131 (a last tile column 2 pixels wide, a last
tile row 3 pixels high), 1, 2 and 5 frames per call of rt_render_device_frames,
with RT_FLAG_CLEAR, CLEAR | HITS_ONLY on a cleared frame and no flag on a frame
that holds a pattern and a finite tPrev. The cameras: an orbit view, two views
whose rectangles lie in opposite corners (the union is larger than both), a view
looking away (empty rectangle: no persistent launch), a camera inside the box
(no rectangle: the whole frame), rectangles clipped by the left and top and by
the right and bottom edges, and views that keep the model in the lower right
or the upper left part of the frame.

What a launch's item grid is meant to be is stated per group (GROUPS) and
checked on the host before the launch (expect_grid): a proper part of the
frame, with a first item column and row above zero where the group says so,
the whole frame, or empty. The 5-frame launches are of the first kind: they
run the fill and, LOWER_RIGHT and MIDDLE, a non-zero origin.

Every frame lies between guard rows of a sentinel: none of them changes, and
with RT_FLAG_CLEAR, where the frame itself starts as the sentinel, none
survives inside the frame.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import cpuref
import rtamd
import scenes as S

pytestmark = pytest.mark.gpu

SIZES = [(200, 120), (250, 131)]
NAMES = ["cube", "spot"]
VIEWS = {  # position, target
    "orbit": ((1.2, 0.8, 2.6), (0.0, 0.0, 0.0)),
    "corner_a": ((0.0, 0.0, 6.0), (2.6, 1.4, 0.0)),
    "corner_b": ((0.0, 0.0, 6.0), (-2.6, -1.4, 0.0)),
    "away": ((0.3, 0.2, 3.0), (0.3, 0.2, 6.0)),
    "inside": ((0.05, 0.02, 0.1), (0.0, 0.0, -1.0)),
    "left_top": ((0.0, 0.0, 6.0), (3.7, -2.1, 0.0)),
    "right_bottom": ((0.0, 0.0, 6.0), (-3.7, 2.1, 0.0)),
    # the model in the lower right part of the frame, clear of the left and top edges
    "lr_near": ((0.5, 0.3, 5.0), (-1.3, 0.7, 0.0)),
    "lr_mid": ((0.0, 0.0, 6.0), (-2.2, 0.9, 0.0)),
    "lr_low": ((-0.4, 0.2, 6.5), (-1.2, 1.5, 0.0)),
    # and in the upper left part, clear of the right and bottom edges
    "ul_near": ((-0.5, -0.3, 5.0), (1.3, -0.7, 0.0)),
    "ul_mid": ((0.0, 0.0, 6.0), (2.2, -0.9, 0.0)),
    "ul_high": ((0.4, -0.2, 6.5), (1.2, -1.5, 0.0)),
}
# 5-frame launches whose union is a proper part of the frame: up to the right
# and bottom edges from a non-zero origin; from the left and top edges; clear
# of the left and top edges in the middle
LOWER_RIGHT = ["lr_near", "away", "lr_mid", "right_bottom", "lr_low"]
UPPER_LEFT = ["ul_mid", "left_top", "away", "ul_near", "ul_high"]
MIDDLE = ["orbit", "lr_near", "ul_near", "lr_mid", "ul_mid"]
# what a launch's item grid is meant to be: "part" (neither whole nor empty),
# "origin" (part, and first item column and row both above zero), "whole", "empty"
GROUPS = [(["orbit"], "part"), (["left_top"], "part"), (["away"], "empty"), (["inside"], "whole"),
          (["corner_a", "corner_b"], "part"), (["away", "away"], "empty"), (["corner_a", "inside"], "whole"),
          (["right_bottom", "away"], "origin"), (LOWER_RIGHT, "origin"), (UPPER_LEFT, "part"), (MIDDLE, "origin")]
KIND = {tuple(v): k for v, k in GROUPS}
KIND[("orbit", "corner_a")] = KIND[("corner_b", "left_top")] = "part"
GX, GY = 2, 1  # a mesh's queue item: 2 x 1 wave tiles (MeshS::kQueueGroup)
CLEAR, HITS_ONLY = rtamd.RT_FLAG_CLEAR, rtamd._lib.RT_FLAG_HITS_ONLY
MODES = {"clear": CLEAR, "hits_only": CLEAR | HITS_ONLY, "tprev": 0}
T_PREV = np.float32(6.0)  # in front of part of what the cameras at distance 6 see
GUARD = 9  # sentinel rows before and after the frame
SENT_C, SENT_T = 0x5A5A5A5A, np.float32(-3.0)  # no pixel a kernel stores holds either


def ref_scene(name):
    rs = S.ref_scene(name + ".obj")
    rs.set_plane(False, (0.0, 1.0, 0.0), -1.0)
    return rs


def gpu_scene(name):
    gs = S.gpu_scene(name + ".obj")
    gs.set_plane(None)
    return gs


def matrices(view, W, H):
    pos, tgt = VIEWS[view]
    return cpuref.camera_matrices(pos, tgt, (0.0, 1.0, 0.0), 45.0, W / H, 0.01, 100.0)


def gpu_params(view, W, H):
    vi, pi = matrices(view, W, H)
    return rtamd.render_params(VIEWS[view][0], vi, pi, (2, 2, 2), 0, True, True)


def start_frame(W, H, mode):
    """what the frame holds before it is rendered"""
    if mode == "tprev":
        c = (np.arange(W * H, dtype=np.uint32).reshape(H, W) * np.uint32(2654435761)) | np.uint32(1)
        return c, np.full((H, W), T_PREV, np.float32)
    if mode == "hits_only":
        return np.zeros((H, W), np.uint32), np.full((H, W), np.inf, np.float32)
    return np.full((H, W), SENT_C, np.uint32), np.full((H, W), SENT_T, np.float32)


@functools.lru_cache(maxsize=None)
def oracle(name, W, H, view, mode):
    rs = ref_scene(name)
    vi, pi = matrices(view, W, H)
    P = cpuref.make_params(VIEWS[view][0], vi, pi, (2, 2, 2), 0, True, True)
    if mode == "tprev":
        c, t = (a.copy() for a in start_frame(W, H, mode))
        rs.render(P, W, H, color=c, t=t)
    else:  # (a cleared frame's hits are the fused clear's)
        c, t, _, _ = rs.render(P, W, H)
    c.setflags(write=False)
    t.setflags(write=False)
    return c, t


class qgrid:
    """the switch for the launches inside the block"""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        rtamd._lib.check(rtamd.lib().rtx_set_queue_grid(int(self.on)))

    def __exit__(self, *a):
        rtamd._lib.check(rtamd.lib().rtx_set_queue_grid(-1))


class Frames:
    """n frames on the device, each between GUARD sentinel rows"""

    def __init__(self, n, W, H, mode):
        import torch
        self.W, self.H = W, H
        c0, t0 = start_frame(W, H, mode)
        c = np.full((H + 2 * GUARD, W), SENT_C, np.uint32)
        t = np.full((H + 2 * GUARD, W), SENT_T, np.float32)
        c[GUARD:GUARD + H], t[GUARD:GUARD + H] = c0, t0
        self.c = [torch.from_numpy(c.view(np.int32).copy()).cuda() for _ in range(n)]
        self.t = [torch.from_numpy(t.copy()).cuda() for _ in range(n)]

    def ptrs(self):
        off = GUARD * self.W * 4
        return [c.data_ptr() + off for c in self.c], [t.data_ptr() + off for t in self.t]

    def download(self, what):
        """-> [(colour, t)] of the frames; the guard rows hold the sentinel"""
        out = []
        for i, (c, t) in enumerate(zip(self.c, self.t)):
            c, t = c.cpu().numpy().view(np.uint32), t.cpu().numpy()
            for rows in (slice(0, GUARD), slice(GUARD + self.H, None)):
                assert (c[rows] == SENT_C).all() and (t[rows] == SENT_T).all(), f"{what}, frame {i}: guard rows written"
            out.append((c[GUARD:GUARD + self.H], t[GUARD:GUARD + self.H]))
        return out


@functools.lru_cache(maxsize=None)
def launch_grid(name, W, H, views):
    """The item grid of a launch of `views`, on the host: rtx_cull_rect on the
    mesh's bounds for each view, then rtx_queue_grid -> (ox, oy, columns, rows)
    in items and the frame's (columns, rows). The library's own rectangles also
    use the root's child boxes and lie inside these, so its grid lies inside
    this one."""
    L = rtamd.lib()
    v = S.inputs(name + ".obj")[1][0]
    p = v[:, :3] / v[:, 3:4]
    box = np.concatenate([p.min(0), p.max(0)]).astype(np.float32)
    cx, cy = np.zeros(len(views), np.uint32), np.zeros(len(views), np.uint32)
    for i, view in enumerate(views):
        P = gpu_params(view, W, H)
        r = np.zeros(4, np.int32)
        if L.rtx_cull_rect(C.byref(P), W, H, box.ctypes.data, r.ctypes.data):
            cx[i], cy[i] = int(r[0]) | (int(r[1]) << 16), int(r[2]) | (int(r[3]) << 16)
        else:  # no rectangle: the whole frame
            cx[i] = cy[i] = 0xFFFF0000
    out = np.zeros(4, np.uint32)
    rtamd._lib.check(L.rtx_queue_grid(cx.ctypes.data, cy.ctypes.data, len(views), W, H, GX, GY, out.ctypes.data))
    return tuple(int(x) for x in out), ((W + 8 * GX - 1) // (8 * GX), (H + 8 * GY - 1) // (8 * GY))


def expect_grid(name, W, H, views):
    """the launch's item grid is what its group is meant to exercise (KIND)"""
    kind = KIND[tuple(views)]
    (ox, oy, nx, ny), (fx, fy) = launch_grid(name, W, H, tuple(views))
    what = f"{name} {W}x{H} {views}: grid {(ox, oy, nx, ny)} of {(fx, fy)}, meant to be {kind}"
    if kind == "empty":
        assert (nx, ny) == (0, 0), what
    elif kind == "whole":
        assert (ox, oy, nx, ny) == (0, 0, fx, fy), what
    else:
        assert nx > 0 and ny > 0 and (nx, ny) != (fx, fy), what
        # (the library's grid lies inside this one: not empty as long as a view has a hit)
        assert any(np.isfinite(oracle(name, W, H, v, "clear")[1]).any() for v in views), what
        if kind == "origin":
            assert ox > 0 and oy > 0, what


def launch(gs, name, fr, views, mode, stream):
    """one call of rt_render_device_frames on `stream` (a torch stream); one
    view: the entry hands it to the one-frame kernel"""
    expect_grid(name, fr.W, fr.H, views)
    cp, tp = fr.ptrs()
    P = [gpu_params(v, fr.W, fr.H) for v in views]
    gs.render_device_frames(P, cp[:len(views)], tp[:len(views)], fr.W, fr.H, MODES[mode], stream=stream.cuda_stream)


def same(a, b, what):
    (ac, at), (bc, bt) = a, b
    assert np.array_equal(ac, bc), f"{what}: {int((ac != bc).sum())} colour words differ"
    assert np.array_equal(at.view(np.uint32), bt.view(np.uint32)), f"{what}: t bits differ"


def no_sentinel(frame, what):
    c, t = frame
    assert not (c == SENT_C).any() and not (t == SENT_T).any(), f"{what}: a sentinel survived inside the frame"


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("name", NAMES)
def test_switch_on_off_and_oracle(gpu, name, W, H, mode):
    import torch
    gs = gpu_scene(name)
    s0 = torch.cuda.current_stream()
    for views, _ in GROUPS:
        got = {}
        for on in (1, 0):
            what = f"{name} {W}x{H} {mode} {views}, grid {on}"
            with qgrid(on):
                fr = Frames(len(views), W, H, mode)
                launch(gs, name, fr, views, mode, s0)
                torch.cuda.synchronize()
            got[on] = fr.download(what)
        for view, a, b in zip(views, got[1], got[0]):
            what = f"{name} {W}x{H} {mode} {view} of {views}"
            same(a, b, what + ": grid on / off")
            same(oracle(name, W, H, view, mode), a, what + ": oracle / grid on")
            if mode == "clear":
                no_sentinel(a, what)
            if mode == "tprev" and view == "away":
                same(start_frame(W, H, mode), a, what + ": the pattern of the frame looking away")


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("name", NAMES)
def test_back_to_back_on_one_stream(gpu, name, W, H):
    """Launches in a row into the same buffers with no wait between them; the
    sentinel is there before the first only. An all-empty launch leaves the
    stream's heads as the next launch needs them."""
    import torch
    gs = gpu_scene(name)
    s0 = torch.cuda.current_stream()
    away2 = ["away", "away"]
    for seq in ([LOWER_RIGHT, UPPER_LEFT], [UPPER_LEFT, LOWER_RIGHT], [MIDDLE, LOWER_RIGHT],
                [away2, ["orbit", "corner_a"]], [["orbit", "corner_a"], away2],
                [away2, away2, ["corner_b", "left_top"]], [["corner_a", "inside"], ["corner_a", "corner_b"]]):
        got = {}
        for on in (1, 0):
            what = f"{name} {W}x{H} {seq}, grid {on}"
            with qgrid(on):
                fr = Frames(len(seq[0]), W, H, "clear")
                for views in seq:
                    launch(gs, name, fr, views, "clear", s0)
                torch.cuda.synchronize()
            got[on] = fr.download(what)
        for view, a, b in zip(seq[-1], got[1], got[0]):
            what = f"{name} {W}x{H} {view}, last of {seq}"
            same(a, b, what + ": grid on / off")
            same(oracle(name, W, H, view, "clear"), a, what + ": oracle / grid on")
            no_sentinel(a, what)


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("name", NAMES)
def test_four_launches_over_two_streams(gpu, name, W, H):
    """Two streams, a set of buffers each, launches alternating between them.
    Every launch has a fill and a persistent launch over part of the frame
    (expect_grid), two of them from a non-zero origin; a stream's second launch
    clears what its first one drew elsewhere."""
    import torch
    gs = gpu_scene(name)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    order = [(0, LOWER_RIGHT), (1, UPPER_LEFT), (0, MIDDLE), (1, LOWER_RIGHT)]  # (stream, views)
    got = {}
    for on in (1, 0):
        what = f"{name} {W}x{H} two streams, grid {on}"
        with qgrid(on):
            frs = [Frames(5, W, H, "clear"), Frames(5, W, H, "clear")]
            for s in (s1, s2):
                s.wait_stream(torch.cuda.current_stream())  # (the uploads)
            for k, views in order:
                launch(gs, name, frs[k], views, "clear", (s1, s2)[k])
            torch.cuda.synchronize()
        got[on] = [fr.download(what) for fr in frs]
    for k, last in ((0, MIDDLE), (1, LOWER_RIGHT)):
        for view, a, b in zip(last, got[1][k], got[0][k]):
            what = f"{name} {W}x{H} {view}, stream {k}"
            same(a, b, what + ": grid on / off")
            same(oracle(name, W, H, view, "clear"), a, what + ": oracle / grid on")
            no_sentinel(a, what)
