"""The item rectangle of a persistent launch (rtq::grid in csrc/rt_queue.h,
reached through the host-only rtx_queue_grid, without a GPU) against a
brute-force union in Python: every tile of every frame's cull rectangle that
has a pixel in the frame lies in the grid, the grid is the smallest such set of
whole items inside the frame's item grid, and a 4-nested loop over the grid's
items and their tiles reproduces exactly those tiles.

A frame's rectangle is two words of 8-pixel tiles, first | (last + 1) << 16,
columns and rows (FrameArgs::cull_x and P.reserved).
"""
import itertools

import numpy as np
import pytest

import rtamd

WHOLE = 0xFFFF0000
SHAPES = ((1, 1), (2, 1), (2, 2))
SIZES = ((250, 131), (1921, 131), (1920, 1080), (200, 120))


def word(first, end):
    return (first & 0xFFFF) | ((end & 0xFFFF) << 16)


def grid(rects, W, rows, gx, gy):
    """rects: [(x first, x end, y first, y end) in tiles, or None for a frame
    without a rectangle] -> (ox, oy, columns, rows) in items"""
    cx = np.array([WHOLE if r is None else word(r[0], r[1]) for r in rects], np.uint32)
    cy = np.array([WHOLE if r is None else word(r[2], r[3]) for r in rects], np.uint32)
    out = np.full(4, 12345, np.uint32)
    cxp = cx.ctypes.data if len(rects) else out.ctypes.data  # (no frames: the pointers are not read)
    cyp = cy.ctypes.data if len(rects) else out.ctypes.data
    rtamd._lib.check(rtamd.lib().rtx_queue_grid(cxp, cyp, len(rects), W, rows, gx, gy, out.ctypes.data))
    return tuple(int(v) for v in out)


def brute(rects, W, rows):
    """the union, tile by tile: a boolean map of the frame's tiles"""
    tw, th = (W + 7) // 8, (rows + 7) // 8
    m = np.zeros((th, tw), bool)
    for r in rects:
        if r is None:
            m[:] = True
            continue
        for ty in range(r[2], min(r[3], th)):
            for tx in range(r[0], min(r[1], tw)):
                m[ty, tx] = True
    return m


def check(rects, W, rows, gx, gy):
    ox, oy, nx, ny = grid(rects, W, rows, gx, gy)
    what = f"{rects} {W}x{rows} items {gx}x{gy} -> {(ox, oy, nx, ny)}"
    m = brute(rects, W, rows)
    th, tw = m.shape
    fx, fy = (W + 8 * gx - 1) // (8 * gx), (rows + 8 * gy - 1) // (8 * gy)
    if not m.any():
        assert (nx, ny) == (0, 0), what
        return
    # whole items inside the frame's item grid
    assert nx > 0 and ny > 0 and ox + nx <= fx and oy + ny <= fy, what
    # the tiles a 4-nested loop over items and their tiles enumerates (the
    # kernel's loop; tiles past the frame have no pixel)
    got = np.zeros_like(m)
    for iy, ix, j, i in itertools.product(range(ny), range(nx), range(gy), range(gx)):
        tx, ty = (ox + ix) * gx + i, (oy + iy) * gy + j
        if tx < tw and ty < th:
            assert not got[ty, tx], what
            got[ty, tx] = True
    # every tile of every rectangle is enumerated
    assert not (m & ~got).any(), what
    # and the grid is the union's bounding box rounded outwards to whole items
    ys, xs = np.flatnonzero(m.any(1)), np.flatnonzero(m.any(0))
    want = np.zeros_like(m)
    want[ys[0] // gy * gy:(ys[-1] // gy + 1) * gy, xs[0] // gx * gx:(xs[-1] // gx + 1) * gx] = True
    assert np.array_equal(got, want), what
    # the same in pixels: the fill's rectangle, clipped to the frame
    px = np.zeros((rows, W), bool)
    px[min(rows, oy * gy * 8):min(rows, (oy + ny) * gy * 8), min(W, ox * gx * 8):min(W, (ox + nx) * gx * 8)] = True
    assert np.array_equal(px, np.kron(got, np.ones((8, 8), bool))[:rows, :W]), what


@pytest.fixture(scope="module", autouse=True)
def _lib(rt):
    return rt.lib()


@pytest.mark.parametrize("gx,gy", SHAPES)
@pytest.mark.parametrize("W,H", SIZES)
def test_one_frame(W, H, gx, gy):
    tw, th = (W + 7) // 8, (H + 7) // 8
    for r in ((3, 8, 1, 4), (5, 6, 5, 6), (1, tw - 1, 1, th - 1), (tw - 3, tw, th - 2, th),
              (0, 3, 0, 3), (0, tw, 0, th), (7, tw, 3, th), (0, 1, th - 1, th)):
        check([r], W, H, gx, gy)


@pytest.mark.parametrize("gx,gy", SHAPES)
@pytest.mark.parametrize("W,H", SIZES)
def test_sixteen_frames(W, H, gx, gy):
    tw, th = (W + 7) // 8, (H + 7) // 8
    rng = np.random.default_rng(W * 131 + H + gx * 7 + gy)
    for _ in range(6):
        rects = []
        for _ in range(16):
            x0, y0 = int(rng.integers(0, tw)), int(rng.integers(0, th))
            rects.append((x0, int(rng.integers(x0 + 1, tw + 1)), y0, int(rng.integers(y0 + 1, th + 1))))
        check(rects, W, H, gx, gy)
    # a drifting rectangle, as an orbit's: odd first and last tile columns
    check([(3 + k // 4, 11 + k // 2, 1 + k // 8, 7 + k // 3) for k in range(16)], W, H, gx, gy)


@pytest.mark.parametrize("gx,gy", SHAPES)
@pytest.mark.parametrize("W,H", SIZES)
def test_disjoint_rectangles(W, H, gx, gy):
    tw, th = (W + 7) // 8, (H + 7) // 8
    check([(1, 4, 1, 3), (tw - 4, tw - 1, th - 4, th - 1)], W, H, gx, gy)  # opposite corners
    check([(tw - 2, tw, 0, 2), (0, 2, th - 2, th)], W, H, gx, gy)
    check([(3, 4, 5, 6), (9, 10, 5, 6), (15, 16, 7, 8)], W, H, gx, gy)


@pytest.mark.parametrize("gx,gy", SHAPES)
@pytest.mark.parametrize("W,H", SIZES)
def test_empty_frames(W, H, gx, gy):
    empty = (0, 0, 0, 0)
    check([(3, 8, 1, 4), empty, (5, 9, 3, 6)], W, H, gx, gy)
    check([empty, (5, 9, 3, 6)], W, H, gx, gy)
    # an empty frame's zeros must not pull the origin to the corner
    assert grid([empty, (5, 9, 3, 6)], W, H, gx, gy) == grid([(5, 9, 3, 6)], W, H, gx, gy)
    for n in (1, 2, 16):
        assert grid([empty] * n, W, H, gx, gy)[2:] == (0, 0)
        check([empty] * n, W, H, gx, gy)
    assert grid([], W, H, gx, gy)[2:] == (0, 0)
    # empty in one direction only, and first past last
    check([(3, 3, 1, 4), (4, 2, 1, 4), (5, 9, 6, 6)], W, H, gx, gy)
    # a rectangle wholly past the frame has no pixel
    tw, th = (W + 7) // 8, (H + 7) // 8
    check([(tw, tw + 3, 0, 2), (0, 2, th, th + 1)], W, H, gx, gy)
    check([(tw - 1, tw + 3, th - 1, th + 5)], W, H, gx, gy)  # clipped to the frame


@pytest.mark.parametrize("gx,gy", SHAPES)
@pytest.mark.parametrize("W,H", SIZES)
def test_whole_frame(W, H, gx, gy):
    fx, fy = (W + 8 * gx - 1) // (8 * gx), (H + 8 * gy - 1) // (8 * gy)
    for rects in ([None], [(3, 8, 1, 4), None, (0, 0, 0, 0)], [None] * 16, [(0, 0, 0, 0), None]):
        assert grid(rects, W, H, gx, gy) == (0, 0, fx, fy), rects
        check(rects, W, H, gx, gy)


@pytest.mark.parametrize("gx,gy", SHAPES)
@pytest.mark.parametrize("W,H", SIZES)
def test_touching_each_edge(W, H, gx, gy):
    tw, th = (W + 7) // 8, (H + 7) // 8
    for r in ((0, 5, 3, 6), (tw - 5, tw, 3, 6), (3, 8, 0, 3), (3, 8, th - 3, th)):
        check([r], W, H, gx, gy)
        check([r, (7, 9, 7, 9)], W, H, gx, gy)


def test_partial_last_item_column():
    """W = 250: 32 tile columns, the last 2 pixels wide; W = 1921: 241 tile
    columns, so the last 2x1 item holds one tile of one pixel column"""
    assert grid([(29, 32, 2, 5)], 250, 131, 2, 1) == (14, 2, 2, 3)
    assert grid([(239, 241, 15, 17)], 1921, 131, 2, 1) == (119, 15, 2, 2)
    assert grid([(239, 241, 15, 17)], 1921, 131, 2, 2) == (119, 7, 2, 2)  # H = 131: 17 tile rows, 9 item rows
    assert grid([(240, 241, 16, 17)], 1921, 131, 2, 2) == (120, 8, 1, 1)
    assert grid([(240, 241, 16, 17)], 1921, 131, 1, 1) == (240, 16, 1, 1)


def test_bad_arguments_are_rejected():
    out = np.zeros(4, np.uint32)
    w = np.array([word(1, 2)], np.uint32)
    L = rtamd.lib()
    assert L.rtx_queue_grid(None, w.ctypes.data, 1, 64, 64, 1, 1, out.ctypes.data) != 0
    assert L.rtx_queue_grid(w.ctypes.data, w.ctypes.data, 1, 64, 64, 1, 1, None) != 0
    assert L.rtx_queue_grid(w.ctypes.data, w.ctypes.data, 1, 0, 64, 1, 1, out.ctypes.data) != 0
    assert L.rtx_queue_grid(w.ctypes.data, w.ctypes.data, 1, 64, 64, 3, 1, out.ctypes.data) != 0
    assert L.rtx_queue_grid(w.ctypes.data, w.ctypes.data, 1, 64, 64, 1, 0, out.ctypes.data) != 0
    assert L.rtx_queue_grid(w.ctypes.data, w.ctypes.data, -1, 64, 64, 1, 1, out.ctypes.data) != 0
