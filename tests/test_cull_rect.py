"""The tile cull's screen rectangle (cull_rect in csrc/rt_device.hip, reached
through the host-only rtx_cull_rect) against the oracle's frames, without a
GPU: no pixel outside the rectangle of a mesh's bounding box may hold a hit.

The box is the mesh's vertex bounds after the reference's /w, i.e. the union of
the root's child boxes (MeshDev::rbox). Frames are 96x72 and 97x73: the odd
size puts a pixel centre on the optical axis, whose ray has exact zero
direction components for an axis-aligned camera (1/d = inf, the exact slab
path).
"""
import ctypes as C
import functools

import numpy as np
import pytest

import cpuref
import rtamd
import scenes as S
from test_gpu_edge import tri_mesh
from test_mesh_resume import CAMS

SIZES = ((96, 72), (97, 73))
RAND = (12, 3000, "rand")


@functools.lru_cache(maxsize=None)
def mesh(name):
    """-> (oracle scene, box as xMin yMin zMin xMax yMax zMax float32)"""
    if name == "cube":
        v, i = S.inputs("cube.obj")[1]
    else:
        v, i = tri_mesh(*RAND)
    p = (v[:, :3] / v[:, 3:4]).astype(np.float32)
    box = np.concatenate([p.min(0), p.max(0)]).astype(np.float32)
    box.setflags(write=False)
    return cpuref.RefScene.mesh(v, i), box


def look(pos, target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), W=96, H=72):
    return cpuref.camera_matrices(pos, target, up, 45.0, W / H, 0.01, 100.0)


def rect(pos, vi, pi, W, H, box):
    """-> None for "whole frame", else (x0, x1, y0, y1) in 8-pixel tiles, ends exclusive"""
    P = rtamd.render_params(pos, vi, pi, (2, 2, 2), 0, True, True)
    out = np.full(4, -7, np.int32)
    ok = rtamd.lib().rtx_cull_rect(C.byref(P), W, H, box.ctypes.data, out.ctypes.data)
    if not ok:
        assert (out == -7).all()
        return None
    x0, x1, y0, y1 = (int(v) for v in out)
    assert 0 <= x0 <= x1 <= (W + 7) // 8 and 0 <= y0 <= y1 <= (H + 7) // 8, out
    return x0, x1, y0, y1


def oracle_hits(rs, pos, vi, pi, W, H):
    c, t, _, _ = rs.render(cpuref.make_params(pos, vi, pi, (2, 2, 2), 0, True, True), W, H)
    return np.isfinite(t) | (c != 0)


def outside(r, W, H):
    """pixels (image rows x columns) the rectangle leaves out"""
    m = np.ones((H, W), bool)
    if r is not None:
        x0, x1, y0, y1 = r
        m[y0 * 8:y1 * 8, x0 * 8:x1 * 8] = False
    else:
        m[:] = False
    return m


def check(name, pos, vi, pi, W, H, what):
    rs, box = mesh(name)
    r = rect(pos, vi, pi, W, H, box)
    hits = oracle_hits(rs, pos, vi, pi, W, H)
    bad = hits & outside(r, W, H)
    assert not bad.any(), f"{what}: {int(bad.sum())} hits outside the rectangle {r}"
    return r, hits


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("name", ["cube", "rand"])
def test_resume_cameras(rt, ref, name, W, H):
    for pos in CAMS:
        vi, pi = look(pos, W=W, H=H)
        r, hits = check(name, pos, vi, pi, W, H, f"{name} {W}x{H} {pos}")
        assert hits.any()
        assert r is not None, f"{name} {pos}: a camera well outside the box gets a rectangle"
        if name == "cube" and (W, H) == (96, 72):
            # the test must not pass by culling nothing: the cube leaves a
            # full 8x8 tile column or row free on some side (checked below on
            # the oracle's own frame too)
            x0, x1, y0, y1 = r
            assert x0 > 0 or x1 < W // 8 or y0 > 0 or y1 < H // 8, r
            cols, rows = np.flatnonzero(hits.any(0)), np.flatnonzero(hits.any(1))
            assert cols[0] >= 8 or cols[-1] < W - 8 or rows[0] >= 8 or rows[-1] < H - 8


def test_random_cameras(rt, ref):
    rng = np.random.default_rng(2024)
    n_rect = n_hit = 0
    for i in range(240):
        name = ("cube", "rand")[i & 1]
        W, H = SIZES[(i >> 1) & 1]
        pos = tuple(float(x) for x in rng.uniform(-3.0, 3.0, 3).astype(np.float32))
        tgt = tuple(float(x) for x in rng.uniform(-1.5, 1.5, 3).astype(np.float32))
        vi, pi = look(pos, tgt, W=W, H=H)
        r, hits = check(name, pos, vi, pi, W, H, f"random {i} {name} {W}x{H} {pos}->{tgt}")
        n_rect += r is not None
        n_hit += bool(hits.any())
    assert n_rect > 120 and n_hit > 120, (n_rect, n_hit)


@pytest.mark.parametrize("name", ["cube", "rand"])
def test_axis_aligned_on_box_bounds(rt, ref, name):
    """Axis-parallel views (exact zero direction components at the centre pixel
    of the odd-sized frame) from positions whose coordinates equal bounds of
    the root box: 0 * inf = NaN slab distances on the exact path."""
    _, box = mesh(name)
    lo, hi = box[:3], box[3:]
    for axis in range(3):
        a, b = (axis + 1) % 3, (axis + 2) % 3
        for sa in (lo[a], hi[a], np.float32(0.5) * (lo[a] + hi[a])):
            for sb in (lo[b], hi[b], np.float32(0.37) * hi[b]):
                for side in (-1.0, 1.0):
                    pos = [0.0, 0.0, 0.0]
                    pos[axis], pos[a], pos[b] = side * 3.0, float(sa), float(sb)
                    tgt = list(pos)
                    tgt[axis] = 0.0
                    up = [0.0, 0.0, 0.0]
                    up[a] = 1.0
                    for W, H in SIZES:
                        vi, pi = look(tuple(pos), tuple(tgt), tuple(up), W, H)
                        r, _ = check(name, tuple(pos), vi, pi, W, H, f"{name} axis {axis} from {pos} {W}x{H}")
                        on_bound = sa in (lo[a], hi[a]) or sb in (lo[b], hi[b])
                        if on_bound:
                            assert r is None, f"camera on a box bound {pos}: whole frame"


def test_looking_away_is_empty(rt, ref):
    for name in ("cube", "rand"):
        pos, tgt = (0.3, 0.2, 3.0), (0.3, 0.2, 6.0)
        for W, H in SIZES:
            vi, pi = look(pos, tgt, W=W, H=H)
            r, hits = check(name, pos, vi, pi, W, H, f"{name} looking away")
            assert r is not None and r[0] == r[1] and r[2] == r[3], r
            assert not hits.any()


def test_box_beside_the_frame_is_empty(rt, ref):
    pos, tgt = (0.0, 0.0, 6.0), (30.0, 0.0, 0.0)
    vi, pi = look(pos, tgt)
    r, hits = check("cube", pos, vi, pi, 96, 72, "box beside the frame")
    assert r is not None and (r[0] == r[1] or r[2] == r[3]) and not hits.any()


def test_camera_inside_is_whole_frame(rt, ref):
    for name in ("cube", "rand"):
        for pos in ((0.0, 0.0, 0.0), (0.1, -0.2, 0.3)):
            vi, pi = look(pos, (0.0, 0.0, -1.0))
            r, _ = check(name, pos, vi, pi, 96, 72, f"{name} inside")
            assert r is None


def test_corner_behind_is_whole_frame(rt, ref):
    for name in ("cube", "rand"):
        _, box = mesh(name)
        z = float(box[5]) + 0.05
        pos, tgt = (0.0, 0.0, z), (5.0, 0.0, z)  # along the box's face: half of it is behind
        vi, pi = look(pos, tgt)
        r, _ = check(name, pos, vi, pi, 96, 72, f"{name} corner behind")
        assert r is None


def test_odd_matrices_are_sound(rt, ref):
    """A sheared, scaled view_inv and a proj_inv with w < 0 (all of it negated:
    the same rays): any sound answer passes."""
    shear = np.eye(4, dtype=np.float32)
    shear[:3, :3] = np.float32([[1.3, 0.2, 0.0], [-0.1, 0.8, 0.3], [0.25, 0.0, 1.1]])
    for name in ("cube", "rand"):
        for pos in CAMS:
            for W, H in SIZES:
                vi, pi = look(pos, W=W, H=H)
                vs = (vi.reshape(4, 4).T @ shear).T.reshape(16).astype(np.float32)  # column-major
                check(name, pos, np.ascontiguousarray(vs), pi, W, H, f"{name} sheared view {pos}")
                r0 = rect(pos, vi, pi, W, H, mesh(name)[1])
                r1, _ = check(name, pos, vi, np.ascontiguousarray(-pi), W, H, f"{name} negated projection {pos}")
                assert r1 == r0
    # w changes sign across the screen: nothing can be said
    vi, pi = look(CAMS[0])
    bad = pi.copy()
    bad[3] = 2.0 * abs(bad[15])
    assert rect(CAMS[0], vi, bad, 96, 72, mesh("cube")[1]) is None
    bad = pi.copy()
    bad[0] = np.nan
    assert rect(CAMS[0], vi, bad, 96, 72, mesh("cube")[1]) is None
