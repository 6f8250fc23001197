"""The keyed expansion of the primary mesh path (expand_keyed, csrc/rt_scenes.h):
children ordered by packed keys, and sort8 itself for a wave in which a lane's
entered children tie in the top 29 bits of t. Colour and t are compared bitwise
with the oracle through the one-frame kernel, the batch launch (2 frames) and
the persistent queue (3 frames), on cube, spot and bunny at 64x64 and 128x72,
from three cameras:

  orbit     (0, 0, 2.5), the parity tests' camera
  closeup   0.3 scene radii from the centre: many children entered per node
  inside    the bunny from (0.35, 0.45, 0.3), inside its bounding box: the rays
            start inside boxes, so entered children tie at t = tNear

and on a 5x2 frame (10 rays: a mostly idle wave).

Which path runs, from the CPU model (tools/trav_sim.cpp --order, wave-level
expansions with a tie in the top 29 bits / all; profiles/r21/trav_sim_order.txt):

  bunny 128x72 orbit     38 / 422; some lane enters 3 or more children in 192
  bunny 128x72 closeup   77 / 1593 (camera rounded to 4 digits); 3 or more in 381
  bunny 128x72 inside    94 / 1716; 3 or more in 663
  bunny 64x64 inside     45 / 796; 3 or more in 298

so every bunny case runs both the keyed order and, in a few per cent of its
expansions, the fallback.
"""
import functools

import numpy as np
import pytest

import rtamd
import scenes as S
from rtamd import _lib

pytestmark = pytest.mark.gpu

BUNNY, SPOT, CUBE = "stanford-bunny.obj", "spot.obj", "cube.obj"
ORBIT = (0.0, 0.0, 2.5)
INSIDE = (0.35, 0.45, 0.3)
SIZES = ((64, 64), (128, 72))


def _closeup(name):
    v, _ = S.inputs(name)[1]
    r = float(np.linalg.norm(v[:, :3] / v[:, 3:4], axis=1).max())
    d = np.array([0.3, 0.2, 1.0])
    return tuple(float(x) for x in d / np.linalg.norm(d) * 0.3 * r)


# id: (mesh, W, H, camera)
CASES = {}
for _m in (CUBE, SPOT, BUNNY):
    for _w, _h in SIZES:
        CASES[f"{_m.split('.')[0]}-orbit-{_w}x{_h}"] = (_m, _w, _h, "orbit")
        CASES[f"{_m.split('.')[0]}-closeup-{_w}x{_h}"] = (_m, _w, _h, "closeup")
for _w, _h in SIZES:
    CASES[f"bunny-inside-{_w}x{_h}"] = (BUNNY, _w, _h, "inside")
CASES["bunny-orbit-5x2"] = (BUNNY, 5, 2, "orbit")
PATHS = ("one_frame", "batch", "persistent")


def _pos(case):
    mesh, _, _, cam = CASES[case]
    return ORBIT if cam == "orbit" else INSIDE if cam == "inside" else _closeup(mesh)


@functools.lru_cache(maxsize=None)
def _oracle(case):
    mesh, W, H, _ = CASES[case]
    c, t = S.ref_frame(mesh, W, H, "primary", _pos(case))
    c.setflags(write=False)
    t.setflags(write=False)
    return c, t


def test_the_inside_camera_is_inside_the_box():
    v, _ = S.inputs(BUNNY)[1]
    p = v[:, :3] / v[:, 3:4]
    assert (p.min(0) < INSIDE).all() and (INSIDE < p.max(0)).all()


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("case", list(CASES))
def test_bitwise_against_the_oracle(gpu, case, path):
    import torch
    mesh, W, H, _ = CASES[case]
    rc, rt_ = _oracle(case)
    gs = S.gpu_scene(mesh)
    gs.set_plane(None)
    P = S.params(mesh, W, H, "primary", _pos(case), "gpu")
    frames = []
    if path == "one_frame":
        c = np.zeros((H, W), np.uint32)
        t = np.full((H, W), np.inf, np.float32)
        gs.render(P, c, t, clear=True)
        frames.append((c, t))
    else:
        # whole frames take the persistent queue; the 8-row bands of two ranks,
        # written into one frame, take the batch kernel (band_takes_queue)
        n = 2 if path == "batch" else 3
        cs = [torch.full((H, W), 5, dtype=torch.int32, device="cuda") for _ in range(n)]
        ts = [torch.zeros((H, W), dtype=torch.float32, device="cuda") for _ in range(n)]
        for tile in ([rtamd.Tile(8, r, 2, 0) for r in range(2)] if path == "batch" else [None]):
            flags = rtamd.RT_FLAG_CLEAR | (_lib.RT_FLAG_TILE_NATURAL if tile is not None else 0)
            gs.render_device_frames([P] * n, [c.data_ptr() for c in cs], [t.data_ptr() for t in ts], W, H, flags,
                                    stream=torch.cuda.current_stream().cuda_stream, tile=tile)
        torch.cuda.synchronize()
        frames += [(c.cpu().numpy().view(np.uint32), t.cpu().numpy()) for c, t in zip(cs, ts)]
    for c, t in frames:
        what = f"{case} {path}"
        assert np.array_equal(np.isfinite(rt_), np.isfinite(t)), f"{what}: coverage differs"
        assert int((rc != c).sum()) == 0, f"{what}: colour differs"
        assert int((rt_.view(np.uint32) != t.view(np.uint32)).sum()) == 0, f"{what}: t differs bitwise"
    if CASES[case][3] != "orbit" or (W, H) != (5, 2):
        assert np.isfinite(rt_).any(), f"{case}: no ray hits"
