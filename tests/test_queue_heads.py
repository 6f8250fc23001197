"""The sharded work queue with more heads than XCDs (render_persist_kernel,
csrc/rt_queue.h): under every head count the queue takes, a multi-frame launch
stores the bits the one-frame kernel stores for each of its frames.

Scenes: the cube, the 3,000-triangle `rand` soup of test_mesh_resume.py and
sdf_5.octree (the queue's non-cooperative path). Items are 2x1 wave tiles
(16x8 pixels), so the frame sizes give 1, 16, 45 and 136 items per frame:
fewer items than heads, an item count that is no multiple of 8, and more items
than the widest head set. One frame per launch goes to the one-frame kernel
(no queue) and three to the queue. Every size is launched three times in a row
on one stream, which re-uses the heads the launch before has reset (with
another head count, too), and then alternating over two streams, each with
its own head set.
"""
import functools

import numpy as np
import pytest

import cpuref
import rtamd
import scenes as S
from test_mesh_resume import CAMS, scenes as soup_scenes

pytestmark = pytest.mark.gpu

RAND = (12, 3000, "rand")
SIZES = [(16, 8), (64, 32), (136, 40), (264, 64)]
HEADS = [8, 16, 32, 64]
SCENES = ["cube", "rand", "sdf_5.octree"]
FILL_C, FILL_T = -0x45454546, -5.0  # what the buffers hold before a launch: RT_FLAG_CLEAR overwrites it


@functools.lru_cache(maxsize=None)
def gpu_scene(name):
    if name == "cube":
        gs = S.gpu_scene("cube.obj")
    elif name == "rand":
        gs = soup_scenes(RAND)[1]
    else:
        gs = S.gpu_scene(name)
    return gs


def params(pos, W, H):
    vi, pi = cpuref.camera_matrices(pos, (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 45.0, W / H, 0.01, 100.0)
    return rtamd.render_params(pos, vi, pi, (2, 2, 2), 0, True, True)


def set_heads(n):
    L = rtamd.lib()
    rtamd._lib.check(L.rtx_set_queue_heads(int(n)))


def buffers(n, W, H):
    import torch
    cs = [torch.full((H, W), FILL_C, dtype=torch.int32, device="cuda") for _ in range(n)]
    ts = [torch.full((H, W), FILL_T, dtype=torch.float32, device="cuda") for _ in range(n)]
    return cs, ts


@functools.lru_cache(maxsize=None)
def one_frame_kernel(name, W, H):
    """each camera's frame by the one-frame kernel (computed once, kept on the device)"""
    import torch
    gs = gpu_scene(name)
    gs.set_plane(None)
    cs, ts = buffers(len(CAMS), W, H)
    st = torch.cuda.current_stream().cuda_stream
    for pos, c, t in zip(CAMS, cs, ts):
        gs.render_device(params(pos, W, H), c.data_ptr(), t.data_ptr(), W, H, clear=True, stream=st)
    torch.cuda.synchronize()
    return tuple((c, t.view(torch.int32)) for c, t in zip(cs, ts))


def launch(gs, cams, W, H, stream):
    import torch
    cs, ts = buffers(len(cams), W, H)
    stream.wait_stream(torch.cuda.current_stream())  # (the fills above)
    gs.render_device_frames([params(p, W, H) for p in cams], [c.data_ptr() for c in cs], [t.data_ptr() for t in ts],
                            W, H, rtamd.RT_FLAG_CLEAR, stream=stream.cuda_stream)
    return cs, ts


def check(name, W, H, cams, got, what):
    import torch
    ref = one_frame_kernel(name, W, H)
    for i, (c, t) in enumerate(zip(*got)):
        rc, rt_ = ref[i]
        bad = int((c != rc).sum()), int((t.view(torch.int32) != rt_).sum())
        assert bad == (0, 0), f"{what}, frame {i}: {bad[0]} colour words, {bad[1]} t words differ"


@pytest.mark.parametrize("heads", HEADS)
@pytest.mark.parametrize("name", SCENES)
def test_launches_equal_the_one_frame_kernel(gpu, name, heads):
    import torch
    gs = gpu_scene(name)
    gs.set_plane(None)
    s0 = torch.cuda.current_stream()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    try:
        for W, H in SIZES:
            one_frame_kernel(name, W, H)
            for n in (1, 3):
                cams = CAMS[:n]
                what = f"{name} {W}x{H} x{n}, {heads} heads"
                set_heads(heads)
                # three launches in a row on one stream: the heads after the reset
                runs = [launch(gs, cams, W, H, s0) for _ in range(3)]
                torch.cuda.synchronize()
                for k, got in enumerate(runs):
                    check(name, W, H, cams, got, f"{what}, launch {k} on one stream")
                # alternating over two streams (a head set each), four launches in flight
                runs = [launch(gs, cams, W, H, s) for s in (s1, s2, s1, s2)]
                torch.cuda.synchronize()
                for k, got in enumerate(runs):
                    check(name, W, H, cams, got, f"{what}, launch {k} over two streams")
    finally:
        set_heads(-1)


def test_head_count_changes_between_launches(gpu):
    """One stream's head set serves launches with different head counts: all
    of its words are zero between launches."""
    import torch
    name, (W, H) = "rand", (136, 40)
    gs = gpu_scene(name)
    gs.set_plane(None)
    s0 = torch.cuda.current_stream()
    try:
        runs = []
        for heads in (64, 8, 32, 16, 64, 8):
            set_heads(heads)
            runs.append((heads, launch(gs, CAMS, W, H, s0)))
        torch.cuda.synchronize()
        for heads, got in runs:
            check(name, W, H, CAMS, got, f"{name} {W}x{H} x3 with {heads} heads in a mixed sequence")
    finally:
        set_heads(-1)


def test_bad_head_count_is_rejected(gpu):
    L = rtamd.lib()
    for heads in (0, 4, 12, 128):
        assert L.rtx_set_queue_heads(heads) != 0
    set_heads(-1)
