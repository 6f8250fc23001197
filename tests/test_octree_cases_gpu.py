"""The hand-built octrees of octree_cases.py on the GPU, bit for bit against
the oracle: every stack class (4, 7, 15 and 31 slots), packed and unpacked
node coordinates (OctS<true> up to 8 levels, OctS<false> from 9 on), stacks
that are full on every level, leaves of every kind on every level, blocks in
any order and shared between parents, roots that are leaves.

Ray queries (rt_intersect_rays, rt_trace_rays_device), frames (rt_render,
rt_render_device_frames), shaded rays (rt_shade_rays_device) and one instanced
scene over three of the trees and a mesh. No tolerance anywhere. That the
inputs reach what they are for -- enough hits, full stacks, every instance
winning rays, frames that show something -- is asserted on the oracle alone in
test_octree_cases_host.py.
"""
import functools

import numpy as np
import pytest
import torch

import instances_common as IC
import octree_cases as OC
import rtamd
import shade_common as SC
import shading_ref as SR
import tlas_common as TC
from test_instances_gpu import _assert_ref
from test_rays_device import _assert_oracle, _bits, _trace
from test_shade_gpu import _assert_oracle as _assert_shaded
from test_shade_gpu import _shade

pytestmark = pytest.mark.gpu

N = OC.N
W, H = OC.FRAME


@functools.lru_cache(maxsize=None)
def _tree(key):
    return rtamd.SDFOctree(OC.case(key)[0])


def _scene(key, plane=False):
    """The tree's GPU scene with its plane set or cleared (the scene is shared
    between the tests), its depth checked first."""
    gs = _tree(key)
    assert gs.tree_stats()[2] == OC.DEPTH[key]
    gs.set_plane(rtamd.Plane(*OC.PLANE) if plane else None)
    return gs


@functools.lru_cache(maxsize=None)
def _rays(key):
    _, _, o, d = OC.case(key)
    return o, d, torch.from_numpy(np.array(o)).cuda(), torch.from_numpy(np.array(d)).cuda()  # (writable copies for torch)


# -------------------------------------------------------------- ray queries --
@pytest.mark.parametrize("tn,tf", OC.INTERVALS)
@pytest.mark.parametrize("key", OC.KEYS)
def test_ray_queries(gpu, key, tn, tf):
    """The 4,096 rays through rt_intersect_rays and through
    rt_trace_rays_device as closest hit with all four outputs, closest hit
    without the normal, and any hit."""
    gs = _scene(key)
    o, d, o_t, d_t = _rays(key)
    ref = OC.oracle(key, tn, tf)
    what = f"{key} [{tn:g}, {tf:g}]"
    g = gs.intersect(o, d, tn, tf)
    h = g.hitten
    assert np.array_equal(ref[0].astype(bool), h), f"{what}: rt_intersect_rays: hit mask differs"
    assert np.array_equal(ref[3], g.prim), f"{what}: rt_intersect_rays: primitive ids differ"
    assert np.array_equal(_bits(ref[1][h]), _bits(g.t[h])), f"{what}: rt_intersect_rays: t differs"
    assert np.array_equal(_bits(ref[2][h]), _bits(g.normal[h])), f"{what}: rt_intersect_rays: normal differs"
    _assert_oracle(ref, _trace(gs, o_t, d_t, N, tn=tn, tf=tf), what)
    _assert_oracle(ref, _trace(gs, o_t, d_t, N, outputs=("hit", "t", "prim"), tn=tn, tf=tf), what + " no normal")
    a = _trace(gs, o_t, d_t, N, outputs=("hit",), tn=tn, tf=tf, any_hit=True)
    assert np.array_equal(ref[0], a["hit"]), f"{what}: any-hit mask differs"


@pytest.mark.parametrize("n", [193, 201])
@pytest.mark.parametrize("key", OC.KEYS)
def test_partial_waves(gpu, key, n):
    """3 x 64 + 1 and + 9 rays, the prefixes of the same set, in all three
    intervals: [0, n) is written, the sentinels behind it are not (_trace)."""
    gs = _scene(key)
    _, _, o_t, d_t = _rays(key)
    for tn, tf in OC.INTERVALS:
        ref = tuple(a[:n] for a in OC.oracle(key, tn, tf))
        what = f"{key} [{tn:g}, {tf:g}] n={n}"
        _assert_oracle(ref, _trace(gs, o_t, d_t, n, tn=tn, tf=tf), what)
        _assert_oracle(ref, _trace(gs, o_t, d_t, n, outputs=("hit", "t", "prim"), tn=tn, tf=tf), what + " no normal")
        a = _trace(gs, o_t, d_t, n, outputs=("hit",), tn=tn, tf=tf, any_hit=True)
        assert np.array_equal(ref[0], a["hit"]), f"{what}: any-hit mask differs"


# ------------------------------------------------------------------- frames --
@pytest.mark.parametrize("mode", list(OC.FRAME_MODES))
@pytest.mark.parametrize("key", OC.KEYS)
def test_frames(gpu, key, mode):
    """96 x 72 from the three cameras of octree_cases.cameras, in primary mode
    and in default mode (plane at -1.2; the shadow and reflection rays run the
    occlusion walk): each as a one-frame rt_render, and the three as one
    rt_render_device_frames launch. Colour and t are the oracle's bits."""
    gs = _scene(key, plane=OC.FRAME_MODES[mode][1])
    P = [OC.frame_params(key, cam, mode, rtamd) for cam in range(3)]
    refs = [OC.oracle_frame(key, cam, mode) for cam in range(3)]
    for cam in range(3):
        c = np.full((H, W), 0x5A5A5A5A, np.uint32)
        t = np.full((H, W), -5.0, np.float32)
        gs.render(P[cam], c, t, clear=True)
        what = f"{key} {mode} camera {cam}"
        assert np.array_equal(refs[cam][0], c), f"{what}: colour differs on {int((refs[cam][0] != c).sum())} pixels"
        assert np.array_equal(_bits(refs[cam][1]), _bits(t)), f"{what}: t differs on {int((_bits(refs[cam][1]) != _bits(t)).sum())} pixels"
    cs = [torch.full((H, W), 0x5A5A5A5A, dtype=torch.int32, device="cuda") for _ in range(3)]
    ts = [torch.full((H, W), -5.0, dtype=torch.float32, device="cuda") for _ in range(3)]
    gs.render_device_frames(P, [c.data_ptr() for c in cs], [t.data_ptr() for t in ts], W, H, rtamd.RT_FLAG_CLEAR)
    torch.cuda.synchronize()
    for cam in range(3):
        c, t = cs[cam].cpu().numpy().view(np.uint32), ts[cam].cpu().numpy()
        what = f"{key} {mode} camera {cam} of one launch"
        assert np.array_equal(refs[cam][0], c), f"{what}: colour differs on {int((refs[cam][0] != c).sum())} pixels"
        assert np.array_equal(_bits(refs[cam][1]), _bits(t)), f"{what}: t differs on {int((_bits(refs[cam][1]) != _bits(t)).sum())} pixels"


# -------------------------------------------------------------- shaded rays --
@functools.lru_cache(maxsize=None)
def _classes():
    """One of the three intervals per ray, seeded."""
    cls = np.random.default_rng(23).integers(0, len(OC.INTERVALS), N)
    tn = np.float32([OC.INTERVALS[c][0] for c in cls])
    tf = np.float32([OC.INTERVALS[c][1] for c in cls])
    assert all((cls == c).sum() > 1000 for c in range(len(OC.INTERVALS)))
    return tn, tf, torch.from_numpy(tn).cuda(), torch.from_numpy(tf).cuda()


@pytest.mark.parametrize("key", OC.KEYS)
def test_shaded_rays(gpu, key):
    """rt_shade_rays_device with RT_SHADE_CLEAR on the 4,096 rays, each under
    one of the three intervals: Lambert with the plane at -1.2, shadows and
    reflections, against shade_common.shade above the oracle."""
    gs = _scene(key, plane=True)
    o, d, o_t, d_t = _rays(key)
    tn, tf, tn_t, tf_t = _classes()
    P = SC.params(W, H, "std", SR.LAMBERT, True, True, SR.CAMERA, module=rtamd)
    ref = SC.shade(OC.ref_scene(key), OC.PLANE, o, d, tn, tf, "std", SR.LAMBERT, True, True)
    got = _shade(gs, o_t, d_t, N, P, tn_t=tn_t, tf_t=tf_t)
    _assert_shaded(ref, got, key, min_defined=0.99)
    if key != "root-never":
        assert int((ref.prim >= 0).sum()) >= 128
    assert int((ref.prim == -2).sum()) >= 128, "the plane is hardly hit"


# ------------------------------------------------------- the instanced scene --
@functools.lru_cache(maxsize=None)
def _instanced(tlas):
    blas = [rtamd.BVHBuilder(rtamd.SimpleMesh(*IC.mesh("cube"))) if k == "cube" else rtamd.SDFOctree(OC.case(k)[0])
            for k in OC.INSTANCE_BLAS]
    gs = rtamd.InstancedScene(blas, OC.instance_defs(), tlas=tlas)
    assert gs.mixed
    return gs


@pytest.mark.parametrize("tlas", [False, True])
def test_instanced_scene(gpu, tlas):
    """A packed tree, a 15-slot and a 31-slot tree and the cube under rigid
    poses in one rt_scene_create_instanced_any scene, flat list and top-level
    tree: closest hit with all four outputs and any hit against the header's
    loop composed from the oracle, on the M (and leaf boxes) the device holds."""
    gs = _instanced(tlas)
    gs.set_plane(None)
    o, d = OC.instance_rays()
    o_t, d_t = torch.from_numpy(np.array(o)).cuda(), torch.from_numpy(np.array(d)).cuda()
    tab = gs.instances()
    refs = OC.instance_refs()
    for tn, tf in OC.INTERVALS:
        if tlas:
            ref = TC.compose_tlas(refs, tab.blas, tab.flags, tab.inv, gs.tlas()[0], o, d, tn, tf, tab.skipped)[:4]
        else:
            ref = IC.compose(refs, tab.blas, tab.flags, tab.inv, o, d, tn, tf, tab.skipped)
        what = f"instanced tlas={tlas} [{tn:g}, {tf:g}]"
        _assert_ref(ref, _trace(gs, o_t, d_t, N, tn=tn, tf=tf), what)
        a = _trace(gs, o_t, d_t, N, outputs=("hit",), tn=tn, tf=tf, any_hit=True)
        assert np.array_equal(ref[0], a["hit"]), f"{what}: any-hit mask differs"
        won = np.bincount((ref[3][ref[0] != 0] >> 32).astype(np.int64), minlength=4)
        assert (won >= 64).all(), f"{what}: wins per instance {won.tolist()}"
