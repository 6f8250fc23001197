"""Ray queries on rays of the exact slab path and on waves of mixed make-up
(the recipes of ray_cases.py, each pinned as discriminating on the oracle alone
by test_ray_cases_host.py), through rt_trace_rays_device and rt_intersect_rays.

Bar, as tests/test_rays_device.py, whose _trace and _assert_oracle these tests
use: sentinel-filled buffers with a 64-element guard, and hit / prim / t /
normal bitwise the oracle's.

What the rays reach that random ones do not (csrc/rt_scenes.h): waves of
trace_rays_kernel that hold fast and exact lanes together, so that
mesh_primary_wave runs both flavours of mesh_run, suspends both and finishes
them in 8-lane groups of either flavour; a prescribed number of rays left at
the first iteration (1, 8, 9, 16, 17; 8 + 8); slab operands 0 * inf = NaN
(origins on box bounds), 1/d = -inf, unnormalised and null directions.
"""
import functools

import numpy as np
import pytest
import torch

import ray_cases as RC
import rtamd
from test_rays_device import ALL, _assert_oracle, _trace

pytestmark = pytest.mark.gpu

PAIRS = RC.PAIRS
N = RC.N
CELLS = [(s, c) for s in RC.SCENES for c in RC.plain_sets(s)]
# (outputs, any_hit): closest hit with the normal, closest hit without (the
# instantiation that computes none), any hit
MODES = [(ALL, False), (("t", "prim"), False), (("hit",), True)]


@functools.lru_cache(maxsize=None)
def _gs(scene):
    return RC.gpu_scene(scene)


def _dev(*arrays):
    return tuple(torch.from_numpy(np.array(a)).cuda() for a in arrays)


def _check(ref, got, any_hit, what):
    if any_hit:
        assert set(got) == {"hit"} and np.array_equal(ref[0], got["hit"]), f"{what}: any-hit mask differs"
    else:
        _assert_oracle(ref, got, what)


def _set_coop(gs, on):
    rtamd._lib.check(rtamd.lib().rtx_set_coop(gs._handle(), int(on)))


@pytest.mark.parametrize("scene,cls", CELLS)
def test_every_class_through_every_instantiation(gpu, scene, cls):
    """4,096 rays of one class x the three intervals x {closest hit with the
    normal, t and prim without it, any hit}, with scalar intervals (the mesh's
    closest hit is then mesh_primary_wave) and with d_tnear / d_tfar tensors
    (the per-lane mesh traversal and the per-ray paths of grid and octree; the
    scalars of that call are other values, which must not be read)."""
    gs = _gs(scene)
    gs.set_plane(None)
    o, d = RC.plain_sets(scene)[cls]
    o_t, d_t = _dev(o, d)
    for tn, tf in PAIRS:
        ref = RC.oracle(scene, cls, tn, tf)
        tn_t, tf_t = _dev(np.full(N, tn, np.float32), np.full(N, tf, np.float32))
        for outputs, any_hit in MODES:
            what = f"{scene} {cls} [{tn}, {tf}] {outputs}"
            _check(ref, _trace(gs, o_t, d_t, N, outputs=outputs, tn=tn, tf=tf, any_hit=any_hit), any_hit, what)
            got = _trace(gs, o_t, d_t, N, outputs=outputs, tn=0.25, tf=3.0, tn_t=tn_t, tf_t=tf_t, any_hit=any_hit)
            _check(ref, got, any_hit, what + " per-ray intervals")


SIZES = (RC.NWAVES * RC.WAVE, 3 * RC.WAVE + 1, 3 * RC.WAVE + 9)


@pytest.mark.parametrize("scene", RC.MESH_SCENES)
@pytest.mark.parametrize("pattern", RC.PATTERNS, ids=RC.pattern_id)
def test_wave_make_up(gpu, scene, pattern):
    """Every compose_waves pattern, closest hit with all outputs, on whole waves
    and on batches that end 1 and 9 rays into a wave, with the cooperative tail
    on and off: both settings equal the oracle."""
    gs = _gs(scene)
    gs.set_plane(None)
    o, d, _ = RC.plain_batch(scene, pattern)
    ref = RC.ref_scene(scene).intersect_rays(o, d, *PAIRS[0])
    o_t, d_t = _dev(o, d)
    try:
        for coop in (True, False):
            _set_coop(gs, coop)
            for n in SIZES:
                _assert_oracle(tuple(a[:n] for a in ref), _trace(gs, o_t, d_t, n),
                               f"{scene} {RC.pattern_id(pattern)} n={n} coop={coop}")
    finally:
        _set_coop(gs, True)


@pytest.mark.parametrize("n", [1, 7, 8, 9, 16, 17])
def test_small_batches_of_exact_rays(gpu, n):
    """n exact-path rays that all hit the lattice mesh, and nothing else in the
    launch: at most 8 rays are left from the first iteration on (n <= 8), or as
    soon as a wave of 9, 16 or 17 has lost rays, so the traversal runs in the
    8-lane groups, mesh_run_coop<false>. Three different sets per n."""
    scene = "lattice"
    gs = _gs(scene)
    gs.set_plane(None)
    po, pd = RC.plain_pools(scene, hit_only=True)["exact"]
    for k in range(3):
        o, d = np.ascontiguousarray(po[k * 32:k * 32 + n]), np.ascontiguousarray(pd[k * 32:k * 32 + n])
        assert len(o) == n and (d == 0).any(axis=1).all()
        ref = RC.ref_scene(scene).intersect_rays(o, d, *PAIRS[0])
        assert ref[0].all()
        o_t, d_t = _dev(o, d)
        _assert_oracle(ref, _trace(gs, o_t, d_t, n), f"{n} exact rays, set {k}")
        _assert_oracle(ref, _trace(gs, o_t, d_t, n, outputs=("t", "prim")), f"{n} exact rays, set {k}, no normal")


@pytest.mark.parametrize("scene", list(RC.SCENES))
@pytest.mark.parametrize("pattern", ["interleave", "shuffled"])
def test_host_entry_on_mixed_waves(gpu, scene, pattern):
    """rt_intersect_rays (rays_kernel: per lane, no cooperative tail) on the
    mixed batches: the same oracle."""
    gs = _gs(scene)
    gs.set_plane(None)
    o, d, _ = RC.plain_batch(scene, pattern)
    for tn, tf in PAIRS:
        ref = RC.ref_scene(scene).intersect_rays(o, d, tn, tf)
        g = gs.intersect(o, d, tn, tf)
        what = f"{scene} {pattern} [{tn}, {tf}] host entry"
        h = ref[0].astype(bool)
        assert h.any() and not h.all()
        # (as tests/test_gpu_parity.py::test_intersect_rays: this entry promises t and normal on hits)
        assert np.array_equal(h, g.hitten), f"{what}: hit mask differs"
        assert np.array_equal(ref[3], g.prim), f"{what}: primitive ids differ"
        assert np.array_equal(ref[1][h].view(np.uint32), g.t[h].view(np.uint32)), f"{what}: t differs"
        assert np.array_equal(ref[2][h].view(np.uint32), g.normal[h].view(np.uint32)), f"{what}: normal differs"
