"""Instanced scenes on rays of the exact slab path (trace_instances_kernel,
csrc/rt_instances.hip): the lattice mesh under four signed permutations times
2^k with integer translations -- two coincident, one mirrored -- and one cube
under a rotation (ray_cases.instanced_def). World-space lattice rays then have
exact zeros in object space and origins on box bounds in the permuted
instances and general directions in the cube, so one wave mixes the fast and
exact flavours of mesh_primary_wave PER INSTANCE of the loop.

The reference is instances_common.compose on the M read back from the device,
as in tests/test_instances_gpu.py, whose _trace and _assert_ref these tests
use; test_ray_cases_host.py pins on the CPU that every set is hit at least 100
times, that every non-coincident instance wins and that the lower of the
coincident pair wins all its ties.
"""
import functools

import numpy as np
import pytest
import torch

import instances_common as IC
import ray_cases as RC
import rtamd
from test_instances_gpu import ALL, _assert_ref, _trace

pytestmark = pytest.mark.gpu

PAIRS = RC.PAIRS
N = RC.N
MODES = [(ALL, False), (("t", "prim"), False), (("hit",), True)]


@functools.lru_cache(maxsize=None)
def _scene():
    blas = [rtamd.BVHBuilder(rtamd.SimpleMesh(*IC.mesh(m))) for m in RC.INST_MESHES]
    return rtamd.InstancedScene(blas, RC.instanced_def()), blas


@functools.lru_cache(maxsize=None)
def _M():
    gs, _ = _scene()
    tab = gs.instances()
    assert not tab.skipped.any() and not tab.flags.any()
    assert tab.blas.tolist() == [b for b, _, _ in RC.instanced_def()]
    return tab.inv


def _dev(*arrays):
    return tuple(torch.from_numpy(np.array(a)).cuda() for a in arrays)


def test_stored_inverse_is_exact(gpu):
    """gs.instances().inv of the four exact poses is bitwise the exact inverse,
    computed in float64 (it is representable)."""
    want = RC.instanced_M()[:RC.N_EXACT_INST]
    got = _M()[:RC.N_EXACT_INST]
    assert np.array_equal(got, want), "M differs by value"
    nz = want != 0
    assert np.array_equal(got.view(np.uint32)[nz], want.view(np.uint32)[nz])
    # an entry that is zero may carry either sign: M[r, 3] = -(row . b) with products +-0
    assert (got[~nz] == 0).all()


@pytest.mark.parametrize("cls", list(RC.instanced_sets()))
def test_every_class_through_every_instantiation(gpu, cls):
    """4,096 world-space rays of one class x the three intervals x {closest hit
    with the normal, t and prim without it, any hit}, with scalar intervals and
    with d_tnear / d_tfar tensors (the per-lane traversal)."""
    gs, _ = _scene()
    gs.set_plane(None)
    o, d = RC.instanced_sets()[cls]
    o_t, d_t = _dev(o, d)
    for tn, tf in PAIRS:
        ref = RC.instanced_ref(o, d, tn, tf, _M())
        if cls == "null_dir":
            assert not ref[0].any()
        else:
            assert int(ref[0].sum()) >= 100
        tn_t, tf_t = _dev(np.full(N, tn, np.float32), np.full(N, tf, np.float32))
        for outputs, any_hit in MODES:
            what = f"instanced {cls} [{tn}, {tf}] {outputs}"
            for kw in (dict(tn=tn, tf=tf), dict(tn=0.25, tf=3.0, tn_t=tn_t, tf_t=tf_t)):
                got = _trace(gs, o_t, d_t, N, outputs=outputs, any_hit=any_hit, **kw)
                if any_hit:
                    assert np.array_equal(ref[0], got["hit"]), f"{what}: any-hit mask differs"
                else:
                    _assert_ref(ref, got, what + (" per-ray intervals" if "tn_t" in kw else ""))


@pytest.mark.parametrize("pattern", RC.PATTERNS, ids=RC.pattern_id)
def test_wave_make_up(gpu, pattern):
    """Every compose_waves pattern in world space, closest hit with all
    outputs and any hit, on whole waves and on batches that end 1 and 9 rays
    into a wave."""
    gs, _ = _scene()
    gs.set_plane(None)
    o, d, _ = RC.instanced_batch(pattern)
    ref = RC.instanced_ref(o, d, *PAIRS[0], _M())
    o_t, d_t = _dev(o, d)
    for n in (RC.NWAVES * RC.WAVE, 3 * RC.WAVE + 1, 3 * RC.WAVE + 9):
        what = f"instanced {RC.pattern_id(pattern)} n={n}"
        _assert_ref(tuple(a[:n] for a in ref), _trace(gs, o_t, d_t, n), what)
        a = _trace(gs, o_t, d_t, n, outputs=("hit",), any_hit=True)
        assert np.array_equal(ref[0][:n], a["hit"]), f"{what}: any-hit mask differs"
