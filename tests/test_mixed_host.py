"""Mixed instanced scenes, host side (rt_scene_create_instanced_any,
include/rtamd.h): conditions on the test inputs of tests/test_mixed_gpu.py,
measured on the composed oracle alone; the header's claim that the any-hit OR
equals the closest-hit flag when SDF kinds are present; the world box of the
SDF kinds' cube; the ABI. No GPU.
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import instances_common as IC
import mixed_common as MC
import tlas_common as TC
from conftest import ROOT

F = np.float32
N = MC.N


def _bits(a):
    return np.asarray(a, F).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _events(rt, name, kind, tree):
    rf, blas, flags, M, wbox = MC.host_scene(rt, name)
    o, d = MC.rays(name, kind)
    kinds = {j: MC.KIND[m] for j, m in enumerate(MC.DEFS[name][0])}
    return MC.compose_events(rf, kinds, blas, flags, M, o, d, 0.01, 100.0, wbox if tree else None), kinds, blas


@pytest.mark.parametrize("name", ["m3", "m9"])
@pytest.mark.parametrize("kind", ["random", "eye"])
def test_inputs_exercise_every_kind(rt, ref, name, kind):
    """Conditions on the inputs, not tolerances: on the composed oracle every
    kind wins at least 5 % of the rays, at least 2 % of the rays have a hit of
    one kind replaced by a later instance of another kind, at least 5 % hit
    nothing. The loop with events is instances_common.compose's."""
    (hit, best, win, replaced), kinds, blas = _events(rt, name, kind, False)
    rf, _, flags, M, _ = MC.host_scene(rt, name)
    o, d = MC.rays(name, kind)
    flat = IC.compose(rf, blas, flags, M, o, d, 0.01, 100.0)
    assert np.array_equal(hit, flat[0]) and np.array_equal(_bits(best), _bits(flat[1]))
    assert np.array_equal(win, np.where(flat[3] >= 0, flat[3] >> 32, -1))
    n = len(o)
    share = {k: float((np.array([kinds[blas[w]] if w >= 0 else 0 for w in win]) == k).mean())
             for k in (MC.MESH, MC.GRID, MC.OCT)}
    print(f"{name} {kind}: wins mesh {share[MC.MESH]:.3f} grid {share[MC.GRID]:.3f} octree {share[MC.OCT]:.3f}, "
          f"replaced across kinds {replaced.mean():.3f}, misses {1.0 - hit.mean():.3f} of {n} rays")
    assert min(share.values()) >= 0.05
    assert replaced.mean() >= 0.02
    assert 1.0 - hit.mean() >= 0.05


@pytest.mark.parametrize("name", ["m3", "m9"])
@pytest.mark.parametrize("tree", [False, True])
@pytest.mark.parametrize("tn,tf", [(0.01, 100.0), (0.5, 2.0)])
def test_any_hit_or_equals_the_closest_hit_flag(rt, ref, name, tree, tn, tf):
    """The header's OR over the instances of the BLAS hit flag under the full
    tFar (for the tree: over those with box_pass under the full tFar) against
    the closest-hit flag of the header's loop, on the same rays. The header
    claims equality for SDF kinds too (best is +inf, so tf_i is tFar, until the
    first accepted hit): the count of differing rays is recorded and must be 0."""
    rf, blas, flags, M, wbox = MC.host_scene(rt, name)
    for kind in ("random", "eye"):
        o, d = MC.rays(name, kind)
        n = len(o)
        if tree:
            closest = TC.compose_tlas(rf, blas, flags, M, wbox, o, d, tn, tf)[0]
            occ = TC.any_hit_tlas(rf, blas, flags, M, wbox, o, d, tn, tf)
        else:
            closest = IC.compose(rf, blas, flags, M, o, d, tn, tf)[0]
            occ = np.zeros(n, np.int32)
            for i in range(len(blas)):
                if flags[i] & IC.DISABLED:
                    continue
                oo, dd = IC.to_object(M[i], o, d)
                occ |= rf[blas[i]].intersect_rays(oo, dd, tn, tf)[0].astype(np.int32)
        differ = int((closest != occ).sum())
        print(f"{name} tree={tree} {kind} [{tn}, {tf}]: any-hit OR differs from the closest-hit flag on {differ} of {n} rays")
        assert differ == 0


def test_world_box_of_the_unit_cube(rt):
    """rt_instance_world_box of (-1,-1,-1, 1,1,1) under every test pose is
    tlas_common.world_box, bitwise."""
    for name in ("m3", "m9", "m130"):
        for b, x, _ in MC.DEFS[name][1]:
            got = rt.instance_world_box(x, MC.UNIT_CUBE)
            assert np.array_equal(_bits(got), _bits(TC.world_box(x, MC.UNIT_CUBE))), (name, b)


def test_abi_and_argument_rules_without_a_device(rt):
    """The entry is exported, declared and bound; the rules checked ahead of
    any device call: NULL arguments and unknown flag bits are RT_E_INVALID and
    leave *out NULL."""
    from rtamd import _lib
    assert "rt_scene_create_instanced_any" in rt.EXPORTED and hasattr(rt.lib(), "rt_scene_create_instanced_any")
    src = open(os.path.join(ROOT, "include", "rtamd.h")).read()
    assert re.search(r"int rt_scene_create_instanced_any\(", src)
    L = rt.lib()
    arr = (_lib.Instance * 1)()
    arr[0].xform[:] = IC.IDENTITY.reshape(12).tolist()
    hs = (C.c_void_p * 1)(None)
    out = C.c_void_p(0x1234)
    assert L.rt_scene_create_instanced_any(None, 1, arr, 1, 0, C.byref(out)) == -1
    assert L.rt_scene_create_instanced_any(hs, 1, None, 1, 0, C.byref(out)) == -1
    assert L.rt_scene_create_instanced_any(hs, 1, arr, 1, 0, None) == -1
    for bad in (2, 3, 0x80000000):
        out = C.c_void_p(0x1234)
        assert L.rt_scene_create_instanced_any(hs, 1, arr, 1, bad, C.byref(out)) == -1
        assert not out.value and L.rt_last_error()
    for nb, ni in ((0, 1), (1, 0)):
        assert L.rt_scene_create_instanced_any(hs, nb, arr, ni, 0, C.byref(out)) == -1
