"""Instanced scenes, host side (include/rtamd.h): rt_affine_inverse, the one
definition of the world-to-object matrix M; the header and the C++ wrapper;
and the issue's rotation recipe, asserted reference against reference (the
composed oracle of instances_common against the oracle on the flattened mesh).
No GPU.
"""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import instances_common as IC
from conftest import ROOT

INCLUDE = os.path.join(ROOT, "include")
RT_E_INVALID = -1


def _inv(rt, x):
    x = np.ascontiguousarray(x, np.float32).reshape(12)
    out = np.full(12, 7.0, np.float32)
    rc = rt.lib().rt_affine_inverse(C.c_void_p(x.ctypes.data), C.c_void_p(out.ctypes.data))
    return rc, out.reshape(3, 4)


def _exact_cases():
    cases = [("identity", np.eye(3), np.zeros(3), np.eye(3), np.zeros(3))]
    b = np.float64([3.0, -5.5, 0.25])
    cases.append(("translation", np.eye(3), b, np.eye(3), -b))
    for s in ([2.0, 0.5, 4.0], [0.25, -8.0, 1.0], [-2.0, -2.0, -0.5]):
        s = np.float64(s)
        # x = s p + b  ->  p = x / s - b / s (every quotient exact)
        cases.append((f"scale {s.tolist()}", np.diag(s), b, np.diag(1 / s), -b / s))
    for perm in itertools.permutations(range(3)):
        for sg in itertools.product([1.0, -1.0], repeat=3):
            P = np.zeros((3, 3))
            for r in range(3):
                P[r, perm[r]] = sg[r]
            # orthogonal with entries 0, +-1: the inverse is the transpose
            cases.append((f"permutation {perm} {sg}", P, b, P.T, -(P.T @ b)))
    return cases


@pytest.mark.parametrize("what,A,b,Ai,bi", _exact_cases(), ids=lambda v: v if isinstance(v, str) else "")
def test_affine_inverse_exact(rt, what, A, b, Ai, bi):
    """By value (-0 == +0), exactly: every product and quotient is exact here."""
    rc, got = _inv(rt, IC.affine(A, b))
    assert rc == 0, rt.lib().rt_last_error()
    assert np.array_equal(got, IC.affine(Ai, bi)), f"{what}: {got}"


def test_affine_inverse_inverts(rt):
    """200 matrices R diag(s) + b (R from a QR of normals, s in [0.5, 2], b in
    [-3, 3]): max |M A - I| in float64 <= 1e-4 -- a wrong convention gives
    errors of order 1, float rounding at condition number <= 4 about 1e-7."""
    rng = np.random.default_rng(14)
    worst = 0.0
    for k in range(200):
        A = IC.rot(100 + k) @ np.diag(rng.uniform(0.5, 2.0, 3))
        x = IC.affine(A, rng.uniform(-3, 3, 3))
        M = rt.affine_inverse(x).astype(np.float64)
        X4 = np.vstack([x.astype(np.float64), [0, 0, 0, 1]])
        M4 = np.vstack([M, [0, 0, 0, 1]])
        worst = max(worst, float(np.abs(M4 @ X4 - np.eye(4)).max()))
    print(f"max |M A - I| = {worst:.3g}")
    assert worst <= 1e-4


def test_affine_inverse_refuses(rt):
    good = IC.affine(np.diag([1.0, 2.0, 3.0]), [1, 2, 3])
    bad = {"rank 2": IC.affine([[1, 2, 3], [2, 4, 6], [0, 1, 0]], [0, 0, 0]),
           "zero": np.zeros((3, 4), np.float32),
           "zero scale": IC.affine(np.diag([1.0, 0.0, 1.0]), [0, 0, 0])}
    for k in range(12):
        for v in (np.nan, np.inf, -np.inf):
            x = good.copy().reshape(12)
            x[k] = v
            bad[f"entry {k} = {v}"] = x
    huge = good.copy()
    huge[:, :3] *= np.float32(1e30)  # the determinant overflows
    bad["determinant not finite"] = huge
    for what, x in bad.items():
        rc, out = _inv(rt, x)
        assert rc == RT_E_INVALID and rt.lib().rt_last_error(), what
        assert (out == 7.0).all(), f"{what}: the output was written"
    assert rt.lib().rt_affine_inverse(None, None) == RT_E_INVALID
    assert _inv(rt, good)[0] == 0
    with pytest.raises(rt.RtError):
        rt.affine_inverse(bad["zero"])


def test_abi_is_additive(rt):
    from rtamd import _lib
    names = ["rt_affine_inverse", "rt_scene_create_instanced", "rt_scene_update_instances",
             "rt_scene_update_instances_device", "rt_scene_get_instances"]
    for name in names:
        assert name in rt.EXPORTED and hasattr(rt.lib(), name)
    assert rt.lib().rt_abi_version() == 8
    src = open(os.path.join(INCLUDE, "rtamd.h")).read()
    assert re.search(r"RT_SCENE_INSTANCED = 4\b", src) and re.search(r"#define RT_INSTANCE_DISABLED 1u", src)
    assert _lib.RT_SCENE_INSTANCED == 4 and _lib.RT_INSTANCE_DISABLED == 1
    assert C.sizeof(_lib.Instance) == 56
    assert C.sizeof(_lib.RayBatch) == 80  # rt_ray_batch keeps its layout (8 + 4 * 8 + 2 * 4 + 4 * 8)


def _compile(tmp_path, name, src, compiler, flags):
    f = tmp_path / name
    f.write_text(src)
    r = subprocess.run([compiler, *flags, "-I", INCLUDE, "-fsyntax-only", str(f)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_header_is_plain_c(tmp_path):
    src = ('#include "rtamd.h"\n'
           "int main(void){ rt_instance i = {0, RT_INSTANCE_DISABLED, {1,0,0,0, 0,1,0,0, 0,0,1,0}}; float m[12];\n"
           "  rt_scene *s = 0, *b = 0; rt_scene *const bl[1] = {b};\n"
           "  int rc = rt_affine_inverse(i.xform, m) + rt_scene_create_instanced(bl, 1, &i, 1, &s)\n"
           "    + rt_scene_update_instances(s, 0, 1, &i) + rt_scene_update_instances_device(s, 0, 1, m, 0)\n"
           "    + rt_scene_get_instances(s, 0, 1, &i, m, 0);\n"
           "  return rc + (RT_SCENE_INSTANCED == 4 ? 0 : 1); }\n")
    _compile(tmp_path, "a.c", src, "gcc", ["-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic"])


def test_cpp_wrapper_has_instanced_scene(tmp_path):
    src = ('#include "rtamd.hpp"\n'
           "int main(){ rtamd::BVHBuilder b; rtamd::InstancedScene s;\n"
           "  std::vector<rt_instance> in(1); std::vector<float> inv; std::vector<uint32_t> sk;\n"
           "  if (in.empty()) { s.perform({&b}, in); s.updateInstances(0, in);\n"
           "    s.updateInstancesDevice(0, 1, nullptr); (void)s.instances(&inv, &sk); (void)s.size(); }\n"
           "  return 0; }\n")
    _compile(tmp_path, "a.cpp", src, "g++", ["-std=c++17", "-Wall", "-Wextra", "-Werror"])


def test_split_prim():
    from rtamd import torch_rays
    prim = np.int64([-1, -2, 5, (3 << 32) | 7, (69 << 32) | 0xFFFFFFFE])
    inst, tri = torch_rays.split_prim(prim)
    assert inst.tolist() == [-1, -1, 0, 3, 69]
    assert tri.tolist() == [-1, -2, 5, 7, 0xFFFFFFFE]


@pytest.mark.parametrize("name", ["bunny", "cube"])
@pytest.mark.parametrize("seed", IC.ROT_SEEDS)
def test_rotation_recipe_reference_against_reference(rt, ref, name, seed):
    """The GPU file's "convention under rotation" bounds hold between the two
    references themselves: the composed oracle of one rotated, scaled instance
    against the oracle on the flattened mesh."""
    x, o, d = IC.rotation_case(name, seed)
    v, i = IC.mesh(name)
    flat = ref.RefScene.mesh(IC.flatten(v, x), i).intersect_rays(o, d, 0.01, 100.0)
    M = rt.affine_inverse(x)
    hit, t, _, _ = IC.compose({0: IC.ref_mesh(name)}, [0], [0], M[None], o, d, 0.01, 100.0)
    IC.assert_rotation_bounds(flat, hit, t, f"{name} seed {seed}")
