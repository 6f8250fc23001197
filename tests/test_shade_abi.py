"""rt_eye_rays_device and rt_shade_rays_device (shaded ray queries on device
buffers): what can be checked without a GPU. Both symbols are exported and
bound, the ABI version stays, the calls that need no scene are refused with a
message, and the C / C++ headers compile for a user of the two entries and of
IScene::shadeDevice. The shaded values are checked on the GPU
(test_shade_gpu.py).
"""
import ctypes as C
import re
import subprocess

from test_rays_abi import _compile

RT_E_INVALID = -1


def test_symbols_exported_and_bound(rt):
    from rtamd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", rt.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    for name, arity in (("rt_eye_rays_device", 6), ("rt_shade_rays_device", 6)):
        assert re.search(rf"\bT {name}$", out, flags=re.M), name
        assert name in rt.EXPORTED
        res, args = _lib._SIGS[name]
        assert res is C.c_int and len(args) == arity
    assert _lib._SIGS["rt_shade_rays_device"][1][1] is C.POINTER(_lib.RayBatch)
    assert _lib.RT_SHADE_CLEAR == 1
    assert rt.lib().rt_abi_version() == 8  # additive: the ABI version stays
    assert C.sizeof(_lib.RayBatch) == 80   # rt_ray_batch is not touched


def _shade(rt, scene, batch, params, color, flags=0):
    rc = rt.lib().rt_shade_rays_device(scene, batch, params, color, flags, None)
    return rc, rt.lib().rt_last_error()


def test_scene_independent_refusals(rt):
    """A NULL scene, a NULL batch before any dereference, a NULL p and a NULL
    d_color, each with a message (a scene needs a GPU to exist: the fake one is
    never read, every refusal here comes first)."""
    from rtamd import _lib
    b = _lib.RayBatch(4, 64, 64, None, None, 0.01, 100.0, None, 64, None, None)
    P = rt.RenderParams()
    fake = C.cast(C.create_string_buffer(4096), C.c_void_p)
    rc, msg = _shade(rt, None, C.byref(b), C.byref(P), 64)
    assert rc == RT_E_INVALID and msg and b"scene" in msg
    rc, msg = _shade(rt, fake, None, C.byref(P), 64)
    assert rc == RT_E_INVALID and msg and b"batch" in msg
    rc, msg = _shade(rt, fake, C.byref(b), None, 64)
    assert rc == RT_E_INVALID and msg and b"params" in msg
    rc, msg = _shade(rt, fake, C.byref(b), C.byref(P), None)
    assert rc == RT_E_INVALID and msg and b"colour" in msg


def test_eye_rays_refusals(rt):
    """check_params' refusals and the two NULL outputs; nothing is launched."""
    P = rt.RenderParams()
    L = rt.lib()
    for args in ((None, 8, 8, 64, 64), (C.byref(P), 0, 8, 64, 64), (C.byref(P), 8, -1, 64, 64),
                 (C.byref(P), 65536, 65536, 64, 64), (C.byref(P), 8, 8, None, None)):
        assert L.rt_eye_rays_device(*args, None) == RT_E_INVALID and L.rt_last_error()
    P.shading_mode = 3
    assert L.rt_eye_rays_device(C.byref(P), 8, 8, 64, 64, None) == RT_E_INVALID


def test_c_user_compiles(tmp_path):
    src = ('#include "rtamd.h"\n'
           "int frame(rt_scene *s, const rt_render_params *p, float *o, float *d, uint32_t *c, float *t, void *st) {\n"
           "  rt_ray_batch b = {0};\n"
           "  int rc = rt_eye_rays_device(p, 64, 48, o, d, st);\n"
           "  if (rc) return rc;\n"
           "  b.n = 64 * 48; b.d_origin = o; b.d_dir = d; b.tnear = 0.01f; b.tfar = 100.0f; b.d_t = t;\n"
           "  rc = rt_shade_rays_device(s, &b, p, c, RT_SHADE_CLEAR, st);\n"
           "  if (rc) return rc;\n"
           "  b.d_tfar = t; /* a second scene over the first: tPrev */\n"
           "  return rt_shade_rays_device(s, &b, p, c, 0u, st);\n"
           "}\n"
           "int main(void){return rt_abi_version();}\n")
    _compile(tmp_path, ("a.c", src), "gcc", ["-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic"])


def test_cpp_shade_device_compiles(tmp_path):
    src = ('#include "rtamd.hpp"\n'
           "void frame(const rtamd::InstancedScene &g, const rtamd::BVHBuilder &m, const rt_render_params &p,\n"
           "           float *o, float *d, uint32_t *c, float *t, void *st) {\n"
           "  rtamd::eyeRaysDevice(p, 64, 48, o, d, st);\n"
           "  rtamd::eyeRaysDevice(p, 64, 48, nullptr, d);\n"
           "  rt_ray_batch b{};\n"
           "  b.n = 64 * 48; b.d_origin = o; b.d_dir = d; b.tnear = 0.01f; b.tfar = 100.0f; b.d_t = t;\n"
           "  g.shadeDevice(b, p, c, RT_SHADE_CLEAR, st);\n"
           "  b.d_tfar = t;\n"
           "  m.shadeDevice(b, p, c, 0u);\n"
           "  m.shadeDevice(b, p, c);\n"
           "}\n"
           "int main(){ return 0; }\n")
    _compile(tmp_path, ("a.cpp", src), "g++", ["-std=c++17", "-Wall", "-Wextra", "-Werror"])
