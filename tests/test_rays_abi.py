"""rt_trace_rays_device (ray queries on device buffers): what can be checked
without a GPU. The symbol is exported and bound, the calls that need no scene
are rejected with a message, and the C / C++ headers compile for a user of
rt_ray_batch and IScene::intersectDevice. The traced values are checked on the
GPU (test_rays_device.py).
"""
import ctypes as C
import os
import re
import subprocess

from conftest import ROOT

INCLUDE = os.path.join(ROOT, "include")
RT_E_INVALID = -1


def test_symbol_exported_and_declared(rt):
    from rtamd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", rt.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    assert re.search(r"\bT rt_trace_rays_device$", out, flags=re.M)
    assert "rt_trace_rays_device" in rt.EXPORTED
    res, args = _lib._SIGS["rt_trace_rays_device"]
    assert res is C.c_int and len(args) == 4 and args[1] is C.POINTER(_lib.RayBatch)
    assert _lib.RT_RAYS_ANY_HIT == 1
    assert rt.lib().rt_abi_version() == 8  # additive: the ABI version stays


def test_ray_batch_layout_matches_header():
    """The ctypes struct has the header's fields in the header's order."""
    from rtamd import _lib
    src = open(os.path.join(INCLUDE, "rtamd.h")).read()
    body = re.search(r"typedef struct rt_ray_batch \{(.*?)\} rt_ray_batch;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        names += [w.strip(" *\n") for w in re.sub(r"^\s*(const\s+)?\w+\s", "", decl.strip()).split(",") if w.strip()]
    assert names == [f[0] for f in _lib.RayBatch._fields_]
    assert C.sizeof(_lib.RayBatch) == 80


def _call(rt, scene, batch, flags=0):
    rc = rt.lib().rt_trace_rays_device(scene, batch, flags, None)
    return rc, rt.lib().rt_last_error()


def test_null_scene_and_null_batch_rejected(rt):
    """The scene-independent invalid calls (a scene needs a GPU to exist)."""
    from rtamd import _lib
    b = _lib.RayBatch(4, 64, 64, None, None, 0.01, 100.0, 64, None, None, None)
    rc, msg = _call(rt, None, C.byref(b))
    assert rc == RT_E_INVALID and msg
    rc, msg = _call(rt, None, None)
    assert rc == RT_E_INVALID and msg
    # a non-NULL scene pointer is never dereferenced before the batch is checked
    fake = C.create_string_buffer(4096)
    rc, msg = _call(rt, C.cast(fake, C.c_void_p), None)
    assert rc == RT_E_INVALID and msg and b"batch" in msg


def _compile(tmp_path, src, compiler, flags):
    f = tmp_path / src[0]
    f.write_text(src[1])
    r = subprocess.run([compiler, *flags, "-I", INCLUDE, "-fsyntax-only", str(f)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_c_user_of_ray_batch_compiles(tmp_path):
    src = ('#include "rtamd.h"\n'
           "int trace(rt_scene *s, const float *o, const float *d, int32_t *hit, void *stream) {\n"
           "  rt_ray_batch b = {0};\n"
           "  b.n = 8; b.d_origin = o; b.d_dir = d; b.tnear = 0.01f; b.tfar = 100.0f; b.d_hit = hit;\n"
           "  return rt_trace_rays_device(s, &b, RT_RAYS_ANY_HIT, stream);\n"
           "}\n"
           "int main(void){return rt_abi_version();}\n")
    _compile(tmp_path, ("a.c", src), "gcc", ["-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic"])


def test_cpp_intersect_device_compiles(tmp_path):
    src = ('#include "rtamd.hpp"\n'
           "void trace(const rtamd::SDFGrid &g, const float *o, const float *d, float *t, int64_t *prim, void *st) {\n"
           "  rt_ray_batch b{};\n"
           "  b.n = 8; b.d_origin = o; b.d_dir = d; b.tnear = 0.01f; b.tfar = 100.0f; b.d_t = t; b.d_prim = prim;\n"
           "  g.intersectDevice(b, 0u, st);\n"
           "  g.intersectDevice(b);\n"
           "}\n"
           "int main(){ return 0; }\n")
    _compile(tmp_path, ("a.cpp", src), "g++", ["-std=c++17", "-Wall", "-Wextra", "-Werror"])
