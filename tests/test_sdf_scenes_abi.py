"""SDF scenes that follow a deforming mesh on the device
(rt_scene_update_grid_device, rt_scene_create_octree_dynamic,
rt_sdf_mesh_octree_device, rt_scene_octree_status, rt_scene_get_octree): what
can be checked without a GPU. The symbols are exported, declared and bound,
the Python methods exist, a C user compiles, and the calls that need no device
are refused with a message. The values are checked on the GPU
(test_sdf_octree_device_gpu.py, test_sdf_grid_update_gpu.py).
"""
import ctypes as C
import os
import re
import subprocess

from conftest import ROOT

INCLUDE = os.path.join(ROOT, "include")
RT_E_INVALID = -1
NAMES = ("rt_scene_update_grid_device", "rt_scene_create_octree_dynamic", "rt_sdf_mesh_octree_device",
         "rt_scene_octree_status", "rt_scene_get_octree")


def test_symbols_exported_declared_and_bound(rt):
    from rtamd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", rt.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    header = open(os.path.join(INCLUDE, "rtamd.h")).read()
    for name in NAMES:
        assert re.search(rf"\bT {name}$", out, flags=re.M), name
        assert name in rt.EXPORTED
        assert re.search(rf"^int {name}\(", header, flags=re.M), name
        assert _lib._SIGS[name][0] is C.c_int
    assert re.search(r"\bT rtx_scene_octree_words$", out, flags=re.M)
    assert "rtx_scene_octree_words" not in header and "rtx_scene_octree_words" in _lib._XSIGS
    assert [len(_lib._SIGS[n][1]) for n in NAMES] == [3, 3, 3, 3, 3]
    assert _lib._SIGS["rt_scene_create_octree_dynamic"][1][:2] == [C.c_int32, C.c_int64]
    assert rt.lib().rt_abi_version() == 8  # additive: the ABI version stays


def test_python_methods_exist(rt):
    from rtamd import torch_rays
    assert callable(rt.SDFGrid.update_device)
    assert isinstance(rt.SDFOctree.__dict__["dynamic"], classmethod)
    for f in ("status", "nodes"):
        assert callable(getattr(rt.SDFOctree, f))
    assert callable(rt.SDFMesh.octree_device)
    assert callable(torch_rays.update_sdf_grid) and callable(torch_rays.update_sdf_octree)


def test_c_user_compiles(tmp_path):
    src = ('#include "rtamd.h"\n'
           "int frame(rt_sdf_mesh *m, rt_scene *grid, rt_scene **oct, float *d_values, void *stream) {\n"
           "  const uint32_t size[3] = {16, 16, 16};\n"
           "  int64_t count = 0;\n"
           "  int32_t overflow = 0;\n"
           "  int rc = rt_sdf_mesh_grid_device(m, size, d_values, stream);\n"
           "  rc += rt_scene_update_grid_device(grid, d_values, stream);\n"
           "  rc += rt_scene_create_octree_dynamic(6, 40000, oct);\n"
           "  rc += rt_sdf_mesh_octree_device(m, *oct, stream);\n"
           "  rc += rt_scene_octree_status(*oct, &count, &overflow);\n"
           "  rc += rt_scene_get_octree(*oct, &count, 0);\n"
           "  return rc;\n"
           "}\n"
           "int main(void){return rt_abi_version();}\n")
    f = tmp_path / "a.c"
    f.write_text(src)
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", INCLUDE, "-fsyntax-only",
                        str(f)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_create_dynamic_refuses_bad_arguments_without_a_device(rt):
    L = rt.lib()
    h = C.c_void_p()
    for depth, cap in ((-1, 100), (13, 100), (4, 0), (4, -5), (4, 1 << 32)):
        rc = L.rt_scene_create_octree_dynamic(depth, cap, C.byref(h))
        assert rc == RT_E_INVALID and L.rt_last_error(), (depth, cap)
        assert b"depth" in L.rt_last_error() or b"max_nodes" in L.rt_last_error()
        assert not h.value
    rc = L.rt_scene_create_octree_dynamic(4, 100, None)
    assert rc == RT_E_INVALID and b"out" in L.rt_last_error()


def test_null_handles_refused(rt):
    L = rt.lib()
    fake = C.cast(C.create_string_buffer(65536), C.c_void_p)
    assert L.rt_scene_update_grid_device(None, 64, None) == RT_E_INVALID and b"scene" in L.rt_last_error()
    # (a scene pointer is not dereferenced before the values are checked)
    assert L.rt_scene_update_grid_device(fake, None, None) == RT_E_INVALID and b"values" in L.rt_last_error()
    assert L.rt_sdf_mesh_octree_device(None, fake, None) == RT_E_INVALID and b"mesh" in L.rt_last_error()
    assert L.rt_sdf_mesh_octree_device(fake, None, None) == RT_E_INVALID and b"scene" in L.rt_last_error()
    n, o = C.c_int64(0), C.c_int32(0)
    assert L.rt_scene_octree_status(None, C.byref(n), C.byref(o)) == RT_E_INVALID and L.rt_last_error()
    assert L.rt_scene_get_octree(None, C.byref(n), None) == RT_E_INVALID and L.rt_last_error()
    assert L.rt_scene_get_octree(fake, None, None) == RT_E_INVALID and b"count" in L.rt_last_error()
