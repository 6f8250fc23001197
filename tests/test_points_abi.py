"""rt_sdf_mesh_points_device / rt_sdf_mesh_grid_device (point queries on device
buffers): what can be checked without a GPU. The symbols are exported and
bound, the ctypes rt_point_batch has the layout a C compiler gives the
header's struct, a C user of it compiles, and the calls that need no handle
are rejected with a message. The values are checked on the GPU
(test_points_device.py).
"""
import ctypes as C
import os
import re
import subprocess

from conftest import ROOT

INCLUDE = os.path.join(ROOT, "include")
RT_E_INVALID = -1
FIELDS = ("n", "d_point", "d_radius", "radius", "d_dist", "d_closest", "d_prim", "d_feature")


def test_symbols_exported_and_declared(rt):
    from rtamd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", rt.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    header = open(os.path.join(INCLUDE, "rtamd.h")).read()
    for name in ("rt_sdf_mesh_points_device", "rt_sdf_mesh_grid_device", "rt_sdf_mesh_device"):
        assert re.search(rf"\bT {name}$", out, flags=re.M), name
        assert name in rt.EXPORTED
        assert re.search(rf"^int {name}\(", header, flags=re.M), name
    res, args = _lib._SIGS["rt_sdf_mesh_points_device"]
    assert res is C.c_int and len(args) == 4 and args[1] is C.POINTER(_lib.PointBatch)
    res, args = _lib._SIGS["rt_sdf_mesh_grid_device"]
    assert res is C.c_int and len(args) == 4
    assert _lib.RT_POINTS_UNSIGNED == 1
    assert rt.lib().rt_abi_version() == 8  # additive: the ABI version stays
    for f in ("points_device", "grid_device", "device"):
        assert callable(getattr(rt.SDFMesh, f))


def test_point_batch_layout_matches_a_compiled_probe(tmp_path):
    """sizeof / offsetof of every field as gcc lays the header's struct out."""
    from rtamd import _lib
    assert tuple(f[0] for f in _lib.PointBatch._fields_) == FIELDS
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "rtamd.h"\n'
           "int main(void) {\n"
           '  printf("%zu", sizeof(rt_point_batch));\n' +
           "".join(f'  printf(" %zu %zu", offsetof(rt_point_batch, {f}), sizeof(((rt_point_batch *)0)->{f}));\n'
                   for f in FIELDS) +
           '  printf(" %u\\n", RT_POINTS_UNSIGNED);\n  return 0;\n}\n')
    (tmp_path / "probe.c").write_text(src)
    exe = tmp_path / "probe"
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", INCLUDE, "-o", str(exe), str(tmp_path / "probe.c")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    nums = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert nums[0] == C.sizeof(_lib.PointBatch)
    for k, f in enumerate(FIELDS):
        d = getattr(_lib.PointBatch, f)
        assert (nums[1 + 2 * k], nums[2 + 2 * k]) == (d.offset, d.size), f
    assert nums[-1] == _lib.RT_POINTS_UNSIGNED


def test_c_user_of_point_batch_compiles(tmp_path):
    src = ('#include <math.h>\n#include "rtamd.h"\n'
           "int query(rt_sdf_mesh *m, const float *p, float *dist, int64_t *prim, int32_t *feat, void *stream) {\n"
           "  rt_point_batch b = {0};\n"
           "  b.n = 8; b.d_point = p; b.radius = INFINITY; b.d_dist = dist; b.d_prim = prim; b.d_feature = feat;\n"
           "  return rt_sdf_mesh_points_device(m, &b, RT_POINTS_UNSIGNED, stream);\n"
           "}\n"
           "int grid(rt_sdf_mesh *m, float *values, void *stream) {\n"
           "  const uint32_t size[3] = {16, 16, 16};\n"
           "  return rt_sdf_mesh_grid_device(m, size, values, stream) + rt_sdf_mesh_device(m);\n"
           "}\n"
           "int main(void){return rt_abi_version();}\n")
    f = tmp_path / "a.c"
    f.write_text(src)
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", INCLUDE, "-fsyntax-only",
                        str(f)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_null_handle_and_null_batch_rejected(rt):
    """The handle-independent invalid calls (a handle needs a GPU to exist)."""
    from rtamd import _lib
    L = rt.lib()
    b = _lib.PointBatch(4, 64, None, float("inf"), 64, None, None, None)
    rc = L.rt_sdf_mesh_points_device(None, C.byref(b), 0, None)
    assert rc == RT_E_INVALID and L.rt_last_error()
    rc = L.rt_sdf_mesh_points_device(None, None, 0, None)
    assert rc == RT_E_INVALID and L.rt_last_error()
    # a non-NULL handle pointer is never dereferenced before the batch is checked
    fake = C.create_string_buffer(4096)
    rc = L.rt_sdf_mesh_points_device(C.cast(fake, C.c_void_p), None, 0, None)
    assert rc == RT_E_INVALID and b"batch" in L.rt_last_error()
    size = (C.c_uint32 * 3)(8, 8, 8)
    assert L.rt_sdf_mesh_grid_device(None, size, 64, None) == RT_E_INVALID and L.rt_last_error()
    assert L.rt_sdf_mesh_grid_device(C.cast(fake, C.c_void_p), None, 64, None) == RT_E_INVALID
    assert L.rt_sdf_mesh_grid_device(C.cast(fake, C.c_void_p), size, None, None) == RT_E_INVALID
    assert L.rt_sdf_mesh_device(None) == RT_E_INVALID
