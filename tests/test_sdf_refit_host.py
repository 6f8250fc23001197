"""The SDF-mesh refit on the host (no GPU): rth::refit_sdf_mesh, through
rtx_sdf_mesh_refit_host, is the definition the device refit (rt_sdf_refit.hip,
test_sdf_refit_gpu.py) is compared with. Here it is pinned to a fresh
rth::prep_sdf_mesh of the moved mesh (pseudonormals and triangle records bit
for bit), to a numpy min/max walk of the tree (the box rule) and to the oracle
(cpuref.sdf_points of the moved mesh).

Deformations are functions of position only (sdf_refit_common.shear), so the
moved mesh has the weld classes of creation; each test asserts that first.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import cpuref
import points_ref as R
import refit_common as RC
import sdf_refit_common as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rtamd.h")
NEW = ("rt_sdf_mesh_create_ex", "rt_sdf_mesh_update_vertices", "rt_sdf_mesh_update_vertices_device",
       "rt_sdf_mesh_get_pseudonormals", "rt_sdf_mesh_device_bytes")
RT_E_INVALID = -1
MESHES = ("one", "nine", "cube", "grid100", "rand100", "grid1500", "rand1500", "spot")


def moved(key):
    v, i = SC.mesh(key)
    w = SC.shear(v)
    assert SC.same_classes(v, w), "the shear changed the weld classes"
    assert not np.array_equal(v, w)
    return v, i, w


def subtree_boxes(nodes, tri):
    """[n_inner, 8, 6] float32: per child the numpy min/max of its subtree's
    corners (xMin xMax yMin yMax zMin zMax), and the mask [n_inner, 8] of the
    slots that hold a child (the rest of the first array is not meaningful)."""
    n = len(nodes)
    words = RC.words(nodes)
    corners = tri.view(np.float32).reshape(-1, 3, 4)[:, :, :3]
    box = np.zeros((n, 8, 6), np.float32)
    used = np.zeros((n, 8), bool)
    for k in range(n - 1, -1, -1):  # children have larger indices
        for c in range(8):
            w = int(words[k, c])
            if w == RC.INVALID:
                continue
            used[k, c] = True
            if w & RC.LEAF:
                first, nt = (w & ~RC.LEAF) >> 3, (w & 7) + 1
                pts = corners[first:first + nt].reshape(-1, 3)
                lo, hi = pts.min(0), pts.max(0)
            else:
                sub = box[w][used[w]]
                lo, hi = sub[:, 0::2].min(0), sub[:, 1::2].max(0)
            box[k, c, 0::2], box[k, c, 1::2] = lo, hi
    return box, used


@pytest.mark.parametrize("key", MESHES)
def test_refit_is_a_fresh_build_of_the_moved_mesh(rt, key):
    v, i, w = moved(key)
    n0, t0, p0 = SC.host_refit(rt, v, i)
    n1, t1, p1 = SC.host_refit(rt, v, i, w)
    nf, tf, pf = SC.host_refit(rt, w, i)
    assert np.array_equal(R.bits(p1), R.bits(pf)), "pseudonormals differ from prep_sdf_mesh of the moved mesh"
    assert np.array_equal(SC.by_id(t1), SC.by_id(tf)), "triangle records differ from the fresh ones"
    assert np.array_equal(np.sort(t1[:, 3]), np.arange(len(i) // 3))
    assert np.array_equal(RC.words(n1), RC.words(n0)), "child words changed"
    assert np.array_equal(t1[:, 3], t0[:, 3]), "leaf order changed"
    assert not np.array_equal(R.bits(p1), R.bits(p0))
    # the w slots of the records and of the pseudonormals stay 0
    assert not t1[:, 7].any() and not t1[:, 11].any() and not R.bits(p1[:, :, 3]).any()


@pytest.mark.parametrize("key", MESHES)
def test_box_rule(rt, key):
    """Every child box is the exact min/max of its subtree's divided corners:
    by value (a zero may carry either sign), refitted and built."""
    v, i, w = moved(key)
    for nodes, tri in (SC.host_refit(rt, v, i, w)[:2], SC.host_refit(rt, v, i)[:2]):
        want, used = subtree_boxes(nodes, tri)
        got = RC.boxes(nodes)
        assert np.array_equal(got[used], want[used])
        assert np.all(np.isposinf(got[~used])), "an empty slot lost its +inf box"
    if key == "one":
        assert len(nodes) == 0  # the root is the leaf


@pytest.mark.parametrize("key", MESHES + SC.HAND_MADE)
def test_identity_refit(rt, key):
    v, i = SC.mesh(key)
    n0, t0, p0 = SC.host_refit(rt, v, i)
    n1, t1, p1 = SC.host_refit(rt, v, i, v)
    assert np.array_equal(t1, t0) and np.array_equal(R.bits(p1), R.bits(p0))
    assert np.array_equal(RC.words(n1), RC.words(n0))
    assert np.array_equal(RC.boxes(n1), RC.boxes(n0))  # by value


@pytest.mark.parametrize("key", SC.HAND_MADE)
def test_hand_made_meshes(rt, key):
    v, i, w = moved(key)
    _, t1, p1 = SC.host_refit(rt, v, i, w)
    _, tf, pf = SC.host_refit(rt, w, i)
    assert np.array_equal(R.bits(p1), R.bits(pf)) and np.array_equal(SC.by_id(t1), SC.by_id(tf))
    assert np.isfinite(p1).all()
    a, b, c = R.corners(w, i)
    if key == "zero_area":
        for t in (1, 2):  # collinear, and a point: no face normal, no contribution to any sum
            assert not np.cross(b[t] - a[t], c[t] - a[t]).any()
            assert not p1[t, 6].any()
            assert not p1[t, 3:6, :3].any() and not p1[t, :3, :3].any()
        assert p1[0, 6, :3].any() and p1[3, 6, :3].any()
    if key == "welded_corner":
        # triangle 1 = (1, 1, 2): zero area; its edges ac and bc are one welded edge, shared with triangle 0's bc
        assert not p1[1, 6].any()
        assert np.array_equal(R.bits(p1[1, 4]), R.bits(p1[1, 5])) and np.array_equal(R.bits(p1[1, 4]), R.bits(p1[0, 5]))
        assert np.array_equal(R.bits(p1[1, 0]), R.bits(p1[1, 1])) and np.array_equal(R.bits(p1[1, 0]), R.bits(p1[0, 1]))
        # triangle 2 = (3, 4, 5) with 3 and 4 on one position
        assert np.array_equal(R.bits(p1[2, 0]), R.bits(p1[2, 1])) and np.array_equal(R.bits(p1[2, 4]), R.bits(p1[2, 5]))
    if key == "three_fan":
        # the shared edge: the double sum of the three face normals in triangle order, rounded once
        e = (p1[0, 6, :3].astype(np.float64) + p1[1, 6, :3]) + p1[2, 6, :3]
        for t, f in ((0, 3), (1, 3), (2, 3)):
            assert np.array_equal(R.bits(p1[t, f, :3]), R.bits(e.astype(np.float32)))
        assert np.array_equal(R.bits(p1[0, 0]), R.bits(p1[1, 1])) and np.array_equal(R.bits(p1[0, 0]), R.bits(p1[2, 0]))
    if key == "boundary":
        # a boundary edge carries its one face normal; the inner edge (1, 2) the sum of both
        assert np.array_equal(R.bits(p1[0, 3]), R.bits(p1[0, 6])) and np.array_equal(R.bits(p1[0, 4]), R.bits(p1[0, 6]))
        assert np.array_equal(R.bits(p1[1, 5]), R.bits(p1[1, 6]))
        e = (p1[0, 6, :3].astype(np.float64) + p1[1, 6, :3]).astype(np.float32)
        assert np.array_equal(R.bits(p1[0, 5, :3]), R.bits(e)) and np.array_equal(R.bits(p1[1, 3, :3]), R.bits(e))


@pytest.mark.parametrize("name,n", [("cube.obj", 100), ("spot.obj", 100)])
def test_signed_distance_is_the_oracles(rt, ref, name, n):
    """Brute-force winner (points_ref) + the refitted pseudonormal of its
    feature = cpuref.sdf_points of the moved mesh, bit for bit."""
    key = name.split(".")[0]
    v, i, w = moved(key)
    p = np.concatenate([R.points(name, n, 11), SC.shear(R.points(name, n // 2, 12))])
    _, _, pn = SC.host_refit(rt, v, i, w)
    bf = R.brute_force(w, i, p)
    got = SC.signed(bf, p, pn)
    want = cpuref.sdf_points(w, i, p, 16)
    assert (want < 0).any() and (want > 0).any()
    assert np.array_equal(R.bits(got), R.bits(want))


def test_header_and_bindings(rt, tmp_path):
    from rtamd import _lib
    text = open(HEADER).read()
    L = rt.lib()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, text), f"{name} is not in rtamd.h"
        assert name in _lib.EXPORTED and hasattr(L, name)
    for name in ("rtx_sdf_mesh_refit_host", "rtx_sdf_mesh_download"):
        assert hasattr(L, name) and not re.search(r"\b%s\b" % name, text)
    assert re.search(r"#define\s+RTAMD_ABI_VERSION\s+8\b", text) and L.rt_abi_version() == 8
    assert len(re.findall(r"#define\s+RT_MESH_DYNAMIC\b", text)) == 1 and _lib.RT_MESH_DYNAMIC == 1
    assert _lib._SIGS["rt_sdf_mesh_device_bytes"][0] is _lib.C.c_int64
    src = tmp_path / "use.c"
    src.write_text('#include "rtamd.h"\n'
                   "int move(rt_sdf_mesh **m, const float *v, int64_t nv, const uint32_t *i, int64_t ni, void *stream,\n"
                   "         float *pn) {\n"
                   "  int rc = rt_sdf_mesh_create_ex(v, nv, i, ni, RT_MESH_DYNAMIC, m);\n"
                   "  if (!rc) rc = rt_sdf_mesh_update_vertices(*m, v, nv);\n"
                   "  if (!rc) rc = rt_sdf_mesh_update_vertices_device(*m, v, nv, stream);\n"
                   "  if (!rc) rc = rt_sdf_mesh_get_pseudonormals(*m, pn, ni / 3);\n"
                   "  return rc ? rc : (int)(rt_sdf_mesh_device_bytes(*m) > 0);\n"
                   "}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.dirname(HEADER), "-c", str(src),
                    "-o", str(tmp_path / "use.o")], check=True)


def test_null_and_flag_refusals_need_no_device(rt):
    """The argument checks that come before any device call."""
    import ctypes as C
    L = rt.lib()
    v, i = SC.mesh("one")
    h = C.c_void_p()
    for flags in (2, 3, 0x80000000):
        assert L.rt_sdf_mesh_create_ex(RC._p(v), len(v), RC._p(i), len(i), flags, C.byref(h)) == RT_E_INVALID
        assert not h.value and L.rt_last_error()
    assert L.rt_sdf_mesh_update_vertices(None, RC._p(v), len(v)) == RT_E_INVALID
    assert L.rt_sdf_mesh_update_vertices_device(None, RC._p(v), len(v), None) == RT_E_INVALID
    assert L.rt_sdf_mesh_get_pseudonormals(None, RC._p(v), 1) == RT_E_INVALID
    assert L.rt_sdf_mesh_device_bytes(None) == RT_E_INVALID
