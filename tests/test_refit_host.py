"""The BVH8 refit, what can be checked without a GPU: the host restatement
rth::refit_bvh8 (through rtx_bvh_refit_host), which defines the evaluation
order the device kernels reproduce, the new symbols, and the headers.

Refit rules (include/rtamd.h, rt_scene_update_vertices*): topology and
triangle order stay, every GTri is rewritten from the new vertices, every child
box is the exact min/max of its subtree.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import refit_common as R
from conftest import ROOT

INCLUDE = os.path.join(ROOT, "include")
RT_E_INVALID = -1
NEW = ("rt_scene_create_mesh_ex", "rt_scene_update_vertices", "rt_scene_update_vertices_device")


# ------------------------------------------------------------ refit rules --
@pytest.mark.parametrize("ntri", [1, 9, 100, 1500])
@pytest.mark.parametrize("mode", ["signed0", "grid", "flat", "rand"])
def test_identity(rt, mode, ntri):
    """A refit from the unchanged vertices: triangles and child words bitwise,
    boxes as float values. The builder computes a child's box before deeper
    splits re-sort that child's range, so on ties between -0 and +0 its
    leftmost triangle can be another one than the refit's: bits may differ
    there, and only there."""
    v, i = R.edge(mode, ntri)
    bn, bt = R.host_refit(rt, v, i)
    rn, rt_ = R.host_refit(rt, v, i, v)
    assert np.array_equal(bt, rt_)
    assert np.array_equal(R.words(bn), R.words(rn))
    assert np.array_equal(R.boxes(bn), R.boxes(rn))  # by value: -0 == +0, inf == inf
    d = bn[:, :48] != rn[:, :48]
    assert ((bn[:, :48][d] | rn[:, :48][d]) == 0x80000000).all(), "bits differ in something else than a zero's sign"
    if (mode, ntri) == ("signed0", 1500):
        # the finding itself: comparisons against BUILT boxes are by value
        assert d.any(), "no zero-sign difference left: has the builder's or the refit's order changed?"
    if mode != "signed0":
        assert not d.any()


@pytest.mark.parametrize("mode,ntri", [("grid", 100), ("grid", 1500), ("signed0", 1500)])
def test_exact_translation_equals_fresh_build(rt, mode, ntri):
    """(8, -16, 4) is added exactly and no coordinate lands on zero: the fresh
    build of the moved mesh has the same topology and order, and the refit of
    the old tree is that tree bit for bit."""
    v, i = R.edge(mode, ntri)
    w = R.translate(v)
    fn, ft = R.host_refit(rt, w, i)
    rn, rt_ = R.host_refit(rt, v, i, w)
    assert np.array_equal(ft, rt_)
    assert np.array_equal(fn, rn)


def _smin(a, b):  # std::min(a, b)
    return b if b < a else a


def _smax(a, b):  # std::max(a, b)
    return b if a < b else a


def _numpy_refit(nodes, tris, w, idx):
    """The refit in the defined order on the device layout: nodes from the last
    to the first; per child slot, a leaf grows from the empty box over its
    triangles in slot order and vertices 0, 1, 2, an inner child over that
    node's child boxes 0 .. nchild-1."""
    nodes, tris = nodes.copy(), tris.copy()
    box = R.boxes(nodes)  # a view: writes land in nodes
    wd = R.words(nodes)
    tf = tris.view(np.float32)
    inf = np.float32(np.inf)
    for n in range(len(nodes) - 1, -1, -1):
        for c in range(8):
            word = int(wd[n, c])
            if word == R.INVALID:
                continue
            mn, mx = [inf] * 3, [-inf] * 3
            if word & R.LEAF:
                first, nt = (word & 0x7FFFFFFF) >> 3, (word & 7) + 1
                for s in range(first, first + nt):
                    p = [w[idx[3 * int(tris[s, 3]) + j]] for j in range(3)]
                    p = [[q[0] / q[3], q[1] / q[3], q[2] / q[3]] for q in p]  # float32 / float32
                    for q in p:
                        for k in range(3):
                            mn[k], mx[k] = _smin(mn[k], q[k]), _smax(mx[k], q[k])
                    for k in range(3):
                        tf[s, k] = p[0][k]
                        tf[s, 4 + k] = p[1][k] - p[0][k]
                        tf[s, 8 + k] = p[2][k] - p[0][k]
            else:
                for cc in range(8):
                    if int(wd[word, cc]) == R.INVALID:
                        continue
                    for k in range(3):
                        mn[k], mx[k] = _smin(mn[k], box[word, cc, 2 * k]), _smax(mx[k], box[word, cc, 2 * k + 1])
            for k in range(3):
                box[n, c, 2 * k], box[n, c, 2 * k + 1] = mn[k], mx[k]
    return nodes, tris


def _subtree_slots(nodes, word, out):
    if word & R.LEAF:
        first, nt = (word & 0x7FFFFFFF) >> 3, (word & 7) + 1
        out.extend(range(first, first + nt))
    else:
        for cw in R.words(nodes)[word]:
            if int(cw) != R.INVALID:
                _subtree_slots(nodes, int(cw), out)


def test_general_deformation(rt):
    v, i = R.edge("rand", 1500)
    w = R.deform(v)
    bn, bt = R.host_refit(rt, v, i)
    rn, rt_ = R.host_refit(rt, v, i, w)
    # (a) the restatement in numpy, bitwise
    en, et = _numpy_refit(bn, bt, w, i)
    assert np.array_equal(et, rt_)
    assert np.array_equal(en, rn)
    # (b) the plain property: every child box is the min/max of its subtree's
    # vertices, by value; topology, order and empty slots untouched
    assert np.array_equal(R.words(bn), R.words(rn)) and np.array_equal(bt[:, 3], rt_[:, 3])
    p = (w[:, :3] / w[:, 3:4]).astype(np.float32)
    box, wd = R.boxes(rn), R.words(rn)
    seen = 0
    for n in range(len(rn)):
        for c in range(8):
            if int(wd[n, c]) == R.INVALID:
                assert np.isposinf(box[n, c]).all()
                continue
            slots = []
            _subtree_slots(rn, int(wd[n, c]), slots)
            vid = i.reshape(-1, 3)[rt_[slots, 3]].ravel()
            assert np.array_equal(box[n, c, 0::2], p[vid].min(0)) and np.array_equal(box[n, c, 1::2], p[vid].max(0))
            seen += n == 0 and len(slots)
    assert seen == 1500  # the root's children cover every triangle once
    # and the triangles are the deformed ones
    tf = rt_.view(np.float32)
    tri = p[i.reshape(-1, 3)[rt_[:, 3]]]
    assert np.array_equal(tf[:, 0:3], tri[:, 0]) and np.array_equal(tf[:, 4:7], tri[:, 1] - tri[:, 0])
    assert np.array_equal(tf[:, 8:11], tri[:, 2] - tri[:, 0])
    assert not rt_[:, 7].any() and not rt_[:, 11].any()


def test_root_leaf_mesh_has_no_nodes(rt):
    v, i = R.edge("rand", 1)
    w = R.deform(v)
    rn, rt_ = R.host_refit(rt, v, i, w)
    assert rn.shape == (0, 56) and rt_.shape == (1, 12)
    p = (w[:, :3] / w[:, 3:4]).astype(np.float32)
    assert np.array_equal(rt_.view(np.float32)[0, 0:3], p[0]) and rt_[0, 3] == 0


# ------------------------------------------------------ symbols and errors --
def test_symbols_exported_and_declared(rt):
    from rtamd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", rt.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    for name in NEW + ("rtx_scene_mesh_download", "rtx_scene_mesh_constants", "rtx_bvh_refit_host"):
        assert re.search(rf"\bT {name}$", out, flags=re.M), name
    for name in NEW:
        assert name in rt.EXPORTED and name in _lib._SIGS
    assert _lib._SIGS["rt_scene_create_mesh_ex"][1][4] is C.c_uint32
    assert len(_lib._SIGS["rt_scene_update_vertices"][1]) == 3
    assert len(_lib._SIGS["rt_scene_update_vertices_device"][1]) == 4
    assert _lib.RT_MESH_DYNAMIC == 1
    assert re.search(r"#define RT_MESH_DYNAMIC 1u", open(os.path.join(INCLUDE, "rtamd.h")).read())
    assert rt.lib().rt_abi_version() == 8  # additive: the ABI version stays


def test_null_arguments_rejected(rt):
    """The scene-independent invalid calls (a scene needs a GPU to exist)."""
    L = rt.lib()
    buf = np.zeros((3, 4), np.float32)
    p = C.c_void_p(buf.ctypes.data)
    for rc in (L.rt_scene_update_vertices(None, p, 3), L.rt_scene_update_vertices_device(None, p, 3, None)):
        msg = L.rt_last_error()
        assert rc == RT_E_INVALID and msg and b"scene" in msg
    h = C.c_void_p()
    rc = L.rt_scene_create_mesh_ex(None, 3, None, 3, 1, C.byref(h))
    assert rc == RT_E_INVALID and L.rt_last_error()
    idx = np.arange(3, dtype=np.uint32)
    rc = L.rt_scene_create_mesh_ex(p, 3, C.c_void_p(idx.ctypes.data), 3, 2, C.byref(h))  # an unknown flag
    assert rc == RT_E_INVALID and b"flags" in L.rt_last_error()


def _compile(tmp_path, src, compiler, flags):
    f = tmp_path / src[0]
    f.write_text(src[1])
    r = subprocess.run([compiler, *flags, "-I", INCLUDE, "-fsyntax-only", str(f)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_c_user_compiles(tmp_path):
    src = ('#include "rtamd.h"\n'
           "int step(const float *v, int64_t nv, const uint32_t *idx, int64_t ni, const float *d_v, void *stream) {\n"
           "  rt_scene *s = 0;\n"
           "  int rc = rt_scene_create_mesh_ex(v, nv, idx, ni, RT_MESH_DYNAMIC, &s);\n"
           "  if (!rc) rc = rt_scene_update_vertices(s, v, nv);\n"
           "  if (!rc) rc = rt_scene_update_vertices_device(s, d_v, nv, stream);\n"
           "  rt_scene_destroy(s);\n"
           "  return rc;\n"
           "}\n"
           "int main(void){return rt_abi_version();}\n")
    _compile(tmp_path, ("a.c", src), "gcc", ["-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic"])


def test_cpp_user_compiles(tmp_path):
    src = ('#include "rtamd.hpp"\n'
           "void step(const rtamd::SimpleMesh &m, const float *d_v, void *st) {\n"
           "  rtamd::BVHBuilder b;\n"
           "  b.perform(m, true);\n"
           "  b.updateVertices(m.vPos4f.data(), (int64_t)(m.vPos4f.size() / 4));\n"
           "  b.updateVerticesDevice(d_v, (int64_t)(m.vPos4f.size() / 4), st);\n"
           "  b.updateVerticesDevice(d_v, (int64_t)(m.vPos4f.size() / 4));\n"
           "  rtamd::BVHBuilder c;\n"
           "  c.perform(m);\n"
           "}\n"
           "int main(){ return 0; }\n")
    _compile(tmp_path, ("a.cpp", src), "g++", ["-std=c++17", "-Wall", "-Wextra", "-Werror"])
