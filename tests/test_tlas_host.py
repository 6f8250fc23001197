"""Instanced scenes with a top-level tree, host side (RT_INSTANCED_TLAS,
include/rtamd.h): rt_instance_world_box and the box test against the numpy
restatement of tlas_common, bitwise; the kernel's cursor walk
(rtx_tlas_candidates) against brute force over all leaves; and the new
definition against the flat list's, reference against reference. No GPU.
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import instances_common as IC
import tlas_common as TC
from conftest import ROOT
from test_instances_host import _exact_cases

F = np.float32
PAIRS = [(0.01, 100.0), (-5.0, 100.0), (0.5, 2.0)]  # tests/test_instances_gpu.py's intervals
N = 4096


def _p(a):
    return C.c_void_p(a.ctypes.data)


def _bits(a):
    return np.asarray(a, F).view(np.uint32)


def _lib_pass(rt, b, o, d, tn, tf):
    b, o, d = (np.ascontiguousarray(a, F) for a in (b, o, d))
    return rt.lib().rtx_tlas_box_pass(_p(b), _p(o), _p(d), float(tn), float(tf))


def _lib_tree(rt, leaves):
    leaves = np.ascontiguousarray(leaves, F).reshape(-1, 6)
    P = TC.leaf_count(len(leaves))
    nodes = np.full((2 * P, 8), 7.0, F)
    assert rt.lib().rtx_tlas_build_host(_p(leaves), len(leaves), _p(nodes)) == 0
    return nodes


def _lib_candidates(rt, nodes8, o, d, tn, tfs):
    P = len(nodes8) // 2
    o, d, tfs = (np.ascontiguousarray(a, F) for a in (o, d, tfs))
    out = np.full(P + 1, -7, np.int32)
    k = rt.lib().rtx_tlas_candidates(_p(nodes8), P, _p(o), _p(d), float(tn), _p(tfs), len(tfs), _p(out), P)
    assert 0 <= k <= P, rt.lib().rt_last_error()
    assert out[P] == -7 and (out[k:P] == -7).all()
    return out[:k].tolist()


def test_abi_is_additive(rt):
    from rtamd import _lib
    for name in ("rt_scene_create_instanced_ex", "rt_instance_world_box", "rt_scene_get_tlas"):
        assert name in rt.EXPORTED and hasattr(rt.lib(), name)
    for name in ("rtx_set_tlas_uniform_min", "rtx_tlas_candidates", "rtx_tlas_box_pass", "rtx_tlas_build_host"):
        assert hasattr(rt.lib(), name)
    src = open(os.path.join(ROOT, "include", "rtamd.h")).read()
    assert re.search(r"#define RT_INSTANCED_TLAS 1u", src) and _lib.RT_INSTANCED_TLAS == 1
    assert callable(rt.morton_order) and callable(rt.instance_world_box)


@pytest.mark.parametrize("what,A,b,Ai,bi", _exact_cases(), ids=lambda v: v if isinstance(v, str) else "")
def test_world_box_exact_cases(rt, what, A, b, Ai, bi):
    """The exact matrices of test_instances_host.py on two object boxes: the
    library's box is the numpy restatement's, bit for bit, and holds the
    corners computed in float64."""
    x = IC.affine(A, b)
    for ob in (F([-1, -1, -1, 1, 1, 1]), F([-0.5, 0.25, -3, 2.5, 0.75, -1])):
        got = rt.instance_world_box(x, ob)
        assert np.array_equal(_bits(got), _bits(TC.world_box(x, ob))), what
        corners = np.array([[ob[3 * ((c >> a) & 1) + a] for a in range(3)] for c in range(8)], np.float64)
        w = corners @ x[:, :3].astype(np.float64).T + x[:, 3].astype(np.float64)
        assert (got[:3] < w.min(0)).all() and (got[3:] > w.max(0)).all(), what


def test_world_box_random(rt):
    """200 matrices R diag(s) + b (test_affine_inverse_inverts' recipe) on
    random boxes: bitwise the restatement; the pad is 2^-16 of the box's scale."""
    rng = np.random.default_rng(18)
    for k in range(200):
        x = IC.affine(IC.rot(100 + k) @ np.diag(rng.uniform(0.5, 2.0, 3)), rng.uniform(-3, 3, 3))
        lo = rng.uniform(-2, 1, 3)
        ob = np.concatenate([lo, lo + rng.uniform(0.01, 3, 3)]).astype(F)
        got, want = rt.instance_world_box(x, ob), TC.world_box(x, ob)
        assert np.array_equal(_bits(got), _bits(want)), k
        assert (got[:3] < got[3:]).all() and np.isfinite(got).all()
    assert rt.lib().rt_instance_world_box(None, None, None) == -1


def test_box_pass_matches_restatement_and_special_boxes(rt):
    """rtx_tlas_box_pass against the numpy restatement on random boxes and
    rays (an eighth of them axis-aligned: a non-finite 1/d passes); the empty
    box never passes, not even for a ray with a zero direction component; the
    unbounded box passes every ray whose interval is not empty."""
    o, d = IC.random_rays(512, 7)
    rng = np.random.default_rng(8)
    n_pass = 0
    for tn, tf in PAIRS + [(0.5, 0.25)]:
        for k in range(6):
            lo = rng.uniform(-2, 1, 3)
            b = np.concatenate([lo, lo + rng.uniform(0.1, 2.5, 3)]).astype(F)
            want = TC.box_pass(b, o, d, tn, tf)
            got = np.array([_lib_pass(rt, b, o[i], d[i], tn, tf) for i in range(len(o))], bool)
            assert np.array_equal(got, want), (tn, tf, k)
            n_pass += int(want.sum())
            zero = (d == 0).any(axis=1)
            assert zero.sum() >= 32 and want[zero].all()
    assert n_pass > 500
    for i in range(len(o)):
        assert _lib_pass(rt, TC.EMPTY, o[i], d[i], 0.01, 100.0) == 0
        assert _lib_pass(rt, TC.UNBOUNDED, o[i], d[i], 0.01, 100.0) == 1
    assert not TC.box_pass(TC.EMPTY, o, d, 0.01, 100.0).any() and TC.box_pass(TC.UNBOUNDED, o, d, 0.01, 100.0).all()
    gen = ~(d == 0).any(axis=1)
    assert not TC.box_pass(TC.UNBOUNDED, o[gen], d[gen], 0.5, 0.25).any()  # tNear > tFar: the slab test's own rule


def _leaf_set(k, seed):
    """k leaf boxes on a jittered lattice in index order; every seventh empty."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(k ** (1 / 3)))
    leaves = np.tile(TC.EMPTY, (k, 1))
    for i in range(k):
        if i % 7 == 3:
            continue
        c = np.float64([i % side, (i // side) % side, i // (side * side)]) * 1.5 - side * 0.75 + rng.uniform(-0.2, 0.2, 3)
        h = rng.uniform(0.2, 0.7, 3)
        leaves[i] = np.concatenate([c - h, c + h]).astype(F)
    return leaves


def _brute(leaves, o, d, tn, tfs):
    out = []
    for i in range(len(leaves)):
        tf = tfs[min(len(out), len(tfs) - 1)]
        if TC.box_pass(leaves[i], o[None], d[None], tn, tf)[0]:
            out.append(i)
    return out


@pytest.mark.parametrize("k", [1, 2, 3, 5, 64, 70, 257])
def test_cursor_walk_against_brute_force(rt, k):
    """The host tree equals the numpy union; the walk's candidates are the
    leaves that pass, in index order: under a fixed tFar, for rays with a zero
    direction component (every non-empty leaf) and under a tFar that shrinks
    after every candidate."""
    leaves = _leaf_set(k, 40 + k)
    nodes8 = _lib_tree(rt, leaves)
    P = TC.leaf_count(k)
    assert np.array_equal(_bits(nodes8[:, :6]), _bits(TC.tree(leaves))) and not nodes8[:, 6:].any()
    assert np.array_equal(_bits(nodes8[P + k:, :6]), _bits(np.tile(TC.EMPTY, (P - k, 1))))
    o, d = IC.random_rays(96, 50 + k, inside_frac=0.3)
    o = (o * F(1.5)).astype(F)
    non_empty = [i for i in range(k) if leaves[i, 0] <= leaves[i, 3]]
    total = 0
    for i in range(len(o)):
        got = _lib_candidates(rt, nodes8, o[i], d[i], 0.01, [100.0])
        assert got == _brute(leaves, o[i], d[i], 0.01, [100.0]), (k, i)
        if (d[i] == 0).any():
            assert got == non_empty
        else:
            total += len(got)
        # tf_i = min(best, tFar) as best improves: from 6 down to 0.3
        tfs = np.linspace(6.0, 0.3, 9).astype(F)
        assert _lib_candidates(rt, nodes8, o[i], d[i], 0.01, tfs) == _brute(leaves, o[i], d[i], 0.01, tfs), (k, i)
    assert (d == 0).any(axis=1).sum() >= 8
    if k >= 64:  # the tree prunes: general rays meet a small part of the leaves
        assert 0 < total < 0.25 * len(non_empty) * len(o)


# ---- the new definition against the flat list's, reference against reference --
def _scene_defs(name):
    if name == "130":
        return TC.scene130()
    from test_instances_gpu import DEFS
    return DEFS[name]


@functools.lru_cache(maxsize=None)
def _host_scene(rt, name):
    """(refs, blas, flags, M, wbox) of a scene from host data alone: M by
    rt_affine_inverse, the root box of a BLAS taken as its vertex box (a
    one-triangle mesh is a leaf root: unbounded)."""
    names, inst = _scene_defs(name)
    refs = {k: IC.ref_mesh(m) for k, m in enumerate(names)}
    boxes = [None if m == "tri" else TC.vertex_box(IC.mesh(m)[0]) for m in names]
    blas = [t[0] for t in inst]
    flags = [t[2] for t in inst]
    M = np.stack([rt.affine_inverse(t[1]) for t in inst])
    wbox = TC.leaf_boxes([t[1] for t in inst], blas, flags, boxes)
    return refs, blas, flags, M, wbox


@pytest.mark.parametrize("name", ["b", "c", "d", "130"])
@pytest.mark.parametrize("tn,tf", PAIRS)
def test_tlas_definition_against_flat_definition(rt, ref, name, tn, tf):
    """compose_tlas against compose on 4096 random rays: 0 rays differ in any
    output. (The world-box test is part of the definition; that it changes no
    answer here is a property of the pad, measured, not proven.)"""
    refs, blas, flags, M, wbox = _host_scene(rt, name)
    o, d = IC.random_rays(N, 20261014)
    flat = IC.compose(refs, blas, flags, M, o, d, tn, tf)
    new = TC.compose_tlas(refs, blas, flags, M, wbox, o, d, tn, tf)
    differ = np.zeros(N, bool)
    for a, b in zip(flat, new[:4]):
        differ |= (_bits(a) != _bits(b)).reshape(N, -1).any(axis=1) if a.dtype == F else (a != b).reshape(N, -1).any(axis=1)
    k = sum(1 for f in flags if not f & IC.DISABLED)
    print(f"{name} [{tn}, {tf}]: {int(differ.sum())} rays differ; BLAS traversals per ray {k} -> {new[4].mean():.2f}; "
          f"{int(flat[0].sum())} hits")
    assert int(flat[0].sum()) > 100
    assert int(differ.sum()) == 0
    assert np.array_equal(TC.any_hit_tlas(refs, blas, flags, M, wbox, o, d, tn, tf), new[0])
    if name in ("d", "130"):
        assert new[4].mean() < 0.35 * k


def test_morton_order(rt):
    """A permutation; neighbours on the curve are neighbours in space: the
    mean step between consecutive centres drops well below a random order's."""
    rng = np.random.default_rng(3)
    c = rng.uniform(-4, 4, (512, 3))
    p = rt.morton_order(c)
    assert sorted(p.tolist()) == list(range(512))
    step = lambda q: np.linalg.norm(np.diff(c[q], axis=0), axis=1).mean()
    assert step(p) < 0.35 * step(np.arange(512))
    assert rt.morton_order(c[:1]).tolist() == [0]
