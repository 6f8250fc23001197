"""Shared by test_refit_host.py and test_refit_gpu.py: the meshes, the
deformations, the host restatement (rtx_bvh_refit_host) and views of the device
layout (rt_layout.h).

A tree is a pair (nodes, tris) of uint32 arrays: nodes [n_inner, 56] -- words
0..47 the eight child boxes as float bits (child c at 6c..6c+5: xMin xMax yMin
yMax zMin zMax), words 48..55 the child words; tris [n_tris, 12] -- v0.xyz,
orig_id, e1.xyz, 0, e2.xyz, 0.
"""
import ctypes as C
import functools

import numpy as np

import scenes as S

LEAF = 0x80000000
INVALID = 0xFFFFFFFF
SEED = 20251
SHIFT = np.float32([8.0, -16.0, 4.0])


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


@functools.lru_cache(maxsize=None)
def edge(mode, ntri):
    """(vPos4f, indices) of scenes.edge_mesh: one vertex per corner. The seed
    is the first from SEED + ntri on that the generator accepts ("signed0"
    wants both zero signs present, which a single triangle does not always have)."""
    seed = SEED + ntri
    while True:
        try:
            v = S.edge_mesh(seed, ntri, mode)
            break
        except AssertionError:
            seed += 1
    i = np.arange(3 * ntri, dtype=np.uint32)
    v.setflags(write=False)
    i.setflags(write=False)
    return v, i


@functools.lru_cache(maxsize=None)
def bunny():
    kind, (v, i), _ = S.inputs("stanford-bunny.obj")
    v = np.ascontiguousarray(v, np.float32)
    i = np.ascontiguousarray(i, np.uint32)
    v.setflags(write=False)
    i.setflags(write=False)
    return v, i


def deform(v, seed=7):
    """A seeded jitter of 0.02 plus the shear x += 0.15 sin(4 y), in float32."""
    rng = np.random.default_rng(seed)
    w = np.array(v, np.float32)
    w[:, :3] += rng.normal(scale=0.02, size=(len(w), 3)).astype(np.float32)
    w[:, 0] += (np.float32(0.15) * np.sin(np.float32(4.0) * w[:, 1])).astype(np.float32)
    return w


def translate(v):
    """v + (8, -16, 4): exact in float32 for the lattice meshes, no coordinate on zero."""
    w = np.array(v, np.float32)
    w[:, :3] += SHIFT
    assert np.array_equal(w[:, :3].astype(np.float64), v[:, :3].astype(np.float64) + SHIFT.astype(np.float64))
    assert (w[:, :3] != 0).all()
    return w


def host_refit(rt, v, i, new_v=None):
    """rtx_bvh_refit_host: the host builder's tree of (v, i), refitted to new_v
    (or as built when new_v is None) -> (nodes, tris)."""
    from rtamd._lib import check
    L = rt.lib()
    v = np.ascontiguousarray(v, np.float32)
    i = np.ascontiguousarray(i, np.uint32)
    nv = None if new_v is None else np.ascontiguousarray(new_v, np.float32)
    ni, nt = C.c_int64(0), C.c_int64(0)
    check(L.rtx_bvh_refit_host(_p(v), len(v), _p(i), len(i), _p(nv), None, C.byref(ni), None, C.byref(nt)))
    nodes = np.zeros((ni.value, 56), np.uint32)
    tris = np.zeros((nt.value, 12), np.uint32)
    check(L.rtx_bvh_refit_host(_p(v), len(v), _p(i), len(i), _p(nv), _p(nodes), C.byref(ni), _p(tris),
                               C.byref(nt)))
    return nodes, tris


def boxes(nodes):
    """The child boxes as float32 [n_inner, 8, 6]."""
    return nodes[:, :48].view(np.float32).reshape(-1, 8, 6)


def words(nodes):
    return nodes[:, 48:]
