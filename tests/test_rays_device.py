"""rt_trace_rays_device: IScene::intersect on device buffers, closest hit and
any hit, in stream order (include/rtamd.h). Device buffers are torch tensors.

Bar: every value the entry writes is the oracle's, bit for bit (hit and prim
everywhere, t and normal on hits), whichever outputs are asked for, for every
ray count around the wave and workgroup edges, and nothing outside [0, n) is
touched.
"""
import contextlib
import ctypes as C
import functools
import zlib

import numpy as np
import pytest
import torch

import cpuref
import scenes as S

pytestmark = pytest.mark.gpu

NAMES = ["cube.obj", "stanford-bunny.obj", "example_grid.grid", "sdf_5.octree"]
PAIRS = [(0.01, 100.0), (-5.0, 100.0), (0.5, 2.0)]  # test_gpu_parity.test_intersect_rays' intervals
N = 4096
GUARD = 64
RT_E_INVALID = -1

# output -> (torch dtype, numpy dtype, words per ray, sentinel bits as an integer
# of that width): no traced value equals a sentinel (a NaN with a payload for
# the floats)
KINDS = {"hit": (torch.int32, np.int32, 1, 0x5A5A5A5A), "t": (torch.float32, np.float32, 1, 0x7FC12345),
         "normal": (torch.float32, np.float32, 3, 0x7FC12345), "prim": (torch.int64, np.int64, 1, 0x5A5A5A5A5A5A5A5A)}
ALL = ("hit", "t", "normal", "prim")


def _random_rays(n, seed, inside_frac=0.5):
    """tests/test_gpu_parity.py's recipe (a copy)."""
    rng = np.random.default_rng(seed)
    o = rng.uniform(-3, 3, (n, 3)).astype(np.float32)
    m = rng.random(n) < inside_frac
    o[m] = rng.uniform(-0.9, 0.9, (int(m.sum()), 3)).astype(np.float32)  # inside the model box
    d = rng.normal(size=(n, 3)).astype(np.float32)
    # axis-aligned directions (1/d = +-inf slabs) and exact zeros
    k = n // 8
    axis = rng.integers(0, 3, k)
    d[:k] = 0.0
    d[np.arange(k), axis] = rng.choice([-1.0, 1.0], k).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True).astype(np.float32)
    return o, d.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _rays(name, n=N):
    o, d = _random_rays(n, zlib.crc32(f"rays-device {name}".encode()))
    return o, d, torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()


def _set_plane(name, plane):
    import rtamd
    rs, gs = S.ref_scene(name), S.gpu_scene(name)
    off = S.inputs(name)[2]
    rs.set_plane(plane, (0, 1, 0), off)
    gs.set_plane(rtamd.Plane((0.0, 1.0, 0.0), off) if plane else None)
    return rs, gs


@functools.lru_cache(maxsize=None)
def _oracle(name, plane, tn, tf, n=N):
    """(hit, t, normal, prim) of the first n rays of _rays(name), computed once."""
    assert n <= N
    rs, _ = _set_plane(name, plane)
    o, d, _, _ = _rays(name)
    out = rs.intersect_rays(o[:n], d[:n], tn, tf)
    for a in out:
        a.setflags(write=False)
    return out


def _oracle_classes(rs, o, d, tn, tf):
    """The oracle on rays with per-ray intervals: one call per (tNear, tFar) class."""
    n = len(o)
    hit, t = np.zeros(n, np.int32), np.zeros(n, np.float32)
    nrm, prim = np.zeros((n, 3), np.float32), np.zeros(n, np.int64)
    for a, b in sorted(set(zip(tn.tolist(), tf.tolist()))):
        m = (tn == np.float32(a)) & (tf == np.float32(b))
        h, tt, nn, pp = rs.intersect_rays(o[m], d[m], a, b)
        hit[m], t[m], nrm[m], prim[m] = h, tt, nn, pp
    return hit, t, nrm, prim


def _trace(gs, o_t, d_t, n, outputs=ALL, tn=0.01, tf=100.0, tn_t=None, tf_t=None, any_hit=False, stream=None):
    """One rt_trace_rays_device call into buffers GUARD elements longer than n,
    pre-filled with a sentinel. Checks that [0, n) is fully written and the
    guard untouched; returns {output: numpy [n(,3)]}."""
    buf = {}
    for k in outputs:
        dt, nt, w, sent = KINDS[k]
        ints = np.int64 if nt == np.int64 else np.int32
        buf[k] = torch.from_numpy(np.full((n + GUARD) * w, sent, ints).view(nt)).cuda()
        assert buf[k].dtype == dt
    ptr = lambda k: buf[k].data_ptr() if k in buf else None
    gs.trace_device(o_t.data_ptr(), d_t.data_ptr(), n, hit_ptr=ptr("hit"), t_ptr=ptr("t"),
                    normal_ptr=ptr("normal"), prim_ptr=ptr("prim"), tnear=tn, tfar=tf,
                    tnear_ptr=tn_t.data_ptr() if tn_t is not None else None,
                    tfar_ptr=tf_t.data_ptr() if tf_t is not None else None, any_hit=any_hit, stream=stream)
    torch.cuda.synchronize()
    out = {}
    for k in outputs:
        _, nt, w, sent = KINDS[k]
        a = buf[k].cpu().numpy()
        bits = a.view(np.int64 if nt == np.int64 else np.int32)
        assert (bits[n * w:] == sent).all(), f"{k}: guard elements past n = {n} were written"
        assert not (bits[:n * w] == sent).any(), f"{k}: elements of [0, {n}) were not written"
        out[k] = a[:n * w].reshape(n, 3) if w == 3 else a[:n * w]
    return out


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _assert_oracle(ref, got, what):
    rh, rt_, rn, rp = ref
    if "hit" in got:
        assert set(np.unique(got["hit"]).tolist()) <= {0, 1}
        assert np.array_equal(rh, got["hit"]), f"{what}: hit mask differs"
    h = rh.astype(bool)
    if "prim" in got:
        assert np.array_equal(rp, got["prim"]), f"{what}: primitive ids differ"
    if "t" in got:
        assert np.array_equal(_bits(rt_[h]), _bits(got["t"][h])), f"{what}: t differs"
        assert np.isposinf(got["t"][~h]).all(), f"{what}: t of a miss is not +inf"
    if "normal" in got:
        assert np.array_equal(_bits(rn[h]), _bits(got["normal"][h])), f"{what}: normal differs"
        assert np.array_equal(got["normal"][~h], np.tile(np.float32([0, 1, 0]), (int((~h).sum()), 1)))


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("plane", [False, True])
@pytest.mark.parametrize("tn,tf", PAIRS)
def test_parity_with_oracle(gpu, name, plane, tn, tf):
    """Closest hit with all four outputs, and any hit, on 4,096 random rays."""
    ref = _oracle(name, plane, tn, tf)
    _, gs = _set_plane(name, plane)
    _, _, o_t, d_t = _rays(name)
    _assert_oracle(ref, _trace(gs, o_t, d_t, N, tn=tn, tf=tf), f"{name} plane={plane} [{tn}, {tf}]")
    a = _trace(gs, o_t, d_t, N, outputs=("hit",), tn=tn, tf=tf, any_hit=True)
    assert np.array_equal(ref[0], a["hit"]), "any-hit mask differs"


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("plane", [False, True])
@pytest.mark.parametrize("tn,tf", PAIRS)
def test_parity_with_oracle_shuffled(gpu, name, plane, tn, tf):
    """test_parity_with_oracle on a seeded permutation of the same rays
    (ray_cases.shuffle_perm): _random_rays puts its exact-path rays into the
    first n / 8, eight whole waves; shuffled, every wave holds rays of both
    flavours (tests/test_ray_cases_host.py asserts that). The oracle answers
    ray by ray, so its result is permuted with the rays."""
    import ray_cases as RC
    perm = RC.shuffle_perm(N)
    ref = tuple(a[perm] for a in _oracle(name, plane, tn, tf))
    _, gs = _set_plane(name, plane)
    o, d, _, _ = _rays(name)
    o_t = torch.from_numpy(np.ascontiguousarray(o[perm])).cuda()
    d_t = torch.from_numpy(np.ascontiguousarray(d[perm])).cuda()
    _assert_oracle(ref, _trace(gs, o_t, d_t, N, tn=tn, tf=tf), f"{name} shuffled plane={plane} [{tn}, {tf}]")
    a = _trace(gs, o_t, d_t, N, outputs=("hit",), tn=tn, tf=tf, any_hit=True)
    assert np.array_equal(ref[0], a["hit"]), "any-hit mask differs"


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("plane", [False, True])
def test_per_ray_intervals(gpu, name, plane):
    """d_tnear / d_tfar: each ray draws one of the three intervals; also one of
    the two pointers NULL (that side's scalar applies)."""
    rs, gs = _set_plane(name, plane)
    o, d, o_t, d_t = _rays(name)
    pick = np.random.default_rng(5).integers(0, 3, N)
    tn = np.float32([p[0] for p in PAIRS])[pick]
    tf = np.float32([p[1] for p in PAIRS])[pick]
    tn_t, tf_t = torch.from_numpy(tn).cuda(), torch.from_numpy(tf).cuda()
    for use_tn, use_tf in ((True, True), (True, False), (False, True)):
        a = tn if use_tn else np.full(N, 0.25, np.float32)
        b = tf if use_tf else np.full(N, 3.0, np.float32)
        ref = _oracle_classes(rs, o, d, a, b)
        kw = dict(tn=0.25, tf=3.0, tn_t=tn_t if use_tn else None, tf_t=tf_t if use_tf else None)
        _assert_oracle(ref, _trace(gs, o_t, d_t, N, **kw), f"{name} per-ray tn={use_tn} tf={use_tf}")
        got = _trace(gs, o_t, d_t, N, outputs=("hit",), any_hit=True, **kw)
        assert np.array_equal(ref[0], got["hit"]), "any-hit mask differs"


# Cells of the scene dispatch (csrc/rt_dispatch.h) that NAMES does not reach:
# key -> (scene, rtx_set_grid_force value or None)
EDGE_MESH = (15, 6000, "same")
DISPATCH = {"mesh-15-slots": (EDGE_MESH, None), "grid-bricked": ("example_grid.grid", 1),
            "grid-bricked-wide": ("example_grid.grid", 3), "sdf_6.octree": ("sdf_6.octree", None)}


@contextlib.contextmanager
def _dispatch_scene(key):
    """-> (the oracle's (hit, t, normal, prim) with the plane off on [0.01,
    100], GPU scene, rays as _rays gives them). The grid is created and traced
    under its forced layout, which is restored afterwards (as
    tests/test_gpu_shading.py does)."""
    import rtamd
    from rtamd import _lib
    scene, force = DISPATCH[key]
    if scene == EDGE_MESH:
        v = S.edge_mesh(*EDGE_MESH)
        i = np.arange(len(v), dtype=np.uint32)
        o, d = _random_rays(N, zlib.crc32(f"rays-dispatch {EDGE_MESH}".encode()))
        with rtamd.BVHBuilder(rtamd.SimpleMesh(v, i)) as gs:
            # 15 stack slots: a tree of 9..16 levels (pick_maxd: depth - 1 slots)
            assert 9 <= gs.tree_stats()[2] <= 16
            ref = cpuref.RefScene.mesh(v, i).intersect_rays(o, d, 0.01, 100.0)
            yield ref, gs, (o, d, torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda())
    elif force is not None:
        L = rtamd.lib()
        L.rtx_set_grid_force.argtypes = [C.c_int]
        _lib.check(L.rtx_set_grid_force(force))
        try:
            with rtamd.SDFGrid(*S.inputs(scene)[1]) as gs:
                yield _oracle(scene, False, 0.01, 100.0), gs, _rays(scene)
        finally:
            _lib.check(L.rtx_set_grid_force(0))
    else:
        ref = _oracle(scene, False, 0.01, 100.0)
        yield ref, _set_plane(scene, False)[1], _rays(scene)


@pytest.mark.parametrize("key", list(DISPATCH))
def test_parity_on_further_dispatch_cells(gpu, key):
    """test_parity_with_oracle (plane off, [0.01, 100]) on a 15-slot mesh, the
    grid's bricked layout with buffer and with 64-bit address loads, and a
    7-slot octree: closest hit with all four outputs and any hit through
    rt_trace_rays_device, then rt_intersect_rays on the same rays."""
    with _dispatch_scene(key) as (ref, gs, (o, d, o_t, d_t)):
        assert int(ref[0].sum()) >= 128, "the oracle hits too few rays for the comparison to mean anything"
        _assert_oracle(ref, _trace(gs, o_t, d_t, N), key)
        a = _trace(gs, o_t, d_t, N, outputs=("hit",), any_hit=True)
        assert np.array_equal(ref[0], a["hit"]), "any-hit mask differs"
        g = gs.intersect(o, d, 0.01, 100.0)
        h = g.hitten  # (test_gpu_parity.test_intersect_rays' comparison)
        assert np.array_equal(ref[0].astype(bool), h), "rt_intersect_rays: hit mask differs"
        assert np.array_equal(ref[3], g.prim), "rt_intersect_rays: primitive ids differ"
        assert np.array_equal(_bits(ref[1][h]), _bits(g.t[h])), "rt_intersect_rays: t differs"
        assert np.array_equal(_bits(ref[2][h]), _bits(g.normal[h])), "rt_intersect_rays: normal differs"


SHAPES = [1, 63, 64, 65, 255, 257, 4 * 256 + 1]


@pytest.mark.parametrize("name", ["stanford-bunny.obj", "sdf_5.octree"])
@pytest.mark.parametrize("n", SHAPES)
def test_partial_waves_and_blocks(gpu, name, n):
    """Ray counts at the wave (64) and workgroup (64 or 256) edges: [0, n) is
    fully written, misses included, and the 64 elements behind it are not."""
    ref = tuple(a[:n] for a in _oracle(name, False, 0.01, 100.0, SHAPES[-1]))
    _, gs = _set_plane(name, False)
    _, _, o_t, d_t = _rays(name)
    _assert_oracle(ref, _trace(gs, o_t, d_t, n), f"{name} n={n}")
    _assert_oracle(ref, _trace(gs, o_t, d_t, n, outputs=("t", "prim")), f"{name} n={n} no normal")
    a = _trace(gs, o_t, d_t, n, outputs=("hit",), any_hit=True)
    assert np.array_equal(ref[0], a["hit"])


@pytest.mark.parametrize("name", ["stanford-bunny.obj", "example_grid.grid", "sdf_5.octree"])
@pytest.mark.parametrize("plane", [False, True])
def test_output_subsets(gpu, name, plane):
    """Every output alone, and t + prim without the normal (the instantiations
    that compute no normal): the same bits as the call with all four."""
    _, gs = _set_plane(name, plane)
    _, _, o_t, d_t = _rays(name)
    full = _trace(gs, o_t, d_t, N, tn=-5.0)
    for sub in (("hit",), ("t",), ("normal",), ("prim",), ("t", "prim")):
        got = _trace(gs, o_t, d_t, N, outputs=sub, tn=-5.0)
        for k in sub:
            assert np.array_equal(_bits(full[k]), _bits(got[k])), f"{name}: {k} of {sub} differs from the full call"


@pytest.mark.parametrize("name", ["stanford-bunny.obj", "example_grid.grid", "sdf_5.octree"])
def test_eye_rays_give_the_rendered_depth(gpu, name):
    """The eye rays of a 64x48 frame through the closest-hit query give
    render_device's t buffer (cleared frame, Normal mode, no plane).
    cpuref.primary_rays already lists the rays in image-row order (its row yo
    is the loop's flipped row H - yo - 1, raytracing.cpp:82)."""
    W, H = 64, 48
    pos = (0.0, 0.0, 2.5)
    _, gs = _set_plane(name, False)
    d = np.ascontiguousarray(cpuref.primary_rays(S.params(name, W, H, "primary", pos, "ref"), W, H).reshape(-1, 3))
    o = np.tile(np.float32(pos), (len(d), 1))
    got = _trace(gs, torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda(), W * H, outputs=("hit", "t"))
    c = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    t = torch.zeros((H, W), dtype=torch.float32, device="cuda")
    gs.render_device(S.params(name, W, H, "primary", pos, "gpu"), c.data_ptr(), t.data_ptr(), W, H, clear=True)
    torch.cuda.synchronize()
    assert int(got["hit"].sum()) > 100
    assert np.array_equal(_bits(t.cpu().numpy().ravel()), _bits(got["t"]))


@pytest.mark.parametrize("name", ["stanford-bunny.obj", "sdf_5.octree"])
def test_stream_order(gpu, name):
    """trace -> torch -> trace on one non-default stream, one synchronise at the
    end: the second query sees the first one's t through o2 = o + t * d."""
    from rtamd import torch_rays
    rs, gs = _set_plane(name, True)
    n = 1 << 15
    _, _, o_t, d_t = _rays(name, n)
    target = torch.tensor([2.0, 2.0, 2.0], device="cuda")
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        r1 = torch_rays.trace(gs, o_t, d_t, outputs=("hit", "t"))
        t = torch.where(r1.hit != 0, r1.t, torch.ones_like(r1.t))  # (a miss's +inf would make o2 NaN)
        o2 = (o_t + t[:, None] * d_t).contiguous()
        d2 = (target - o2).contiguous()
        r2 = torch_rays.trace(gs, o2, d2, any_hit=True)
    st.synchronize()
    assert r1.hit.dtype == torch.int32 and r1.normal is None and r1.prim is None
    assert r2.hit.dtype == torch.int32 and r2.t is None
    rh, _, _, _ = rs.intersect_rays(o2.cpu().numpy(), d2.cpu().numpy(), 0.01, 100.0)
    assert np.array_equal(rh, r2.hit.cpu().numpy())
    assert 0 < int(rh.sum()) < n


def test_torch_front_end(gpu):
    from rtamd import torch_rays
    name = "cube.obj"
    rs, gs = _set_plane(name, False)
    o, d, o_t, d_t = _rays(name)
    r = torch_rays.trace(gs, o_t, d_t, tnear=torch.full((N,), 0.01, device="cuda"), tfar=100.0)
    torch.cuda.synchronize()
    got = {k: getattr(r, k).cpu().numpy() for k in ALL}
    assert r.hit.dtype == torch.int32 and r.prim.dtype == torch.int64 and tuple(r.normal.shape) == (N, 3)
    _assert_oracle(_oracle(name, False, 0.01, 100.0), got, "torch front end")
    bad = [
        (o_t.double(), d_t),                      # float64
        (o_t, torch.zeros((N, 4), device="cuda")),  # [N,4]
        (o_t.t().contiguous().t(), d_t),          # not contiguous
        (o_t.cpu(), d_t),                         # on the CPU
        (o_t[:8], d_t),                           # shapes differ
    ]
    for oo, dd in bad:
        with pytest.raises(ValueError):
            torch_rays.trace(gs, oo, dd)
    with pytest.raises(ValueError):
        torch_rays.trace(gs, o_t, d_t, tnear=torch.zeros(N, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        torch_rays.trace(gs, o_t, d_t, outputs=("hit", "depth"))
    with pytest.raises(ValueError):
        torch_rays.trace(gs, o_t, d_t, any_hit=True, outputs=("hit", "t"))


def test_invalid_calls_rejected(gpu):
    """Every invalid call is RT_E_INVALID with a message, before any launch."""
    from rtamd import _lib
    L = gpu.lib()
    _, gs = _set_plane("cube.obj", False)
    _, _, o_t, d_t = _rays("cube.obj")
    hit = torch.zeros(N, dtype=torch.int32, device="cuda")
    t = torch.zeros(N, dtype=torch.float32, device="cuda")
    o, d, h, tt = o_t.data_ptr(), d_t.data_ptr(), hit.data_ptr(), t.data_ptr()

    def call(n=N, o=o, d=d, hit=h, t=None, normal=None, prim=None, flags=0, scene=gs._handle()):
        b = _lib.RayBatch(n, o, d, None, None, 0.01, 100.0, hit, t, normal, prim)
        return L.rt_trace_rays_device(scene, C.byref(b), flags, None), L.rt_last_error()

    cases = {
        "NULL origins": dict(o=None), "NULL directions": dict(d=None), "n < 0": dict(n=-1),
        "no output": dict(hit=None), "unknown flag": dict(flags=2), "any-hit with t": dict(flags=1, t=tt),
        "any-hit without hit": dict(flags=1, hit=None, t=tt), "n beyond one launch": dict(n=1 << 32),
        "NULL scene": dict(scene=None),
    }
    for what, kw in cases.items():
        rc, msg = call(**kw)
        assert rc == RT_E_INVALID and msg, what
    assert L.rt_trace_rays_device(gs._handle(), None, 0, None) == RT_E_INVALID
    torch.cuda.synchronize()
    assert int(hit.sum()) == 0 and int(t.sum()) == 0  # none of them launched
    assert call(n=0)[0] == 0
    assert call()[0] == 0
    torch.cuda.synchronize()
