"""Instanced scenes on the GPU (RT_SCENE_INSTANCED, include/rtamd.h): rigid
copies of mesh scenes under rt_trace_rays_device and rt_intersect_rays.

Bar, as tests/test_rays_device.py: sentinel-filled buffers with guards, and
every value bitwise the reference's. The reference is composed from the oracle
alone (instances_common.compose): the oracle's mesh intersection per instance
in index order, on rays transformed in numpy float32 with the header's
expressions and the M read back from the device.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import cpuref
import instances_common as IC
import rtamd
from rtamd import _lib, torch_rays

pytestmark = pytest.mark.gpu

PAIRS = [(0.01, 100.0), (-5.0, 100.0), (0.5, 2.0)]  # tests/test_rays_device.py's intervals
N = 4096
GUARD = 64
PLANE_OFF = -0.75
RT_E_INVALID, RT_E_STATE = -1, -4
KINDS = {"hit": (torch.int32, np.int32, 1, 0x5A5A5A5A), "t": (torch.float32, np.float32, 1, 0x7FC12345),
         "normal": (torch.float32, np.float32, 3, 0x7FC12345), "prim": (torch.int64, np.int64, 1, 0x5A5A5A5A5A5A5A5A)}
ALL = ("hit", "t", "normal", "prim")


def _pose(seed, scale, b):
    return IC.affine(IC.rot(seed) @ np.diag(np.float64(scale)), b)


def _defs():
    """name -> (BLAS mesh names, [(blas, xform, flags)])."""
    d = {f"a-{m}": ((m,), [(0, IC.IDENTITY, 0)]) for m in ("cube", "bunny", "grid", "tri")}
    # (b) cube, bunny, cube with overlapping boxes: rotation, non-uniform scale, translation
    d["b"] = (("cube", "bunny"), [(0, _pose(11, (0.6, 0.9, 0.5), (-0.3, 0.1, 0.2)), 0),
                                  (1, _pose(12, (1.3, 0.8, 1.1), (0.1, -0.1, 0.0)), 0),
                                  (0, _pose(13, (0.5, 0.5, 1.2), (0.4, 0.2, -0.3)), 0)])
    # (c) a mirrored instance, two coincident instances of one BLAS, one disabled
    mirror = IC.affine(IC.rot(21) @ np.diag([-1.1, 0.9, 1.0]), (0.2, 0.0, -0.2))
    assert np.linalg.det(mirror[:, :3].astype(np.float64)) < 0
    twin = _pose(22, (0.7, 0.6, 0.8), (-0.4, -0.2, 0.3))
    d["c"] = (("tri", "bunny", "cube", "grid"), [(0, _pose(23, (2.0, 2.5, 2.0), (0.5, 0.4, 0.6)), 0), (1, mirror, 0),
                                                 (2, twin, 0), (2, twin, 0),
                                                 (3, _pose(24, (0.25, 0.25, 0.25), (-1.0, -1.0, -1.0)), IC.DISABLED)])
    # (d) 70 small cubes: more instances than lanes
    rng = np.random.default_rng(31)
    cubes = []
    for k in range(70):
        c = np.float64([k % 5, (k // 5) % 5, k // 25]) * 0.7 - [1.4, 1.4, 0.7]
        cubes.append((0, _pose(100 + k, rng.uniform(0.12, 0.22, 3), c), 0))
    d["d"] = (("cube",), cubes)
    return d


DEFS = _defs()
SCENES = list(DEFS)


@functools.lru_cache(maxsize=None)
def _blas(name):
    return rtamd.BVHBuilder(rtamd.SimpleMesh(*IC.mesh(name)))


def _build(name):
    names, inst = DEFS[name]
    return rtamd.InstancedScene([_blas(m) for m in names], inst)


@functools.lru_cache(maxsize=None)
def _scene(name):
    return _build(name)


def _refs(name):
    return {k: IC.ref_mesh(m) for k, m in enumerate(DEFS[name][0])}


@functools.lru_cache(maxsize=None)
def _rays(n=N):
    o, d = IC.random_rays(n, 20261014)
    return o, d, torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()


def _compose(name, gs, o, d, tn, tf):
    tab = gs.instances()
    return IC.compose(_refs(name), tab.blas, tab.flags, tab.inv, o, d, tn, tf, tab.skipped)


@functools.lru_cache(maxsize=None)
def _ref(name, tn, tf):
    """The composed reference of scene `name` without its plane on _rays(), once."""
    o, d, _, _ = _rays()
    out = _compose(name, _scene(name), o, d, tn, tf)
    for a in out:
        a.setflags(write=False)
    return out


def _ref_plane(name, plane, tn, tf, n=N):
    o, d, _, _ = _rays()
    res = tuple(a[:n] for a in _ref(name, tn, tf))
    return IC.with_plane(res, o[:n], d[:n], tn, tf, PLANE_OFF) if plane else res


def _set_plane(gs, plane):
    gs.set_plane(rtamd.Plane((0.0, 1.0, 0.0), PLANE_OFF) if plane else None)


def _trace(gs, o_t, d_t, n, outputs=ALL, tn=0.01, tf=100.0, tn_t=None, tf_t=None, any_hit=False, stream=None):
    """tests/test_rays_device.py's _trace: buffers GUARD elements longer than
    n, sentinel-filled; [0, n) fully written, the guard untouched."""
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


def _assert_ref(ref, got, what):
    rh, rt_, rn, rp = ref
    h = rh.astype(bool)
    if "hit" in got:
        assert set(np.unique(got["hit"]).tolist()) <= {0, 1}
        assert np.array_equal(rh, got["hit"]), f"{what}: hit mask differs on {int((rh != got['hit']).sum())} rays"
    if "prim" in got:
        assert np.array_equal(rp, got["prim"]), f"{what}: primitive ids differ on {int((rp != got['prim']).sum())} rays"
    if "t" in got:
        assert np.array_equal(_bits(rt_[h]), _bits(got["t"][h])), f"{what}: t differs"
        assert np.isposinf(got["t"][~h]).all(), f"{what}: t of a miss is not +inf"
    if "normal" in got:
        assert np.array_equal(_bits(rn[h]), _bits(got["normal"][h])), f"{what}: normal differs"
        assert np.array_equal(got["normal"][~h], np.tile(np.float32([0, 1, 0]), (int((~h).sum()), 1)))


def _same(a, b, what):
    for k in a:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), f"{what}: {k} differs"


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("plane", [False, True])
@pytest.mark.parametrize("tn,tf", PAIRS)
def test_parity_with_composed_oracle(gpu, name, plane, tn, tf):
    """Closest hit with all four outputs, and any hit, on 4,096 random rays."""
    gs = _scene(name)
    _set_plane(gs, plane)
    ref = _ref_plane(name, plane, tn, tf)
    _, _, o_t, d_t = _rays()
    _assert_ref(ref, _trace(gs, o_t, d_t, N, tn=tn, tf=tf), f"{name} plane={plane} [{tn}, {tf}]")
    a = _trace(gs, o_t, d_t, N, outputs=("hit",), tn=tn, tf=tf, any_hit=True)
    assert np.array_equal(ref[0], a["hit"]), "any-hit mask differs"
    if not plane and tn == 0.01:
        inst, _ = torch_rays.split_prim(ref[3])
        assert int((inst >= 0).sum()) > 100, "the scene is hardly hit"
        if name == "c":  # the lower index wins every tie; the disabled instance never answers
            assert (inst == 2).any() and not (inst == 3).any() and not (inst == 4).any()
            assert (inst == 0).any() and (inst == 1).any()
        if name == "d":
            assert len(np.unique(inst[inst >= 0])) > 64


@pytest.mark.parametrize("mesh", ["cube", "bunny", "grid", "tri"])
@pytest.mark.parametrize("tn,tf", PAIRS)
def test_identity_instance_is_the_plain_blas(gpu, mesh, tn, tf):
    """K = 1 with the identity: hit, t and prim's low word are bitwise the
    plain BLAS trace. (Not the normal: the winner's is normalised once more
    after M^T, which may move the last bit of an already normalised vector.)"""
    gs, bl = _scene(f"a-{mesh}"), _blas(mesh)
    _set_plane(gs, False)
    bl.set_plane(None)
    _, _, o_t, d_t = _rays()
    got = _trace(gs, o_t, d_t, N, tn=tn, tf=tf)
    plain = _trace(bl, o_t, d_t, N, tn=tn, tf=tf)
    assert np.array_equal(got["hit"], plain["hit"])
    assert np.array_equal(_bits(got["t"]), _bits(plain["t"]))
    h = plain["hit"] != 0
    assert np.array_equal(got["prim"][h] & 0xFFFFFFFF, plain["prim"][h]) and (got["prim"][h] >> 32 == 0).all()
    assert (got["prim"][~h] == -1).all()


@pytest.mark.parametrize("name", ["b", "d"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_partial_waves(gpu, name, n):
    """Ray counts around the wave edge: [0, n) fully written, misses included,
    the 64 elements behind it not."""
    gs = _scene(name)
    _set_plane(gs, False)
    ref = _ref_plane(name, False, 0.01, 100.0, n)
    _, _, o_t, d_t = _rays()
    _assert_ref(ref, _trace(gs, o_t, d_t, n), f"{name} n={n}")
    _assert_ref(ref, _trace(gs, o_t, d_t, n, outputs=("t", "prim")), f"{name} n={n} no normal")
    a = _trace(gs, o_t, d_t, n, outputs=("hit",), any_hit=True)
    assert np.array_equal(ref[0], a["hit"])


@pytest.mark.parametrize("plane", [False, True])
def test_output_subsets(gpu, plane):
    """Every output alone, and t + prim without the normal: the same bits as
    the call with all four."""
    gs = _scene("c")
    _set_plane(gs, plane)
    _, _, o_t, d_t = _rays()
    full = _trace(gs, o_t, d_t, N, tn=-5.0)
    for sub in (("hit",), ("t",), ("normal",), ("prim",), ("t", "prim"), ("hit", "normal")):
        _same(_trace(gs, o_t, d_t, N, outputs=sub, tn=-5.0), full, f"outputs {sub}")


@pytest.mark.parametrize("name", ["b", "c"])
@pytest.mark.parametrize("plane", [False, True])
def test_per_ray_intervals(gpu, name, plane):
    """d_tnear / d_tfar tensors (the per-lane traversal): each ray draws one of
    the three intervals; also one of the two pointers NULL."""
    gs = _scene(name)
    _set_plane(gs, plane)
    o, d, o_t, d_t = _rays()
    pick = np.random.default_rng(5).integers(0, 3, N)
    tn = np.float32([p[0] for p in PAIRS])[pick]
    tf = np.float32([p[1] for p in PAIRS])[pick]
    tn_t, tf_t = torch.from_numpy(tn).cuda(), torch.from_numpy(tf).cuda()
    for use_tn, use_tf in ((True, True), (True, False), (False, True)):
        a = tn if use_tn else np.full(N, 0.25, np.float32)
        b = tf if use_tf else np.full(N, 3.0, np.float32)
        ref = _compose(name, gs, o, d, a, b)
        if plane:
            ref = IC.with_plane(ref, o, d, a, b, PLANE_OFF)
        kw = dict(tn=0.25, tf=3.0, tn_t=tn_t if use_tn else None, tf_t=tf_t if use_tf else None)
        _assert_ref(ref, _trace(gs, o_t, d_t, N, **kw), f"{name} per-ray tn={use_tn} tf={use_tf}")
        got = _trace(gs, o_t, d_t, N, outputs=("hit",), any_hit=True, **kw)
        assert np.array_equal(ref[0], got["hit"]), "any-hit mask differs"


def test_stream_and_host_entries(gpu):
    """torch_rays.trace on a non-default stream, and rt_intersect_rays on host
    buffers: the same reference."""
    gs = _scene("c")
    _set_plane(gs, True)
    ref = _ref_plane("c", True, 0.01, 100.0)
    o, d, o_t, d_t = _rays()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        r = torch_rays.trace(gs, o_t, d_t)
        a = torch_rays.trace(gs, o_t, d_t, any_hit=True)
    st.synchronize()
    _assert_ref(ref, {k: getattr(r, k).cpu().numpy() for k in ALL}, "non-default stream")
    assert np.array_equal(ref[0], a.hit.cpu().numpy())
    h = gs.intersect(o, d, 0.01, 100.0)
    _assert_ref(ref, {"hit": h.hitten.astype(np.int32), "t": h.t, "normal": h.normal, "prim": h.prim}, "host entry")


def test_translation_is_exact(gpu):
    """Convention, end to end without tolerance: an instance of the lattice
    mesh translated by (8, -16, 4), ray origins on multiples of 1/64, equals a
    plain mesh scene built from the translated vertices in all four outputs,
    bitwise: every subtraction is exact and the tree is the same one."""
    shift = np.float64([8.0, -16.0, 4.0])
    v, i = IC.mesh("grid")
    w = np.array(v)
    w[:, :3] += shift.astype(np.float32)
    assert np.array_equal(w[:, :3].astype(np.float64), v[:, :3].astype(np.float64) + shift)
    plain = rtamd.BVHBuilder(rtamd.SimpleMesh(w, i))
    gs = rtamd.InstancedScene([_blas("grid")], [(0, IC.affine(np.eye(3), shift), 0)])
    assert np.array_equal(gs.instances().inv[0], IC.affine(np.eye(3), -shift))
    rng = np.random.default_rng(64)
    o = (rng.integers(-3 * 64, 10 * 64, (N, 3)) / 64.0 + shift).astype(np.float32)
    # aimed at the lattice (0 .. 7 before the shift); no zero component
    d = (rng.uniform(0.5, 6.5, (N, 3)) + shift - o).astype(np.float32)
    assert (d != 0).all()
    o_t, d_t = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    for tn, tf in PAIRS:
        a, b = _trace(gs, o_t, d_t, N, tn=tn, tf=tf), _trace(plain, o_t, d_t, N, tn=tn, tf=tf)
        assert int(b["hit"].sum()) > 1000
        _same(a, b, f"translated instance [{tn}, {tf}]")


@pytest.mark.parametrize("mesh", ["bunny", "cube"])
@pytest.mark.parametrize("seed", IC.ROT_SEEDS)
def test_rotation_against_the_flattened_scene(gpu, mesh, seed):
    """Convention under rotation: one mesh under A = Q diag(s), b in [-1, 1],
    against the oracle on the flattened mesh (vertices transformed in float64,
    rounded once). At most 4 of 4096 hit flags differ and |dt| <= 1e-4 max(1, t)
    on common hits (tests/test_instances_host.py asserts the same bounds
    reference against reference: 0 flags, 5.5e-6)."""
    x, o, d = IC.rotation_case(mesh, seed)
    v, i = IC.mesh(mesh)
    flat = cpuref.RefScene.mesh(IC.flatten(v, x), i).intersect_rays(o, d, 0.01, 100.0)
    gs = rtamd.InstancedScene([_blas(mesh)], [(0, x, 0)])
    got = _trace(gs, torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda(), N, outputs=("hit", "t"))
    IC.assert_rotation_bounds(flat, got["hit"], got["t"], f"{mesh} seed {seed}")


def _host_inverse(x):
    return np.stack([rtamd.affine_inverse(m) for m in x])


def test_poses_from_the_device(gpu):
    """torch_rays.update_instances of all poses, then of a sub-range first > 0,
    on the stream that produced the tensor: the stored M is rt_affine_inverse
    of the same matrices bitwise, every traced output equals that of a scene
    created fresh with those poses; a singular matrix makes the scene answer as
    the scene without that instance, and a later valid update brings it back."""
    names, inst = DEFS["b"]
    gs = _build("b")
    _, _, o_t, d_t = _rays()
    fresh = lambda poses, flags=(0, 0, 0): rtamd.InstancedScene(
        [_blas(m) for m in names], [(inst[k][0], poses[k], flags[k]) for k in range(3)])
    p1 = np.stack([_pose(40 + k, (0.8, 0.7 + 0.1 * k, 0.9), (0.1 * k, -0.1, 0.05 * k)) for k in range(3)])
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        x = torch.from_numpy(p1).cuda() * 1.0  # produced by a torch kernel on this stream
        torch_rays.update_instances(gs, x)
        r = torch_rays.trace(gs, o_t, d_t)
    st.synchronize()
    tab = gs.instances()
    assert np.array_equal(_bits(tab.inv.ravel()), _bits(_host_inverse(p1).ravel())) and not tab.skipped.any()
    assert tab.blas.tolist() == [0, 1, 0] and not tab.flags.any()
    want = _trace(fresh(p1), o_t, d_t, N)
    _same({k: getattr(r, k).cpu().numpy() for k in ALL}, want, "all poses from the device")
    # a sub-range, [K, 12] layout
    p2 = p1.copy()
    p2[1:] = np.stack([_pose(50 + k, (1.1, 0.6, 0.7), (-0.2, 0.1 * k, 0.1)) for k in range(2)])
    with torch.cuda.stream(st):
        torch_rays.update_instances(gs, (torch.from_numpy(p2[1:]).cuda() * 1.0).reshape(2, 12), first=1)
    st.synchronize()
    assert np.array_equal(_bits(gs.instances().inv.ravel()), _bits(_host_inverse(p2).ravel()))
    _same(_trace(gs, o_t, d_t, N), _trace(fresh(p2), o_t, d_t, N), "a sub-range from the device")
    # a singular matrix: the instance is skipped until its next update
    bad = p2[1:2].copy()
    bad[0, 2, :3] = bad[0, 1, :3]
    torch_rays.update_instances(gs, torch.from_numpy(bad).cuda(), first=1)
    tab = gs.instances()
    assert tab.skipped.tolist() == [0, 1, 0] and tab.blas.tolist() == [0, 1, 0]
    without = _trace(fresh(p2, (0, IC.DISABLED, 0)), o_t, d_t, N)
    _same(_trace(gs, o_t, d_t, N), without, "a skipped instance")
    a = _trace(gs, o_t, d_t, N, outputs=("hit",), any_hit=True)
    assert np.array_equal(a["hit"], without["hit"])
    torch_rays.update_instances(gs, torch.from_numpy(p2[1:2]).cuda(), first=1)
    assert not gs.instances().skipped.any()
    _same(_trace(gs, o_t, d_t, N), _trace(fresh(p2), o_t, d_t, N), "the instance is back")
    # bad tensors and ranges are refused before anything is launched
    good = torch.from_numpy(p1).cuda()
    for t, first in ((good.double(), 0), (good.cpu(), 0), (good[:, :, :3], 0), (good.reshape(3, 12).t(), 0), (good, 1),
                     (good, -1), (good.permute(0, 2, 1).contiguous().permute(0, 2, 1), 0)):
        with pytest.raises(ValueError):
            torch_rays.update_instances(gs, t, first=first)
    assert np.array_equal(_bits(gs.instances().inv.ravel()), _bits(_host_inverse(p2).ravel()))


def test_host_pose_update(gpu):
    """update_instances from host matrices, with new flags: as a fresh scene."""
    names, inst = DEFS["b"]
    gs = _build("b")
    _, _, o_t, d_t = _rays()
    p = np.stack([_pose(60 + k, (0.9, 0.8, 0.7), (0.1, 0.1 * k, -0.1)) for k in range(2)])
    gs.update_instances(p, first=1, flags=[IC.DISABLED, 0])
    want = rtamd.InstancedScene([_blas(m) for m in names], [inst[0], (1, p[0], IC.DISABLED), (0, p[1], 0)])
    _same(_trace(gs, o_t, d_t, N), _trace(want, o_t, d_t, N), "host update")
    assert gs.instances().flags.tolist() == [0, IC.DISABLED, 0]


def test_dynamic_blas(gpu):
    """After update_vertices of a dynamic BLAS the instanced scene's next trace
    sees the refitted tree: the answers of a scene created afterwards."""
    v, i = IC.mesh("grid")
    bl = rtamd.BVHBuilder(rtamd.SimpleMesh(v, i), dynamic=True)
    inst = [(0, _pose(70, (0.3, 0.25, 0.3), (-0.8, -0.7, -0.9)), 0), (1, _pose(71, (0.9, 0.9, 0.9), (0.3, 0.2, 0.0)), 0)]
    gs = rtamd.InstancedScene([bl, _blas("cube")], inst)
    _, _, o_t, d_t = _rays()
    before = _trace(gs, o_t, d_t, N)
    w = np.array(v)
    w[:, :3] += np.random.default_rng(72).normal(scale=0.3, size=(len(w), 3)).astype(np.float32)
    torch_rays.update_vertices(bl, torch.from_numpy(w).cuda())
    after = _trace(gs, o_t, d_t, N)
    again = _trace(rtamd.InstancedScene([bl, _blas("cube")], inst), o_t, d_t, N)
    _same(after, again, "after the refit")
    assert not np.array_equal(_bits(before["t"]), _bits(after["t"]))
    a = _trace(gs, o_t, d_t, N, outputs=("hit",), any_hit=True)
    assert np.array_equal(a["hit"], again["hit"])


def test_errors(gpu):
    """Every refusal returns its code and leaves the answers unchanged; every
    unsupported entry gives RT_E_STATE. (The refusal of a BLAS on another
    device needs two GPUs and is not exercised here.)"""
    L = gpu.lib()
    names, inst = DEFS["b"]
    gs = _build("b")
    _, _, o_t, d_t = _rays()
    before = _trace(gs, o_t, d_t, N)
    blas = [_blas(m)._handle() for m in names]
    grid = rtamd.SDFGrid(np.uint32([4, 4, 4]), np.ones(64, np.float32))

    def arr(items):
        a = (_lib.Instance * len(items))()
        for k, (b, x, f) in enumerate(items):
            a[k].blas, a[k].flags = b, f
            a[k].xform[:] = np.asarray(x, np.float32).reshape(12).tolist()
        return a

    def create(handles, items, n=None, k=None, out=True):
        h = C.c_void_p()
        hs = (C.c_void_p * max(1, len(handles)))(*handles)
        rc = L.rt_scene_create_instanced(hs, len(handles) if n is None else n, arr(items) if items is not None else None,
                                         len(items or []) if k is None else k, C.byref(h) if out else None)
        assert rc != 0 and not h.value and L.rt_last_error()
        return rc

    sing = IC.affine(np.ones((3, 3)), (0, 0, 0))
    nan = IC.IDENTITY.copy()
    nan[1, 3] = np.nan
    ok = [(0, IC.IDENTITY, 0)]
    assert create(blas, ok, n=0) == RT_E_INVALID and create(blas, ok, k=0) == RT_E_INVALID
    assert create(blas, None, k=1) == RT_E_INVALID and create(blas, ok, out=False) == RT_E_INVALID
    assert L.rt_scene_create_instanced(None, 1, arr(ok), 1, C.byref(C.c_void_p())) == RT_E_INVALID
    assert create([blas[0], None], ok) == RT_E_INVALID
    assert create(blas, [(2, IC.IDENTITY, 0)]) == RT_E_INVALID and create(blas, [(-1, IC.IDENTITY, 0)]) == RT_E_INVALID
    assert create(blas, [(0, IC.IDENTITY, 2)]) == RT_E_INVALID
    assert create(blas, [(0, sing, 0)]) == RT_E_INVALID and create(blas, ok + [(1, nan, 0)]) == RT_E_INVALID
    assert create([blas[0], grid._handle()], ok) == RT_E_STATE
    assert create([gs._handle()], ok) == RT_E_STATE  # an instanced scene is no BLAS
    # updates: refused as a whole, the scene unchanged
    h = gs._handle()
    upd = lambda first, items, k=None: L.rt_scene_update_instances(h, first, len(items) if k is None else k, arr(items))
    moved = (0, _pose(80, (1, 1, 1), (0.5, 0.5, 0.5)), 0)
    for rc in (upd(0, [moved, (5, IC.IDENTITY, 0)]), upd(1, [moved, (0, sing, 0)]), upd(2, [moved, moved]),
               upd(-1, [moved]), upd(0, [(0, IC.IDENTITY, 4)]), upd(0, [moved], k=-1),
               L.rt_scene_update_instances(h, 0, 1, None), L.rt_scene_update_instances(None, 0, 1, arr([moved])),
               L.rt_scene_update_instances_device(h, 0, 1, None, None),
               L.rt_scene_update_instances_device(h, 2, 2, C.c_void_p(o_t.data_ptr()), None),
               L.rt_scene_update_instances_device(h, -1, 1, C.c_void_p(o_t.data_ptr()), None),
               L.rt_scene_get_instances(h, 1, 3, None, None, None), L.rt_scene_get_instances(None, 0, 1, None, None, None)):
        assert rc == RT_E_INVALID and L.rt_last_error()
    mesh = blas[0]
    assert L.rt_scene_update_instances(mesh, 0, 1, arr([moved])) == RT_E_STATE
    assert L.rt_scene_update_instances_device(mesh, 0, 1, C.c_void_p(o_t.data_ptr()), None) == RT_E_STATE
    assert L.rt_scene_get_instances(mesh, 0, 1, None, None, None) == RT_E_STATE
    # the entries that do not take the kind
    P = rtamd.render_params((0, 0, 2.5), *cpuref.camera_matrices((0, 0, 2.5), aspect=1.0))
    c = torch.zeros((8, 8), dtype=torch.int32, device="cuda")
    t = torch.zeros((8, 8), dtype=torch.float32, device="cuda")
    hc, ht = np.zeros((8, 8), np.uint32), np.zeros((8, 8), np.float32)
    cp, tp = (C.c_void_p * 1)(c.data_ptr()), (C.c_void_p * 1)(t.data_ptr())
    mean, total, out = C.c_float(), C.c_float(), C.c_void_p()
    cnt = np.zeros(9, np.int64)
    vtx = np.zeros((8, 4), np.float32)
    n64, d32 = C.c_int64(), C.c_int32()
    pv = lambda a: C.c_void_p(a.ctypes.data)
    dev = (C.c_int32 * 1)(0)
    state = {
        "rt_render": L.rt_render(h, C.byref(P), pv(hc), pv(ht), 8, 8, 1, None),
        "rt_render_device": L.rt_render_device(h, C.byref(P), c.data_ptr(), t.data_ptr(), 8, 8, 1, None, None),
        "rt_render_device_frames": L.rt_render_device_frames(h, C.byref(P), 1, cp, tp, 8, 8, 1, None, None),
        "rt_bench_frames": L.rt_bench_frames(h, C.byref(P), 1, 8, 8, 1, C.byref(mean), C.byref(total)),
        "rt_count_work": L.rt_count_work(h, C.byref(P), 1, 8, 8, 1, None, pv(cnt)),
        "rt_scene_replicate": L.rt_scene_replicate(h, 0, C.byref(out)),
        "rt_multi_create": L.rt_multi_create(h, dev, 1, 8, C.byref(out)),
        "rt_scene_update_vertices": L.rt_scene_update_vertices(h, pv(vtx), 8),
        "rt_scene_update_vertices_device": L.rt_scene_update_vertices_device(h, C.c_void_p(o_t.data_ptr()), 8, None),
        "rt_scene_bvh_stats": L.rt_scene_bvh_stats(h, C.byref(n64), C.byref(n64), C.byref(d32)),
    }
    assert state == {k: RT_E_STATE for k in state}
    torch.cuda.synchronize()
    assert not out.value and not hc.any() and not ht.any() and int(c.sum()) == 0 and float(t.sum()) == 0 and not cnt.any()
    # what does work on the kind
    assert L.rt_scene_kind(h) == _lib.RT_SCENE_INSTANCED and L.rt_scene_device(h) == torch.cuda.current_device()
    assert gs.device_bytes() == 3 * 64 + 2 * 56
    _same(_trace(gs, o_t, d_t, N), before, "after the refused calls")
    # rt_trace_rays_device keeps its argument rules
    hit = torch.zeros(N, dtype=torch.int32, device="cuda")
    for kw in (dict(d_origin=None), dict(n=-1), dict(d_hit=None), dict(flags=2), dict(flags=1, d_t=t.data_ptr())):
        f = dict(n=N, d_origin=o_t.data_ptr(), d_dir=d_t.data_ptr(), d_hit=hit.data_ptr(), d_t=None, flags=0)
        f.update(kw)
        b = _lib.RayBatch(f["n"], f["d_origin"], f["d_dir"], None, None, 0.01, 100.0, f["d_hit"], f["d_t"], None, None)
        assert L.rt_trace_rays_device(h, C.byref(b), f["flags"], None) == RT_E_INVALID
    torch.cuda.synchronize()
    assert int(hit.sum()) == 0
    gs.close()
    grid.close()
