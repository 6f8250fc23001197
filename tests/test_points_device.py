"""rt_sdf_mesh_points_device / rt_sdf_mesh_grid_device on the GPU, from torch
tensors through rtamd.torch_rays.closest / sdf_grid: every value bit for bit
the definition's (include/rtamd.h). The signed distance is the oracle's
(cpuref.sdf_points); closest point, triangle and feature are tests/points_ref.py's
numpy statement of sdfref::closest, which test_points_host.py pins to the
oracle. Under a radius the expected values follow the header's rule
r >= 0 && d2 <= r*r applied to the unbounded winner (test_points_host.py
checks that this is what the brute force over the candidates gives).
"""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

import cpuref
import points_ref as R

pytestmark = pytest.mark.gpu

ALL = ("dist", "closest", "prim", "feature")
MESHES = {"cube": ("cube.obj", 3000), "spot": ("spot.obj", 1500), "bunny": ("stanford-bunny.obj", 700)}
INF = np.float32(np.inf)


class Case:
    def __init__(self, key):
        name, n = MESHES[key]
        self.v, self.i = R.mesh(name)
        self.p = R.points(name, n, 11)
        self.signed = cpuref.sdf_points(self.v, self.i, self.p, 16)
        # (the bunny: the same brute force without the triangles that cannot win)
        self.ref = R.brute_force_near(self.v, self.i, self.p, self.signed) if key == "bunny" else \
            R.brute_force(self.v, self.i, self.p)
        for a in (self.p, self.signed, *self.ref.values()):
            a.setflags(write=False)

    def expected(self, radius=np.inf, rows=None):
        """The four outputs under `radius` (scalar or [N]) for points `rows`."""
        rows = np.arange(len(self.p)) if rows is None else rows
        r = np.broadcast_to(np.asarray(radius, np.float32), (len(rows),))
        d2 = self.ref["d2"][rows]
        with np.errstate(invalid="ignore"):
            hit = (r >= 0) & (d2 <= r * r)
        return {"dist": np.where(hit, self.signed[rows], INF),
                "closest": np.where(hit[:, None], self.ref["closest"][rows], self.p[rows]),
                "prim": np.where(hit, self.ref["prim"][rows], -1),
                "feature": np.where(hit, self.ref["feature"][rows], -1).astype(np.int32)}, hit


@functools.lru_cache(maxsize=None)
def case(key):
    return Case(key)


@pytest.fixture(scope="module")
def handles(gpu, rt):
    """One SDFMesh per mesh, made on first use, closed after the module."""
    made = {}

    def get(key):
        if key not in made:
            c = case(key)
            made[key] = rt.SDFMesh(rt.SimpleMesh(c.v, c.i))
        return made[key]

    yield get
    import torch
    torch.cuda.synchronize()
    for m in made.values():
        m.close()


def query(m, p, radius=np.inf, outputs=ALL, unsigned=False):
    """torch_rays.closest on a numpy point set -> {output: numpy array}"""
    import torch
    from rtamd import torch_rays
    t = torch.from_numpy(np.array(p, np.float32)).cuda()
    r = torch.from_numpy(np.ascontiguousarray(radius, np.float32)).cuda() if isinstance(radius, np.ndarray) else radius
    h = torch_rays.closest(m, t, radius=r, outputs=outputs, unsigned=unsigned)
    got = {k: getattr(h, k) for k in ALL}
    assert all((got[k] is not None) == (k in outputs) for k in ALL)
    return {k: x.cpu().numpy() for k, x in got.items() if x is not None}


def same(got, want, keys=None):
    for k in keys or got:
        bad = np.flatnonzero((R.bits(got[k]) != R.bits(np.asarray(want[k], got[k].dtype))).reshape(len(got[k]), -1).any(1))
        assert bad.size == 0, f"{k}: {bad.size} of {len(got[k])} differ, e.g. at {bad[:3]}: {got[k][bad[:3]]} " \
                              f"expected {want[k][bad[:3]]}"


@pytest.mark.parametrize("key", list(MESHES))
def test_all_outputs_unbounded(handles, key):
    c = case(key)
    got = query(handles(key), c.p)
    want, hit = c.expected()
    assert hit.all()
    same(got, want, ALL)
    assert got["dist"].dtype == np.float32 and got["closest"].shape == (len(c.p), 3)
    assert got["prim"].dtype == np.int64 and got["feature"].dtype == np.int32


def _buffers(torch, n, guard=8):
    """sentinel-filled output buffers for n points with `guard` more elements each"""
    return {"dist": torch.full((n + guard,), -7.5, dtype=torch.float32, device="cuda"),
            "closest": torch.full((n + guard, 3), -7.5, dtype=torch.float32, device="cuda"),
            "prim": torch.full((n + guard,), -77, dtype=torch.int64, device="cuda"),
            "feature": torch.full((n + guard,), -77, dtype=torch.int32, device="cuda")}


def _untouched(buf, first=0):
    for k, x in buf.items():
        tail = x[first:].cpu().numpy()
        assert np.all(tail == (-7.5 if x.dtype.is_floating_point else -77)), f"{k}: written past its end or unasked"


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_wave_tail_and_guards(handles, n):
    """A last wave with 1, 63, 64 and 1 live lanes; lanes past n write nothing."""
    import torch
    c = case("spot")
    rows = np.arange(1500 - 30, 1500 - 30 + n)  # uniform points, then near-surface ones
    pts = torch.from_numpy(c.p[rows].copy()).cuda()
    buf = _buffers(torch, n)
    handles("spot").points_device(pts.data_ptr(), n, **{k + "_ptr": x.data_ptr() for k, x in buf.items()},
                                  stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    same({k: x[:n].cpu().numpy() for k, x in buf.items()}, c.expected(rows=rows)[0])
    _untouched(buf, first=n)


def test_each_output_alone_and_each_pair(handles):
    import torch
    c = case("spot")
    rows = np.arange(1400, 1700)
    want = c.expected(rows=rows)[0]
    pts = torch.from_numpy(c.p[rows].copy()).cuda()
    m = handles("spot")
    for sel in [s for k in (1, 2) for s in itertools.combinations(ALL, k)]:
        buf = _buffers(torch, len(rows), guard=0)
        m.points_device(pts.data_ptr(), len(rows), **{k + "_ptr": buf[k].data_ptr() for k in sel},
                        stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        same({k: buf[k].cpu().numpy() for k in sel}, want)
        _untouched({k: x for k, x in buf.items() if k not in sel})
        same(query(m, c.p[rows], outputs=sel), want)


@pytest.mark.parametrize("key", ["cube", "spot"])
def test_unsigned_is_abs_of_signed(handles, key):
    c = case(key)
    got = query(handles(key), c.p, unsigned=True)
    want = dict(c.expected()[0])
    want["dist"] = np.abs(want["dist"])
    assert (c.signed < 0).any() and np.signbit(want["dist"]).sum() == 0
    same(got, want, ALL)
    same(query(handles(key), c.p, outputs=("dist",), unsigned=True), want)


@pytest.mark.parametrize("key", ["cube", "spot", "bunny"])
def test_scalar_radius(handles, key):
    c = case(key)
    want, hit = c.expected(0.05)
    assert 0.3 < hit.mean() < 0.8
    got = query(handles(key), c.p, radius=0.05)
    same(got, want, ALL)
    assert np.all(np.isposinf(got["dist"][~hit])) and np.all(got["prim"][~hit] == -1)
    assert np.array_equal(R.bits(got["closest"][~hit]), R.bits(c.p[~hit]))


@pytest.mark.parametrize("key", ["cube", "spot"])
def test_radius_zero_hits_the_on_vertex_points(handles, key):
    """d2 = 0 <= 0: the on-vertex points hit, at distance +-0, and among the
    triangles around the vertex (all tied at 0) the lowest id wins."""
    c = case(key)
    n = len(c.p) // 3
    want, hit = c.expected(0.0)
    assert hit[2 * n:].all() and hit[:2 * n].sum() < 10
    got = query(handles(key), c.p, radius=0.0)
    same(got, want, ALL)
    assert np.all(got["dist"][2 * n:] == 0)
    a, b, cc = R.corners(c.v, c.i)
    for k in range(2 * n, 2 * n + 16):
        on = np.flatnonzero((a == c.p[k]).all(1) | (b == c.p[k]).all(1) | (cc == c.p[k]).all(1))
        assert got["prim"][k] == on[0] and on.size >= 2


@pytest.mark.parametrize("key", ["cube", "spot", "bunny"])
def test_per_point_radius(handles, key):
    c = case(key)
    r = np.empty(len(c.p), np.float32)
    r[0::5], r[1::5], r[2::5], r[3::5], r[4::5] = np.inf, 0.05, 0.0, -1.0, np.nan
    want, hit = c.expected(r)
    assert hit[0::5].all() and hit[1::5].any() and hit[2::5].any() and not hit[3::5].any() and not hit[4::5].any()
    same(query(handles(key), c.p, radius=r), want, ALL)
    same(query(handles(key), c.p, radius=r, outputs=("prim",)), want)


def test_nan_and_huge_points_leave_their_neighbours_alone(handles):
    """NaN and +-1e30 points in the waves of ordinary ones: the ordinary lanes
    get what they get without them; a NaN point has no candidate."""
    c = case("spot")
    rows = np.arange(1436, 1436 + 128)
    p = c.p[rows].copy()
    odd = np.array([3, 17, 40, 63, 64, 90, 127])
    p[odd[0]] = np.nan
    p[odd[1]] = (np.nan, 0.1, 0.2)
    p[odd[2]] = 1e30
    p[odd[3]] = -1e30
    p[odd[4]] = (1e30, -1e30, 0.0)
    p[odd[5]] = (0.0, 0.0, np.nan)
    p[odd[6]] = (0.3, 1e30, 0.3)
    m = handles("spot")
    plain = np.setdiff1d(np.arange(128), odd)
    for radius in (np.inf, 0.05):
        got = query(m, p, radius=radius)
        want = c.expected(radius, rows)[0]
        same({k: x[plain] for k, x in got.items()}, {k: x[plain] for k, x in want.items()})
        alone = query(m, c.p[rows], radius=radius)
        same({k: x[plain] for k, x in got.items()}, {k: x[plain] for k, x in alone.items()})
        for k in odd[[0, 1, 5]]:  # NaN points: no candidate
            assert np.isposinf(got["dist"][k]) and got["prim"][k] == -1 and got["feature"][k] == -1
            assert np.array_equal(R.bits(got["closest"][k]), R.bits(p[k]))
    far = query(m, p, radius=0.05)
    for k in odd[[2, 3, 4, 6]]:  # out of every triangle's reach
        assert np.isposinf(far["dist"][k]) and far["prim"][k] == -1
        assert np.array_equal(R.bits(far["closest"][k]), R.bits(p[k]))


@pytest.mark.parametrize("key", ["spot", "bunny"])
def test_mixed_wave_retiring_and_deep_lanes(handles, key):
    """Even lanes 10 units away with r = 0.05 are done at the root node, odd
    lanes near the surface walk to the leaves, in the same waves."""
    c = case(key)
    n = len(c.p) // 3
    rows = np.arange(n, n + 320)  # near-surface points
    p = c.p[rows].copy()
    p[0::2] += np.float32(10.0)
    want, hit = c.expected(0.05, rows)
    for k in want:
        want[k] = want[k].copy()
    want["dist"][0::2], want["closest"][0::2], want["prim"][0::2], want["feature"][0::2] = INF, p[0::2], -1, -1
    assert hit[1::2].mean() > 0.9
    same(query(handles(key), p, radius=0.05), want, ALL)


def test_stream_order_and_two_handles_at_once(gpu, rt, handles):
    """The query is queued behind the torch kernel that produces its points on
    a side stream (no synchronisation in between), while a second handle is
    queried on a second stream; both give the bits of the serial runs."""
    import torch
    from rtamd import torch_rays
    c1, c2 = case("spot"), case("cube")
    m1 = handles("spot")
    perm = np.random.default_rng(3).permutation(len(c1.p))
    shuffled = torch.from_numpy(c1.p[perm].copy()).cuda()
    back = torch.from_numpy(np.argsort(perm)).cuda()
    p2 = torch.from_numpy(c2.p.copy()).cuda()
    big = torch.ones((1 << 24,), device="cuda")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with rt.SDFMesh(rt.SimpleMesh(c2.v, c2.i)) as m2:
        with torch.cuda.stream(s1):
            for _ in range(4):  # keeps the stream busy ahead of the gather
                big = torch.sin(big) * 1.0001
            pts = torch.index_select(shuffled, 0, back)  # = c1.p, written by a torch kernel on s1
            h1 = torch_rays.closest(m1, pts, outputs=ALL)
        with torch.cuda.stream(s2):
            h2 = torch_rays.closest(m2, p2, radius=0.05, outputs=ALL)
        s1.synchronize()
        s2.synchronize()
        same({k: getattr(h1, k).cpu().numpy() for k in ALL}, c1.expected()[0])
        same({k: getattr(h2, k).cpu().numpy() for k in ALL}, c2.expected(0.05)[0])
        same({k: getattr(h2, k).cpu().numpy() for k in ALL}, query(m2, c2.p, radius=0.05))


@pytest.mark.parametrize("key,size", [("cube", (17, 17, 17)), ("spot", (20, 23, 18))])
def test_sdf_grid_is_the_host_grid(rt, handles, key, size):
    import torch
    from rtamd import torch_rays
    m = handles(key)
    g = torch_rays.sdf_grid(m, size)
    assert g.dtype == torch.float32 and tuple(g.shape) == size and g.is_cuda
    _, host = m.grid(size)
    assert np.array_equal(R.bits(g.cpu().numpy().ravel()), R.bits(host))
    c = case(key)
    ref = cpuref.sdf_points(c.v, c.i, cpuref.lattice_points(size), 16)
    assert np.array_equal(R.bits(host), R.bits(ref))
    for bad in ((1, 8, 8), (8, 8), (8, 8, 4097)):
        with pytest.raises(ValueError):
            torch_rays.sdf_grid(m, bad)
    out = torch.full((8 * 8 * 8,), -7.5, device="cuda")
    with pytest.raises(rt.RtError):
        m.grid_device((1, 8, 8), out.data_ptr())
    with pytest.raises(rt.RtError):
        m.grid_device((8, 8, 8), None)
    torch.cuda.synchronize()
    assert bool((out == -7.5).all())


def test_refusals_launch_nothing(gpu, rt, handles):
    import torch
    from rtamd import _lib, torch_rays
    c = case("cube")
    m = handles("cube")
    n = 64
    pts = torch.from_numpy(c.p[:n].copy()).cuda()
    buf = _buffers(torch, n, guard=0)
    out = {k + "_ptr": x.data_ptr() for k, x in buf.items()}
    with pytest.raises(rt.RtError):
        m.points_device(pts.data_ptr(), -1, **out)
    with pytest.raises(rt.RtError):
        m.points_device(None, n, **out)
    with pytest.raises(rt.RtError):
        m.points_device(pts.data_ptr(), n)  # no output at all
    for bad in (float("nan"), -0.5, -float("inf")):
        with pytest.raises(rt.RtError):
            m.points_device(pts.data_ptr(), n, radius=bad, **out)
        with pytest.raises(ValueError):
            torch_rays.closest(m, pts, radius=bad)
    b = _lib.PointBatch(n, pts.data_ptr(), None, float("inf"), *(x.data_ptr() for x in buf.values()))
    L = rt.lib()
    for flags in (2, 3, 0x80000000):
        assert L.rt_sdf_mesh_points_device(m._h, C.byref(b), flags, None) == -1 and L.rt_last_error()
    assert L.rt_sdf_mesh_points_device(None, C.byref(b), 0, None) == -1
    assert L.rt_sdf_mesh_points_device(m._h, None, 0, None) == -1
    torch.cuda.synchronize()
    _untouched(buf)
    # a negative scalar beside a radius array is not read, and n == 0 is no error
    r = torch.full((n,), 0.05, device="cuda")
    m.points_device(pts.data_ptr(), n, radius=-1.0, radius_ptr=r.data_ptr(), **out)
    m.points_device(None, 0, **out)
    torch.cuda.synchronize()
    same({k: x.cpu().numpy() for k, x in buf.items()}, c.expected(0.05, np.arange(n))[0])
    empty = torch_rays.closest(m, pts[:0], outputs=ALL)
    assert empty.dist.shape == (0,) and empty.closest.shape == (0, 3)


def test_bad_tensors_raise_before_a_launch(handles):
    import torch
    from rtamd import torch_rays
    m = handles("cube")
    good = torch.zeros((8, 3), device="cuda")
    bad_points = [good.double(), torch.zeros((8, 4), device="cuda"), torch.zeros((24,), device="cuda"),
                  torch.zeros((8, 3)), torch.zeros((3, 8), device="cuda").t(), torch.zeros((8, 6), device="cuda")[:, ::2],
                  np.zeros((8, 3), np.float32), None]
    for x in bad_points:
        with pytest.raises(ValueError):
            torch_rays.closest(m, x)
    bad_radius = [torch.zeros((7,), device="cuda"), torch.zeros((8,), device="cuda", dtype=torch.float64),
                  torch.zeros((8,)), torch.zeros((8, 1), device="cuda"), torch.zeros((16,), device="cuda")[::2]]
    for r in bad_radius:
        with pytest.raises(ValueError):
            torch_rays.closest(m, good, radius=r)
    for outputs in ((), ("dist", "dist"), ("t",), ("dist", "normal")):
        with pytest.raises(ValueError):
            torch_rays.closest(m, good, outputs=outputs)
