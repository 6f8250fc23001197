"""rt_sdf_mesh_update_vertices* on the GPU: the refit of an RT_MESH_DYNAMIC
SDF-mesh handle (rt_sdf_refit.hip) against its host restatement
(rtx_sdf_mesh_refit_host, pinned by test_sdf_refit_host.py), and the point
queries after an update against the definition on the moved mesh
(points_ref.brute_force, cpuref.sdf_points).

Deformations are functions of position only (sdf_refit_common.shear), so the
moved mesh has the weld classes of creation; each test asserts that first.

The sign rule: face and edge pseudonormals are bit for bit the host's; a vertex
pseudonormal goes through acos in double, where the device's and the host
library's may differ in the last bits, so a component may round to the
neighbouring float. A signed value is compared with the oracle's wherever the
winning (triangle, feature) entry reads back bit-equal to a fresh handle's; the
other points, at most 1 % (a condition, not a tolerance), are compared without
their sign. The count of differing components is printed; 0 is expected.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import cpuref
import points_ref as R
import refit_common as RC
import sdf_refit_common as SC

pytestmark = pytest.mark.gpu

ALL = ("dist", "closest", "prim", "feature")
NAMES = {"cube": ("cube.obj", 3000), "spot": ("spot.obj", 1500), "bunny": ("stanford-bunny.obj", 700)}
INF = np.float32(np.inf)
RT_E_INVALID, RT_E_STATE = -1, -4


def moved(key):
    v, i = SC.mesh(key)
    w = SC.shear(v)
    assert SC.same_classes(v, w), "the shear changed the weld classes"
    return v, i, w


class Case:
    """A mesh, its sheared copy and the definition's answers on the sheared copy."""

    def __init__(self, key):
        name, n = NAMES[key]
        self.v, self.i, self.w = moved(key)
        assert np.abs(self.w[:, :3]).max() <= 0.69  # inside the slack's domain
        self.p = R.points(name, n, 11)
        if key != "bunny":  # and points near, and on, the moved surface
            self.p = np.ascontiguousarray(np.concatenate([self.p, SC.shear(R.points(name, n // 5, 12))]))
        self.signed = cpuref.sdf_points(self.w, self.i, self.p, 16)
        self.ref = R.brute_force_near(self.w, self.i, self.p, self.signed) if key == "bunny" else \
            R.brute_force(self.w, self.i, self.p)
        for a in (self.p, self.signed, *self.ref.values()):
            a.setflags(write=False)

    def expected(self, radius=np.inf):
        r = np.broadcast_to(np.asarray(radius, np.float32), (len(self.p),))
        d2 = self.ref["d2"]
        hit = (r >= 0) & (d2 <= r * r)
        return {"dist": np.where(hit, self.signed, INF),
                "closest": np.where(hit[:, None], self.ref["closest"], self.p),
                "prim": np.where(hit, self.ref["prim"], -1),
                "feature": np.where(hit, self.ref["feature"], -1).astype(np.int32)}, hit


@functools.lru_cache(maxsize=None)
def case(key):
    return Case(key)


def dynamic(rt, v, i):
    return rt.SDFMesh(rt.SimpleMesh(v, i), dynamic=True)


def query(m, p, radius=np.inf, unsigned=False):
    import torch
    from rtamd import torch_rays
    t = torch.from_numpy(np.array(p, np.float32)).cuda()
    h = torch_rays.closest(m, t, radius=radius, outputs=ALL, unsigned=unsigned)
    return {k: getattr(h, k).cpu().numpy() for k in ALL}


def to_device(torch, a):
    return torch.from_numpy(np.array(a, order="C")).cuda()  # (a copy: the shared arrays are read-only)


def same(got, want, keys):
    for k in keys:
        bad = np.flatnonzero((R.bits(got[k]) != R.bits(np.asarray(want[k], got[k].dtype))).reshape(len(got[k]), -1).any(1))
        assert bad.size == 0, f"{k}: {bad.size} of {len(got[k])} differ, e.g. at {bad[:3]}: {got[k][bad[:3]]} " \
                              f"expected {want[k][bad[:3]]}"


def same_signed(got, want, prim, feat, pn, pn_fresh, what="dist"):
    """The sign rule of the module docstring for signed values `got` against
    `want`, whose winners are (prim, feat); -1 = no winner (nothing to exclude)."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert np.array_equal(R.bits(np.abs(got)), R.bits(np.abs(want))), f"{what}: magnitudes differ"
    won = prim >= 0
    entry = np.ones(len(got), bool)
    entry[won] = (R.bits(pn[prim[won], feat[won], :3]) == R.bits(pn_fresh[prim[won], feat[won], :3])).all(1)
    print(f"{what}: {int((~entry).sum())} of {len(got)} points excluded from the sign comparison")
    assert (~entry).mean() <= 0.01, f"{what}: {(~entry).mean():.2%} of the points have a differing pseudonormal entry"
    assert np.array_equal(R.bits(got)[entry], R.bits(want)[entry]), f"{what}: signs differ"


def check_queries(got, want, pn, pn_fresh, signed=True):
    same(got, want, ("closest", "prim", "feature"))
    if signed:
        same_signed(got["dist"], want["dist"], want["prim"], want["feature"], pn, pn_fresh)
    else:
        same(got, want, ("dist",))


def fresh_pn(rt, w, i):
    with rt.SDFMesh(rt.SimpleMesh(w, i)) as f:
        return f.pseudonormals()


DEVICE_MESHES = ("one", "nine", "cube") + SC.HAND_MADE + ("grid1500", "spot")


@pytest.mark.parametrize("key", DEVICE_MESHES)
def test_device_refit_is_the_host_restatement(gpu, rt, key):
    """Nodes, triangle records, face and edge pseudonormals bit for bit;
    vertex pseudonormals within one float ulp at the normal's scale,
    2^-23 * max|component|: a last-bits difference of the double sum cannot
    move the float rounding further."""
    v, i, w = moved(key)
    with dynamic(rt, v, i) as m:
        n0, t0, p0 = SC.host_refit(rt, v, i)
        nodes, tri = SC.download(rt, m)
        assert np.array_equal(nodes, n0) and np.array_equal(tri, t0)
        assert np.array_equal(R.bits(m.pseudonormals()), R.bits(p0))
        m.update_vertices(w)
        n1, t1, p1 = SC.host_refit(rt, v, i, w)
        nodes, tri = SC.download(rt, m)
        pn = m.pseudonormals()
    assert len(nodes) == len(n1)
    assert len(nodes) == 0 if key == "one" else len(nodes) > 8 if key in ("grid1500", "spot") else True
    assert np.array_equal(nodes, n1), "tree differs from rth::refit_sdf_mesh"
    assert np.array_equal(tri, t1), "triangle records differ"
    assert np.array_equal(R.bits(pn[:, 3:]), R.bits(p1[:, 3:])), "edge or face pseudonormals differ"
    assert not R.bits(pn[:, :, 3]).any()
    diff = R.bits(pn[:, :3, :3]) != R.bits(p1[:, :3, :3])
    print(f"{key}: {int(diff.sum())} of {diff.size} vertex-normal components differ from the host's")
    bound = np.float32(2.0 ** -23) * np.abs(p1[:, :3, :3]).max(axis=2, keepdims=True)
    assert np.all(np.abs(pn[:, :3, :3].astype(np.float64) - p1[:, :3, :3]) <= bound)


@pytest.mark.parametrize("key", ["cube", "spot", "bunny"])
def test_queries_after_an_update(gpu, rt, key):
    import torch
    from rtamd import torch_rays
    c = case(key)
    pnf = fresh_pn(rt, c.w, c.i)
    with dynamic(rt, c.v, c.i) as m:
        torch_rays.update_sdf_mesh(m, to_device(torch, c.w))
        got = query(m, c.p)
        pn = m.pseudonormals()
        want, hit = c.expected()
        assert hit.all()
        check_queries(got, want, pn, pnf)
        # |dist| is the brute force's and the oracle's
        assert np.array_equal(R.bits(np.abs(got["dist"])), R.bits(np.sqrt(c.ref["d2"])))
        assert np.array_equal(R.bits(np.abs(got["dist"])), R.bits(np.abs(c.signed)))
        if key == "spot":
            want, hit = c.expected(0.05)
            assert hit.sum() > 100 and (~hit).sum() > 100
            check_queries(query(m, c.p, radius=0.05), want, pn, pnf)
            want = dict(c.expected()[0])
            want["dist"] = np.abs(want["dist"])
            check_queries(query(m, c.p, unsigned=True), want, pn, pnf, signed=False)
            want = dict(c.expected(0.05)[0])
            want["dist"] = np.abs(want["dist"])
            check_queries(query(m, c.p, radius=0.05, unsigned=True), want, pn, pnf, signed=False)
        torch.cuda.synchronize()


def _busy(torch, n=1 << 24, rounds=4):
    big = torch.ones((n,), device="cuda")
    for _ in range(rounds):  # keeps the stream busy ahead of what follows
        big = torch.sin(big) * 1.0001
    return big


def test_host_entries_after_a_device_update(gpu, rt):
    """points(), grid_device and octree(3) of the handle itself after an update
    queued on a busy side stream, with no synchronisation in between: the
    handle's event orders them; the octree cached before the update is dropped."""
    import torch
    from rtamd import torch_rays
    c = case("spot")
    size = (9, 8, 7)
    lat = cpuref.lattice_points(size)
    with rt.SDFMesh(rt.SimpleMesh(c.w, c.i)) as f, dynamic(rt, c.v, c.i) as m:
        pnf = f.pseudonormals()
        want_p = f.points(c.p)
        want_g = torch_rays.sdf_grid(f, size).cpu().numpy().ravel()
        want_o = f.octree(3)
        before = m.octree(3)  # cached, of the mesh as created
        assert len(before) != len(want_o) or not np.array_equal(before, want_o)
        verts = to_device(torch, c.w)
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            _busy(torch)
            torch_rays.update_sdf_mesh(m, verts)
        got_p = m.points(c.p)  # the handle's own stream, behind the event
        side.synchronize()
        pn = m.pseudonormals()
        same_signed(got_p, want_p, c.ref["prim"], c.ref["feature"], pn, pnf, "points()")
        got_g = torch_rays.sdf_grid(m, size).cpu().numpy().ravel()
        host_g = m.grid(size)[1]
        assert np.array_equal(R.bits(got_g), R.bits(host_g))
        win = query(m, lat)
        same_signed(got_g, want_g, win["prim"], win["feature"], pn, pnf, "grid")
        got_o = m.octree(3)
        assert len(got_o) == len(want_o)
        go, wo = got_o.reshape(-1, 36), want_o.reshape(-1, 36)
        assert np.array_equal(go[:, 32:], wo[:, 32:]), "octree structure differs"
        gv, wv = go[:, :32].copy().view(np.float32), wo[:, :32].copy().view(np.float32)
        assert np.array_equal(R.bits(np.abs(gv)), R.bits(np.abs(wv)))
        if np.array_equal(R.bits(pn), R.bits(pnf)):
            assert np.array_equal(got_o, want_o)
        else:
            assert (R.bits(gv) != R.bits(wv)).mean() <= 0.01
        assert np.array_equal(m.octree(3), got_o)  # cached again


@pytest.mark.parametrize("cols", [3, 4])
def test_stream_order(gpu, rt, cols):
    """The vertices are written by a torch kernel on the current (side)
    stream, then update_sdf_mesh, then closest, with no synchronisation in
    between. [V, 4] input carries w = 2 on some vertices (x, y, z doubled:
    the divided positions keep their bits)."""
    import torch
    from rtamd import torch_rays
    c = case("spot")
    w = np.array(c.w, np.float32)
    if cols == 4:
        w[5::7] *= np.float32(2.0)
        assert np.array_equal(w[:, :3] / w[:, 3:4], c.w[:, :3]) and (w[:, 3] == 2).sum() > 100
    else:
        w = np.ascontiguousarray(w[:, :3])
    perm = np.random.default_rng(5).permutation(len(w))
    shuffled = to_device(torch, w[perm])
    back = to_device(torch, np.argsort(perm))
    pts = to_device(torch, c.p)
    pnf = fresh_pn(rt, c.w, c.i)
    side = torch.cuda.Stream()
    with dynamic(rt, c.v, c.i) as m:
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            _busy(torch)
            verts = torch.index_select(shuffled, 0, back)  # = w, written by a torch kernel on `side`
            torch_rays.update_sdf_mesh(m, verts)
            h = torch_rays.closest(m, pts, outputs=ALL)
        side.synchronize()
        got = {k: getattr(h, k).cpu().numpy() for k in ALL}
        check_queries(got, c.expected()[0], m.pseudonormals(), pnf)


def test_round_trip(gpu, rt):
    """A -> B -> A: the outputs of the handle as created."""
    c = case("spot")
    b = SC.shear_back(c.w)
    assert SC.same_classes(c.v, b)
    with dynamic(rt, c.v, c.i) as m:
        pn0, (n0, t0) = m.pseudonormals(), SC.download(rt, m)
        out0 = query(m, c.p)
        m.update_vertices(b)
        assert not np.array_equal(SC.download(rt, m)[1], t0)
        m.update_vertices(c.v)
        n1, t1 = SC.download(rt, m)
        assert np.array_equal(t1, t0)
        assert np.array_equal(RC.words(n1), RC.words(n0)) and np.array_equal(RC.boxes(n1), RC.boxes(n0))  # by value
        check_queries(query(m, c.p), out0, m.pseudonormals(), pn0)


def test_an_update_leaves_a_second_handle_alone(gpu, rt):
    """Two handles of one mesh, both queried; the first is then moved under the
    points it was queried with: the second, untouched, answers as before."""
    c = case("cube")
    with dynamic(rt, c.v, c.i) as m1, dynamic(rt, c.v, c.i) as m2:
        a1, a2 = query(m1, c.p), query(m2, c.p)
        same(a1, a2, ALL)
        pn2, (n2, t2) = m2.pseudonormals(), SC.download(rt, m2)
        m1.update_vertices(c.w)
        check_queries(query(m1, c.p), c.expected()[0], m1.pseudonormals(), fresh_pn(rt, c.w, c.i))
        same(query(m2, c.p), a2, ALL)
        n, t = SC.download(rt, m2)
        assert np.array_equal(n, n2) and np.array_equal(t, t2) and np.array_equal(R.bits(m2.pseudonormals()), R.bits(pn2))


def test_refusals_launch_nothing(gpu, rt):
    import torch
    from rtamd import torch_rays
    L = rt.lib()
    c = case("cube")
    nv = len(c.v)
    good = to_device(torch, c.w)
    with dynamic(rt, c.v, c.i) as m, rt.SDFMesh(rt.SimpleMesh(c.v, c.i)) as plain:
        before = (query(m, c.p), m.pseudonormals(), SC.download(rt, m), m.octree(2))
        ptr = C.c_void_p(good.data_ptr())
        host = RC._p(c.w)
        for n in (nv - 1, nv + 1, 0, -1):
            assert L.rt_sdf_mesh_update_vertices_device(m._h, ptr, n, None) == RT_E_INVALID and L.rt_last_error()
            assert L.rt_sdf_mesh_update_vertices(m._h, host, n) == RT_E_INVALID
        assert L.rt_sdf_mesh_update_vertices_device(m._h, None, nv, None) == RT_E_INVALID
        assert L.rt_sdf_mesh_update_vertices(m._h, None, nv) == RT_E_INVALID
        assert L.rt_sdf_mesh_update_vertices_device(None, ptr, nv, None) == RT_E_INVALID
        assert L.rt_sdf_mesh_update_vertices_device(plain._h, ptr, nv, None) == RT_E_STATE and L.rt_last_error()
        assert L.rt_sdf_mesh_update_vertices(plain._h, host, nv) == RT_E_STATE
        with pytest.raises(rt.RtError):
            plain.update_vertices(c.w)
        with pytest.raises(rt.RtError):
            m.update_vertices(c.w[:, :3])
        h = C.c_void_p()
        for flags in (2, 3, 0x80000000):
            assert L.rt_sdf_mesh_create_ex(RC._p(c.v), nv, RC._p(c.i), len(c.i), flags, C.byref(h)) == RT_E_INVALID
            assert not h.value
        pn = np.zeros((len(c.i) // 3 + 1, 7, 4), np.float32)
        assert L.rt_sdf_mesh_get_pseudonormals(m._h, RC._p(pn), len(pn)) == RT_E_INVALID
        assert L.rt_sdf_mesh_get_pseudonormals(m._h, None, len(pn) - 1) == RT_E_INVALID
        bad = [good.double(), good[:, :2].contiguous(), good.cpu(), good.reshape(-1), good[:0],
               torch.zeros((4, nv), device="cuda").t(), torch.zeros((nv, 8), device="cuda")[:, ::2], c.w, None]
        for x in bad:
            with pytest.raises(ValueError):
                torch_rays.update_sdf_mesh(m, x)
        for x in (good[:-1], good[:-1, :3].contiguous()):  # well-formed, one vertex short: the library refuses it
            with pytest.raises(rt.RtError):
                torch_rays.update_sdf_mesh(m, x)
        with pytest.raises(rt.RtError):
            torch_rays.update_sdf_mesh(plain, good)
        torch.cuda.synchronize()
        same(query(m, c.p), before[0], ALL)
        assert np.array_equal(R.bits(m.pseudonormals()), R.bits(before[1]))
        n, t = SC.download(rt, m)
        assert np.array_equal(n, before[2][0]) and np.array_equal(t, before[2][1])
        assert np.array_equal(m.octree(2), before[3])
        same(query(plain, c.p), before[0], ALL)


@pytest.mark.parametrize("key", ["one", "cube", "spot"])
def test_byte_counts(gpu, rt, key):
    v, i = SC.mesh(key)
    T, V = len(i) // 3, len(v)
    wv, we = SC.welded_counts(v, i)
    with rt.SDFMesh(rt.SimpleMesh(v, i)) as plain, dynamic(rt, v, i) as m:
        nodes, tri = SC.download(rt, plain)
        three = 224 * len(nodes) + 48 * len(tri) + 112 * T
        assert len(tri) == T and plain.device_bytes() == three
        added = 12 * T + 16 * V + 4 * V + 12 * T + (4 * (wv + 1) + 12 * T) + (4 * (we + 1) + 12 * T) + 16 * T + 24 * T + \
            16 * wv + 16 * we
        assert m.device_bytes() == three + added
