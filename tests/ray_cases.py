"""Ray recipes for the exact slab path and for waves of mixed make-up, shared
by test_ray_cases_host.py (which asserts on the oracle alone that every set
does what it claims), test_rays_exact_paths.py, test_instances_exact_paths.py
and test_refit_gpu.py. A plain module: no fixtures, no GPU.

"Exact" is mesh_primary_wave's word (csrc/rt_scenes.h): a ray with a
non-finite 1/d component, or with dot(d, d) > dmax2, takes the ISPC slab forms
with their NaN rules (csrc/rt_math.h, and the lemma above cull_rect in
csrc/rt_device.hip) and the division of the triangle test; every other ray is
"fast". The decision is per lane, so a wave can hold both, and the rays a wave
has left when it hands over to its 8-lane groups can be of both flavours.

Every recipe is deterministic from its arguments and returns float32 (o, d).

SAFETY RULE FOR THE SDF SCENES (grid and octree): every direction has unit
length and finite components. The sphere march advances t by the sampled
distance, so a ray that does not move in space (d = 0) never leaves the box --
in the reference as well -- and a shrunk direction multiplies the step count.
`scaled` and `null_dir` are therefore for mesh and instanced scenes only: mesh
traversal visits each node at most once and always ends. plain_sets() and
every caller keep to this.
"""
import functools
import zlib

import numpy as np

WAVE = 64
N = 4096
PAIRS = [(0.01, 100.0), (-5.0, 100.0), (0.5, 2.0)]  # tests/test_rays_device.py's intervals
POOLS = ("fast", "exact", "away")
FAST, EXACT, AWAY = 0, 1, 2


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _f32(*arrays):
    return tuple(np.ascontiguousarray(a, np.float32) for a in arrays)


def _lattice(rng, lo, hi, step, shape):
    """lo + k step in [lo, hi] (exact in float32 for dyadic lo and step)."""
    lo = np.broadcast_to(np.asarray(lo, np.float64), shape[-1:])
    hi = np.broadcast_to(np.asarray(hi, np.float64), shape[-1:])
    k = rng.integers(0, np.floor((hi - lo) / step).astype(np.int64) + 1, shape)
    return lo + k * np.float64(step)


# ------------------------------------------------------------------ recipes --
def lattice_axis(n, lo, hi, step, seed=0):
    """Axis-parallel unit directions from origins on lo + multiples of `step`
    in [lo, hi] (tests/test_mesh_resume.py's second half). For: the exact branch
    with two infinite 1/d components; on the two zero axes the origin equals
    box bounds, so their slab operands are 0 * inf = NaN."""
    rng = _rng("lattice_axis", n, seed)
    o = _lattice(rng, lo, hi, step, (n, 3))
    d = np.zeros((n, 3))
    d[np.arange(n), rng.integers(0, 3, n)] = rng.choice([-1.0, 1.0], n)
    return _f32(o, d)


def in_plane(n, y, seed=0, extent=1.5):
    """Rays inside the plane of the flat mesh (o.y = y, d.y = 0, unit length;
    tests/test_mesh_resume.py's first half). For: the exact branch on boxes of
    zero thickness -- every box of that mesh gives NaN entry distances on y,
    which are kept and visited; every triangle's determinant is 0, so no such
    ray hits (a set of these is discriminating only by its company)."""
    rng = _rng("in_plane", n, seed)
    o = rng.uniform(-extent, extent, (n, 3))
    o[:, 1] = y
    a = rng.uniform(0.0, 2.0 * np.pi, n)
    d = np.stack([np.cos(a), np.zeros(n), np.sin(a)], axis=1)
    return _f32(o, d)


def one_zero(n, targets, origins, seed=0, axis=None):
    """General unit directions with exactly one component zero, half of the
    zeros -0.0 (1/d = -inf); the origin's coordinate on that axis is on the
    lattice lo + k origins[2], the other two components aim at a point of the box
    targets = (lo, hi) from an origin in origins = (lo, hi, step). For: the
    exact branch with one infinite 1/d component -- a slab that is NaN on one
    axis and decided by the two others, the reference's "whatever the other
    axes say" rule. axis: the zero axis of every ray (default: drawn per ray)."""
    rng = _rng("one_zero", n, seed)
    olo, ohi, step = origins
    o = rng.uniform(np.broadcast_to(olo, (3,)), np.broadcast_to(ohi, (3,)), (n, 3))
    onl = _lattice(rng, olo, ohi, step, (n, 3))
    axis = rng.integers(0, 3, n) if axis is None else np.full(n, axis)
    r = np.arange(n)
    o[r, axis] = onl[r, axis]
    o = o.astype(np.float32).astype(np.float64)
    p = rng.uniform(np.broadcast_to(targets[0], (3,)), np.broadcast_to(targets[1], (3,)), (n, 3))
    d = p - o
    d[r, axis] = 0.0
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d = d.astype(np.float32)
    d[r, axis] = np.where(rng.random(n) < 0.5, np.float32(-0.0), np.float32(0.0))
    assert ((d == 0).sum(axis=1) == 1).all()
    return _f32(o, d)


def scaled(o, d, k=8, seed=0):
    """The rays with d * (u 2^e), e drawn per ray from -k..k and u from [1, 2):
    unnormalised directions; zero components stay zero. For: a slab and a
    triangle test that must not assume |d| = 1 (t scales by 1 / (u 2^e), so the
    interval cuts differently), and the dot(d, d) side of the fast / exact
    decision. MESH AND INSTANCED SCENES ONLY (see the safety rule above)."""
    rng = _rng("scaled", len(o), k, seed)
    f = rng.uniform(1.0, 2.0, len(o)) * np.exp2(rng.integers(-k, k + 1, len(o)))
    return _f32(o, d * f.astype(np.float32)[:, None])


def null_dir(n, lo=-1.5, hi=1.5, seed=0):
    """d = (0, 0, 0) from origins in [lo, hi]: every 1/d is +inf and every slab
    operand 0 * inf or +-inf. The oracle reports no hit. MESH AND INSTANCED
    SCENES ONLY (see the safety rule above)."""
    rng = _rng("null_dir", n, seed)
    o = rng.uniform(np.broadcast_to(lo, (3,)), np.broadcast_to(hi, (3,)), (n, 3))
    o[: n // 2] = np.round(o[: n // 2])  # half of them on integer coordinates
    return _f32(o, np.zeros((n, 3)))


def ulp_twin(o, d, seed=0):
    """The same rays with every origin coordinate on a zero axis of d moved by
    one np.nextafter step, up or down by a seeded draw: no slab operand is
    0 * inf any more. The control set for classes that the reference misses by
    its NaN rule."""
    rng = _rng("ulp_twin", len(o), seed)
    up = np.where(rng.random(o.shape) < 0.5, np.float32(np.inf), np.float32(-np.inf))
    t = np.where(d == 0, np.nextafter(o, up), o)
    return _f32(t, d)


def aimed(n, targets, origins, seed=0, unit=True):
    """Ordinary rays: origins in the box origins = (lo, hi), aimed at points of
    targets = (lo, hi); no zero component. The `fast` pool."""
    rng = _rng("aimed", n, seed)
    o = rng.uniform(np.broadcast_to(origins[0], (3,)), np.broadcast_to(origins[1], (3,)), (n, 3)).astype(np.float32)
    p = rng.uniform(np.broadcast_to(targets[0], (3,)), np.broadcast_to(targets[1], (3,)), (n, 3))
    d = p - o
    if unit:
        d /= np.linalg.norm(d, axis=1, keepdims=True)
    d = d.astype(np.float32)
    assert (d != 0).all()
    return _f32(o, d)


def away(n, hi, seed=0):
    """Rays whose root-box test fails: origins 1 to 3 beyond the box's upper x
    bound `hi`, d.x >= 0.8, so x only grows (for tNear >= 0). The `away` pool: such a lane
    never enters the traversal loop, and does not count towards the rays a
    wave has left."""
    rng = _rng("away", n, seed)
    o = rng.uniform(-1.0, 1.0, (n, 3))
    o[:, 0] = hi + rng.uniform(1.0, 3.0, n)
    d = rng.uniform(-0.5, 0.5, (n, 3))
    d[:, 0] = rng.uniform(1.0, 2.0, n)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o, d = _f32(o, d)
    assert is_away(o, d, hi).all()
    return o, d


def is_away(o, d, hi):
    """o.x at least 1 beyond hi and d.x >= 0.5: for tNear >= 0 no point of the
    ray has x <= hi, and the x slab alone fails."""
    return (o[:, 0] >= np.float32(hi) + 1) & (d[:, 0] >= 0.5)


# ------------------------------------------------------------ wave make-up --
def _lanes(rng, nwaves, k):
    """k distinct lanes per wave, seeded."""
    return np.stack([rng.permutation(WAVE)[:k] for _ in range(nwaves)])


def compose_waves(pools, pattern, nwaves, seed=0):
    """A batch of nwaves 64-ray waves with a prescribed make-up from the pools
    {"fast": (o, d), "exact": (o, d), "away": (o, d)} (each pool is consumed in
    order and wraps around). Patterns:
      "interleave"            fast and exact on alternating lanes
      ("single", lane)        one exact ray among 63 fast ones
      ("single_inv", lane)    one fast ray among 63 exact ones
      ("survivors", k, f)     k rays of the pools fast / exact (f = "fast",
                              "exact" or "half": k // 2 fast, the rest exact)
                              on seeded lanes, the other 64 - k rays `away`:
                              exactly k lanes enter the traversal loop
      "shuffled"              half fast, half exact, under a seeded permutation
                              of the whole batch
    For: the hand-over of mesh_primary_wave (at most kCoopRays = 8 rays left
    PER FLAVOUR, so 8 + 8 suspends both branches at once; 9 and 17 need a wave
    to lose a ray first), the gather of the owners' state by __shfl and the
    fast / exact dispatch of the 8-lane groups.
    -> (o, d, labels) with labels[i] indexing POOLS."""
    rng = _rng("compose_waves", repr(pattern), nwaves, seed)
    lab = np.zeros((nwaves, WAVE), np.int64)
    kind = pattern if isinstance(pattern, str) else pattern[0]
    if kind == "interleave":
        lab[:, 1::2] = EXACT
    elif kind == "single":
        lab[:, pattern[1]] = EXACT
    elif kind == "single_inv":
        lab[:] = EXACT
        lab[:, pattern[1]] = FAST
    elif kind == "survivors":
        _, k, flavour = pattern
        nfast = {"fast": k, "exact": 0, "half": k // 2}[flavour]
        lab[:] = AWAY
        lanes = _lanes(rng, nwaves, k)
        rows = np.arange(nwaves)[:, None]
        lab[rows, lanes[:, :nfast]] = FAST
        lab[rows, lanes[:, nfast:]] = EXACT
    elif kind == "shuffled":
        lab = lab.ravel()
        lab[len(lab) // 2:] = EXACT
        lab = lab[rng.permutation(len(lab))]
    else:
        raise ValueError(pattern)
    lab = lab.ravel()
    o = np.zeros((len(lab), 3), np.float32)
    d = np.zeros((len(lab), 3), np.float32)
    for p, name in enumerate(POOLS):
        m = np.flatnonzero(lab == p)
        if len(m):
            po, pd = pools[name]
            idx = np.arange(len(m)) % len(po)
            o[m], d[m] = po[idx], pd[idx]
    return o, d, lab


def shuffle_perm(n, seed=0):
    """The seeded permutation of "shuffled", for a batch that exists already."""
    return _rng("shuffle_perm", n, seed).permutation(n)


PATTERNS = (["interleave", "shuffled"]
            + [(s, lane) for s in ("single", "single_inv") for lane in (0, 7, 8, 63)]
            + [("survivors", k, f) for k in (1, 8, 9, 16, 17) for f in ("fast", "exact", "half")])


def pattern_id(p):
    return p if isinstance(p, str) else "-".join(str(x) for x in p)


# ------------------------------------------------------------ plain scenes --
# name -> how the scene is made; box: the model's bounds, rounded outwards
SCENES = {
    "lattice": dict(kind="mesh", box=(0.0, 6.0)),          # instances_common.mesh("grid"): integer lattice soup
    "flat": dict(kind="mesh", box=(-0.8, 0.8)),            # tri_mesh(14, 2500, "flat"): all in y = -0.25
    "stanford-bunny.obj": dict(kind="mesh", box=(-1.0, 1.0)),
    "example_grid.grid": dict(kind="sdf", box=(-1.0, 1.0)),
    "sdf_5.octree": dict(kind="sdf", box=(-1.0, 1.0)),
    "sdf_6.octree": dict(kind="sdf", box=(-1.0, 1.0)),
}
FLAT_TARGET = ((-0.7, -0.25, -0.7), (0.7, -0.25, 0.7))  # points of the flat mesh's plane
MESH_SCENES = [s for s, v in SCENES.items() if v["kind"] == "mesh"]


@functools.lru_cache(maxsize=None)
def scene_input(name):
    """-> (kind, payload) as scenes.inputs gives it: the same arrays go to the
    oracle and to the GPU."""
    if name == "lattice":
        import instances_common as IC
        return "mesh", IC.mesh("grid")
    if name == "flat":
        from test_gpu_edge import tri_mesh
        return "mesh", tri_mesh(14, 2500, "flat")
    import scenes as S
    return S.inputs(name)[:2]


@functools.lru_cache(maxsize=None)
def ref_scene(name):
    import cpuref
    kind, payload = scene_input(name)
    if kind == "mesh":
        return cpuref.RefScene.mesh(*payload)
    if kind == "grid":
        return cpuref.RefScene.grid(*payload)
    return cpuref.RefScene.octree(payload)


def gpu_scene(name):
    import rtamd
    kind, payload = scene_input(name)
    if kind == "mesh":
        return rtamd.BVHBuilder(rtamd.SimpleMesh(*payload))
    if kind == "grid":
        return rtamd.SDFGrid(*payload)
    return rtamd.SDFOctree(payload)


def _mix(*sets):
    """Sets of equal size interleaved ray by ray."""
    o = np.stack([s[0] for s in sets], axis=1).reshape(-1, 3)
    d = np.stack([s[1] for s in sets], axis=1).reshape(-1, 3)
    return _f32(o, d)


@functools.lru_cache(maxsize=None)
def plain_sets(name, n=N):
    """class -> (o, d), n rays each, for one scene of SCENES. The SDF scenes
    get unit directions only (the safety rule)."""
    S32 = 1.0 / 32.0
    if name == "lattice":
        sets = {"lattice_axis": lattice_axis(n, -2.0, 8.0, 0.5, 1),
                "one_zero": one_zero(n, (0.5, 5.5), (-2.0, 8.0, 0.5), 2)}
        sets["scaled"] = scaled(*_mix(lattice_axis(n // 2, -2.0, 8.0, 0.5, 3), one_zero(n // 2, (0.5, 5.5), (-2.0, 8.0, 0.5), 4)),
                                k=8, seed=5)
        sets["null_dir"] = null_dir(n, -2.0, 8.0, 6)
    elif name == "flat":
        # in-plane rays cannot hit (determinant 0): they travel with the axis rays, as in test_mesh_resume.py
        sets = {"in_plane+lattice_axis": _mix(in_plane(n // 2, -0.25, 1), lattice_axis(n // 2, -1.0, 1.0, 0.25, 2)),
                "one_zero": one_zero(n, FLAT_TARGET, (-1.5, 1.5, 0.25), 3)}
        sets["scaled"] = scaled(*_mix(lattice_axis(n // 2, -1.0, 1.0, 0.25, 4), one_zero(n // 2, FLAT_TARGET, (-1.5, 1.5, 0.25), 5)),
                                k=8, seed=6)
        sets["null_dir"] = null_dir(n, -1.5, 1.5, 7)
    elif name == "stanford-bunny.obj":
        sets = {"lattice_axis": lattice_axis(n, -1.0, 1.0, S32, 1),
                "one_zero": one_zero(n, (-0.5, 0.5), (-1.5, 1.5, S32), 2)}
        sets["scaled"] = scaled(*_mix(lattice_axis(n // 2, -1.0, 1.0, S32, 3), one_zero(n // 2, (-0.5, 0.5), (-1.5, 1.5, S32), 4)),
                                k=8, seed=5)
        sets["null_dir"] = null_dir(n, -1.5, 1.5, 6)
    elif name == "example_grid.grid":
        # 65^3 samples over [-1, 1]^3: cell faces on multiples of 1/32
        sets = {"lattice_axis": lattice_axis(n, -1.0, 1.0, S32, 1),
                "one_zero": one_zero(n, (-0.5, 0.5), (-1.5, 1.5, S32), 2),
                # origins on a face of the box [-1, 1]^3, tangent to it. On this grid the surface reaches
                # the box only in a patch of 16 samples of the face z = -1, so these rays hit 6 to 15 times
                # of 4096 and their ulp_twin no more often (profiles/r15/README.md): the set is neither
                # discriminating alone nor missed by rule, and travels with one_zero rays
                "one_zero+face_tangent": _mix(one_zero(n // 2, (-0.5, 0.5), (-1.5, 1.5, S32), 3),
                                              one_zero(n // 2, (-0.6, 0.6), (-1.0, 1.0, 2.0), 4))}
    elif name == "sdf_5.octree":
        # depth 5: leaf faces on multiples of 1/16
        sets = {"lattice_axis": lattice_axis(n, -1.0, 1.0, S32, 1),
                "one_zero": one_zero(n, (-0.5, 0.5), (-1.5, 1.5, S32), 2),
                "node_planes": one_zero(n, (-0.5, 0.5), (-1.0, 1.0, 0.25), 3)}
    elif name == "sdf_6.octree":
        # depth 6: leaf faces on multiples of 1/32 -- every lattice coordinate is on one
        sets = {"lattice_axis": lattice_axis(n, -1.0, 1.0, S32, 1),
                "one_zero": one_zero(n, (-0.5, 0.5), (-1.5, 1.5, S32), 2)}
    else:
        raise KeyError(name)
    for o, d in sets.values():
        o.setflags(write=False)
        d.setflags(write=False)
    return sets


# (scene, class): sets that the reference misses by its NaN rule. Not vacuous:
# test_ray_cases_host.py asserts for each that the ulp_twin of the set gets at
# least 100 oracle hits in every interval and the set itself fewer than half.
MISSES_BY_RULE = {
    ("sdf_5.octree", "node_planes"),
    ("sdf_6.octree", "lattice_axis"),
    ("sdf_6.octree", "one_zero"),
}


@functools.lru_cache(maxsize=None)
def oracle(name, cls, tn, tf, twin=False):
    """(hit, t, normal, prim) of plain_sets(name)[cls] (or of its ulp_twin),
    computed once and shared, read-only."""
    o, d = plain_sets(name)[cls]
    if twin:
        o, d = ulp_twin(o, d)
    out = ref_scene(name).intersect_rays(o, d, tn, tf)
    for a in out:
        a.setflags(write=False)
    return out


# --------------------------------------------------- pools of a plain scene --
@functools.lru_cache(maxsize=None)
def plain_pools(name, hit_only=False, n=1024):
    """{"fast", "exact", "away"} for compose_waves on one scene: `fast` aimed
    at the model from around it (unit directions), `exact` the scene's
    lattice_axis and one_zero classes ray about (and the in-plane rays on the
    flat mesh), `away` beyond the box. hit_only: fast and exact keep only rays
    that the oracle hits in PAIRS[0] -- the `survivors` patterns count on every
    such ray entering the traversal loop."""
    lo, hi = SCENES[name]["box"]
    c, h = (lo + hi) / 2, (hi - lo) / 2
    tgt = FLAT_TARGET if name == "flat" else (c - 0.5 * h, c + 0.5 * h)
    fast = aimed(4 * n, tgt, (c - 2.5 * h, c + 2.5 * h), 11)
    sets = plain_sets(name)
    names = [k for k in sets if k not in ("scaled", "null_dir")][:2]
    exact = _mix(*[(sets[k][0][:2 * n], sets[k][1][:2 * n]) for k in names])
    assert (exact[1] == 0).any(axis=1).all() and (fast[1] != 0).all()
    if hit_only:
        rs = ref_scene(name)
        fast = tuple(a[rs.intersect_rays(*fast, *PAIRS[0])[0] != 0] for a in fast)
        exact = tuple(a[rs.intersect_rays(*exact, *PAIRS[0])[0] != 0] for a in exact)
    pools = {"fast": (fast[0][:n], fast[1][:n]), "exact": (exact[0][:n], exact[1][:n]), "away": away(n, hi, 12)}
    for o, d in pools.values():
        o.setflags(write=False)
        d.setflags(write=False)
    return pools


NWAVES = 4  # waves per composed batch; its prefixes of 3 * 64 + 1 and 3 * 64 + 9 rays are traced as well


@functools.lru_cache(maxsize=None)
def plain_batch(name, pattern):
    """compose_waves of plain_pools(name) -> (o, d, labels), NWAVES waves."""
    pools = plain_pools(name, hit_only=not isinstance(pattern, str) and pattern[0] == "survivors")
    return compose_waves(pools, pattern, NWAVES, seed=zlib.crc32(name.encode()))


# -------------------------------------------------------- instanced scene --
def signed_perm(perm, signs, k):
    """A[r, perm[r]] = signs[r] 2^k: a signed permutation times a power of two."""
    A = np.zeros((3, 3))
    for r in range(3):
        A[r, perm[r]] = signs[r] * 2.0 ** k
    return A


def exact_inverse(x):
    """World-to-object [3, 4] of x = [s P | b] (P a signed permutation, s a
    power of two) in float64: (P^T / s) (p - b), every entry representable."""
    x = np.asarray(x, np.float64)
    A, b = x[:, :3], x[:, 3]
    s2 = float((A * A).sum()) / 3.0
    Ai = A.T / s2
    assert np.array_equal(Ai @ A, np.eye(3))
    return np.concatenate([Ai, -(Ai @ b)[:, None]], axis=1)


INST_MESHES = ("grid", "cube")
N_EXACT_INST = 4  # instances 0..3: the lattice mesh under exact poses; 4: a cube under a rotation
TWINS = (1, 2)    # coincident: the lower index wins every tie


@functools.lru_cache(maxsize=None)
def instanced_def():
    """-> [(blas, xform float32 [3, 4], flags)]: the lattice mesh under four
    signed permutations times 2^k with integer translations (k = 0; k = -1
    twice, coincident; k = 1 mirrored, det < 0), which keep lattice coordinates
    exact, and one cube under a rotation, where object-space rays are general."""
    import instances_common as IC
    pair = IC.affine(signed_perm((1, 2, 0), (1, 1, 1), -1), (8, 0, 1))
    mirror = IC.affine(signed_perm((1, 0, 2), (-1, 1, -1), 1), (-1, 7, -1))
    assert np.linalg.det(mirror[:, :3].astype(np.float64)) < 0
    cube = IC.affine(IC.rot(5) * 1.5, (3.0, -4.0, 2.0))
    return [(0, IC.affine(np.eye(3), (0, 0, 0)), 0), (0, pair, 0), (0, pair, 0), (0, mirror, 0), (1, cube, 0)]


@functools.lru_cache(maxsize=None)
def instanced_boxes():
    """World bounds (lo, hi) [K, 3] of the placed instances, rounded outwards to integers."""
    import instances_common as IC
    lo, hi = [], []
    for b, x, _ in instanced_def():
        w = IC.flatten(IC.mesh(INST_MESHES[b])[0], x)[:, :3].astype(np.float64)
        lo.append(np.floor(w.min(0)))
        hi.append(np.ceil(w.max(0)))
    return np.array(lo), np.array(hi)


def _per_box(n, fn):
    """fn(m, lo, hi, k) for every placed box k, m = n / K rays each, mixed ray by ray."""
    lo, hi = instanced_boxes()
    K = len(lo)
    assert n % K == 0 or n % WAVE == 0
    m = -(-n // K)
    o, d = _mix(*[fn(m, lo[k], hi[k], k) for k in range(K)])
    return o[:n].copy(), d[:n].copy()


@functools.lru_cache(maxsize=None)
def instanced_sets(n=N):
    """class -> world-space (o, d): origins confined to the placed boxes plus a
    margin of 1, on the lattice of step 1/2 where the class has one. Object-
    space rays then have exact zeros and origins on box bounds in instances
    0..3 and general directions in the cube: a wave mixes the flavours PER
    INSTANCE."""
    inner = lambda lo, hi: (lo + 0.25 * (hi - lo), hi - 0.25 * (hi - lo))
    sets = {
        "lattice_axis": _per_box(n, lambda m, lo, hi, k: lattice_axis(m, lo - 1, hi + 1, 0.5, 20 + k)),
        "one_zero": _per_box(n, lambda m, lo, hi, k: one_zero(m, inner(lo, hi), (lo - 1, hi + 1, 0.5), 30 + k)),
    }
    half = _mix(*[(a[: n // 2], b[: n // 2]) for a, b in (
        _per_box(n, lambda m, lo, hi, k: lattice_axis(m, lo - 1, hi + 1, 0.5, 40 + k)),
        _per_box(n, lambda m, lo, hi, k: one_zero(m, inner(lo, hi), (lo - 1, hi + 1, 0.5), 50 + k)))])
    sets["scaled"] = scaled(*half, k=8, seed=7)
    sets["null_dir"] = _per_box(n, lambda m, lo, hi, k: null_dir(m, lo - 1, hi + 1, 60 + k))
    for o, d in sets.values():
        o.setflags(write=False)
        d.setflags(write=False)
    return sets


@functools.lru_cache(maxsize=None)
def instanced_M():
    """The world-to-object matrices from float64: exact_inverse for instances
    0..3 (the library's must equal these bitwise), numpy's inverse rounded once
    for the cube. float32 [K, 3, 4]."""
    M = []
    for k, (_, x, _) in enumerate(instanced_def()):
        if k < N_EXACT_INST:
            M.append(exact_inverse(x))
        else:
            x4 = np.vstack([x.astype(np.float64), [0, 0, 0, 1]])
            M.append(np.linalg.inv(x4)[:3])
    M = np.array(M)
    assert np.array_equal(M[:N_EXACT_INST], M[:N_EXACT_INST].astype(np.float32))
    return M.astype(np.float32)


def instanced_ref(o, d, tn, tf, M=None):
    """instances_common.compose of the scene on (o, d): with the M given (the
    one read back from the device), or with instanced_M()."""
    import instances_common as IC
    inst = instanced_def()
    refs = {k: IC.ref_mesh(m) for k, m in enumerate(INST_MESHES)}
    return IC.compose(refs, [b for b, _, _ in inst], [f for _, _, f in inst], instanced_M() if M is None else M,
                      o, d, tn, tf)


@functools.lru_cache(maxsize=None)
def instanced_pools(hit_only=False, n=1024):
    """The pools of compose_waves in world space (see plain_pools)."""
    inner = lambda lo, hi: (lo + 0.25 * (hi - lo), hi - 0.25 * (hi - lo))
    _, bhi = instanced_boxes()
    s = instanced_sets()
    fast = _per_box(4 * n, lambda m, lo, hi, k: aimed(m, inner(lo, hi), (lo - 1, hi + 1), 70 + k))
    exact = _mix((s["lattice_axis"][0][: 2 * n], s["lattice_axis"][1][: 2 * n]),
                 (s["one_zero"][0][: 2 * n], s["one_zero"][1][: 2 * n]))
    if hit_only:
        fast = tuple(a[instanced_ref(*fast, *PAIRS[0])[0] != 0] for a in fast)
        exact = tuple(a[instanced_ref(*exact, *PAIRS[0])[0] != 0] for a in exact)
    pools = {"fast": (fast[0][:n], fast[1][:n]), "exact": (exact[0][:n], exact[1][:n]),
             "away": away(n, float(bhi[:, 0].max()), 13)}
    for o, d in pools.values():
        o.setflags(write=False)
        d.setflags(write=False)
    return pools


@functools.lru_cache(maxsize=None)
def instanced_batch(pattern):
    """compose_waves of instanced_pools() -> (o, d, labels), NWAVES waves."""
    pools = instanced_pools(hit_only=not isinstance(pattern, str) and pattern[0] == "survivors")
    return compose_waves(pools, pattern, NWAVES, seed=77)
