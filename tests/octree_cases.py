"""Hand-built SDF octrees and the rays for them, shared by
test_octree_cases_host.py (which asserts on the oracle alone that every tree
and ray set does what it claims) and test_octree_cases_gpu.py. A plain module:
numpy only, no fixtures, no GPU. The ray side's counterpart is ray_cases.py.

Every other octree of the suite comes from the surface-refinement generator
(cpuref.sdf_octree): BFS order with childrenOffset % 8 == 1, zeros in inner
nodes, leaves that can hit at the deepest level only, at most 8 levels. The
trees here are what that generator never makes: up to 24 levels (the stack
classes of 4, 7, 15 and 31 slots, csrc/rt_scene.hip pick_maxd, and the unpacked
node coordinates from 9 levels on, csrc/rt_dispatch.h), a frame pushed on
every level, leaves of every kind on every level, blocks stored in any order
and shared between parents.

Node format (octree_raytracing.hpp:8-18): 8 float32 corner values
values[(x << 2) + (y << 1) + z], then uint32 childrenOffset (0 = leaf); the 8
children of a node are contiguous, child id (x << 2) | (y << 1) | z; the root
is node 0 over [-1, 1]^3. A node's level is its distance from the root; a
tree's depth is the number of inner nodes on its longest path
(rt_scene_bvh_stats' max_depth), so a tree of depth D has leaves at level D.

SAFETY RULE: every corner value of every node is finite -- no NaN, no
infinity, unreferenced nodes included -- and every direction is finite, of
unit length and without a zero component (ray_cases.py's rule for the SDF
scenes: the sphere march advances by the sampled distance). Leaves that are
marched are planes with a unit gradient (the march converges on them) or
decoys whose value is about 1 (one step leaves the box).
"""
import functools
import types
import zlib

import numpy as np

F = np.float32
N_EACH = 2048            # rays per recipe and tree
N = 2 * N_EACH
# (tNear, tFar): 2^-40 is csrc/rt_scenes.h's FAST condition with origins that
# may lie deep inside the tree; a negative tNear is the other path
INTERVALS = [(2.0 ** -40, 100.0), (-5.0, 100.0), (0.01, 100.0)]
# (layout, axis, bit) of the parametrised trees
SETTINGS = [("bfs", 0, 0), ("shuffled", 1, 1), ("shuffled", 2, 0)]

# kinds of a node (description.kind)
INNER, SURFACE, DECOY, NEVER_10, NEVER_0, NEVER_ABOVE, UNREF = range(7)
NEVER = (NEVER_10, NEVER_0, NEVER_ABOVE)
THRESH = F(1e-4)  # octree_raytracing.cpp:125-133, the march's hit threshold


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _unit(rng, n=None):
    v = rng.normal(size=(3,) if n is None else (n, 3))
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


CORNERS = np.array([(k >> 2, (k >> 1) & 1, k & 1) for k in range(8)], np.float64)


def child_box(lo, hi, c):
    """divide_box_8 (ray_pack.ispc:220-239) for child c; exact on dyadic boxes."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    mid = (lo + hi) / 2
    b = CORNERS[c]
    clo = np.where(b == 0, lo, mid)
    return clo, clo + (mid - lo)


# ------------------------------------------------------------- leaf values --
def surface_values(rng, size):
    """A plane through the centre of a box of edge `size`, unit gradient,
    seeded normal: the signed distance at the 8 corners."""
    n = _unit(rng)
    return ((CORNERS - 0.5) * size) @ n


def decoy_values(rng):
    """Seven corners at 1.0 and one at 5e-5: not "all >= 1e-4", so the mask
    pass must call it hittable; the interpolated value falls below 1e-4 only
    within 1e-4 of that corner, and one march step of about 1 leaves any box
    (no box below the root is larger than 1)."""
    v = np.ones(8)
    v[rng.integers(0, 8)] = 5e-5
    return v


def never_values(rng, rule, edge):
    """A leaf that never hits, by one rule of rth::flatten_octree (the
    reference's isEmpty, octree_raytracing.hpp:12-17, and intersectLeaf's
    all >= 1e-4). edge: with the value at which the rule turns.
    NEVER_10 all > 10 -- edge: one corner exactly 10.0 (not > 10: the leaf is
                 then empty by the third rule alone);
    NEVER_0  all == 0 -- edge: a mix of 0.0 and -0.0 (sampled, it would hit
                 at once: 0 < 1e-4);
    NEVER_ABOVE all >= 1e-4 -- edge: one corner exactly float32(1e-4)."""
    if rule == NEVER_10:
        v = rng.uniform(10.5, 2000.0, 8)
        if edge:
            v[rng.integers(0, 8)] = 10.0
    elif rule == NEVER_0:
        v = np.zeros(8)
        if edge:
            v[rng.permutation(8)[:rng.integers(1, 8)]] = -0.0
    else:
        v = rng.uniform(2e-4, 9.0, 8)
        if edge:
            v[rng.integers(0, 8)] = np.float64(THRESH)
    return v


def garbage_values(rng):
    """Finite junk for nodes whose values nothing may read (inner nodes,
    unreferenced nodes): large, small, negative, and zeros."""
    v = rng.uniform(-1.0, 1.0, 8) * np.exp2(rng.integers(-30, 12, 8))
    v[rng.random(8) < 0.2] = 0.0
    return v


def records(vals, off):
    """(values [n, 8], childrenOffset [n]) -> the 36-byte node records, uint8 [36 n]."""
    vals = np.ascontiguousarray(vals, F)
    off = np.ascontiguousarray(off, np.uint32)
    assert np.isfinite(vals).all(), "SAFETY RULE: every corner value is finite"
    rec = np.zeros((len(vals), 36), np.uint8)
    rec[:, :32] = vals.view(np.uint8).reshape(len(vals), 32)
    rec[:, 32:] = off.view(np.uint8).reshape(len(vals), 4)
    out = rec.ravel()
    out.setflags(write=False)
    return out


def unpack(nodes):
    """The 36-byte records -> (values float32 [n, 8], childrenOffset uint32 [n])."""
    rec = np.ascontiguousarray(nodes).view(np.uint8).reshape(-1, 36)
    return (np.ascontiguousarray(rec[:, :32]).view(F).reshape(-1, 8),
            np.ascontiguousarray(rec[:, 32:]).view(np.uint32).reshape(-1))


# --------------------------------------------------------------- the spine --
@functools.lru_cache(maxsize=None)
def spine_tree(depth, seed=0, layout="bfs", axis=0, bit=0, shared=()):
    """One chain of `depth` inner nodes S_0 (the root) .. S_{depth-1}.

    The child id taken at each level is seeded; its bit of `axis` is `bit` on
    every level, the other two are drawn. (A ray leaves the nested boxes
    through a face that is interior to every ancestor only if the path keeps
    one coordinate bit constant; only then can a frame be pushed on every
    level. With bit = 1 the packed coordinate of that axis is all ones.)

    The block of S_l, l < depth - 1, holds the next spine node, one surface
    leaf, three decoys -- the face neighbour of the spine child across `axis`
    is one -- and one never-hitting leaf per rule (never_values; edge values on
    every second level, starting with the first). The last block holds four
    surface leaves and four decoys. Inner nodes hold garbage_values.

    shared: levels l (0 <= l <= depth - 3) on which one decoy that is not the
    face neighbour is instead an inner node whose children block is the last
    block: that block then has several parents, at different levels.

    layout "bfs": the generator's order, root, then the blocks by level.
    layout "shuffled": the root, then the blocks in a seeded permutation, each
    behind a gap of 1..4 unreferenced nodes (garbage values; childrenOffset 0 or
    any offset that passes validation), so some children sit ahead of their
    parent and offsets are not 1 mod 8; no gap behind the last stored block:
    its offset is count - 8, the last legal one.

    -> (nodes uint8 [36 count], description): description.path [depth] child
    ids, .lo / .hi [depth, 3] the boxes of S_0 .. S_{depth-1} (float64, exact),
    .spine [depth] node indices, .kind / .level [count] per node (level of an
    unreferenced node: -1; of the last block: depth, also where it is shared),
    .offset [depth] the blocks' offsets, .depth, .axis, .bit, .layout."""
    assert depth >= 1 and layout in ("bfs", "shuffled") and axis in (0, 1, 2) and bit in (0, 1)
    assert all(0 <= l <= depth - 3 for l in shared)
    rng = _rng("spine_tree", depth, seed, layout, axis, bit, shared)
    sh = 2 - axis  # the child id's bit of `axis`
    path = rng.integers(0, 8, depth)
    path = (path & ~(1 << sh)) | (bit << sh)
    # block offsets
    if layout == "bfs":
        offset = 1 + 8 * np.arange(depth)
        count = 1 + 8 * depth
    else:
        order = rng.permutation(depth)
        if depth > 1 and (order == np.arange(depth)).all():
            order = order[::-1].copy()
        gaps = rng.integers(1, 5, depth)
        offset = np.zeros(depth, np.int64)
        pos = 1
        for j, blk in enumerate(order):
            pos += gaps[j]
            offset[blk] = pos
            pos += 8
        count = pos
    vals = np.zeros((count, 8))
    off = np.zeros(count, np.uint32)
    kind = np.full(count, UNREF, np.int64)
    level = np.full(count, -1, np.int64)
    spine = np.zeros(depth, np.int64)
    lo, hi = np.zeros((depth, 3)), np.zeros((depth, 3))
    lo[0], hi[0] = -1.0, 1.0
    for l in range(depth):
        node = spine[l]
        kind[node], level[node] = INNER, l
        vals[node] = garbage_values(rng)
        off[node] = offset[l]
        base = offset[l]
        size = 2.0 ** -l  # edge of the children's boxes
        level[base:base + 8] = l + 1
        if l == depth - 1:
            # by the two bits across `axis`: two columns along the axis are
            # decoys (a ray along the axis passes through), two are surfaces
            col = np.array([SURFACE, SURFACE, DECOY, DECOY])[rng.permutation(4)]
            lat = [s for s in (2, 1, 0) if s != sh]
            k = np.array([col[2 * ((j >> lat[0]) & 1) + ((j >> lat[1]) & 1)] for j in range(8)])
        else:
            c = int(path[l])
            spine[l + 1] = base + c
            lo[l + 1], hi[l + 1] = child_box(lo[l], hi[l], c)
            k = np.zeros(8, np.int64)
            k[c] = INNER
            k[c ^ (1 << sh)] = DECOY
            rest = [j for j in range(8) if j not in (c, c ^ (1 << sh))]
            fill = [SURFACE, DECOY, DECOY, NEVER_10, NEVER_0, NEVER_ABOVE]
            for j, kk in zip(rng.permutation(rest), fill):
                k[j] = kk
        for j in range(8):
            n = base + j
            if k[j] == INNER:
                continue  # the next level fills it in
            kind[n] = k[j]
            if k[j] == SURFACE:
                vals[n] = surface_values(rng, size)
            elif k[j] == DECOY:
                vals[n] = decoy_values(rng)
            else:
                vals[n] = never_values(rng, k[j], edge=(l % 2 == 0))
        if l in shared:
            alias = [j for j in range(8) if k[j] == DECOY and j != (c ^ (1 << sh))][0]
            n = base + alias
            kind[n] = INNER
            vals[n] = garbage_values(rng)
            off[n] = offset[depth - 1]
    for n in np.flatnonzero(kind == UNREF):
        vals[n] = garbage_values(rng)
        # (an unreachable node's offset is still validated: 0, or a legal one)
        off[n] = 0 if rng.random() < 0.5 else rng.integers(1, count - 7)
    if layout == "shuffled":
        assert offset.max() == count - 8
        assert (offset % 8 != 1).any(), "some offset must not be 1 mod 8"
        assert depth == 1 or (offset[1:] < spine[1:]).any(), "some block must sit ahead of its parent"
    desc = types.SimpleNamespace(path=path, lo=lo, hi=hi, spine=spine, kind=kind, level=level, offset=offset,
                                 depth=depth, axis=axis, bit=bit, layout=layout, shared=tuple(shared), count=count)
    for a in (path, lo, hi, spine, kind, level, offset):
        a.setflags(write=False)
    return records(vals, off), desc


def shared_spine(depth=9, seed=0, layout="shuffled", axis=1, bit=1):
    """The deeper shared variant: a spine whose decoy slot on two levels (the
    first and the last that spine_tree allows) is an inner node pointing at the
    last block. The longest path is still the spine's."""
    return spine_tree(depth, seed, layout, axis, bit, shared=(0, depth - 3))


# --------------------------------------------------------- small fixed trees --
def _small_desc(kind, level, depth):
    kind, level = np.asarray(kind, np.int64), np.asarray(level, np.int64)
    return types.SimpleNamespace(kind=kind, level=level, depth=depth, count=len(kind), layout="bfs")


@functools.lru_cache(maxsize=None)
def root_leaf(hittable, seed=0):
    """One node: a root that is itself a leaf (oct_start's own branch). A plane
    through the origin, or a never-hitting leaf by the third rule alone."""
    rng = _rng("root_leaf", hittable, seed)
    v = surface_values(rng, 2.0) if hittable else never_values(rng, NEVER_ABOVE, True)
    return records(v[None], [0]), _small_desc([SURFACE if hittable else NEVER_ABOVE], [0], 0)


@functools.lru_cache(maxsize=None)
def shared_blocks(k, seed=0):
    """17 nodes: the root, its block 1..8, and one block 9..16 of surface
    leaves that k in 1..8 nodes of the first block all have as their children.
    The other 8 - k nodes alternate between decoys and never-hitting leaves.
    (All level-2 boxes have edge 0.5, so each leaf is a plane through the
    centre of its box under every parent.) Depth 2."""
    assert 1 <= k <= 8
    rng = _rng("shared_blocks", k, seed)
    vals, off = np.zeros((17, 8)), np.zeros(17, np.uint32)
    kind, level = [INNER], [0]
    vals[0], off[0] = garbage_values(rng), 1
    parents = set(rng.permutation(8)[:k].tolist())
    other = 0
    for j in range(8):
        if j in parents:
            vals[1 + j], off[1 + j] = garbage_values(rng), 9
            kind.append(INNER)
        else:
            rule = (DECOY, NEVER_10, DECOY, NEVER_0, DECOY, NEVER_ABOVE, DECOY)[other]
            vals[1 + j] = decoy_values(rng) if rule == DECOY else never_values(rng, rule, True)
            kind.append(rule)
            other += 1
        level.append(1)
    for j in range(8):
        vals[9 + j] = surface_values(rng, 0.5)
        kind.append(SURFACE)
        level.append(2)
    return records(vals, off), _small_desc(kind, level, 2)


def with_offset(nodes, node, value):
    """A copy of the records with node `node`'s childrenOffset replaced."""
    vals, off = unpack(nodes)
    off = off.copy()
    off[node] = np.uint32(value)
    return records(vals, off)


def cyclic_self():
    """A node whose children block contains itself: node 3 of the root's block
    1..8 points back at block 1. FOR THE FLATTEN HOOK ONLY: the reference's
    recursion (and the oracle's) would not end on it."""
    nodes, _ = shared_blocks(1)
    return with_offset(nodes, 3, 1)


def cyclic_pair():
    """A two-node cycle through two blocks: a node of block 1..8 points at block
    9..16, a node of which points back at block 1. FOR THE FLATTEN HOOK ONLY."""
    nodes, desc = shared_blocks(1)
    parent = 1 + int(np.flatnonzero(desc.kind[1:9] == INNER)[0])
    assert unpack(nodes)[1][parent] == 9
    return with_offset(nodes, 12, 1)


# -------------------------------------------------------------------- rays --
def _finish(o, d):
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    o, d = np.ascontiguousarray(o, F), np.ascontiguousarray(d, F)
    assert np.isfinite(o).all() and np.isfinite(d).all() and (d != 0).all()
    assert np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1.0).max() < 1e-6
    return o, d


def _levels(rng, n, depth):
    """A seeded level per ray: a third of them over all levels of the spine; a
    third among the first three, whose boxes the origin then lies outside of
    (a negative tNear lists a box only from outside); a third among levels 5
    to 9 (or the tree's last), from where the deepest boxes are a little more
    than 0.01 away (tNear = 0.01 lists a box only if it ends beyond that) and
    still near enough for float32 to resolve them."""
    a = rng.integers(0, depth, n)
    b = rng.integers(0, min(3, depth), n)
    c = rng.integers(min(5, depth - 1), min(10, depth), n)
    u = rng.random(n)
    return np.where(u < 1 / 3, a, np.where(u < 2 / 3, b, c))


def aimed(desc, n=N_EACH, seed=0):
    """Each ray targets a seeded point of the spine box of a seeded level, from
    2 to 32 edges of that box away, in a seeded direction."""
    rng = _rng("aimed", desc.depth, desc.layout, desc.axis, desc.bit, n, seed)
    lv = _levels(rng, n, desc.depth)
    lo, hi = desc.lo[lv], desc.hi[lv]
    p = lo + rng.random((n, 3)) * (hi - lo)
    d = _unit(rng, n)
    d = np.where(np.abs(d) < 1e-3, 1e-3, d)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    dist = rng.uniform(2.0, 32.0, n) * (hi - lo)[:, 0]
    return _finish(p - d * dist[:, None], d)


def axial(desc, n=N_EACH, seed=0):
    """Directions within a cone about `axis` (tangent of the angle 0.01 to
    0.3), with the sign that leaves the spine's boxes through their interior
    face: + for bit 0, - for bit 1. Each ray targets a seeded point of the
    deepest inner box, from 2 to 8 edges of a seeded level's box away."""
    rng = _rng("axial", desc.depth, desc.layout, desc.axis, desc.bit, n, seed)
    lv = _levels(rng, n, desc.depth)
    lo, hi = desc.lo[-1], desc.hi[-1]
    p = lo + rng.random((n, 3)) * (hi - lo)
    d = np.zeros((n, 3))
    d[:, desc.axis] = 1.0 if desc.bit == 0 else -1.0
    a = rng.uniform(0.0, 2.0 * np.pi, n)
    r = rng.uniform(0.01, 0.3, n)
    u, v = [k for k in range(3) if k != desc.axis]
    d[:, u], d[:, v] = r * np.cos(a), r * np.sin(a)
    d[:, u] = np.where(np.abs(d[:, u]) < 1e-3, 1e-3, d[:, u])
    d[:, v] = np.where(np.abs(d[:, v]) < 1e-3, 1e-3, d[:, v])
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    dist = rng.uniform(2.0, 8.0, n) * (desc.hi[lv] - desc.lo[lv])[:, 0]
    return _finish(p - d * dist[:, None], d)


@functools.lru_cache(maxsize=None)
def spine_rays(depth, seed=0, layout="bfs", axis=0, bit=0, shared=()):
    """The 4,096 rays of a spine tree: 2,048 aimed, then 2,048 axial, in a
    seeded permutation (every wave holds both)."""
    _, desc = spine_tree(depth, seed, layout, axis, bit, shared)
    o1, d1 = aimed(desc, seed=seed)
    o2, d2 = axial(desc, seed=seed)
    perm = _rng("spine_rays", depth, seed).permutation(N)
    o, d = np.concatenate([o1, o2])[perm], np.concatenate([d1, d2])[perm]
    o, d = np.ascontiguousarray(o), np.ascontiguousarray(d)
    o.setflags(write=False)
    d.setflags(write=False)
    return o, d


@functools.lru_cache(maxsize=None)
def box_rays(n=N, seed=0, half=1.0):
    """Rays for the small fixed trees: origins within 3 of the centre, half of
    them inside [-half, half]^3, aimed at points of that box."""
    rng = _rng("box_rays", n, seed, half)
    o = rng.uniform(-3.0, 3.0, (n, 3))
    m = rng.random(n) < 0.5
    o[m] = rng.uniform(-half, half, (int(m.sum()), 3))
    p = rng.uniform(-half, half, (n, 3))
    d = p - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d = np.where(np.abs(d) < 1e-3, 1e-3, d)
    o, d = _finish(o, d)
    o.setflags(write=False)
    d.setflags(write=False)
    return o, d


# -------------------------------------------------------------- full stack --
def _slabs(lo, hi, o, inv, tn, tf):
    """intersect_box_8's entry / exit (ray_pack.ispc:241-273) in float64 for one
    box per ray -> (entry clamped to tNear, exit clamped to tFar, the largest
    |slab distance|: the scale of the float32 computation's rounding)."""
    t1, t2 = (lo - o) * inv, (hi - o) * inv
    mn, mx = np.minimum(t1, t2), np.maximum(t1, t2)
    big = np.maximum(np.abs(t1), np.abs(t2)).max(axis=1)
    return np.maximum(mn.max(axis=1), tn), np.minimum(mx.min(axis=1), tf), big


def full_stack(o, d, tree, tn, tf):
    """bool [n]: a float64 restatement of a condition sufficient for the ray to
    push a frame on every level above the last when it descends the spine. On
    each such level l, in the children of S_l:
      - the spine child is listed: entry <= exit, exit >= 0 and entry > 0 (the
        reference visits a child iff its clamped entry distance is > 0,
        octree_raytracing.cpp:166-202);
      - a sibling that can hit (a surface leaf, a decoy, or an inner node above
        surface leaves) is listed too, and entered later than the spine child
        by more than 1e-3 of the child edge.
    Every comparison also keeps a margin of 2^-20 of the largest slab distance
    involved. A float32 slab distance (b - o) * (1 / d) carries three roundings,
    3 * 2^-24 of itself, so two of them move a difference by less than 2^-21 of
    the larger: the float32 walk lists and orders the two children the same way. The walk descends into the earlier child and keeps
    the later one: a frame. A ray for which this holds on every level, and
    which reaches the last block (its oracle hit lies there, or it hits
    nothing at all, or only something the walk visits later), held depth - 1
    frames at once. tree: (nodes, description) of spine_tree."""
    nodes, desc = tree
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    inv = 1.0 / d
    _, off = unpack(nodes)
    ok = np.ones(len(o), bool)
    for l in range(desc.depth - 1):
        size = 2.0 ** -l
        c = int(desc.path[l])
        clo, chi = child_box(desc.lo[l], desc.hi[l], c)
        e0, x0, b0 = _slabs(clo, chi, o, inv, tn, tf)
        g0 = b0 * 2.0 ** -20
        listed = (x0 - e0 > g0) & (x0 > g0) & (e0 > (0.0 if tn > 0 else g0))
        later = np.zeros(len(o), bool)
        base = int(off[desc.spine[l]])
        for j in range(8):
            k = desc.kind[base + j]
            if j == c or k in NEVER:
                continue
            slo, shi = child_box(desc.lo[l], desc.hi[l], j)
            e, x, b = _slabs(slo, shi, o, inv, tn, tf)
            g = np.maximum(b, b0) * 2.0 ** -20
            later |= (x - e > g) & (x > g) & (e - e0 > np.maximum(1e-3 * size, g))
        ok &= listed & later
    return ok


def spine_outcome(tree, o, d, tn, tf, hit, prim):
    """From the oracle's (hit, prim) of the rays -> (full, ends, passes), bool
    [n]: full_stack; full and the hit lies in the last block; full and the
    walk goes on past the last block with its stack full -- no hit at all, or a
    hit in a leaf of some S_l's block, l < depth - 1, that is entered later
    than the spine child there (by full_stack's margins), so the reference had
    finished the whole spine below without a hit when it got there."""
    nodes, desc = tree
    full = full_stack(o, d, tree, tn, tf)
    hit = np.asarray(hit).astype(bool)
    prim = np.asarray(prim, np.int64)
    _, off = unpack(nodes)
    last = int(desc.offset[desc.depth - 1])
    in_last = hit & (prim >= last) & (prim < last + 8)
    o64, d64 = np.asarray(o, np.float64), np.asarray(d, np.float64)
    inv = 1.0 / d64
    later = np.zeros(len(hit), bool)
    for l in range(desc.depth - 1):
        base = int(off[desc.spine[l]])
        c = int(desc.path[l])
        clo, chi = child_box(desc.lo[l], desc.hi[l], c)
        for j in range(8):
            m = hit & (prim == base + j)
            if j == c or not m.any():
                continue
            slo, shi = child_box(desc.lo[l], desc.hi[l], j)
            e0, _, b0 = _slabs(clo, chi, o64[m], inv[m], tn, tf)
            e, _, b = _slabs(slo, shi, o64[m], inv[m], tn, tf)
            later[np.flatnonzero(m)[e - e0 > np.maximum(b, b0) * 2.0 ** -20]] = True
    return full, full & in_last, full & (~hit | later)


# ---------------------------------------------- the rules, restated in numpy --
def expected_words(nodes):
    """rtl::OctWord {child, masks} of every node reachable from the root, from
    the rules alone -> (child uint32 [n], masks uint32 [n], reachable bool [n]).
    child: 0 a leaf that can hit, 0xFFFFFFFF a leaf that never hits (isEmpty:
    all > 10 or all == 0; or all >= 1e-4), else childrenOffset. masks of an
    inner node: bit k = child k can hit (a leaf that can, or an inner node one
    of whose children can), bit 8 + k = child k is a leaf that can hit.
    For acyclic trees only."""
    vals, off = unpack(nodes)
    never = (vals > F(10.0)).all(1) | (vals == F(0.0)).all(1) | (vals >= THRESH).all(1)
    child = np.where(off == 0, np.where(never, np.uint32(0xFFFFFFFF), np.uint32(0)), off).astype(np.uint32)
    masks = np.zeros(len(off), np.uint32)
    reach = np.zeros(len(off), bool)

    def can(n):
        reach[n] = True
        if off[n] == 0:
            return not never[n]
        m = 0
        for k in range(8):
            c = int(off[n]) + k
            if can(c):
                m |= 1 << k
            if off[c] == 0 and not never[c]:
                m |= 1 << (8 + k)
        masks[n] = m
        return bool(m & 0xFF)
    can(0)
    return child, masks, reach


# ------------------------------------------------------------ the test set --
# (depth, layout, axis, bit): all three settings at the depths where the stack
# class or the coordinate packing changes hands (8 | 9: 7 -> 15 slots and packed
# -> unpacked; 17: the first 31-slot depth; 24: the deepest tree accepted), one
# setting at the others
SPINES = [(1, "shuffled", 2, 0), (5, "bfs", 0, 0), (6, "shuffled", 1, 1), (16, "shuffled", 2, 0)] + \
         [(dp,) + s for dp in (8, 9, 17, 24) for s in SETTINGS]
SHARED_SPINE = (9, "shuffled", 1, 1)


def spine_key(depth, layout, axis, bit):
    return f"spine-{depth}-{layout}-{'xyz'[axis]}{bit}"


SPINE_KEYS = [spine_key(*s) for s in SPINES]
SMALL_KEYS = ["root-hit", "root-never", "shared-2", "shared-8"]
KEYS = SPINE_KEYS + SMALL_KEYS + ["shared-spine"]
DEPTH = dict([(spine_key(*s), s[0]) for s in SPINES] +
             [("root-hit", 0), ("root-never", 0), ("shared-2", 2), ("shared-8", 2), ("shared-spine", SHARED_SPINE[0])])


@functools.lru_cache(maxsize=None)
def case(key):
    """-> (nodes, description, origins, directions) of a tree of KEYS and its
    4,096 rays."""
    if key in SPINE_KEYS:
        dp, layout, axis, bit = SPINES[SPINE_KEYS.index(key)]
        return spine_tree(dp, 0, layout, axis, bit) + spine_rays(dp, 0, layout, axis, bit)
    if key == "shared-spine":
        dp, layout, axis, bit = SHARED_SPINE
        sh = (0, dp - 3)
        return spine_tree(dp, 0, layout, axis, bit, shared=sh) + spine_rays(dp, 0, layout, axis, bit, shared=sh)
    if key.startswith("root-"):
        return root_leaf(key == "root-hit") + box_rays()
    return shared_blocks(int(key.split("-")[1])) + box_rays()


@functools.lru_cache(maxsize=None)
def ref_scene(key):
    import cpuref
    return cpuref.RefScene.octree(case(key)[0])


@functools.lru_cache(maxsize=None)
def oracle(key, tn, tf, n=N):
    """The oracle's (hit, t, normal, prim) of the first n rays of case(key),
    computed once and read-only."""
    _, _, o, d = case(key)
    out = ref_scene(key).intersect_rays(o[:n], d[:n], tn, tf)
    for a in out:
        a.setflags(write=False)
    return out


# frames: 96 x 72, the two modes of tests/scenes.py with the plane at -1.2
FRAME = (96, 72)
PLANE = ((0.0, 1.0, 0.0), -1.2)
FRAME_MODES = {"primary": (0, False), "default": (1, True)}  # shading mode, plane


def cameras(key):
    """Three (position, target, up) per tree: outside the root box; inside it,
    looking along the spine's axis at the end of the spine; within 4 edges of
    the deepest inner box. The small trees: outside, inside, and close to the
    centre of a level-2 box."""
    _, desc, _, _ = case(key)
    if not hasattr(desc, "path"):
        return [((0.9, 0.7, 2.3), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0)),
                ((0.35, 0.3, 0.8), (-0.1, -0.05, 0.0), (0.0, 1.0, 0.0)),
                ((0.3, 0.35, 0.55), (0.25, 0.25, 0.25), (0.0, 1.0, 0.0))]
    lo, hi = desc.lo[-1], desc.hi[-1]
    c = (lo + hi) / 2
    edge = float(hi[0] - lo[0])
    up = (0.0, 0.0, 1.0) if desc.axis == 1 else (0.0, 1.0, 0.0)
    inside = c + np.array([0.05, 0.04, 0.03])
    inside[desc.axis] = c[desc.axis] + (0.7 if desc.bit == 0 else -0.7)
    inside = np.clip(inside, -0.9, 0.9)
    # the close camera looks at the largest surface leaf, the root's child: from
    # the depths of a tall tree nothing nearer than the frame's tNear = 0.01 shows
    near = c + np.array([0.5, 0.4, 0.75]) / np.linalg.norm([0.5, 0.4, 0.75]) * 3.0 * edge
    j = int(np.flatnonzero(desc.kind[desc.offset[0]:desc.offset[0] + 8] == SURFACE)[0])
    slo, shi = child_box(desc.lo[0], desc.hi[0], j)
    t3 = lambda v: tuple(float(F(x)) for x in v)
    return [((0.9, 0.7, 2.3), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0)), (t3(inside), t3(c), up),
            (t3(near), t3((slo + shi) / 2), (0.0, 1.0, 0.0))]


def frame_params(key, cam, mode, module=None):
    """Render parameters of camera `cam` (0..2) of cameras(key); module: cpuref
    (the default) or rtamd."""
    import cpuref
    pos, target, up = cameras(key)[cam]
    W, H = FRAME
    vi, pi = cpuref.camera_matrices(pos, target, up, 45.0, W / H, 0.01, 100.0)
    sm = FRAME_MODES[mode][0]
    if module is None or module is cpuref:
        return cpuref.make_params(pos, vi, pi, (2.0, 2.0, 2.0), sm, True, True)
    return module.render_params(pos, vi, pi, (2.0, 2.0, 2.0), sm, True, True)


@functools.lru_cache(maxsize=None)
def oracle_frame(key, cam, mode):
    """The oracle's (colour, t) of one frame, computed once and read-only."""
    rs = ref_scene(key)
    rs.set_plane(FRAME_MODES[mode][1], *PLANE)
    W, H = FRAME
    c, t, _, _ = rs.render(frame_params(key, cam, mode), W, H)
    rs.set_plane(False, *PLANE)  # ref_scene(key) is shared: every other user wants it bare
    c.setflags(write=False)
    t.setflags(write=False)
    return c, t


# ------------------------------------------------------ the instanced scene --
# one instance each of a packed tree, a 15-slot and a 31-slot tree (both with
# unpacked coordinates) and the cube mesh, under rigid poses (an SDF instance
# wants one: the march steps in units of the transformed direction)
INSTANCE_BLAS = (spine_key(8, "bfs", 0, 0), spine_key(9, "shuffled", 1, 1), spine_key(17, "shuffled", 2, 0), "cube")
INSTANCE_CENTRES = [(-1.2, -1.2, 0.1), (1.2, -1.2, -0.1), (-1.2, 1.2, -0.2), (1.2, 1.2, 0.2)]


def instance_defs():
    """[(blas, xform, flags)] of the four instances."""
    import mixed_common as MC
    return [(i, MC.rigid(7100 + i, c), 0) for i, c in enumerate(INSTANCE_CENTRES)]


@functools.lru_cache(maxsize=None)
def instance_refs():
    """BLAS index -> oracle scene."""
    import instances_common as IC
    return {i: IC.ref_mesh(k) if k == "cube" else ref_scene(k) for i, k in enumerate(INSTANCE_BLAS)}


@functools.lru_cache(maxsize=None)
def instance_rays(n=N, seed=0):
    """Origins within 4 of the centre, each aimed at a point within 0.9 of a
    seeded instance's centre."""
    rng = _rng("instance_rays", n, seed)
    o = rng.uniform(-4.0, 4.0, (n, 3))
    p = np.asarray(INSTANCE_CENTRES)[rng.integers(0, 4, n)] + rng.uniform(-0.9, 0.9, (n, 3))
    o, d = _finish(o, np.where(np.abs(p - o) < 1e-3, 1e-3, p - o))
    o.setflags(write=False)
    d.setflags(write=False)
    return o, d


def instance_host_oracle(rt, tlas, tn, tf):
    """The header's loop composed from the oracle on host data alone (M by
    rt_affine_inverse; the leaf boxes from the unit cube and the mesh's
    vertex box, as mixed_common.host_scene does) -> (hit, t, normal, prim)."""
    import instances_common as IC
    import mixed_common as MC
    import tlas_common as TC
    inst = instance_defs()
    blas, flags = [t[0] for t in inst], [t[2] for t in inst]
    M = np.stack([rt.affine_inverse(t[1]) for t in inst])
    o, d = instance_rays()
    if not tlas:
        return IC.compose(instance_refs(), blas, flags, M, o, d, tn, tf)
    boxes = [TC.vertex_box(IC.mesh("cube")[0]) if k == "cube" else MC.UNIT_CUBE for k in INSTANCE_BLAS]
    wbox = TC.leaf_boxes([t[1] for t in inst], blas, flags, boxes)
    return TC.compose_tlas(instance_refs(), blas, flags, M, wbox, o, d, tn, tf)[:4]
