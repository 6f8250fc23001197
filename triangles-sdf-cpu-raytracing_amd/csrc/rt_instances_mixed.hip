// rt_instances_mixed.hip -- instanced scenes whose bottom-level scenes are not
// all meshes (rt_scene_create_instanced_any, include/rtamd.h; DESIGN.md section
// 4a, "Mixed bottom-level kinds"): the trace kernels over the flat list and the
// top-level tree, the two adapters that give shade_one (rt_shade.h) such a
// scene with the interface of MeshS and their shade kernels. (The tree's leaf
// boxes are rt_tlas.hip's tlas_box_kernel over this table, a dynamic mesh's
// entry blas_entry_launch on the record's mesh view.)
//
// A translation unit of its own, as rt_instances.hip, rt_tlas.hip and
// rt_shade_instances.hip, on the same shared pieces (rt_instance_dev.h,
// rt_ray_io.h). Mesh-only scenes never come here.
//
// What is compile time and what is run time. The stack slots (with_slots over
// the deepest mesh or octree BLAS; both traversals use frames of 3 words, so
// one LdsStack serves both) and the ray mode are template arguments. The kind
// of a BLAS, a grid's launch mode and an octree's PACK bit are run-time
// branches on the table record: templating on them as well would multiply to
// hundreds of kernels. Every such branch is taken on a wave-uniform value: in
// the flat list the record's address is uniform; in the tree a round handles
// its lanes kind by kind, and inside an SDF kind BLAS by BLAS (the lanes that
// hold the lowest pending BLAS run together, its record read through a uniform
// address), so the compiler never has three traversals under one mask, a
// grid's buffer resource stays in SGPRs and the switch over its mode is a
// scalar branch.
//
// The SDF winner's normal. grid_intersect and oct_intersect evaluate the normal
// at every hit; here a candidate's normal is evaluated only in the modes that
// return one (kRaysNormal, shading) and only when the candidate is accepted
// (t < best), at that moment, from the march's hit point: the same function on
// the same operands as the plain kind's, so the same bits. A mesh winner's
// normal is taken from its triangle after the loop, as in the mesh-only
// kernels. All stores are plain vector stores; there is no inline assembly and
// no device-scope waiting.
#include <hip/hip_runtime.h>

#include "rt_dispatch.h"
#include "rt_error.h"
#include "rt_instance_dev.h"
#include "rt_ray_io.h"
#include "rt_shade_rays.h"

using namespace rtd;

namespace {

constexpr int kMBlock = 64;  // one wave, as trace_instances_kernel
static_assert(kMBlock == kSBlock, "the trace and the shade kernels share the per-lane code");
// rt_tlas.hip's threshold: a round of the tree trace takes the wave-level mesh
// traversal when at least this many lanes hold the wave's lowest candidate
constexpr int kUniformMin = 16;
constexpr uint32_t kNoKind = 0xFFFFFFFFu;

// What a lane keeps of its best candidate so far: t, the instance, the
// primitive (mesh: triangle slot; grid: cell; octree: node) and, for an SDF
// candidate in a mode with normals, the object-space normal.
struct Winner {
  float best = kInf;
  int32_t wi = -1;
  uint32_t wk = 0;
  f3 n{0.0f, 0.0f, 0.0f};
};

// ---- one SDF BLAS on one lane ------------------------------------------------
// SDFGrid::intersect of the plain kind (grid_intersect, rt_scenes.h) with the
// normal put off until the hit is accepted
template <int kMode, bool NORMAL, class CT>
__device__ __forceinline__ void try_grid(const GridDev &g, f3 oo, f3 dd, float tn, float tfi, int32_t k, Winner &w,
                                         CT &cnt) {
  float t;
  f3 hp;
  uint32_t cell;
  if (grid_march<kMode>(g, oo, dd, tn, tfi, t, hp, cell, cnt) && t < w.best) {  // ties keep the lower index
    w.best = t;
    w.wi = k;
    w.wk = cell;
    if constexpr (NORMAL) w.n = grid_normal<kMode>(g, hp, cnt);
  }
}
// the switch over a grid's launch mode: rt_dispatch.h's three instantiations
template <bool NORMAL, class CT>
__device__ __forceinline__ void try_grid_var(uint32_t var, const GridDev &g, f3 oo, f3 dd, float tn, float tfi,
                                             int32_t k, Winner &w, CT &cnt) {
  switch (var) {
    case kGridBuf | kGridBricked: try_grid<kGridBuf | kGridBricked, NORMAL>(g, oo, dd, tn, tfi, k, w, cnt); break;
    case kGridBricked: try_grid<kGridBricked, NORMAL>(g, oo, dd, tn, tfi, k, w, cnt); break;
    default: try_grid<kGridBuf, NORMAL>(g, oo, dd, tn, tfi, k, w, cnt); break;
  }
}
template <class CT>
__device__ __forceinline__ bool occ_grid_var(uint32_t var, const GridDev &g, f3 oo, f3 dd, float tn, float tf,
                                             CT &cnt) {
  switch (var) {
    case kGridBuf | kGridBricked: return grid_occluded<kGridBuf | kGridBricked>(g, oo, dd, tn, tf, cnt);
    case kGridBricked: return grid_occluded<kGridBricked>(g, oo, dd, tn, tf, cnt);
    default: return grid_occluded<kGridBuf>(g, oo, dd, tn, tf, cnt);
  }
}

// SDFOctree::intersect of the plain kind (oct_trace, rt_scenes.h) that hands
// out the hit point instead of the normal
template <int B, bool PACK, class CT>
__device__ __forceinline__ bool oct_trace_hp(const OctDev &sc, f3 o, f3 d, float tNear, float tFar,
                                             LdsStack<B, kOctFields> st, float &out_t, OctHitPt &hp, CT &cnt) {
  const f3 inv{1.0f / d.x, 1.0f / d.y, 1.0f / d.z};
  OctRay R;
  int s;
  if (__builtin_isfinite(inv.x) && __builtin_isfinite(inv.y) && __builtin_isfinite(inv.z) && tNear > 0.0f) {
    s = oct_start<true>(sc, o, d, inv, tNear, tFar, R, out_t, hp, cnt);
    if (s == RAY_PENDING) s = oct_run<B, true, false, PACK>(sc, o, d, inv, tNear, tFar, st, R, 0, out_t, hp, cnt);
  } else {
    s = oct_start<false>(sc, o, d, inv, tNear, tFar, R, out_t, hp, cnt);
    if (s == RAY_PENDING) s = oct_run<B, false, false, PACK>(sc, o, d, inv, tNear, tFar, st, R, 0, out_t, hp, cnt);
  }
  return s == RAY_HIT;
}
template <int B, bool PACK, bool NORMAL, class CT>
__device__ __forceinline__ void try_oct(const OctDev &sc, f3 oo, f3 dd, float tn, float tfi, int32_t k,
                                        LdsStack<B, kOctFields> st, Winner &w, CT &cnt) {
  float t;
  OctHitPt hp;
  if (oct_trace_hp<B, PACK>(sc, oo, dd, tn, tfi, st, t, hp, cnt) && t < w.best) {  // ties keep the lower index
    w.best = t;
    w.wi = k;
    w.wk = hp.node;
    if constexpr (NORMAL) w.n = oct_normal_at(sc, hp, cnt);
  }
}

// One SDF BLAS, its record read through a wave-uniform address: the switches
// over kind, grid mode and PACK are scalar branches.
template <int B, bool NORMAL, class CT>
__device__ __forceinline__ void try_sdf(const rti::BlasRec *__restrict__ e, f3 oo, f3 dd, float tn, float tfi,
                                        int32_t k, LdsStack<B, kOctFields> st, Winner &w, CT &cnt) {
  const uint32_t var = e->var;
  if (e->kind == RT_SCENE_GRID) {
    const GridDev g = e->grid;
    try_grid_var<NORMAL>(var, g, oo, dd, tn, tfi, k, w, cnt);
  } else {
    const OctDev oc = e->oct;
    if (var)
      try_oct<B, true, NORMAL>(oc, oo, dd, tn, tfi, k, st, w, cnt);
    else
      try_oct<B, false, NORMAL>(oc, oo, dd, tn, tfi, k, st, w, cnt);
  }
}
template <int B, class CT>
__device__ __forceinline__ bool occ_sdf(const rti::BlasRec *__restrict__ e, f3 oo, f3 dd, float tn, float tf,
                                        LdsStack<B, kOctFields> st, CT &cnt) {
  const uint32_t var = e->var;
  if (e->kind == RT_SCENE_GRID) {
    const GridDev g = e->grid;
    return occ_grid_var(var, g, oo, dd, tn, tf, cnt);
  }
  const OctDev oc = e->oct;
  return var ? oct_occluded<B, true>(oc, oo, dd, tn, tf, st, cnt) : oct_occluded<B, false>(oc, oo, dd, tn, tf, st, cnt);
}

// The winner's Hit, per lane (lanes differ in wi): prim = (instance << 32) | p,
// p what the plain kind reports (original triangle id, grid cell, octree
// node); the object-space normal (the triangle's, or the one kept at the
// accept) under M^T, normalised.
template <bool NORMAL>
__device__ __forceinline__ Hit winner_hit(const rti::InstRec *inst, const rti::BlasRec *tab, const Winner &w) {
  Hit h = miss_hit();
  if (w.wi >= 0) {
    const rti::InstRec *rp = inst + w.wi;
    const rti::BlasRec *e = tab + rp->blas;
    f3 n = w.n;
    uint32_t p = w.wk;
    if (e->kind == RT_SCENE_MESH) {
      const rtl::GTri *tris = e->mesh.tris;
      if constexpr (NORMAL) n = tri_normal(tris, w.wk);
      p = tris[w.wk].orig_id;
    }
    h.hit = true;
    h.t = w.best;
    if constexpr (NORMAL) h.n = world_normal(rp->m, n);
    h.prim = inst_prim(w.wi, p);
  }
  return h;
}

// ---- the per-lane round of the tree ------------------------------------------
// Every lane with `have` searches its own candidate `cand` under tfi (any hit:
// the full tFar). Nothing here needs the whole wave: the lanes that are in the
// call take part in the ballots, the others are not waited for, so the shade
// adapter calls it inside shade_one's divergent branches. Phases: the lanes
// with a mesh candidate (record and MeshDev per lane, the per-lane traversal),
// then the grids, then the octrees, an SDF phase BLAS by BLAS in the order of
// the lanes that hold them; a phase nobody is in is skipped by its ballot.
template <int B, bool ANY, bool NORMAL, class CT>
__device__ __forceinline__ void round_lanes(const rti::InstRec *__restrict__ inst,
                                            const rti::BlasRec *__restrict__ tab, bool have, uint32_t cand, f3 o,
                                            f3 d, float tn, float tfi, LdsStack<B, 3> st, Winner &w, bool &occ,
                                            CT &cnt) {
  uint32_t kind = kNoKind;
  int32_t bl = 0;
  f3 oo{0.0f, 0.0f, 0.0f}, dd{0.0f, 0.0f, 1.0f};
  if (have) {
    const rti::InstRec *rp = inst + cand;
    const uint32_t off = (rp->flags & RT_INSTANCE_DISABLED) | rp->skipped;
    if (!off) {
      bl = rp->blas;
      kind = tab[bl].kind;
      float m[12];
      load_m(rp, m);
      oo = xf_point(m, o);
      dd = xf_dir(m, d);
    }
  }
  if (__ballot(kind == (uint32_t)RT_SCENE_MESH) != 0) {
    if (kind == (uint32_t)RT_SCENE_MESH) {
      const MeshDev md = load_md(&tab[bl].mesh);
      if (md.root != rtl::kInvalidChild) {
        if constexpr (ANY) {
          if (mesh_occluded<B>(md, oo, dd, tn, tfi, st, cnt)) occ = true;
        } else {
          float t = kInf;
          uint32_t tri = 0;
          if (mesh_trace<B, false>(md, oo, dd, tn, tfi, st, t, tri, cnt) && t < w.best) {
            w.best = t;
            w.wi = (int32_t)cand;
            w.wk = tri;
          }
        }
      }
    }
  }
#pragma unroll 1
  for (uint32_t phase = (uint32_t)RT_SCENE_GRID; phase <= (uint32_t)RT_SCENE_OCTREE; ++phase) {
    uint64_t mk = __ballot(kind == phase);
    while (mk != 0) {
      const int32_t ub = __builtin_amdgcn_readlane(bl, (int)__builtin_ctzll(mk));  // a pending lane's BLAS
      const bool me = kind == phase && bl == ub;
      const rti::BlasRec *e = tab + ub;
      if (me) {
        if constexpr (ANY) {
          if (occ_sdf<B>(e, oo, dd, tn, tfi, st, cnt)) occ = true;
        } else {
          try_sdf<B, NORMAL>(e, oo, dd, tn, tfi, (int32_t)cand, st, w, cnt);
        }
      }
      mk &= ~__ballot(me);
    }
  }
}

// ---- the flat list -----------------------------------------------------------
// The header's loop, wave-uniform over the instances as trace_instances_kernel:
// record and table entry through uniform addresses. A mesh instance keeps that
// kernel's body (the root pre-test, mesh_primary_wave where the batch has one
// tNear); an SDF instance runs its march or its octree traversal per lane. An
// SDF instance is skipped by nothing but its own intersection's tests.
template <int SLOTS, int MODE>
__global__ __launch_bounds__(kMBlock) void trace_mixed_kernel(const rti::InstRec *__restrict__ inst,
                                                              const rti::BlasRec *__restrict__ tab, int32_t ninst,
                                                              PlaneDev pl, rt_ray_batch b) {
  __shared__ uint32_t stk[SLOTS * 3 * kMBlock];
  const int64_t i = (int64_t)blockIdx.x * kMBlock + threadIdx.x;
  // a partial last wave keeps its lanes without a ray (mesh_primary_wave needs
  // the whole wave): they carry active = false and touch no memory
  const bool active = i < b.n;
  LdsStack<kMBlock, 3> st{stk + threadIdx.x};
  const RayIn ray = load_ray(b, i, active);
  const f3 o = ray.o, d = ray.d;
  const float tn = ray.tn, tf = ray.tf;
  NoCnt cnt;
  if constexpr (MODE == kRaysAny) {
    // OR over the instances of the bottom-level any hit under the full tFar;
    // a lane that has its hit goes inactive, the wave stops when none is left
    bool live = active, occ = false;
    for (int32_t k = 0; k < ninst; ++k) {
      if (__ballot(live) == 0) break;
      const rti::InstRec r = inst[k];
      if ((r.flags & RT_INSTANCE_DISABLED) || r.skipped) continue;
      const rti::BlasRec *e = tab + r.blas;
      if (e->kind == (uint32_t)RT_SCENE_MESH) {
        const MeshDev md = e->mesh;
        if (md.root == rtl::kInvalidChild) continue;
        if (live) {
          const f3 oo = xf_point(r.m, o), dd = xf_dir(r.m, d);
          if (root_passes(md, oo, dd, tn, tf) && mesh_occluded<kMBlock>(md, oo, dd, tn, tf, st, cnt)) {
            occ = true;
            live = false;
          }
        }
      } else if (live) {
        if (occ_sdf<kMBlock>(e, xf_point(r.m, o), xf_dir(r.m, d), tn, tf, st, cnt)) {
          occ = true;
          live = false;
        }
      }
    }
    if (!active) return;
    store_any(b, i, pl, ray, occ);
  } else {
    constexpr bool NORMAL = MODE == kRaysNormal;
    Winner w;
    for (int32_t k = 0; k < ninst; ++k) {
      const rti::InstRec r = inst[k];
      if ((r.flags & RT_INSTANCE_DISABLED) || r.skipped) continue;
      const rti::BlasRec *e = tab + r.blas;
      const f3 oo = xf_point(r.m, o), dd = xf_dir(r.m, d);
      const float tfi = w.best < tf ? w.best : tf;
      if (e->kind == (uint32_t)RT_SCENE_MESH) {
        const MeshDev md = e->mesh;
        if (md.root == rtl::kInvalidChild) continue;
        const bool go = active && root_passes(md, oo, dd, tn, tfi);
        if (__ballot(go) == 0) continue;  // the whole wave misses this instance's root box
        float t = kInf;
        uint32_t tri = 0;
        bool h;
        // mesh_primary_wave takes one tNear for the wave (tFar is per ray):
        // batches with a d_tnear array take the per-lane traversal
        if (!b.d_tnear)
          h = mesh_primary_wave<kMBlock, 3>(md, oo, dd, tn, tfi, go, stk, t, tri) && go;
        else
          h = go && mesh_trace<kMBlock, false>(md, oo, dd, tn, tfi, st, t, tri, cnt);
        if (h && t < w.best) {  // ties keep the lower index
          w.best = t;
          w.wi = k;
          w.wk = tri;
        }
      } else if (active) {
        try_sdf<kMBlock, NORMAL>(e, oo, dd, tn, tfi, k, st, w, cnt);
      }
    }
    if (!active) return;
    store_closest<MODE>(b, i, pl, ray, winner_hit<NORMAL>(inst, tab, w));
  }
}

// ---- the top-level tree --------------------------------------------------------
// trace_tlas_kernel's loop (rt_tlas.hip): each lane walks its cursor to its
// next candidate; a round then handles either the wave's lowest candidate for
// the lanes that hold it, when it is a mesh and enough lanes share it (the flat
// kernel's mesh body with the wave-level traversal), or every lane's own
// candidate kind by kind (round_lanes). Both give the same bits.
template <int SLOTS, int MODE>
__global__ __launch_bounds__(kMBlock) void trace_mixed_tlas_kernel(const rti::InstRec *__restrict__ inst,
                                                                   const rti::BlasRec *__restrict__ tab,
                                                                   const rtt::TNode *__restrict__ nodes, uint32_t P,
                                                                   PlaneDev pl, rt_ray_batch b) {
  __shared__ uint32_t stk[SLOTS * 3 * kMBlock];
  const int64_t i = (int64_t)blockIdx.x * kMBlock + threadIdx.x;
  // a partial last wave keeps its lanes without a ray (the wave-level steps
  // need the whole wave): their cursor starts at 0 and they touch no memory
  const bool active = i < b.n;
  LdsStack<kMBlock, 3> st{stk + threadIdx.x};
  const RayIn ray = load_ray(b, i, active);
  const f3 o = ray.o, d = ray.d;
  const float tn = ray.tn, tf = ray.tf;
  const f3 inv{1.0f / d.x, 1.0f / d.y, 1.0f / d.z};  // of the WORLD ray: the tree's test
  NoCnt cnt;
  constexpr bool kAny = MODE == kRaysAny;
  constexpr bool NORMAL = MODE == kRaysNormal;
  // the wave-level mesh traversal exists for closest hits of a batch with one tNear
  const bool can_share = !kAny && !b.d_tnear;
  uint32_t n = active ? 1u : 0u;  // the cursor; 0: the walk is over
  bool have = false;              // n rests on a leaf that passed and is not handled yet
  Winner w;
  bool occ = false;
  for (;;) {
    // closest hit: tf_i = best < tFar ? best : tFar; any hit: the full tFar
    const float tfi = kAny ? tf : (w.best < tf ? w.best : tf);
    if (!have) {
      n = lane_next(nodes, P, n, o, inv, tn, tfi);
      have = n != 0u;
    }
    if (__ballot(have) == 0) break;
    const uint32_t cand = have ? n - P : 0xFFFFFFFFu;
    bool handled = have;
    bool shared = false;
    if (can_share) {
      const uint32_t low = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave_min(cand));
      const bool mine = have && cand == low;
      const rti::InstRec r = inst[low];
      const rti::BlasRec *e = tab + r.blas;
      if ((int)__popcll(__ballot(mine)) >= kUniformMin && e->kind == (uint32_t)RT_SCENE_MESH) {
        shared = true;
        handled = mine;
        const MeshDev md = e->mesh;
        if (!((r.flags & RT_INSTANCE_DISABLED) || r.skipped || md.root == rtl::kInvalidChild)) {
          const f3 oo = xf_point(r.m, o), dd = xf_dir(r.m, d);
          const bool go = mine && root_passes(md, oo, dd, tn, tfi);
          if (__ballot(go) != 0) {
            float t = kInf;
            uint32_t tri = 0;
            const bool h = mesh_primary_wave<kMBlock, 3>(md, oo, dd, tn, tfi, go, stk, t, tri) && go;
            if (h && t < w.best) {  // ties keep the lower index
              w.best = t;
              w.wi = (int32_t)low;
              w.wk = tri;
            }
          }
        }
      }
    }
    if (!shared) round_lanes<kMBlock, kAny, NORMAL>(inst, tab, have, cand, o, d, tn, tfi, st, w, occ, cnt);
    if (handled) {
      // any hit: a lane that has its hit is done
      n = (kAny && occ) ? 0u : rtt::walk_skip(n);
      have = false;
    }
  }
  if (!active) return;
  if constexpr (kAny)
    store_any(b, i, pl, ray, occ);
  else
    store_closest<MODE>(b, i, pl, ray, winner_hit<NORMAL>(inst, tab, w));
}

// ---- the adapters of the shade kernels ----------------------------------------
// Per lane only, for the reason rt_shade_instances.hip gives: shade_one calls
// them inside lane-divergent branches. The flat adapter's loop stays uniform
// over the lanes that are in the call (they all start at instance 0 and skip on
// values they share), so records and table entries still arrive by scalar
// loads and the kind switch is a scalar branch.
struct MixedFlatS {
  static constexpr int kFields = 3;
  const rti::InstRec *__restrict__ inst;
  const rti::BlasRec *__restrict__ tab;
  int32_t ninst;
  template <int B, class CT>
  __device__ __forceinline__ Hit intersect(f3 o, f3 d, float tn, float tf, LdsStack<B, kFields> st, CT &cnt) const {
    Winner w;
    for (int32_t k = 0; k < ninst; ++k) {
      const rti::InstRec r = inst[k];
      if ((r.flags & RT_INSTANCE_DISABLED) || r.skipped) continue;
      const rti::BlasRec *e = tab + r.blas;
      const f3 oo = xf_point(r.m, o), dd = xf_dir(r.m, d);
      const float tfi = w.best < tf ? w.best : tf;
      if (e->kind == (uint32_t)RT_SCENE_MESH) {
        const MeshDev md = e->mesh;
        if (md.root == rtl::kInvalidChild) continue;
        const bool go = root_passes(md, oo, dd, tn, tfi);
        if (__ballot(go) == 0) continue;  // every lane of the call misses this instance's root box
        float t = kInf;
        uint32_t tri = 0;
        if (go && mesh_trace<B, false>(md, oo, dd, tn, tfi, st, t, tri, cnt) && t < w.best) {
          w.best = t;
          w.wi = k;
          w.wk = tri;
        }
      } else {
        try_sdf<B, true>(e, oo, dd, tn, tfi, k, st, w, cnt);
      }
    }
    return winner_hit<true>(inst, tab, w);
  }
  // OR over the instances of the bottom-level any hit under the full tFar; a
  // lane that has its hit waits, the loop ends when none of the call's lanes is left
  template <int B, class CT>
  __device__ __forceinline__ bool occluded(f3 o, f3 d, float tn, float tf, LdsStack<B, kFields> st, CT &cnt) const {
    bool live = true;
    for (int32_t k = 0; k < ninst; ++k) {
      if (__ballot(live) == 0) break;
      const rti::InstRec r = inst[k];
      if ((r.flags & RT_INSTANCE_DISABLED) || r.skipped) continue;
      const rti::BlasRec *e = tab + r.blas;
      if (e->kind == (uint32_t)RT_SCENE_MESH) {
        const MeshDev md = e->mesh;
        if (md.root == rtl::kInvalidChild) continue;
        if (live) {
          const f3 oo = xf_point(r.m, o), dd = xf_dir(r.m, d);
          if (root_passes(md, oo, dd, tn, tf) && mesh_occluded<B>(md, oo, dd, tn, tf, st, cnt)) live = false;
        }
      } else if (live) {
        if (occ_sdf<B>(e, xf_point(r.m, o), xf_dir(r.m, d), tn, tf, st, cnt)) live = false;
      }
    }
    return !live;
  }
};

// The top-level tree: each lane walks its own cursor and searches its own
// candidates in index order; a round is round_lanes over the lanes of the call
// that still have a candidate.
struct MixedTlasS {
  static constexpr int kFields = 3;
  const rti::InstRec *__restrict__ inst;
  const rti::BlasRec *__restrict__ tab;
  const rtt::TNode *__restrict__ nodes;
  uint32_t P;
  template <int B, class CT>
  __device__ __forceinline__ Hit intersect(f3 o, f3 d, float tn, float tf, LdsStack<B, kFields> st, CT &cnt) const {
    const f3 inv{1.0f / d.x, 1.0f / d.y, 1.0f / d.z};  // of the WORLD ray: the tree's test
    Winner w;
    bool occ = false;
    uint32_t n = 1u;
    for (;;) {
      const float tfi = w.best < tf ? w.best : tf;
      n = lane_next(nodes, P, n, o, inv, tn, tfi);
      const bool have = n != 0u;
      if (__ballot(have) == 0) break;
      round_lanes<B, false, true>(inst, tab, have, have ? n - P : 0u, o, d, tn, tfi, st, w, occ, cnt);
      if (have) n = rtt::walk_skip(n);
    }
    return winner_hit<true>(inst, tab, w);
  }
  // the candidates under the full tFar; a lane stops walking at its first hit
  template <int B, class CT>
  __device__ __forceinline__ bool occluded(f3 o, f3 d, float tn, float tf, LdsStack<B, kFields> st, CT &cnt) const {
    const f3 inv{1.0f / d.x, 1.0f / d.y, 1.0f / d.z};
    Winner w;
    bool occ = false;
    uint32_t n = 1u;
    for (;;) {
      n = occ ? 0u : lane_next(nodes, P, n, o, inv, tn, tf);
      const bool have = n != 0u;
      if (__ballot(have) == 0) break;
      round_lanes<B, true, false>(inst, tab, have, have ? n - P : 0u, o, d, tn, tf, st, w, occ, cnt);
      if (have) n = rtt::walk_skip(n);
    }
    return occ;
  }
};

template <int SLOTS>
__global__ __launch_bounds__(kSBlock) __attribute__((amdgpu_waves_per_eu(RT_SHADE_WAVES)))
void shade_mixed_kernel(const rti::InstRec *__restrict__ inst, const rti::BlasRec *__restrict__ tab, int32_t ninst,
                        PlaneDev pl, rt_render_params P, rt_ray_batch b, uint32_t *d_color, uint32_t flags) {
  __shared__ uint32_t stk[SLOTS * 3 * kSBlock];
  const MixedFlatS sc{inst, tab, ninst};
  shade_rays_body<MixedFlatS, SLOTS>(sc, pl, P, b, d_color, flags, stk);
}

template <int SLOTS>
__global__ __launch_bounds__(kSBlock) __attribute__((amdgpu_waves_per_eu(RT_SHADE_WAVES)))
void shade_mixed_tlas_kernel(const rti::InstRec *__restrict__ inst, const rti::BlasRec *__restrict__ tab,
                             const rtt::TNode *__restrict__ nodes, uint32_t leaves, PlaneDev pl, rt_render_params P,
                             rt_ray_batch b, uint32_t *d_color, uint32_t flags) {
  __shared__ uint32_t stk[SLOTS * 3 * kSBlock];
  const MixedTlasS sc{inst, tab, nodes, leaves};
  shade_rays_body<MixedTlasS, SLOTS>(sc, pl, P, b, d_color, flags, stk);
}

template <int SLOTS>
void launch_trace_t(const rti::MixedArgs &m, const PlaneDev &pl, const rt_ray_batch &b, int mode, hipStream_t st) {
  const unsigned blocks = (unsigned)((b.n + kMBlock - 1) / kMBlock);
  const rti::InstArgs &a = m.a;
  const uint32_t P = (uint32_t)a.tlas_leaves;
  with_mode(mode, [&](auto md) {
    constexpr int M = decltype(md)::value;
    if (a.tlas)
      trace_mixed_tlas_kernel<SLOTS, M><<<blocks, kMBlock, 0, st>>>(a.inst, m.tab, a.tlas, P, pl, b);
    else
      trace_mixed_kernel<SLOTS, M><<<blocks, kMBlock, 0, st>>>(a.inst, m.tab, a.ninst, pl, b);
  });
}

}  // namespace

namespace rti {

int trace_mixed_launch(const MixedArgs &a, const PlaneDev &pl, const rt_ray_batch &b, int mode, hipStream_t st) {
  with_slots(a.a.maxd, [&](auto slots) { launch_trace_t<decltype(slots)::value>(a, pl, b, mode, st); });
  HIP_TRY(hipGetLastError());
  return RT_OK;
}

int shade_mixed_launch(const MixedArgs &m, const PlaneDev &pl, const rt_render_params &p, const rt_ray_batch &b,
                       uint32_t *d_color, uint32_t flags, hipStream_t st) {
  const unsigned blocks = (unsigned)((b.n + kSBlock - 1) / kSBlock);
  const InstArgs &a = m.a;
  with_slots(a.maxd, [&](auto slots) {
    constexpr int N = decltype(slots)::value;
    if (a.tlas)
      shade_mixed_tlas_kernel<N><<<blocks, kSBlock, 0, st>>>(a.inst, m.tab, a.tlas, (uint32_t)a.tlas_leaves, pl, p, b,
                                                             d_color, flags);
    else
      shade_mixed_kernel<N><<<blocks, kSBlock, 0, st>>>(a.inst, m.tab, a.ninst, pl, p, b, d_color, flags);
  });
  HIP_TRY(hipGetLastError());
  return RT_OK;
}

}  // namespace rti
