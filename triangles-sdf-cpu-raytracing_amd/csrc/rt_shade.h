// rt_shade.h -- device code the kernels of several units share (gfx950): the
// scene adapters that give the three scene kinds one interface (MeshS, GridS,
// OctS), their LDS stacks, the scene-and-plane union, the shading of one ray
// and the modes of a ray batch. Included by the units that define kernels over
// scenes (rt_device.hip, rt_instances.hip) and by rt_dispatch.h; everything
// here is internal to the including unit, so a kernel's name does not depend
// on the unit that instantiates it.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/rtamd.h"
#include "rt_math.h"
#include "rt_scenes.h"

using namespace rtd;

namespace {

constexpr int kBlock = 256;  // 4 waves, 16x16 pixels

// ---------------------------------------------------------- scene adapters --
// kFields = LDS words per traversal frame (mesh: node, list|count, best t;
// octree: children block, list|count, leaf mask|depth; grid: none). StackOf:
// the adapter's per-lane stack; stack_words: its LDS words per lane at SLOTS
// slots.
// occupancy floors (min_waves below), overridable for A/B builds
#ifndef RT_GRID_WAVES
#define RT_GRID_WAVES 1
#endif
#ifndef RT_OCT_WAVES
#define RT_OCT_WAVES 6
#endif
// mesh primary: a floor of 5 waves per SIMD (102 VGPRs). Built without the SLP
// vectorizer (Makefile) the persistent kernel takes 96 VGPRs and 36 B of
// scratch per lane at 5 waves, and is faster than at 4 (117 VGPRs, no
// scratch): bunny 8 x 2 0.0855 -> 0.0825, the 1.1 M-triangle stand-in 0.3314 ->
// 0.3149 ms/frame (profiles/r05/slp_ab.txt, two rounds). With SLP on, 5 waves
// were slower.
#ifndef RT_MESH_WAVES
#define RT_MESH_WAVES 5
#endif
// shading kernels (GENERAL, the reference's default mode): a floor of 4 waves
// per SIMD. The mesh's takes 135 VGPRs (3 waves) on its own; at 4 it gets 127
// and spills 12 B per lane, and is faster: bunny default mode 1080p, 8 frames
// x 2 / x 1 streams, 0.2267 -> 0.2068 / 0.2877 -> 0.2738 ms/frame (same box).
// 1 = the compiler's choice (A/B switch).
#ifndef RT_GENERAL_WAVES
#define RT_GENERAL_WAVES 4
#endif
template <class S, int B>
using StackOf = LdsStack<B, S::kFields>;
template <class S, int SLOTS>
constexpr int stack_words() { return SLOTS * S::kFields; }
struct MeshS {
  static constexpr int kFields = 3;
  static constexpr bool kCoop = true;  // primary rays: wave-cooperative tail (mesh_primary_wave)
  static constexpr int kMinWaves = RT_MESH_WAVES;
  static constexpr int kQueueGroup = 2;  // wave tiles per work-queue item (render_persist_kernel)
  MeshDev d;
  // rays at or below which the wave hands its remaining rays to 8-lane groups
  // (wave-uniform; the persistent kernel raises it for a wave's last item)
  int coop_rays = kCoopRays;
  // traversal iterations after which a wave raises its priority (0: never;
  // the persistent kernel sets RT_HEAVY_PRIO, the one-frame kernel keeps 0)
  int prio_iters = 0;
  template <int B>
  __device__ __forceinline__ Hit primary(f3 o, f3 dir, float tn, float tf, bool active,
                                         uint32_t *stk) const {
    float t;
    uint32_t k;
    Hit h = miss_hit();
    if (mesh_primary_wave<B, kFields, true>(d, o, dir, tn, tf, active, stk, t, k, coop_rays, prio_iters) && active) {
      h.hit = true;
      h.t = t;
      h.n = tri_normal(d.tris, k);
      h.prim = (int64_t)d.tris[k].orig_id;
    }
    return h;
  }
  // the counting kernel's primary rays: the same wave path with the work
  // counters, its cooperative tail off (the 8-lane groups do not count; they
  // start below the shared fetch's lane threshold, so the wave-level counters
  // are the timed kernels')
  template <int B, class CT>
  __device__ __forceinline__ Hit primary_counted(f3 o, f3 dir, float tn, float tf, bool active, uint32_t *stk,
                                                 CT &cnt) const {
    float t;
    uint32_t k;
    Hit h = miss_hit();
    MeshDev dc = d;
    dc.coop = false;
    if (mesh_primary_wave<B, kFields, true>(dc, o, dir, tn, tf, active, stk, t, k, kCoopRays, 0, cnt) && active) {
      h.hit = true;
      h.t = t;
      h.n = tri_normal(d.tris, k);
      h.prim = (int64_t)d.tris[k].orig_id;
    }
    return h;
  }
  template <int B, class CT>
  __device__ __forceinline__ Hit intersect(f3 o, f3 dir, float tn, float tf,
                                           LdsStack<B, kFields> st, CT &cnt) const {
    return mesh_intersect<B>(d, o, dir, tn, tf, st, cnt);
  }
  template <int B, class CT>
  __device__ __forceinline__ bool occluded(f3 o, f3 dir, float tn, float tf,
                                           LdsStack<B, kFields> st, CT &cnt) const {
    return mesh_occluded<B>(d, o, dir, tn, tf, st, cnt);
  }
};
template <int kMode>
struct GridS {
  static constexpr int kFields = 1;  // no traversal stack (one unused LDS word per lane)
  static constexpr bool kCoop = false;
  static constexpr int kMinWaves = RT_GRID_WAVES;
  // block dispatch: a grid tile is too short for the queue's claims to pay
  // (256^3, 8 frames x 2 streams: 0.0506 ms/frame vs 0.0541 at 4 tiles per claim)
  static constexpr int kQueueGroup = 0;
  GridDev d;
  template <int B, class CT>
  __device__ __forceinline__ Hit intersect(f3 o, f3 dir, float tn, float tf,
                                           LdsStack<B, kFields> st, CT &cnt) const {
    return grid_intersect<kMode>(d, o, dir, tn, tf, cnt);
  }
  template <int B, class CT>
  __device__ __forceinline__ bool occluded(f3 o, f3 dir, float tn, float tf,
                                           LdsStack<B, kFields> st, CT &cnt) const {
    return grid_occluded<kMode>(d, o, dir, tn, tf, cnt);
  }
};
// PACK: the traversal carries the node coordinates packed in one register
// (OctXYZ; trees of depth <= 8, i.e. up to 7 stack slots)
template <bool PACK>
struct OctS {
  static constexpr int kFields = kOctFields;
  static constexpr bool kCoop = false;
  static constexpr int kMinWaves = RT_OCT_WAVES;
  static constexpr int kQueueGroup = 2;
  OctDev d;
  template <int B, class CT>
  __device__ __forceinline__ Hit intersect(f3 o, f3 dir, float tn, float tf,
                                           LdsStack<B, kFields> st, CT &cnt) const {
    return oct_intersect<B, PACK>(d, o, dir, tn, tf, st, cnt);
  }
  template <int B, class CT>
  __device__ __forceinline__ bool occluded(f3 o, f3 dir, float tn, float tf,
                                           LdsStack<B, kFields> st, CT &cnt) const {
    return oct_occluded<B, PACK>(d, o, dir, tn, tf, st, cnt);
  }
};

// SceneUnion(scene, plane)::intersect (raytracing.hpp:87-93): both are
// intersected, the smaller t wins, ties go to the plane.
struct SurfHit {
  Hit h;
  float albedo;   // grey albedo: mesh/SDF 1.0, plane checker 0.0 / 1.0
  float refl;     // reflectiveness: plane 0.3, else 0
};
template <class S, int B, class CT>
__device__ __forceinline__ SurfHit union_intersect(const S &sc, const PlaneDev &pl, f3 o, f3 d,
                                                   float tn, float tf, StackOf<S, B> st, CT &cnt) {
  cnt.add(C_RAYS, 1);
  SurfHit r{sc.template intersect<B>(o, d, tn, tf, st, cnt), 1.0f, 0.0f};
  if (pl.on) {
    float tp = kInf, ap = 1.0f;
    const bool ph = plane_hit(pl, o, d, tn, tf, tp, ap);
    if (!(r.h.t < (ph ? tp : kInf))) {
      if (ph) {
        r.h = Hit{true, tp, pl.n, -2};
        r.albedo = ap;
        r.refl = 0.3f;
      } else {
        r.h = miss_hit();
        r.albedo = 1.0f;
        r.refl = 0.0f;
      }
    }
  }
  return r;
}
// Shadow query: HitInfo::hitten of the union is the OR of both hitten flags.
template <class S, int B, class CT>
__device__ __forceinline__ bool union_occluded(const S &sc, const PlaneDev &pl, f3 o, f3 d, float tn,
                                               float tf, StackOf<S, B> st, CT &cnt) {
  cnt.add(C_RAYS, 1);
  if (sc.template occluded<B>(o, d, tn, tf, st, cnt)) return true;
  if (pl.on) {
    float tp, ap;
    return plane_hit(pl, o, d, tn, tf, tp, ap);
  }
  return false;
}

// Renderer::intersectionColor (raytracing.cpp:13-65) for one ray; the one
// reflection bounce (maxDepth 2 -> 1) is expanded in place, no recursion.
template <class S, int B, class CT>
__device__ __forceinline__ f4 lambert_color(const S &sc, const PlaneDev &pl,
                                            const rt_render_params &P, f3 o, f3 d,
                                            const SurfHit &sh, f3 n, StackOf<S, B> st, CT &cnt) {
  bool visible = true;
  const f3 point = o + sh.h.t * d;
  const f3 L{P.light_pos[0], P.light_pos[1], P.light_pos[2]};
  if (P.enable_shadows) {
    const f3 sd = normalize(L - point);
    visible = !union_occluded<S, B>(sc, pl, point + 0.3f * sd, sd, 0.01f, 100.0f, st, cnt);
  }
  const float a = sh.albedo;
  if (!visible) return f4{a * 0.1f, a * 0.1f, a * 0.1f, 1.0f};
  const f3 ld = normalize(point - L);
  const float lam = std_max(dot(-ld, n), 0.0f);  // Lambert (raytracing.cpp:8-11)
  const f3 c = f3{a * 0.1f, a * 0.1f, a * 0.1f} + lam * f3{a, a, a};
  return f4{std_min(c.x, 1.0f), std_min(c.y, 1.0f), std_min(c.z, 1.0f), 1.0f};
}

// tNear: the primary ray's (the frames' constant 0.01; a ray batch passes its
// own, rt_shade_rays.h); the secondary rays keep the reference's constants.
template <class S, int B, class CT>
__device__ __forceinline__ f4 shade_one(const S &sc, const PlaneDev &pl, const rt_render_params &P,
                                        f3 o, f3 d, float tFarEff, bool allow_refl, bool &hit,
                                        float &t_out, StackOf<S, B> st, int64_t *prim, CT &cnt,
                                        float tNear = 0.01f) {
  const SurfHit sh = union_intersect<S, B>(sc, pl, o, d, tNear, tFarEff, st, cnt);
  if (prim) *prim = sh.h.hit ? sh.h.prim : -1;
  if (!sh.h.hit) {
    hit = false;
    t_out = kInf;
    return f4{0.0f, 0.0f, 0.0f, 1.0f};
  }
  hit = true;
  t_out = sh.h.t;
  f3 n = sh.h.n;
  if (dot(n, d) > 0) n = n * -1.0f;
  f4 c;
  if (P.shading_mode == RT_SHADING_NORMAL) {
    c = f4{(n.x + 1.0f) / 2.0f, (n.y + 1.0f) / 2.0f, (n.z + 1.0f) / 2.0f, (1.0f + 1.0f) / 2.0f};
  } else if (P.shading_mode == RT_SHADING_COLOR) {
    c = f4{sh.albedo, sh.albedo, sh.albedo, 1.0f};
  } else {
    c = lambert_color<S, B>(sc, pl, P, o, d, sh, n, st, cnt);
    if (allow_refl && P.enable_reflections && sh.refl > 0.0f) {
      const float dn = dot(d, n);
      const f3 R = normalize(n * dn * (-2.0f) + d);  // LiteMath reflect(dir, normal)
      const f3 point = o + sh.h.t * d;
      // recursive call with maxDepth 1, tPrev = +inf (raytracing.cpp:51-61)
      const SurfHit rh = union_intersect<S, B>(sc, pl, point + 0.02f * R, R, 0.01f, 100.0f, st, cnt);
      f4 rc{0.0f, 0.0f, 0.0f, 1.0f};
      if (rh.h.hit) {
        f3 rn = rh.h.n;
        if (dot(rn, R) > 0) rn = rn * -1.0f;
        rc = lambert_color<S, B>(sc, pl, P, point + 0.02f * R, R, rh, rn, st, cnt);
      }
      const float r = sh.refl, k = 1.0f - sh.refl;
      c = f4{c.x * k + r * rc.x, c.y * k + r * rc.y, c.z * k + r * rc.z, c.w * k + r * rc.w};
    }
  }
  return c;
}

// -------------------------------------------------------------- ray batches --
// The kernels over an rt_ray_batch (trace_rays_kernel, trace_instances_kernel)
// trace one ray per lane, the work chosen at compile time. kRaysAny: any hit,
// one word per ray; kRaysClosest: closest hit, no normal is computed;
// kRaysNormal: closest hit with the normal. The ray load and the store tails
// are rt_ray_io.h's; trace_rays_kernel keeps its own ray load (behind the
// shared one its any-hit kernels compiled to other loops, profiles/r24/README.md).
enum { kRaysAny = 0, kRaysClosest = 1, kRaysNormal = 2 };

}  // namespace
