// rt_shade_rays.h -- the per-ray body of Renderer::draw as a ray query
// (rt_shade_rays_device, include/rtamd.h): one ray of an rt_ray_batch per lane
// through shade_one (rt_shade.h), the packed colour and t stored by the frame
// kernels' rule. Shared by the units that instantiate it: rt_shade_rays.hip
// (meshes, grids, octrees) and rt_shade_instances.hip (instanced scenes, whose
// adapters give shade_one the interface of MeshS).
//
// Every traversal under shade_one is the per-lane one: the shadow ray exists
// only on lanes that hit, the reflection ray only on lanes that hit the plane,
// so nothing below the first branch may need the whole wave. A lane without a
// ray therefore simply leaves.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/rtamd.h"
#include "rt_shade.h"

namespace {

// Workgroup of shade_rays_kernel: one wave, as trace_rays_kernel (a workgroup
// keeps its LDS stacks until its slowest wave ends).
constexpr int kSBlock = 64;
// a launch's global size is a 32-bit count of work-items (rt_trace_rays_device's limit)
constexpr int64_t kMaxShadeBlocks = (int64_t)(0xFFFFFFFFu / (uint32_t)kSBlock);

// Occupancy floor of the shading ray kernels (waves per SIMD). 1: the
// compiler's choice, 4 waves without scratch in every mesh and instanced
// kernel (105 / 111 / 121 VGPRs). Floors of 5 and 6 were measured against it
// (profiles/r19/README.md, 1080p, three alternating rounds): the bunny under
// its plane 311 -> 311 -> 338 us; the 64-bunny lattice through the flat list
// 1236 -> 1185 -> 1208 us, through the top-level tree 694 -> 766 -> 937 us.
// Nothing wins across the kernels, so none is set.
#ifndef RT_SHADE_WAVES
#define RT_SHADE_WAVES 1
#endif

// Its own ray load and its own plain vector stores (rt_shade.h: behind helpers
// shared with the trace kernels those compiled to other code). Each ray reads
// its interval before its stores and no ray reads another's, so d_tfar may be
// d_t: the previous t of a frame that already holds something (tPrev).
template <class S, int SLOTS>
__device__ __forceinline__ void shade_rays_body(const S &sc, const PlaneDev &pl, const rt_render_params &P,
                                                const rt_ray_batch &b, uint32_t *d_color, uint32_t flags,
                                                uint32_t *stk) {
  const int64_t i = (int64_t)blockIdx.x * kSBlock + threadIdx.x;
  if (i >= b.n) return;
  StackOf<S, kSBlock> st{stk + threadIdx.x};
  const f3 o{b.d_origin[3 * i], b.d_origin[3 * i + 1], b.d_origin[3 * i + 2]};
  const f3 d{b.d_dir[3 * i], b.d_dir[3 * i + 1], b.d_dir[3 * i + 2]};
  const float tn = b.d_tnear ? b.d_tnear[i] : b.tnear;
  const float tf = b.d_tfar ? b.d_tfar[i] : b.tfar;
  NoCnt cnt;
  bool hit;
  float t;
  int64_t prim;
  const f4 c = shade_one<S, kSBlock>(sc, pl, P, o, d, tf, true, hit, t, st, &prim, cnt, tn);
  // the reference stores only when !isinf(tNew) (raytracing.cpp:91-94)
  const bool store = hit && !__builtin_isinf(t);
  if (store) {
    d_color[i] = pack_rgba(c);
    if (b.d_t) b.d_t[i] = t;
  } else if (flags & RT_SHADE_CLEAR) {
    d_color[i] = 0u;
    if (b.d_t) b.d_t[i] = kInf;
  }
  if (b.d_hit) b.d_hit[i] = store ? 1 : 0;
  if (b.d_prim) b.d_prim[i] = prim;
}

}  // namespace
