// rt_ray_io.h -- a ray batch in and out of a trace kernel (gfx950): the ray of
// lane i of an rt_ray_batch, and the two store tails that close a query over
// the union of a scene and its plane. Shared by the trace kernels over device
// buffers: trace_rays_kernel (rt_device.hip), trace_instances_kernel,
// trace_tlas_kernel, trace_mixed_kernel and trace_mixed_tlas_kernel. The
// shading kernels keep their own load and stores (rt_shade_rays.h). All stores
// are plain vector stores.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/rtamd.h"
#include "rt_shade.h"

namespace {

struct RayIn {
  f3 o, d;
  float tn, tf;
};
// A lane without a ray (a partial last wave keeps its lanes: the wave-level
// traversals need the whole wave) gets a harmless ray and touches no memory.
__device__ __forceinline__ RayIn load_ray(const rt_ray_batch &b, int64_t i, bool active) {
  RayIn r{f3{0.0f, 0.0f, 0.0f}, f3{0.0f, 0.0f, 1.0f}, b.tnear, b.tfar};
  if (active) {
    r.o = f3{b.d_origin[3 * i], b.d_origin[3 * i + 1], b.d_origin[3 * i + 2]};
    r.d = f3{b.d_dir[3 * i], b.d_dir[3 * i + 1], b.d_dir[3 * i + 2]};
    if (b.d_tnear) r.tn = b.d_tnear[i];
    if (b.d_tfar) r.tf = b.d_tfar[i];
  }
  return r;
}
// any hit: `occ` of the scene, OR the plane
__device__ __forceinline__ void store_any(const rt_ray_batch &b, int64_t i, const PlaneDev &pl, const RayIn &r,
                                          bool occ) {
  if (!occ && pl.on) {  // HitInfo::hitten of the union: the OR of both
    float tp, ap;
    occ = plane_hit(pl, r.o, r.d, r.tn, r.tf, tp, ap);
  }
  b.d_hit[i] = occ ? 1 : 0;
}
// closest hit: the scene's `h` merged with the plane's, then the outputs the
// caller asked for (d_normal only in kRaysNormal)
template <int MODE>
__device__ __forceinline__ void store_closest(const rt_ray_batch &b, int64_t i, const PlaneDev &pl, const RayIn &r,
                                              Hit h) {
  if (pl.on) {  // SceneUnion::intersect, as union_intersect
    float tp = kInf, ap = 1.0f;
    const bool ph = plane_hit(pl, r.o, r.d, r.tn, r.tf, tp, ap);
    if (!(h.t < (ph ? tp : kInf))) h = ph ? Hit{true, tp, pl.n, -2} : miss_hit();
  }
  if (b.d_hit) b.d_hit[i] = h.hit ? 1 : 0;
  if (b.d_t) b.d_t[i] = h.t;
  if constexpr (MODE == kRaysNormal) {
    b.d_normal[3 * i] = h.n.x;
    b.d_normal[3 * i + 1] = h.n.y;
    b.d_normal[3 * i + 2] = h.n.z;
  }
  if (b.d_prim) b.d_prim[i] = h.hit ? h.prim : -1;
}

}  // namespace
