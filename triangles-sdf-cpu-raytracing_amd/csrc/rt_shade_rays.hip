// rt_shade_rays.hip -- shaded ray queries (gfx950): rt_shade_rays_device, the
// per-ray body of Renderer::draw (intersectionColor, color_pack_rgba, the
// store rule) on rays in device buffers, and rt_eye_rays_device, the
// reference's eye rays written as such a batch. Semantics: include/rtamd.h;
// DESIGN.md section 4b.
//
// A translation unit of its own: the kernels of rt_device.hip compile exactly
// as before whatever is instantiated here. The kernels of meshes, grids and
// octrees are here, through rt_dispatch.h's scene dispatch; an instanced
// scene's are in rt_shade_instances.hip. Both entries only launch.
#include <hip/hip_runtime.h>

#include <string>
#include <type_traits>

#include "../../include/rtamd.h"
#include "rt_dispatch.h"
#include "rt_error.h"
#include "rt_instances.h"
#include "rt_scene.h"
#include "rt_shade_rays.h"

using namespace rtd;

namespace {

template <class S, int SLOTS>
__global__ __launch_bounds__(kSBlock) __attribute__((amdgpu_waves_per_eu(RT_SHADE_WAVES)))
void shade_rays_kernel(S sc, PlaneDev pl, rt_render_params P, rt_ray_batch b, uint32_t *d_color, uint32_t flags) {
  __shared__ uint32_t stk[stack_words<S, SLOTS>() * kSBlock];
  shade_rays_body<S, SLOTS>(sc, pl, P, b, d_color, flags, stk);
}

// Ray y * W + x = pixel (x, y) of rt_render's frame (image row y is loop row
// H - y - 1, raytracing.cpp:82): eye_ray in its plain form, the bits of the
// diagnostic rtx_eye_rays. n = W * H <= 2^31 (check_params).
constexpr int kEBlock = 256;
__global__ __launch_bounds__(kEBlock) void eye_rays_device_kernel(rt_render_params P, int32_t W, int32_t H,
                                                                  float *d_origin, float *d_dir) {
  const uint32_t i = blockIdx.x * (uint32_t)kEBlock + threadIdx.x;
  if (i >= (uint32_t)W * (uint32_t)H) return;
  const uint32_t yo = i / (uint32_t)W, x = i - yo * (uint32_t)W;
  const size_t k = 3 * (size_t)i;
  if (d_dir) {
    const f3 d = eye_ray((int)x, H - (int)yo - 1, W, H, P.proj_inv, P.view_inv);
    d_dir[k] = d.x;
    d_dir[k + 1] = d.y;
    d_dir[k + 2] = d.z;
  }
  if (d_origin) {
    d_origin[k] = P.camera_pos[0];
    d_origin[k + 1] = P.camera_pos[1];
    d_origin[k + 2] = P.camera_pos[2];
  }
}

}  // namespace

extern "C" {

int rt_eye_rays_device(const rt_render_params *p, int32_t W, int32_t H, float *d_origin, float *d_dir,
                       void *stream) {
  if (int rc = check_params(p, W, H)) return rc;
  if (!d_origin && !d_dir) return set_err(RT_E_INVALID, "rt_eye_rays_device: both outputs are NULL");
  const uint32_t n = (uint32_t)((int64_t)W * H);
  eye_rays_device_kernel<<<(n - 1u) / (uint32_t)kEBlock + 1u, kEBlock, 0, (hipStream_t)stream>>>(*p, W, H, d_origin,
                                                                                                 d_dir);
  HIP_TRY(hipGetLastError());
  return RT_OK;
}

int rt_shade_rays_device(rt_scene *s, const rt_ray_batch *b, const rt_render_params *p, uint32_t *d_color,
                         uint32_t flags, void *stream) {
  if (!s) return set_err(RT_E_INVALID, "scene is NULL");
  if (!b) return set_err(RT_E_INVALID, "ray batch is NULL");
  if (!p) return set_err(RT_E_INVALID, "params is NULL");
  if (!d_color) return set_err(RT_E_INVALID, "NULL colour buffer");
  if (flags & ~RT_SHADE_CLEAR) return set_err(RT_E_INVALID, "unknown shade flag");
  if (b->n < 0) return set_err(RT_E_INVALID, "negative ray count");
  if (!b->d_origin || !b->d_dir) return set_err(RT_E_INVALID, "NULL ray origins or directions");
  if (b->d_normal)
    return set_err(RT_E_INVALID, "rt_shade_rays_device writes no normal: d_normal must be NULL (rt_trace_rays_device)");
  if (b->n / kSBlock + (b->n % kSBlock != 0) > kMaxShadeBlocks)
    return set_err(RT_E_INVALID, "ray count exceeds one launch (" + std::to_string(kMaxShadeBlocks * kSBlock) +
                                     " rays): split the batch");
  if (p->shading_mode < 0 || p->shading_mode > 2) return set_err(RT_E_INVALID, "bad shading mode");
  if (p->reserved != 0) return set_err(RT_E_INVALID, "rt_shade_rays_device: params.reserved must be 0");
  if (b->n == 0) return RT_OK;
  const hipStream_t st = (hipStream_t)stream;
  if (s->info.kind == RT_SCENE_INSTANCED) {
    if (int rc = rti::instanced_sync(s, st)) return rc;
    const rti::InstArgs a{s->inst.recs.p, s->inst.tab.p, s->inst.n, s->info.maxd, s->inst.tlas.p, s->inst.tlas_leaves};
    if (s->inst.mixed.p) return rti::shade_mixed_launch(rti::MixedArgs{a, s->inst.mixed.p}, s->info.plane, *p, *b, d_color, flags, st);
    return rti::shade_instances_launch(a, s->info.plane, *p, *b, d_color, flags, st);
  }
  const unsigned blocks = (unsigned)((b->n + kSBlock - 1) / kSBlock);
  if (!dispatch_scene(s, [&](const auto &sc, auto slots) {
        shade_rays_kernel<std::decay_t<decltype(sc)>, decltype(slots)::value>
            <<<blocks, kSBlock, 0, st>>>(sc, s->info.plane, *p, *b, d_color, flags);
      }))
    return set_err(RT_E_STATE, "scene has no geometry");
  HIP_TRY(hipGetLastError());
  return RT_OK;
}

}  // extern "C"
