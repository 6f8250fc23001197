// rt_instances.hip -- instanced scenes on the device (gfx950): the trace kernel
// that walks a flat list of placements of mesh scenes, the pose update that
// inverts object-to-world matrices, and the one-entry write of the table of
// bottom-level scenes. Semantics: include/rtamd.h and DESIGN.md section 4a.
//
// A translation unit of its own: the kernels of rt_device.hip compile exactly
// as before whatever is instantiated here. The stack slot and mode switches
// are rt_dispatch.h's, the per-lane helpers rt_instance_dev.h's, the ray load
// and the store tails rt_ray_io.h's.
//
// The instance loop is wave-uniform. An instance record (64 bytes) and the
// MeshDev of its bottom-level scene are read through addresses every lane
// shares, from memory no kernel of a trace writes (__restrict__ const), so they
// arrive by scalar loads and the MeshDev handed to the traversal stays in
// SGPRs, as the by-value kernel argument of trace_rays_kernel does. Per lane
// the loop keeps the world ray, tNear / tFar, the best t and the winner
// (instance, triangle slot). All stores are plain vector stores; there is no
// inline assembly and no device-scope waiting.
#include <hip/hip_runtime.h>

#include "rt_dispatch.h"
#include "rt_error.h"
#include "rt_instance_dev.h"
#include "rt_ray_io.h"

using namespace rtd;

namespace {

constexpr int kIBlock = 64;  // one wave, as trace_rays_kernel (rt_device.hip)

template <int SLOTS, int MODE>
__global__ __launch_bounds__(kIBlock) void trace_instances_kernel(const rti::InstRec *__restrict__ inst,
                                                                  const MeshDev *__restrict__ tab, int32_t ninst,
                                                                  PlaneDev pl, rt_ray_batch b) {
  __shared__ uint32_t stk[SLOTS * MeshS::kFields * kIBlock];
  const int64_t i = (int64_t)blockIdx.x * kIBlock + threadIdx.x;
  // a partial last wave keeps its lanes without a ray (mesh_primary_wave needs
  // the whole wave): they carry active = false and touch no memory
  const bool active = i < b.n;
  LdsStack<kIBlock, MeshS::kFields> st{stk + threadIdx.x};
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
      const MeshDev md = tab[r.blas];
      if (md.root == rtl::kInvalidChild) continue;
      if (live) {
        const f3 oo = xf_point(r.m, o), dd = xf_dir(r.m, d);
        if (root_passes(md, oo, dd, tn, tf) && mesh_occluded<kIBlock>(md, oo, dd, tn, tf, st, cnt)) {
          occ = true;
          live = false;
        }
      }
    }
    if (!active) return;
    store_any(b, i, pl, ray, occ);
  } else {
    float best = kInf;
    int32_t wi = -1;      // winning instance
    uint32_t wk = 0;      // its triangle slot
    for (int32_t k = 0; k < ninst; ++k) {
      const rti::InstRec r = inst[k];
      if ((r.flags & RT_INSTANCE_DISABLED) || r.skipped) continue;
      const MeshDev md = tab[r.blas];
      if (md.root == rtl::kInvalidChild) continue;
      const f3 oo = xf_point(r.m, o), dd = xf_dir(r.m, d);
      const float tfi = best < tf ? best : tf;
      const bool go = active && root_passes(md, oo, dd, tn, tfi);
      if (__ballot(go) == 0) continue;  // the whole wave misses this instance's root box
      float t = kInf;
      uint32_t tri = 0;
      bool h;
      // mesh_primary_wave takes one tNear for the wave (tFar is per ray):
      // batches with a d_tnear array take the per-lane traversal
      if (!b.d_tnear)
        h = mesh_primary_wave<kIBlock, MeshS::kFields>(md, oo, dd, tn, tfi, go, stk, t, tri) && go;
      else
        h = go && mesh_trace<kIBlock, false>(md, oo, dd, tn, tfi, st, t, tri, cnt);
      if (h && t < best) {  // ties keep the lower index
        best = t;
        wi = k;
        wk = tri;
      }
    }
    if (!active) return;
    const Hit h = mesh_winner_hit<MODE == kRaysNormal>(inst, tab, best, wi, wk, b.d_prim);
    store_closest<MODE>(b, i, pl, ray, h);
  }
}

// One table entry, taken by value and written word by word by one lane.
__global__ void blas_entry_kernel(MeshDev *entry, MeshDev md) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  entry->nodes = md.nodes;
  entry->tris = md.tris;
  entry->root = md.root;
  for (int k = 0; k < 6; ++k) entry->rbox[k] = md.rbox[k];
  entry->coop = md.coop;
  entry->dmax2 = md.dmax2;
}

// One matrix per lane: twelve loads, rti::affine_inverse, three 16-byte stores
// of M and the skipped word. blas and flags are not touched.
__global__ __launch_bounds__(64) void pose_kernel(rti::InstRec *inst, int32_t first, int32_t count,
                                                  const float *__restrict__ xf) {
  const int32_t j = (int32_t)(blockIdx.x * 64u + threadIdx.x);
  if (j >= count) return;
  float x[12], m[12] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int k = 0; k < 12; ++k) x[k] = xf[12 * (int64_t)j + k];
  const bool ok = rti::affine_inverse(x, m);
  rti::InstRec *r = inst + (int64_t)first + j;
  float4 *q = reinterpret_cast<float4 *>(r->m);
  q[0] = make_float4(m[0], m[1], m[2], m[3]);
  q[1] = make_float4(m[4], m[5], m[6], m[7]);
  q[2] = make_float4(m[8], m[9], m[10], m[11]);
  r->skipped = ok ? 0u : 1u;
}

template <int SLOTS>
void launch_t(const rti::InstArgs &a, const PlaneDev &pl, const rt_ray_batch &b, int mode, hipStream_t st) {
  const unsigned blocks = (unsigned)((b.n + kIBlock - 1) / kIBlock);
  with_mode(mode, [&](auto m) {
    trace_instances_kernel<SLOTS, decltype(m)::value><<<blocks, kIBlock, 0, st>>>(a.inst, a.blas, a.ninst, pl, b);
  });
}

}  // namespace

namespace rti {

int trace_instances_launch(const InstArgs &a, const PlaneDev &pl, const rt_ray_batch &b, int mode, hipStream_t st) {
  with_slots(a.maxd, [&](auto slots) { launch_t<decltype(slots)::value>(a, pl, b, mode, st); });
  HIP_TRY(hipGetLastError());
  return RT_OK;
}

int blas_entry_launch(MeshDev *entry, const MeshDev &md, hipStream_t st) {
  blas_entry_kernel<<<1, 64, 0, st>>>(entry, md);
  HIP_TRY(hipGetLastError());
  return RT_OK;
}

int pose_launch(InstRec *inst, int32_t first, int32_t count, const float *d_xform12, hipStream_t st) {
  pose_kernel<<<(unsigned)((count + 63) / 64), 64, 0, st>>>(inst, first, count, d_xform12);
  HIP_TRY(hipGetLastError());
  return RT_OK;
}

}  // namespace rti

extern "C" int rt_affine_inverse(const float xform[12], float inv[12]) {
  if (!xform || !inv) return set_err(RT_E_INVALID, "rt_affine_inverse: NULL argument");
  float m[12];
  if (!rti::affine_inverse(xform, m))
    return set_err(RT_E_INVALID, "rt_affine_inverse: the matrix is singular or has a non-finite entry");
  for (int k = 0; k < 12; ++k) inv[k] = m[k];
  return RT_OK;
}
