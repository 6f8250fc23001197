// rt_shade_instances.hip -- shaded ray queries of instanced scenes (gfx950):
// the two scene adapters that give shade_one (rt_shade.h) an instanced scene
// with the interface of MeshS -- the flat list of rt_instances.hip's
// trace_instances_kernel and the top-level tree of rt_tlas.hip's
// trace_tlas_kernel -- and the shade_rays kernels over them. Semantics:
// include/rtamd.h (the header's loop, with its box_pass line for
// RT_INSTANCED_TLAS, applied to every ray shade_one traces); DESIGN.md
// section 4b.
//
// A translation unit of its own, as rt_instances.hip and rt_tlas.hip; the
// per-lane helpers and the winner's Hit are rt_instance_dev.h's.
//
// shade_one calls intersect and occluded inside lane-divergent branches (the
// shadow ray exists on lanes that hit, the reflection ray on lanes that hit
// the plane), so nothing in an adapter may need the whole wave: the
// bottom-level traversal is the per-lane one (mesh_trace, mesh_occluded),
// never mesh_primary_wave. The flat adapter's instance loop stays uniform over
// the lanes that are in the call: they all start at instance 0 and skip on
// conditions every one of them shares (the record's flags, the table entry, a
// ballot over those lanes), so the record and the MeshDev still arrive by
// scalar loads. The tree adapter walks per lane (rt_tlas.h's cursor walk) and
// reads its candidate's record and MeshDev per lane, as the per-lane rounds of
// trace_tlas_kernel do. All stores are plain vector stores; there is no inline
// assembly and no device-scope waiting.
#include <hip/hip_runtime.h>

#include "rt_dispatch.h"
#include "rt_error.h"
#include "rt_instance_dev.h"
#include "rt_shade_rays.h"

using namespace rtd;

namespace {

// The flat list: the header's loop, the body of trace_instances_kernel's with
// the per-lane traversal. `go`-less lanes of the call wait in the loop, so k
// and with it the record's address stay uniform.
struct InstFlatS {
  static constexpr int kFields = MeshS::kFields;
  const rti::InstRec *__restrict__ inst;
  const MeshDev *__restrict__ tab;
  int32_t ninst;
  template <int B, class CT>
  __device__ __forceinline__ Hit intersect(f3 o, f3 d, float tn, float tf, LdsStack<B, kFields> st, CT &cnt) const {
    float best = kInf;
    int32_t wi = -1;  // winning instance
    uint32_t wk = 0;  // its triangle slot
    for (int32_t k = 0; k < ninst; ++k) {
      const rti::InstRec r = inst[k];
      if ((r.flags & RT_INSTANCE_DISABLED) || r.skipped) continue;
      const MeshDev md = tab[r.blas];
      if (md.root == rtl::kInvalidChild) continue;
      const f3 oo = xf_point(r.m, o), dd = xf_dir(r.m, d);
      const float tfi = best < tf ? best : tf;
      const bool go = root_passes(md, oo, dd, tn, tfi);
      if (__ballot(go) == 0) continue;  // every lane of the call misses this instance's root box
      float t = kInf;
      uint32_t tri = 0;
      if (go && mesh_trace<B, false>(md, oo, dd, tn, tfi, st, t, tri, cnt) && t < best) {  // ties keep the lower index
        best = t;
        wi = k;
        wk = tri;
      }
    }
    return mesh_winner_hit<true>(inst, tab, best, wi, wk, true);
  }
  // OR over the instances of the bottom-level any hit under the full tFar (the
  // closest-hit flag, include/rtamd.h); a lane that has its hit waits, the
  // loop ends when none of the call's lanes is left
  template <int B, class CT>
  __device__ __forceinline__ bool occluded(f3 o, f3 d, float tn, float tf, LdsStack<B, kFields> st, CT &cnt) const {
    bool live = true;
    for (int32_t k = 0; k < ninst; ++k) {
      if (__ballot(live) == 0) break;
      const rti::InstRec r = inst[k];
      if ((r.flags & RT_INSTANCE_DISABLED) || r.skipped) continue;
      const MeshDev md = tab[r.blas];
      if (md.root == rtl::kInvalidChild) continue;
      if (live) {
        const f3 oo = xf_point(r.m, o), dd = xf_dir(r.m, d);
        if (root_passes(md, oo, dd, tn, tf) && mesh_occluded<B>(md, oo, dd, tn, tf, st, cnt)) live = false;
      }
    }
    return !live;
  }
};

// The top-level tree: each lane walks its own cursor (rtt::walk_skip, box_pass
// on 16-byte loads) and searches its own candidates in index order, the
// per-lane round of trace_tlas_kernel. Nothing here is wave-level.
struct InstTlasS {
  static constexpr int kFields = MeshS::kFields;
  const rti::InstRec *__restrict__ inst;
  const MeshDev *__restrict__ tab;
  const rtt::TNode *__restrict__ nodes;
  uint32_t P;
  template <int B, class CT>
  __device__ __forceinline__ Hit intersect(f3 o, f3 d, float tn, float tf, LdsStack<B, kFields> st, CT &cnt) const {
    const f3 inv{1.0f / d.x, 1.0f / d.y, 1.0f / d.z};  // of the WORLD ray: the tree's test
    float best = kInf;
    int32_t wi = -1;
    uint32_t wk = 0;
    uint32_t n = 1u;
    for (;;) {
      const float tfi = best < tf ? best : tf;
      n = lane_next(nodes, P, n, o, inv, tn, tfi);
      if (n == 0u) break;
      const uint32_t cand = n - P;
      const rti::InstRec *rp = inst + cand;
      const uint32_t off = (rp->flags & RT_INSTANCE_DISABLED) | rp->skipped;
      const MeshDev md = load_md(tab + rp->blas);
      if (!off && md.root != rtl::kInvalidChild) {
        float m[12];
        load_m(rp, m);
        const f3 oo = xf_point(m, o), dd = xf_dir(m, d);
        float t = kInf;
        uint32_t tri = 0;
        if (mesh_trace<B, false>(md, oo, dd, tn, tfi, st, t, tri, cnt) && t < best) {
          best = t;
          wi = (int32_t)cand;
          wk = tri;
        }
      }
      n = rtt::walk_skip(n);
    }
    return mesh_winner_hit<true>(inst, tab, best, wi, wk, true);
  }
  // the candidates under the full tFar; a lane stops at its first hit
  template <int B, class CT>
  __device__ __forceinline__ bool occluded(f3 o, f3 d, float tn, float tf, LdsStack<B, kFields> st, CT &cnt) const {
    const f3 inv{1.0f / d.x, 1.0f / d.y, 1.0f / d.z};
    uint32_t n = 1u;
    for (;;) {
      n = lane_next(nodes, P, n, o, inv, tn, tf);
      if (n == 0u) return false;
      const rti::InstRec *rp = inst + (n - P);
      const uint32_t off = (rp->flags & RT_INSTANCE_DISABLED) | rp->skipped;
      const MeshDev md = load_md(tab + rp->blas);
      if (!off && md.root != rtl::kInvalidChild) {
        float m[12];
        load_m(rp, m);
        if (mesh_occluded<B>(md, xf_point(m, o), xf_dir(m, d), tn, tf, st, cnt)) return true;
      }
      n = rtt::walk_skip(n);
    }
  }
};

// The records, the table and the tree come as __restrict__ const kernel
// arguments (memory no kernel of a query writes), as in the trace kernels.
template <int SLOTS>
__global__ __launch_bounds__(kSBlock) __attribute__((amdgpu_waves_per_eu(RT_SHADE_WAVES)))
void shade_instances_kernel(const rti::InstRec *__restrict__ inst, const MeshDev *__restrict__ tab, int32_t ninst,
                            PlaneDev pl, rt_render_params P, rt_ray_batch b, uint32_t *d_color, uint32_t flags) {
  __shared__ uint32_t stk[SLOTS * MeshS::kFields * kSBlock];
  const InstFlatS sc{inst, tab, ninst};
  shade_rays_body<InstFlatS, SLOTS>(sc, pl, P, b, d_color, flags, stk);
}

template <int SLOTS>
__global__ __launch_bounds__(kSBlock) __attribute__((amdgpu_waves_per_eu(RT_SHADE_WAVES)))
void shade_tlas_kernel(const rti::InstRec *__restrict__ inst, const MeshDev *__restrict__ tab,
                       const rtt::TNode *__restrict__ nodes, uint32_t leaves, PlaneDev pl, rt_render_params P,
                       rt_ray_batch b, uint32_t *d_color, uint32_t flags) {
  __shared__ uint32_t stk[SLOTS * MeshS::kFields * kSBlock];
  const InstTlasS sc{inst, tab, nodes, leaves};
  shade_rays_body<InstTlasS, SLOTS>(sc, pl, P, b, d_color, flags, stk);
}

}  // namespace

namespace rti {

int shade_instances_launch(const InstArgs &a, const PlaneDev &pl, const rt_render_params &p, const rt_ray_batch &b,
                           uint32_t *d_color, uint32_t flags, hipStream_t st) {
  const unsigned blocks = (unsigned)((b.n + kSBlock - 1) / kSBlock);
  with_slots(a.maxd, [&](auto slots) {
    constexpr int N = decltype(slots)::value;
    if (a.tlas)
      shade_tlas_kernel<N><<<blocks, kSBlock, 0, st>>>(a.inst, a.blas, a.tlas, (uint32_t)a.tlas_leaves, pl, p, b,
                                                       d_color, flags);
    else
      shade_instances_kernel<N><<<blocks, kSBlock, 0, st>>>(a.inst, a.blas, a.ninst, pl, p, b, d_color, flags);
  });
  HIP_TRY(hipGetLastError());
  return RT_OK;
}

}  // namespace rti
