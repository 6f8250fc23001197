// rt_shade_instances.hip -- shaded ray queries of instanced scenes (gfx950):
// the two scene adapters that give shade_one (rt_shade.h) an instanced scene
// with the interface of MeshS -- the flat list of rt_instances.hip's
// trace_instances_kernel and the top-level tree of rt_tlas.hip's
// trace_tlas_kernel -- and the shade_rays kernels over them. Semantics:
// include/rtamd.h (the header's loop, with its box_pass line for
// RT_INSTANCED_TLAS, applied to every ray shade_one traces); DESIGN.md
// section 4b.
//
// A translation unit of its own, as rt_instances.hip and rt_tlas.hip: nothing
// instantiated here moves a block of a kernel that existed before.
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
#include "rt_instances.h"
#include "rt_layout.h"
#include "rt_math.h"
#include "rt_scenes.h"
#include "rt_shade_rays.h"
#include "rt_tlas.h"

using namespace rtd;

namespace {

// world -> object, with the operation order of include/rtamd.h (no fusing)
__device__ __forceinline__ f3 xf_point(const float *m, f3 p) {
  return f3{((m[0] * p.x + m[1] * p.y) + m[2] * p.z) + m[3], ((m[4] * p.x + m[5] * p.y) + m[6] * p.z) + m[7],
            ((m[8] * p.x + m[9] * p.y) + m[10] * p.z) + m[11]};
}
__device__ __forceinline__ f3 xf_dir(const float *m, f3 d) {
  return f3{(m[0] * d.x + m[1] * d.y) + m[2] * d.z, (m[4] * d.x + m[5] * d.y) + m[6] * d.z,
            (m[8] * d.x + m[9] * d.y) + m[10] * d.z};
}

// as rt_instances.hip: the traversal's own root test, ahead of the traversal
__device__ __forceinline__ bool root_passes(const MeshDev &md, f3 o, f3 d, float tn, float tf) {
  if (md.root & rtl::kLeafBit) return true;
  const f3 inv{1.0f / d.x, 1.0f / d.y, 1.0f / d.z};
  return !root_box_miss(md.rbox, o, inv, tn, tf);
}

// a lane's own copy of a record's matrix and of a table entry (vector loads)
__device__ __forceinline__ void load_m(const rti::InstRec *r, float m[12]) {
  const float4 *q = reinterpret_cast<const float4 *>(r->m);
  const float4 a = q[0], b = q[1], c = q[2];
  m[0] = a.x; m[1] = a.y; m[2] = a.z; m[3] = a.w;
  m[4] = b.x; m[5] = b.y; m[6] = b.z; m[7] = b.w;
  m[8] = c.x; m[9] = c.y; m[10] = c.z; m[11] = c.w;
}
__device__ __forceinline__ MeshDev load_md(const MeshDev *e) {
  MeshDev md{e->nodes, e->tris, e->root, {}, e->coop, e->dmax2};
#pragma unroll
  for (int k = 0; k < 6; ++k) md.rbox[k] = e->rbox[k];
  return md;
}

// The winner's Hit, per lane (lanes differ in wi): the object-space normal
// under the inverse transpose of the object-to-world map, M^T n, normalised;
// prim = (instance << 32) | original triangle index.
__device__ __forceinline__ Hit winner_hit(const rti::InstRec *inst, const MeshDev *tab, int32_t wi, uint32_t wk,
                                          float best) {
  Hit h = miss_hit();
  if (wi >= 0) {
    const float *m = inst[wi].m;
    const rtl::GTri *tris = tab[inst[wi].blas].tris;
    const f3 n = tri_normal(tris, wk);  // object space
    h.hit = true;
    h.t = best;
    h.n = normalize(f3{(m[0] * n.x + m[4] * n.y) + m[8] * n.z, (m[1] * n.x + m[5] * n.y) + m[9] * n.z,
                       (m[2] * n.x + m[6] * n.y) + m[10] * n.z});
    h.prim = (int64_t)(((uint64_t)(uint32_t)wi << 32) | (uint64_t)tris[wk].orig_id);
  }
  return h;
}

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
    return winner_hit(inst, tab, wi, wk, best);
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
  // a lane's walk to its next candidate: rtt::walk_next on 16-byte loads
  __device__ __forceinline__ uint32_t next(uint32_t n, f3 o, f3 inv, float tn, float tf) const {
    while (n != 0u) {
      const float4 *q = reinterpret_cast<const float4 *>(nodes + n);
      const float4 a = q[0], c = q[1];
      const float bx[6] = {a.x, a.y, a.z, a.w, c.x, c.y};
      if (rtt::box_pass_inv(bx, o.x, o.y, o.z, inv.x, inv.y, inv.z, tn, tf)) {
        if (n >= P) return n;
        n = 2u * n;
      } else {
        n = rtt::walk_skip(n);
      }
    }
    return 0u;
  }
  template <int B, class CT>
  __device__ __forceinline__ Hit intersect(f3 o, f3 d, float tn, float tf, LdsStack<B, kFields> st, CT &cnt) const {
    const f3 inv{1.0f / d.x, 1.0f / d.y, 1.0f / d.z};  // of the WORLD ray: the tree's test
    float best = kInf;
    int32_t wi = -1;
    uint32_t wk = 0;
    uint32_t n = 1u;
    for (;;) {
      const float tfi = best < tf ? best : tf;
      n = next(n, o, inv, tn, tfi);
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
    return winner_hit(inst, tab, wi, wk, best);
  }
  // the candidates under the full tFar; a lane stops at its first hit
  template <int B, class CT>
  __device__ __forceinline__ bool occluded(f3 o, f3 d, float tn, float tf, LdsStack<B, kFields> st, CT &cnt) const {
    const f3 inv{1.0f / d.x, 1.0f / d.y, 1.0f / d.z};
    uint32_t n = 1u;
    for (;;) {
      n = next(n, o, inv, tn, tf);
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
