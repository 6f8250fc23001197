// rt_instance_dev.h -- what the kernels of instanced scenes share on the device
// (gfx950): the world-to-object arithmetic, a lane's copies of a record and a
// table entry, the wave minimum and the cursor walk of the top-level tree, the
// prim packing and the Hit of a mesh winner. Included by rt_instances.hip,
// rt_tlas.hip, rt_shade_instances.hip and rt_instances_mixed.hip; everything
// is __device__ __forceinline__ and internal to the including unit, as
// rt_shade_rays.h. Semantics: include/rtamd.h, DESIGN.md section 4a.
//
// The candidate bodies of the instance loops (wave-level and per-lane) are not
// here: behind a function every spelling tried changed the loops of the
// kernels that called it, and so did a struct for the loop-carried winner of
// the mesh-only kernels (profiles/r24/README.md). Each loop keeps its body.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/rtamd.h"
#include "rt_instances.h"
#include "rt_layout.h"
#include "rt_math.h"
#include "rt_scenes.h"
#include "rt_shade.h"
#include "rt_tlas.h"

namespace {

// world -> object. The operation order is part of the bit-exact contract of
// include/rtamd.h: sums left to right, nothing fused.
__device__ __forceinline__ f3 xf_point(const float *m, f3 p) {
  return f3{((m[0] * p.x + m[1] * p.y) + m[2] * p.z) + m[3], ((m[4] * p.x + m[5] * p.y) + m[6] * p.z) + m[7],
            ((m[8] * p.x + m[9] * p.y) + m[10] * p.z) + m[11]};
}
__device__ __forceinline__ f3 xf_dir(const float *m, f3 d) {
  return f3{(m[0] * d.x + m[1] * d.y) + m[2] * d.z, (m[4] * d.x + m[5] * d.y) + m[6] * d.z,
            (m[8] * d.x + m[9] * d.y) + m[10] * d.z};
}
// the inverse transpose of the object-to-world map on an object-space normal: M^T n, normalised
__device__ __forceinline__ f3 world_normal(const float *m, f3 n) {
  return normalize(f3{(m[0] * n.x + m[4] * n.y) + m[8] * n.z, (m[1] * n.x + m[5] * n.y) + m[9] * n.z,
                      (m[2] * n.x + m[6] * n.y) + m[10] * n.z});
}

// The mesh traversal's own root test on the transformed ray, ahead of the
// traversal: mesh_root evaluates root_box_miss on exactly these operands first,
// so a lane it rejects here would return "no hit" there. A leaf root has no
// such test and is never pre-culled. (root_box_miss itself passes every ray
// whose 1/d has a non-finite component.)
__device__ __forceinline__ bool root_passes(const MeshDev &md, f3 o, f3 d, float tn, float tf) {
  if (md.root & rtl::kLeafBit) return true;
  const f3 inv{1.0f / d.x, 1.0f / d.y, 1.0f / d.z};
  return !root_box_miss(md.rbox, o, inv, tn, tf);
}

// a lane's own copy of a record's matrix and of a mesh view (vector loads)
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

// the smallest value of the wave (all 64 lanes call it)
__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    const uint32_t w = (uint32_t)__shfl_xor((int)v, s, 64);
    v = w < v ? w : v;
  }
  return v;
}

// a lane's walk to its next candidate: rtt::walk_next on 16-byte loads
__device__ __forceinline__ uint32_t lane_next(const rtt::TNode *__restrict__ nodes, uint32_t P, uint32_t n, f3 o,
                                              f3 inv, float tn, float tf) {
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

// prim of an instanced scene: (instance << 32) | what the bottom-level kind reports
__device__ __forceinline__ int64_t inst_prim(int32_t wi, uint32_t p) {
  return (int64_t)(((uint64_t)(uint32_t)wi << 32) | (uint64_t)p);
}

// The Hit of a lane's winner in a table of meshes, per lane (lanes differ in
// wi): the miss without one (wi < 0), else the triangle's normal under M^T
// and prim from the original triangle id. want_prim is tested as the caller
// spells it, a bool or the batch's d_prim pointer (the trace kernels' epilogue
// compiles differently for the two).
template <bool NORMAL, class P>
__device__ __forceinline__ Hit mesh_winner_hit(const rti::InstRec *inst, const MeshDev *tab, float best, int32_t wi,
                                               uint32_t wk, P want_prim) {
  Hit h = miss_hit();
  if (wi >= 0) {
    const float *m = inst[wi].m;
    const rtl::GTri *tris = tab[inst[wi].blas].tris;
    h.hit = true;
    h.t = best;
    if constexpr (NORMAL) h.n = world_normal(m, tri_normal(tris, wk));
    if (want_prim) h.prim = inst_prim(wi, tris[wk].orig_id);
  }
  return h;
}

}  // namespace
