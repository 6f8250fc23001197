// rt_points.h -- what the two closest-point units share: the SDF-mesh handle
// (rt_sdfgen.hip creates, updates and destroys it, rt_points.hip only reads
// its device arrays, which change only under an update of an RT_MESH_DYNAMIC
// handle, in stream order) and the device pieces of the closest-point walk
// over the BVH8 (DESIGN.md sections 9 and 9a): Ericson's closest point on a
// triangle with its Voronoi region, the squared distance to a child box and
// the prune bound with its absolute slack.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/rtamd.h"
#include "rt_host.h"
#include "rt_layout.h"
#include "rt_math.h"
#include "rt_mem.h"

// rt_sdf_mesh_destroy makes `device` current, drains qs and deletes: after
// that the order in which the owners (rt_mem.h) release is immaterial.
struct rt_sdf_mesh {
  rth::SdfMeshHost host;
  rtmem::DevArray<rtl::GNode> d_nodes;
  rtmem::DevArray<float4> d_tri, d_pn;
  uint32_t root = rtl::kInvalidChild;
  int32_t stack_cap = 0;
  int device = 0;
  int32_t oct_depth = -1;          // octree cache (two-call protocol of rt_sdf_mesh_octree)
  std::vector<uint8_t> oct_nodes;
  // point queries: the handle's own non-blocking stream, and pinned host /
  // device staging for up to q_cap points, reused across calls
  rtmem::Stream qs;
  rtmem::Pinned<float> h_stage;  // q_cap * 4 floats: points (3 per point), then distances
  rtmem::DevArray<float> d_p3, d_out;
  int64_t q_cap = 0;
  // RT_MESH_DYNAMIC only (rt_sdf_mesh_update_vertices*, rt_sdf_refit.hip): the
  // creation topology on the device, scratch, and the event every update
  // records after its last kernel. The host copies host.tri / host.pn are
  // dropped at creation: after an update only the device arrays are current.
  bool dynamic = false;
  int64_t nverts = 0, ntri = 0;
  uint32_t n_wverts = 0, n_wedges = 0;
  rtmem::DevArray<uint32_t> d_idx, d_weld, d_tri_edge, d_v_off, d_v_inc, d_e_off, d_e_inc;
  rtmem::DevArray<float4> d_vstage, d_fn, d_vn, d_en;
  rtmem::DevArray<double> d_ang;  // 3 per triangle
  std::vector<uint32_t> level_first;
  rtmem::Event updated;
  int64_t dev_bytes = 0;  // what the handle's mesh arrays hold on the device (rt_sdf_mesh_device_bytes)
};

namespace rtsdf {

using namespace rtd;

constexpr int kWave = 64;

// The handle's immutable device arrays, as the kernels take them.
struct SdfDev {
  const rtl::GNode *nodes;
  const float4 *tri;   // 3 per triangle in leaf order: corners a, b, c; a.w = the original triangle id
  const float4 *pn;    // 7 per original triangle: the pseudonormals of features 0..6
  uint32_t root;
};

inline SdfDev dev_of(const rt_sdf_mesh *m) { return SdfDev{m->d_nodes.p, m->d_tri.p, m->d_pn.p, m->root}; }

// Dynamic LDS of one 64-lane workgroup: stack_cap entries of (box distance^2,
// child word) per lane, lane-interleaved.
inline size_t lds_bytes(const rt_sdf_mesh *m) { return (size_t)m->stack_cap * kWave * 8; }

// Ericson, Real-Time Collision Detection 5.1.5 ClosestPtPointTriangle, with
// the Voronoi region reported: 0..2 vertex a,b,c; 3 ab; 4 ac; 5 bc; 6 face.
__device__ __forceinline__ f3 closest_on_tri(f3 p, f3 a, f3 b, f3 c, int &feat) {
  const f3 ab = b - a, ac = c - a, ap = p - a;
  const float d1 = dot(ab, ap), d2 = dot(ac, ap);
  if (d1 <= 0.0f && d2 <= 0.0f) { feat = 0; return a; }
  const f3 bp = p - b;
  const float d3 = dot(ab, bp), d4 = dot(ac, bp);
  if (d3 >= 0.0f && d4 <= d3) { feat = 1; return b; }
  const float vc = d1 * d4 - d3 * d2;
  if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) {
    const float v = d1 / (d1 - d3);
    feat = 3;
    return a + ab * v;
  }
  const f3 cp = p - c;
  const float d5 = dot(ab, cp), d6 = dot(ac, cp);
  if (d6 >= 0.0f && d5 <= d6) { feat = 2; return c; }
  const float vb = d5 * d2 - d1 * d6;
  if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) {
    const float w = d2 / (d2 - d6);
    feat = 4;
    return a + ac * w;
  }
  const float va = d3 * d6 - d5 * d4;
  if (va <= 0.0f && (d4 - d3) >= 0.0f && (d5 - d6) >= 0.0f) {
    const float w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
    feat = 5;
    return b + (c - b) * w;
  }
  const float denom = 1.0f / (va + vb + vc);
  const float v = vb * denom, w = vc * denom;
  feat = 6;
  return a + ab * v + ac * w;
}

// bx: xMin xMax yMin yMax zMin zMax (rt_layout.h GNode)
__device__ __forceinline__ float box_d2(const float *bx, f3 p) {
  const float dx = fmaxf(fmaxf(bx[0] - p.x, p.x - bx[1]), 0.0f);
  const float dy = fmaxf(fmaxf(bx[2] - p.y, p.y - bx[3]), 0.0f);
  const float dz = fmaxf(fmaxf(bx[4] - p.z, p.z - bx[5]), 0.0f);
  return dx * dx + dy * dy + dz * dz;
}

__device__ __forceinline__ float prune_bound(float best) {
  if (!(best < kInf)) return kInf;
  const float r = __builtin_sqrtf(best) + 1e-5f;
  return r * r;
}

}  // namespace rtsdf
