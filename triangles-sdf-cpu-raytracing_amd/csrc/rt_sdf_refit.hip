// rt_sdf_refit.hip -- refit of an SDF-mesh handle on the device (gfx950): the
// tree, the triangle records and the 7 pseudonormals per triangle over new
// vertex positions, as rth::refit_sdf_mesh (rt_meshops.cpp) states them.
//
// Tree: as rt_refit.hip. bvh_layout stores the inner nodes in BFS order, so
// the refit is one launch per depth level, deepest first, 8 lanes per node,
// one lane per child slot. A leaf child's lane rewrites its (at most 8)
// triangle records -- three float4 each: the divided corners, a.w keeps the
// original id -- and grows the box over them in slot order, corners a, b, c;
// an inner child's lane grows over the eight boxes of the finished child node.
// Levels are separated by kernel boundaries: no device-scope atomics, no
// spin-waits, no cooperative launch.
//
// Pseudonormals: four kernels in stream order, none with an atomic.
//   tri_terms     one lane per original triangle: the face normal in float
//                 (cross, sqrt, divide; zero for a zero length) and the three
//                 corner angles in double (sqrt, divide, clamp, acos);
//   vertex_sums   one lane per welded vertex walks its incidence list in the
//                 stored order (ascending triangle, then corner) and sums
//                 ang * nf in double: a multiply, then an add (-ffp-contract=off);
//   edge_sums     one lane per welded edge, the same over nf;
//   scatter_pn    one lane per (triangle, feature) copies the float4 into pn.
// Each sum is evaluated sequentially by one lane and rounded to float once, so
// the result does not depend on scheduling. Every operation but acos is an
// IEEE operation in the host's order; the device's acos may differ from the
// host library's in the last bits of the double (include/rtamd.h).
//
// Topology (child words, triangle order, ids, weld map, incidence lists) is
// only read and was built from checked indices at creation, so no vertex value
// can make this or a later walk index out of bounds. All stores are plain
// vector stores.
#include <hip/hip_runtime.h>

#include "rt_error.h"
#include "rt_layout.h"
#include "rt_sdf_refit.h"

namespace {

struct RBox {
  float mn[3], mx[3];
};
__device__ __forceinline__ RBox rb_empty() {
  const float inf = __builtin_huge_valf();
  return RBox{{inf, inf, inf}, {-inf, -inf, -inf}};
}
// std::min / std::max as rth's grow uses them (the left operand stays on a
// tie or a NaN); not fminf / fmaxf, whose zero-sign and NaN rules differ
__device__ __forceinline__ void rb_grow(RBox &b, const float mn[3], const float mx[3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    b.mn[k] = (mn[k] < b.mn[k]) ? mn[k] : b.mn[k];
    b.mx[k] = (b.mx[k] < mx[k]) ? mx[k] : b.mx[k];
  }
}

// v / v.w, the correctly rounded division of refit_leaf (rt_refit.hip)
__device__ __forceinline__ void divided(const float4 *__restrict__ vpos, uint32_t v, float out[3]) {
  const float4 p = vpos[v];
  out[0] = p.x / p.w;
  out[1] = p.y / p.w;
  out[2] = p.z / p.w;
}

// One leaf child: its triangle records rewritten from the new vertices and the
// box of their divided corners.
__device__ __forceinline__ RBox refit_leaf(uint32_t word, float4 *tri, const float4 *__restrict__ vpos,
                                           const uint32_t *__restrict__ idx) {
  const uint32_t first = (word & ~rtl::kLeafBit) >> 3, nt = (word & 7u) + 1u;
  RBox b = rb_empty();
  for (uint32_t k = 0; k < nt; ++k) {
    float4 *g = tri + 3 * ((size_t)first + k);
    const uint32_t id = __float_as_uint(g[0].w);
    float v[3][3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      divided(vpos, idx[3 * (size_t)id + j], v[j]);
      rb_grow(b, v[j], v[j]);
    }
    g[0] = float4{v[0][0], v[0][1], v[0][2], __uint_as_float(id)};
    g[1] = float4{v[1][0], v[1][1], v[1][2], 0.0f};
    g[2] = float4{v[2][0], v[2][1], v[2][2], 0.0f};
  }
  return b;
}

// Nodes [first, first + count) of one depth level; lane t handles child slot
// t & 7 of node first + (t >> 3). The level below is finished (an earlier
// launch on the stream).
__global__ __launch_bounds__(256) void sdf_refit_level_kernel(rtl::GNode *nodes, float4 *tri,
                                                              const float4 *__restrict__ vpos,
                                                              const uint32_t *__restrict__ idx, uint32_t first,
                                                              uint32_t count) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  const uint32_t n = t >> 3, c = t & 7u;
  if (n >= count) return;
  rtl::GNode *g = nodes + (size_t)first + n;
  const uint32_t w = g->child[c];
  if (w == rtl::kInvalidChild) return;  // an empty slot keeps its +inf box
  RBox b;
  if (w & rtl::kLeafBit) {
    b = refit_leaf(w, tri, vpos, idx);
  } else {
    const rtl::GNode *ch = nodes + w;
    b = rb_empty();
#pragma unroll
    for (int cc = 0; cc < 8; ++cc)
      if (ch->child[cc] != rtl::kInvalidChild) {
        const float mn[3] = {ch->box[cc][0], ch->box[cc][2], ch->box[cc][4]};
        const float mx[3] = {ch->box[cc][1], ch->box[cc][3], ch->box[cc][5]};
        rb_grow(b, mn, mx);
      }
  }
  float2 *o = reinterpret_cast<float2 *>(g->box[c]);  // (24 c bytes into a 32-byte aligned node)
  o[0] = float2{b.mn[0], b.mx[0]};
  o[1] = float2{b.mn[1], b.mx[1]};
  o[2] = float2{b.mn[2], b.mx[2]};
}

// A tree without inner nodes: the root word is the one leaf, no box is kept.
__global__ void sdf_refit_root_leaf_kernel(uint32_t root, float4 *tri, const float4 *__restrict__ vpos,
                                           const uint32_t *__restrict__ idx) {
  if (blockIdx.x == 0 && threadIdx.x == 0) (void)refit_leaf(root, tri, vpos, idx);
}

// Interior angle at corner o between the edges to u and w (prep_sdf_mesh):
// 0 when an edge has zero length, the cosine clamped with std::min / std::max.
__device__ __forceinline__ double corner_angle(const float o[3], const float u[3], const float w[3]) {
  const double ux = (double)u[0] - o[0], uy = (double)u[1] - o[1], uz = (double)u[2] - o[2];
  const double wx = (double)w[0] - o[0], wy = (double)w[1] - o[1], wz = (double)w[2] - o[2];
  const double lu = __builtin_sqrt(ux * ux + uy * uy + uz * uz), lw = __builtin_sqrt(wx * wx + wy * wy + wz * wz);
  if (!(lu > 0.0 && lw > 0.0)) return 0.0;
  const double q = (ux * wx + uy * wy + uz * wz) / (lu * lw);
  const double lo = (-1.0 < q) ? q : -1.0;   // std::max(-1.0, q)
  const double cs = (lo < 1.0) ? lo : 1.0;   // std::min(1.0, lo)
  return acos(cs);
}

__global__ __launch_bounds__(256) void sdf_tri_terms_kernel(const float4 *__restrict__ vpos,
                                                            const uint32_t *__restrict__ idx, uint32_t ntri,
                                                            float4 *__restrict__ fn, double *__restrict__ ang) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t >= ntri) return;
  float v[3][3];
#pragma unroll
  for (int j = 0; j < 3; ++j) divided(vpos, idx[3 * (size_t)t + j], v[j]);
  const float e1[3] = {v[1][0] - v[0][0], v[1][1] - v[0][1], v[1][2] - v[0][2]};
  const float e2[3] = {v[2][0] - v[0][0], v[2][1] - v[0][1], v[2][2] - v[0][2]};
  const float nx = e1[1] * e2[2] - e1[2] * e2[1];
  const float ny = e1[2] * e2[0] - e1[0] * e2[2];
  const float nz = e1[0] * e2[1] - e1[1] * e2[0];
  const float l = __builtin_sqrtf(nx * nx + ny * ny + nz * nz);
  fn[t] = l > 0.0f ? float4{nx / l, ny / l, nz / l, 0.0f} : float4{0.0f, 0.0f, 0.0f, 0.0f};
  ang[3 * (size_t)t + 0] = corner_angle(v[0], v[1], v[2]);
  ang[3 * (size_t)t + 1] = corner_angle(v[1], v[2], v[0]);
  ang[3 * (size_t)t + 2] = corner_angle(v[2], v[0], v[1]);
}

__global__ __launch_bounds__(256) void sdf_vertex_sums_kernel(const uint32_t *__restrict__ off,
                                                              const uint32_t *__restrict__ inc,
                                                              const float4 *__restrict__ fn,
                                                              const double *__restrict__ ang, uint32_t n,
                                                              float4 *__restrict__ vn) {
  const uint32_t w = blockIdx.x * 256u + threadIdx.x;
  if (w >= n) return;
  double ax = 0.0, ay = 0.0, az = 0.0;
  const uint32_t end = off[w + 1];
  for (uint32_t j = off[w]; j < end; ++j) {
    const uint32_t e = inc[j];  // 3 * triangle + corner
    const float4 nf = fn[e / 3u];
    const double a = ang[e];
    ax += a * nf.x;
    ay += a * nf.y;
    az += a * nf.z;
  }
  vn[w] = float4{(float)ax, (float)ay, (float)az, 0.0f};
}

__global__ __launch_bounds__(256) void sdf_edge_sums_kernel(const uint32_t *__restrict__ off,
                                                            const uint32_t *__restrict__ inc,
                                                            const float4 *__restrict__ fn, uint32_t n,
                                                            float4 *__restrict__ en) {
  const uint32_t e = blockIdx.x * 256u + threadIdx.x;
  if (e >= n) return;
  double ax = 0.0, ay = 0.0, az = 0.0;
  const uint32_t end = off[e + 1];
  for (uint32_t j = off[e]; j < end; ++j) {
    const float4 nf = fn[inc[j]];
    ax += nf.x;
    ay += nf.y;
    az += nf.z;
  }
  en[e] = float4{(float)ax, (float)ay, (float)az, 0.0f};
}

// pn[7 t + f]: f = 0..2 the welded vertex of corner f, 3..5 the welded edge ab, ac, bc, 6 the face.
__global__ __launch_bounds__(256) void sdf_scatter_pn_kernel(const uint32_t *__restrict__ idx,
                                                             const uint32_t *__restrict__ weld,
                                                             const uint32_t *__restrict__ tri_edge,
                                                             const float4 *__restrict__ vn,
                                                             const float4 *__restrict__ en,
                                                             const float4 *__restrict__ fn, uint32_t ntri,
                                                             float4 *__restrict__ pn) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= 7ull * ntri) return;
  const uint32_t t = (uint32_t)(i / 7u), f = (uint32_t)(i % 7u);
  float4 v;
  if (f < 3u) v = vn[weld[idx[3 * (size_t)t + f]]];
  else if (f < 6u) v = en[tri_edge[3 * (size_t)t + (f - 3u)]];
  else v = fn[t];
  pn[i] = v;
}

inline uint32_t blocks_of(uint64_t n) { return (uint32_t)((n + 255u) / 256u); }

}  // namespace

namespace rtsdf {
int sdf_refit_launch(const SdfRefitArgs &a, hipStream_t st) {
  const float4 *vpos = reinterpret_cast<const float4 *>(a.vpos4);
  if (a.ntri == 0) return RT_OK;
  sdf_tri_terms_kernel<<<blocks_of(a.ntri), 256, 0, st>>>(vpos, a.idx, a.ntri, a.fn, a.ang);
  HIP_TRY(hipGetLastError());
  if (a.levels <= 0) {
    if (a.root != rtl::kInvalidChild) {
      sdf_refit_root_leaf_kernel<<<1, 64, 0, st>>>(a.root, a.tri, vpos, a.idx);
      HIP_TRY(hipGetLastError());
    }
  } else {
    for (int32_t l = a.levels - 1; l >= 0; --l) {
      const uint32_t first = a.level_first[l], count = a.level_first[l + 1] - first;
      sdf_refit_level_kernel<<<blocks_of((uint64_t)count * 8u), 256, 0, st>>>(a.nodes, a.tri, vpos, a.idx, first, count);
      HIP_TRY(hipGetLastError());
    }
  }
  sdf_vertex_sums_kernel<<<blocks_of(a.n_wverts), 256, 0, st>>>(a.v_off, a.v_inc, a.fn, a.ang, a.n_wverts, a.vn);
  HIP_TRY(hipGetLastError());
  sdf_edge_sums_kernel<<<blocks_of(a.n_wedges), 256, 0, st>>>(a.e_off, a.e_inc, a.fn, a.n_wedges, a.en);
  HIP_TRY(hipGetLastError());
  sdf_scatter_pn_kernel<<<blocks_of(7ull * a.ntri), 256, 0, st>>>(a.idx, a.weld, a.tri_edge, a.vn, a.en, a.fn, a.ntri,
                                                                 a.pn);
  HIP_TRY(hipGetLastError());
  return RT_OK;
}
}  // namespace rtsdf
