// rt_sdf_octree.hip -- an SDF octree rebuilt on the device from an SDF-mesh
// handle (rt_sdf_mesh_octree_device): the tree of
// rth::build_sdf_octree in the device layout of rth::flatten_octree, written
// into the scratch of a scene made by rt_scene_create_octree_dynamic and
// published into the scene's arrays by the last launch, unless it overflowed.
//
// The launches are listed in rt_sdf_octree.h. No workgroup waits on another:
// the ordered scan of a level's refine flags is three launches (block sums,
// one block over the sums, the ranked scatter), and the levels are separate
// launches that pass their sizes through the level table on the device. The
// host knows no level size: every launch is sized by the scene's capacity, and
// a work-item beyond its level's size returns at once.
//
// The distances are those of rt_sdf_mesh_points for the same points: the walk
// below is rt_sdfgen.hip's sdf_query over the shared pieces of rt_points.h
// (nearest box first, the (d^2, id) winner, prune_bound's slack, the sign from
// the winning feature's pseudonormal), one point per lane with the same
// lane-interleaved LDS stack.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/rtamd.h"
#include "rt_error.h"
#include "rt_layout.h"
#include "rt_math.h"
#include "rt_points.h"
#include "rt_scene.h"
#include "rt_sdf_octree.h"

using namespace rtd;
using namespace rtsdf;

namespace {

constexpr int kScanBlock = 256;

// Signed distance at p. st_d / st_w: this lane's LDS stack columns (stride 64).
__device__ float sdf_walk(const SdfDev &m, f3 p, float *st_d, uint32_t *st_w) {
  float best = kInf, bound = kInf;
  uint32_t best_id = 0xFFFFFFFFu;
  int best_feat = 0;
  f3 best_q{0.0f, 0.0f, 0.0f};
  int sp = 0;
  uint32_t word = m.root;
  while (word != rtl::kInvalidChild) {
    if (word & rtl::kLeafBit) {
      const uint32_t first = (word >> 3) & rtl::kMaxLeafFirstTri, n = (word & 7u) + 1u;
      for (uint32_t k = 0; k < n; ++k) {
        const float4 A = m.tri[3 * (first + k)], B = m.tri[3 * (first + k) + 1], C = m.tri[3 * (first + k) + 2];
        int feat;
        const f3 q = closest_on_tri(p, f3{A.x, A.y, A.z}, f3{B.x, B.y, B.z}, f3{C.x, C.y, C.z}, feat);
        const f3 e = p - q;
        const float d2 = dot(e, e);
        const uint32_t id = __float_as_uint(A.w);
        if (d2 < best || (d2 == best && id < best_id)) {
          best = d2;
          best_id = id;
          best_feat = feat;
          best_q = q;
          bound = prune_bound(best);
        }
      }
    } else {
      const rtl::GNode &nd = m.nodes[word];
      float bx[48];
      const float4 *b4 = reinterpret_cast<const float4 *>(nd.box);
#pragma unroll
      for (int i = 0; i < 12; ++i) {
        const float4 v = b4[i];
        bx[4 * i] = v.x; bx[4 * i + 1] = v.y; bx[4 * i + 2] = v.z; bx[4 * i + 3] = v.w;
      }
      const uint4 c0 = reinterpret_cast<const uint4 *>(nd.child)[0];
      const uint4 c1 = reinterpret_cast<const uint4 *>(nd.child)[1];
      float t[8];
      uint32_t id[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
#pragma unroll
      for (int c = 0; c < 8; ++c) t[c] = id[c] == rtl::kInvalidChild ? kInf : box_d2(bx + 6 * c, p);
      sort8(t, id);
      // push farthest first so the nearest is popped next; a node pops one
      // entry and pushes at most eight, so sp stays below cap = 7 * depth + 1
#pragma unroll
      for (int c = 7; c >= 0; --c) {
        if (id[c] != rtl::kInvalidChild && t[c] <= bound) {
          st_d[sp * kWave] = t[c];
          st_w[sp * kWave] = id[c];
          ++sp;
        }
      }
    }
    // pop the next box that can still hold a closer triangle
    word = rtl::kInvalidChild;
    while (sp > 0) {
      --sp;
      if (st_d[sp * kWave] <= bound) {
        word = st_w[sp * kWave];
        break;
      }
    }
  }
  if (best_id == 0xFFFFFFFFu) return kInf;
  const float4 N = m.pn[7u * best_id + (uint32_t)best_feat];
  const f3 e = p - best_q;
  const float s = e.x * N.x + e.y * N.y + e.z * N.z;
  const float d = __builtin_sqrtf(best);
  return s < 0.0f ? -d : d;
}

// 2^e for e in [-126, 127] (std::ldexp(1.0f, e) on the host)
__device__ __forceinline__ float pow2f(int e) { return __uint_as_float((uint32_t)(127 + e) << 23); }

__device__ __forceinline__ uint64_t cell_pack(uint32_t x, uint32_t y, uint32_t z) {
  return (uint64_t)x | ((uint64_t)y << 16) | ((uint64_t)z << 32);
}
__device__ __forceinline__ uint32_t cell_x(uint64_t c) { return (uint32_t)c & 0xFFFFu; }
__device__ __forceinline__ uint32_t cell_y(uint64_t c) { return (uint32_t)(c >> 16) & 0xFFFFu; }
__device__ __forceinline__ uint32_t cell_z(uint64_t c) { return (uint32_t)(c >> 32) & 0xFFFFu; }

// Exclusive scan of v over the block's 256 lanes in lane order; total = the
// block's sum. Every lane of the block calls it.
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t &total) {
  __shared__ uint32_t wsum[kScanBlock / kWave];
  const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
  uint32_t inc = v;
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const uint32_t u = __shfl_up(inc, o, kWave);
    if (lane >= o) inc += u;
  }
  if (lane == kWave - 1) wsum[w] = inc;
  __syncthreads();
  uint32_t before = 0, all = 0;
#pragma unroll
  for (int k = 0; k < kScanBlock / kWave; ++k) {
    const uint32_t s = wsum[k];
    if (k < w) before += s;
    all += s;
  }
  __syncthreads();  // (wsum is written again by the caller's next scan)
  total = all;
  return before + inc - v;
}

// The level table of a new build: level 0 is the root's cell, nothing has
// overflowed.
__global__ __launch_bounds__(kWave) void oct_begin_kernel(uint32_t *lvl, uint64_t *cells) {
  if (threadIdx.x < kOctLvlWords) lvl[threadIdx.x] = threadIdx.x == 1 ? 1u : 0u;
  if (threadIdx.x == 0) cells[0] = 0;
}

// The centre of cell (x, y, z) of level d.
__device__ __forceinline__ f3 cell_centre(uint32_t x, uint32_t y, uint32_t z, int d) {
  const float half = pow2f(-d);
  return f3{(float)(2 * x + 1) * half - 1.0f, (float)(2 * y + 1) * half - 1.0f, (float)(2 * z + 1) * half - 1.0f};
}

// The SDF at the centre of EVERY cell of levels 0 .. top - 1, one cell per
// lane, whether the tree will hold the cell or not: top[oct_top_first(d) +
// (x << 2d | y << d | z)]. A walk from a cell centre far from the surface is
// long and a level of a few cells is one such walk after another, so the top
// levels are taken out of the level-by-level chain: their walks run side by
// side here, and their level launches only look the values up.
__global__ __launch_bounds__(kWave) void oct_top_kernel(SdfDev m, int cap, int top_levels, float *top) {
  extern __shared__ uint32_t lds[];
  float *st_d = reinterpret_cast<float *>(lds) + threadIdx.x;
  uint32_t *st_w = lds + (size_t)cap * kWave + threadIdx.x;
  const uint32_t g = blockIdx.x * kWave + threadIdx.x;
  if (g >= oct_top_first(top_levels)) return;
  int d = 0;
  while (g >= oct_top_first(d + 1)) ++d;
  const uint32_t i = g - oct_top_first(d), mask = (1u << d) - 1u;
  top[g] = sdf_walk(m, cell_centre(i >> (2 * d), (i >> d) & mask, i & mask, d), st_d, st_w);
}

// Level d < depth, one node per lane: refined iff |sdf(centre)| <= sqrt(3) *
// the half size; the SDF from the table of the top levels (d < top_levels) or
// from a walk. Dynamic LDS: cap x 64 floats then cap x 64 child words.
__global__ __launch_bounds__(kWave) void oct_centre_kernel(SdfDev m, int cap, const uint32_t *lvl, int d,
                                                          const uint64_t *cells, const float *top, int top_levels,
                                                          uint32_t *flag) {
  extern __shared__ uint32_t lds[];
  float *st_d = reinterpret_cast<float *>(lds) + threadIdx.x;
  uint32_t *st_w = lds + (size_t)cap * kWave + threadIdx.x;
  const uint32_t first = lvl[2 * d], n = lvl[2 * d + 1];
  const uint64_t j = (uint64_t)blockIdx.x * kWave + threadIdx.x;
  if (j >= n) return;
  const uint64_t c = cells[first + j];
  const uint32_t x = cell_x(c), y = cell_y(c), z = cell_z(c);
  const float s = d < top_levels ? top[oct_top_first(d) + ((x << (2 * d)) | (y << d) | z)]
                                 : sdf_walk(m, cell_centre(x, y, z, d), st_d, st_w);
  flag[j] = fabsf(s) <= 1.7320508f * pow2f(-d) ? 1u : 0u;
}

// The four flags lane t of tile b owns (nodes b * 1024 + 4 t ..), those past
// the level's size as 0. flag holds a whole number of tiles.
__device__ __forceinline__ uint4 tile_flags(const uint32_t *flag, uint64_t i0, uint32_t n) {
  uint4 f = *reinterpret_cast<const uint4 *>(flag + i0);
  f.x = i0 < n ? f.x : 0u;
  f.y = i0 + 1 < n ? f.y : 0u;
  f.z = i0 + 2 < n ? f.z : 0u;
  f.w = i0 + 3 < n ? f.w : 0u;
  return f;
}

// bsum[b] = the refined nodes among tile b's 1024
__global__ __launch_bounds__(kScanBlock) void oct_flag_sum_kernel(const uint32_t *lvl, int d, const uint32_t *flag,
                                                                 uint32_t *bsum) {
  const uint32_t n = lvl[2 * d + 1];
  const uint64_t base = (uint64_t)blockIdx.x * kOctScanTile;
  if (base >= n) return;  // (the whole block)
  const uint4 f = tile_flags(flag, base + 4 * threadIdx.x, n);
  uint32_t total;
  block_scan(f.x + f.y + f.z + f.w, total);
  if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// One block: bsum becomes its exclusive scan, and level d + 1 gets its first
// node and its size, 8 per refined node -- or, if the tree would pass
// max_nodes, size 0 and the overflow flag, which empties every later launch.
__global__ __launch_bounds__(kScanBlock) void oct_level_close_kernel(uint32_t *lvl, int d, uint32_t *bsum,
                                                                    uint32_t max_nodes) {
  const uint32_t n = lvl[2 * d + 1];
  const uint32_t nb = (uint32_t)(((uint64_t)n + kOctScanTile - 1) / kOctScanTile);
  uint32_t carry = 0;
  for (uint32_t b0 = 0; b0 < nb; b0 += kScanBlock) {
    const uint32_t b = b0 + threadIdx.x;
    const uint32_t v = b < nb ? bsum[b] : 0u;
    uint32_t total;
    const uint32_t ex = block_scan(v, total);
    if (b < nb) bsum[b] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) {
    const uint64_t next_first = (uint64_t)lvl[2 * d] + n, next_n = 8ull * carry;
    const bool ovf = lvl[kOctLvlOvf] != 0 || next_first + next_n > max_nodes;
    lvl[2 * d + 2] = (uint32_t)next_first;
    lvl[2 * d + 3] = ovf ? 0u : (uint32_t)next_n;
    lvl[kOctLvlOvf] = ovf ? 1u : 0u;
  }
}

// Level d's node records, and the cells of level d + 1 in the order of their
// parents: the r-th refined node's children are nodes next_first + 8 r + id.
__global__ __launch_bounds__(kScanBlock) void oct_scatter_kernel(const uint32_t *lvl, int d, const uint32_t *flag,
                                                                const uint32_t *bsum, uint64_t *cells,
                                                                rtl::OctWord *s_child, rtl::OctVals *s_vals) {
  const uint32_t first = lvl[2 * d], n = lvl[2 * d + 1], next_first = lvl[2 * d + 2];
  const uint64_t base = (uint64_t)blockIdx.x * kOctScanTile;
  if (base >= n || lvl[kOctLvlOvf] != 0) return;  // (the whole block)
  const uint64_t i0 = base + 4 * threadIdx.x;
  const uint4 f4 = tile_flags(flag, i0, n);
  const uint32_t f[4] = {f4.x, f4.y, f4.z, f4.w};
  uint32_t total;
  uint32_t r = bsum[blockIdx.x] + block_scan(f4.x + f4.y + f4.z + f4.w, total);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (i0 + k >= n) break;
    const uint32_t node = first + (uint32_t)(i0 + k);
    float4 *v4 = reinterpret_cast<float4 *>(s_vals[node].v);
    if (!f[k]) {  // an empty leaf (every value > 10: it never hits)
      s_child[node] = rtl::OctWord{rtl::kOctNeverHits, 0u};
      v4[0] = v4[1] = float4{1000.0f, 1000.0f, 1000.0f, 1000.0f};
      continue;
    }
    const uint32_t off = next_first + 8u * r;
    ++r;
    s_child[node] = rtl::OctWord{off, 0u};
    v4[0] = v4[1] = float4{0.0f, 0.0f, 0.0f, 0.0f};
    const uint64_t c = cells[node];
    const uint32_t x = 2 * cell_x(c), y = 2 * cell_y(c), z = 2 * cell_z(c);
#pragma unroll
    for (uint32_t id = 0; id < 8; ++id) cells[off + id] = cell_pack(x + (id >> 2), y + ((id >> 1) & 1u), z + (id & 1u));
  }
}

// The level-`depth` leaves, one corner per lane: values[(x << 2) | (y << 1) | z].
__global__ __launch_bounds__(kWave) void oct_corner_kernel(SdfDev m, int cap, const uint32_t *lvl, int depth,
                                                          const uint64_t *cells, rtl::OctVals *s_vals) {
  extern __shared__ uint32_t lds[];
  float *st_d = reinterpret_cast<float *>(lds) + threadIdx.x;
  uint32_t *st_w = lds + (size_t)cap * kWave + threadIdx.x;
  const uint32_t first = lvl[2 * depth], n = lvl[2 * depth + 1];
  const uint64_t i = (uint64_t)blockIdx.x * kWave + threadIdx.x;
  const uint64_t j = i >> 3;
  const uint32_t k = (uint32_t)i & 7u;
  if (j >= n) return;
  const uint64_t c = cells[first + j];
  const float size = pow2f(1 - depth);
  const f3 p{(float)(cell_x(c) + (k >> 2)) * size - 1.0f, (float)(cell_y(c) + ((k >> 1) & 1u)) * size - 1.0f,
             (float)(cell_z(c) + (k & 1u)) * size - 1.0f};
  s_vals[first + j].v[k] = sdf_walk(m, p, st_d, st_w);
}

// Their words: rth::flatten_octree's leaf rule.
__global__ __launch_bounds__(kScanBlock) void oct_leaf_word_kernel(const uint32_t *lvl, int depth,
                                                                  const rtl::OctVals *s_vals, rtl::OctWord *s_child) {
  const uint32_t first = lvl[2 * depth], n = lvl[2 * depth + 1];
  const uint64_t j = (uint64_t)blockIdx.x * kScanBlock + threadIdx.x;
  if (j >= n) return;
  const float4 *v4 = reinterpret_cast<const float4 *>(s_vals[first + j].v);
  const float4 a = v4[0], b = v4[1];
  const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  bool all10 = true, all0 = true, all_above = true;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    all10 = all10 && (v[k] > 10.0f);
    all0 = all0 && (v[k] == 0.0f);
    all_above = all_above && (v[k] >= 1e-4f);
  }
  s_child[first + j] = rtl::OctWord{(all10 || all0 || all_above) ? rtl::kOctNeverHits : 0u, 0u};
}

// The child masks of level d's inner nodes from the words of level d + 1,
// whose masks the launch before this one wrote.
__global__ __launch_bounds__(kScanBlock) void oct_mask_kernel(const uint32_t *lvl, int d, rtl::OctWord *s_child) {
  const uint32_t first = lvl[2 * d], n = lvl[2 * d + 1];
  const uint64_t j = (uint64_t)blockIdx.x * kScanBlock + threadIdx.x;
  if (j >= n || lvl[kOctLvlOvf] != 0) return;
  const uint32_t c = s_child[first + j].child;
  if (c == 0u || c == rtl::kOctNeverHits) return;
  uint32_t mask = 0;
#pragma unroll
  for (uint32_t k = 0; k < 8; ++k) {
    const rtl::OctWord w = s_child[c + k];
    if (w.child == 0u)
      mask |= (1u << k) | (1u << (8 + k));
    else if (w.child != rtl::kOctNeverHits && (w.masks & 0xFFu))
      mask |= 1u << k;
  }
  s_child[first + j].masks = mask;
}

// Scratch -> scene, one node per lane, and the scene's status; a build that
// overflowed only records that it was dropped.
__global__ __launch_bounds__(kScanBlock) void oct_publish_kernel(const uint32_t *lvl, int depth,
                                                                const rtl::OctWord *s_child, const rtl::OctVals *s_vals,
                                                                rtl::OctWord *child, rtl::OctVals *ovals,
                                                                uint32_t *status) {
  const uint64_t i = (uint64_t)blockIdx.x * kScanBlock + threadIdx.x;
  if (lvl[kOctLvlOvf] != 0) {
    if (i == 0) status[1] = 1u;
    return;
  }
  const uint32_t total = lvl[2 * depth] + lvl[2 * depth + 1];
  if (i == 0) {
    status[0] = total;
    status[1] = 0u;
  }
  if (i >= total) return;
  child[i] = s_child[i];
  const float4 *src = reinterpret_cast<const float4 *>(s_vals[i].v);
  float4 *dst = reinterpret_cast<float4 *>(ovals[i].v);
  dst[0] = src[0];
  dst[1] = src[1];
}

// blocks of `block` lanes over min(max_nodes, 8^d) nodes, `per` lanes each
uint32_t level_blocks(uint32_t max_nodes, int d, uint32_t block, uint32_t per = 1) {
  const uint64_t nodes = std::min<uint64_t>(max_nodes, 1ull << (3 * d));
  return (uint32_t)((nodes * per + block - 1) / block);
}

}  // namespace

namespace rtsdf {

int octree_build_launch(const rt_sdf_mesh *m, const OctBuildArgs &a, hipStream_t st) {
  const SdfDev sd = dev_of(m);
  const size_t lds = lds_bytes(m);
  const uint32_t C = a.max_nodes;
  const int top = oct_top_levels(a.depth);
  hipLaunchKernelGGL(oct_begin_kernel, dim3(1), dim3(kWave), 0, st, a.lvl, a.cells);
  if (top > 0)
    hipLaunchKernelGGL(oct_top_kernel, dim3((oct_top_first(top) + kWave - 1) / kWave), dim3(kWave), lds, st, sd,
                       m->stack_cap, top, a.top);
  for (int d = 0; d < a.depth; ++d) {
    const uint32_t tiles = level_blocks(C, d, kOctScanTile);
    // (a level of the table needs no stack)
    hipLaunchKernelGGL(oct_centre_kernel, dim3(level_blocks(C, d, kWave)), dim3(kWave), d < top ? 0 : lds, st, sd,
                       m->stack_cap, a.lvl, d, a.cells, a.top, top, a.flag);
    hipLaunchKernelGGL(oct_flag_sum_kernel, dim3(tiles), dim3(kScanBlock), 0, st, a.lvl, d, a.flag, a.bsum);
    hipLaunchKernelGGL(oct_level_close_kernel, dim3(1), dim3(kScanBlock), 0, st, a.lvl, d, a.bsum, C);
    hipLaunchKernelGGL(oct_scatter_kernel, dim3(tiles), dim3(kScanBlock), 0, st, a.lvl, d, a.flag, a.bsum, a.cells,
                       a.s_child, a.s_vals);
  }
  hipLaunchKernelGGL(oct_corner_kernel, dim3(level_blocks(C, a.depth, kWave, 8)), dim3(kWave), lds, st, sd,
                     m->stack_cap, a.lvl, a.depth, a.cells, a.s_vals);
  hipLaunchKernelGGL(oct_leaf_word_kernel, dim3(level_blocks(C, a.depth, kScanBlock)), dim3(kScanBlock), 0, st, a.lvl,
                     a.depth, a.s_vals, a.s_child);
  for (int d = a.depth - 1; d >= 0; --d)
    hipLaunchKernelGGL(oct_mask_kernel, dim3(level_blocks(C, d, kScanBlock)), dim3(kScanBlock), 0, st, a.lvl, d,
                       a.s_child);
  hipLaunchKernelGGL(oct_publish_kernel, dim3((uint32_t)(((uint64_t)C + kScanBlock - 1) / kScanBlock)),
                     dim3(kScanBlock), 0, st, a.lvl, a.depth, a.s_child, a.s_vals, a.child, a.ovals, a.status);
  HIP_TRY(hipGetLastError());
  return RT_OK;
}

}  // namespace rtsdf

extern "C" {

int rt_sdf_mesh_octree_device(rt_sdf_mesh *m, rt_scene *s, void *stream) {
  if (!m) return rterr::set(RT_E_INVALID, "rt_sdf_mesh_octree_device: SDF mesh is NULL");
  if (!s) return rterr::set(RT_E_INVALID, "rt_sdf_mesh_octree_device: scene is NULL");
  if (s->info.kind != RT_SCENE_OCTREE || !s->octdyn.on)
    return rterr::set(RT_E_STATE, "rt_sdf_mesh_octree_device: the scene was not made by rt_scene_create_octree_dynamic");
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (m->device != dev || s->device != dev)
    return rterr::set(RT_E_INVALID, "rt_sdf_mesh_octree_device: handle (device " + std::to_string(m->device) +
                                        ") and scene (device " + std::to_string(s->device) +
                                        ") must live on the current device " + std::to_string(dev));
  OctBuildArgs a{};
  a.depth = s->oct.depth;
  a.max_nodes = s->octdyn.max_nodes;
  a.child = s->geo.child.p;
  a.ovals = s->geo.ovals.p;
  a.status = s->octdyn.status.p;
  a.s_child = s->octdyn.s_child.p;
  a.s_vals = s->octdyn.s_vals.p;
  a.cells = s->octdyn.cells.p;
  a.flag = s->octdyn.flag.p;
  a.bsum = s->octdyn.bsum.p;
  a.lvl = s->octdyn.lvl.p;
  a.top = s->octdyn.top.p;
  return octree_build_launch(m, a, (hipStream_t)stream);
}

}  // extern "C"
