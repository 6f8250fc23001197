// rt_refit.hip -- refit of a mesh scene's BVH8 on the device (gfx950): the
// tree of the same topology over new vertex positions, bit for bit what
// rth::refit_bvh8 (rt_host.cpp) computes.
//
// bvh_layout stores the inner nodes in BFS order: every depth level is one
// contiguous index range and children have larger indices than their parent.
// So the refit is one launch per level, deepest first, 8 lanes per node, one
// lane per child slot. A leaf child's lane gathers its (at most 8) triangles'
// vertices through the creation index array, rewrites the GTri records and
// grows the box over them in slot order; an inner child's lane reads the eight
// boxes of the already finished child node and grows over them in child order.
// Each slot is evaluated sequentially by one lane, which is what keeps the
// order -- and with it the sign of a zero that ties -- the host's.
//
// Levels are separated by kernel boundaries: no device-scope atomics, no
// spin-waits, no cooperative launch (the eight XCDs have an L2 each; a kernel
// boundary is the one hand-off that needs no protocol). All stores are plain
// vector stores. Topology (child words, triangle order, orig_id) is only read,
// so no vertex value can make this or a later traversal index out of bounds.
#include <hip/hip_runtime.h>

#include "rt_error.h"
#include "rt_layout.h"
#include "rt_refit.h"

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

// One leaf child: its triangles rewritten from the new vertices (v /= v.w with
// the correctly rounded division of k_fill_tris, e1 = v1 - v0, e2 = v2 - v0,
// orig_id kept; three 16-byte stores per triangle) and the box of their
// vertices -- of the divided vertices themselves, never of v0 + e1, which is
// not exact.
__device__ __forceinline__ RBox refit_leaf(uint32_t word, rtl::GTri *tris, const float4 *__restrict__ vpos,
                                           const uint32_t *__restrict__ idx) {
  const uint32_t first = (word & ~rtl::kLeafBit) >> 3, nt = (word & 7u) + 1u;
  RBox b = rb_empty();
  for (uint32_t k = 0; k < nt; ++k) {
    rtl::GTri *g = tris + (size_t)first + k;
    const uint32_t id = g->orig_id;
    float v[3][3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const float4 p = vpos[idx[3 * (size_t)id + j]];
      v[j][0] = p.x / p.w;
      v[j][1] = p.y / p.w;
      v[j][2] = p.z / p.w;
      rb_grow(b, v[j], v[j]);
    }
    uint4 *q = reinterpret_cast<uint4 *>(g);
    q[0] = uint4{__float_as_uint(v[0][0]), __float_as_uint(v[0][1]), __float_as_uint(v[0][2]), id};
    float4 *f = reinterpret_cast<float4 *>(g);
    f[1] = float4{v[1][0] - v[0][0], v[1][1] - v[0][1], v[1][2] - v[0][2], 0.0f};
    f[2] = float4{v[2][0] - v[0][0], v[2][1] - v[0][1], v[2][2] - v[0][2], 0.0f};
  }
  return b;
}

// Nodes [first, first + count) of one depth level; lane t handles child slot
// t & 7 of node first + (t >> 3). The level below is finished (an earlier
// launch on the stream).
__global__ __launch_bounds__(256) void refit_level_kernel(rtl::GNode *nodes, rtl::GTri *tris,
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
    b = refit_leaf(w, tris, vpos, idx);
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
__global__ void refit_root_leaf_kernel(uint32_t root, rtl::GTri *tris, const float4 *__restrict__ vpos,
                                       const uint32_t *__restrict__ idx) {
  if (blockIdx.x == 0 && threadIdx.x == 0) (void)refit_leaf(root, tris, vpos, idx);
}

}  // namespace

namespace rti {
int refit_launch(const RefitArgs &a, hipStream_t st) {
  const float4 *vpos = reinterpret_cast<const float4 *>(a.vpos4);
  if (a.levels <= 0) {
    if (a.root == rtl::kInvalidChild) return RT_OK;
    refit_root_leaf_kernel<<<1, 64, 0, st>>>(a.root, a.tris, vpos, a.idx);
    HIP_TRY(hipGetLastError());
    return RT_OK;
  }
  for (int32_t l = a.levels - 1; l >= 0; --l) {
    const uint32_t first = a.level_first[l], count = a.level_first[l + 1] - first;
    const uint32_t blocks = (uint32_t)(((uint64_t)count * 8u + 255u) / 256u);
    refit_level_kernel<<<blocks, 256, 0, st>>>(a.nodes, a.tris, vpos, a.idx, first, count);
    HIP_TRY(hipGetLastError());
  }
  return RT_OK;
}
}  // namespace rti
