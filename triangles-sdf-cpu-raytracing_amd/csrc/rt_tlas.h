// rt_tlas.h -- the top-level tree of an instanced scene created with
// RT_INSTANCED_TLAS (include/rtamd.h): the two functions
// that DEFINE the mode (world_box, box_pass), the implicit tree's node record
// and the cursor walk, written once for the host and the device. Plain float
// operations in the written order, never fused (-ffp-contract=off on both
// sides), so the host entries, the kernels of rt_tlas.hip and the tests' numpy
// restatement (tests/tlas_common.py) give the same bits. Includes nothing of
// HIP: a plain C++ program may include it.
#pragma once
#include <stdint.h>

#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif

namespace rtt {

// One node of the tree, 32 bytes: lo.xyz, hi.xyz, two pad words (zero). The
// tree is the complete binary tree over P = the smallest power of two >= K
// leaves in heap order: node 1 is the root, node n has the children 2n and
// 2n + 1, leaf P + i holds instance i's world box (the empty box for i >= K).
// Node 0 is not used. For K = 1 node 1 is the leaf.
struct TNode {
  float b[6];
  uint32_t pad[2];
};
static_assert(sizeof(TNode) == 32, "top-level node: 32 bytes");

constexpr float kTInf = __builtin_huge_valf();
constexpr float kPad = 1.0f / 65536.0f;  // 2^-16 of the box's own scale (world_box)

__host__ __device__ inline int32_t leaf_count(int32_t k) {
  int32_t p = 1;
  while (p < k) p <<= 1;
  return p;
}

// the one encoding of "no box": lo = +inf, hi = -inf (box_pass tests b[0] > b[3])
__host__ __device__ inline void empty_box(float b[6]) {
  b[0] = b[1] = b[2] = kTInf;
  b[3] = b[4] = b[5] = -kTInf;
}
// the box of an instance whose BLAS is one leaf (no root box): every ray passes
__host__ __device__ inline void unbounded_box(float b[6]) {
  b[0] = b[1] = b[2] = -kTInf;
  b[3] = b[4] = b[5] = kTInf;
}

__host__ __device__ inline float tmin(float a, float b) { return a < b ? a : b; }  // isp_min (rt_math.h)
__host__ __device__ inline float tmax(float a, float b) { return a > b ? a : b; }  // isp_max

// wb = the world box of object box ob (lo.xyz, hi.xyz) under the object-to-world
// map x (row-major 3x4): the eight corners (bit a of c picks hi on axis a), each
// p[r] = ((x[4r]*c.x + x[4r+1]*c.y) + x[4r+2]*c.z) + x[4r+3], folded in corner
// order with a < b ? a : b and a > b ? a : b; then padded on every side by
// e = 2^-16 * (max_r max(|lo_r|, |hi_r|) + max_r (hi_r - lo_r)).
__host__ __device__ inline void world_box(const float x[12], const float ob[6], float wb[6]) {
  float lo[3] = {0.0f, 0.0f, 0.0f}, hi[3] = {0.0f, 0.0f, 0.0f};
  for (int c = 0; c < 8; ++c) {
    const float cx = ob[(c & 1) ? 3 : 0], cy = ob[(c & 2) ? 4 : 1], cz = ob[(c & 4) ? 5 : 2];
    for (int r = 0; r < 3; ++r) {
      const float p = ((x[4 * r] * cx + x[4 * r + 1] * cy) + x[4 * r + 2] * cz) + x[4 * r + 3];
      lo[r] = c == 0 ? p : tmin(lo[r], p);
      hi[r] = c == 0 ? p : tmax(hi[r], p);
    }
  }
  float mag = 0.0f, ext = 0.0f;
  for (int r = 0; r < 3; ++r) {
    const float al = __builtin_fabsf(lo[r]), ah = __builtin_fabsf(hi[r]);
    const float a = tmax(al, ah);
    const float w = hi[r] - lo[r];
    mag = r == 0 ? a : tmax(mag, a);
    ext = r == 0 ? w : tmax(ext, w);
  }
  const float e = kPad * (mag + ext);
  for (int r = 0; r < 3; ++r) {
    wb[r] = lo[r] - e;
    wb[3 + r] = hi[r] + e;
  }
}

// root_box_miss (rt_scenes.h) negated, on a world box and the world ray, with
// that function's expressions verbatim; inv = 1 / d per component. False for
// the empty box. Passes when a component of inv is not finite.
__host__ __device__ inline bool box_pass_inv(const float b[6], float ox, float oy, float oz, float ix, float iy,
                                             float iz, float tn, float tf) {
  if (b[0] > b[3]) return false;
  if (!(__builtin_isfinite(ix) && __builtin_isfinite(iy) && __builtin_isfinite(iz))) return true;
  const float t1x = (b[0] - ox) * ix, t1y = (b[1] - oy) * iy, t1z = (b[2] - oz) * iz;
  const float t2x = (b[3] - ox) * ix, t2y = (b[4] - oy) * iy, t2z = (b[5] - oz) * iz;
  float tMin = tmax(tmin(t1x, t2x), tmax(tmin(t1y, t2y), tmin(t1z, t2z)));
  float tMax = tmin(tmax(t1x, t2x), tmin(tmax(t1y, t2y), tmax(t1z, t2z)));
  tMin = tmax(tMin, tn);
  tMax = tmin(tMax, tf);
  return !(tMax < 0.0f || tMin > tMax);
}
__host__ __device__ inline bool box_pass(const float b[6], const float o[3], const float d[3], float tn, float tf) {
  return box_pass_inv(b, o[0], o[1], o[2], 1.0f / d[0], 1.0f / d[1], 1.0f / d[2], tn, tf);
}

// node = the exact min / max of two nodes (the empty box is the neutral element)
__host__ __device__ inline void box_union(const float a[6], const float c[6], float out[6]) {
  for (int r = 0; r < 3; ++r) {
    out[r] = tmin(a[r], c[r]);
    out[3 + r] = tmax(a[3 + r], c[3 + r]);
  }
}

// The cursor walk, without a stack. Leaving node n (a failed node, or a leaf
// that was handled) the walk goes on at the next node in depth-first order
// that is not below n: (n + 1) with its trailing zero bits shifted out. 0: the
// walk is over (the successor would be the root).
__host__ __device__ inline uint32_t walk_skip(uint32_t n) {
  uint32_t m = n + 1u;
  m >>= __builtin_ctz(m);
  return m == 1u ? 0u : m;
}
// From cursor n (0: over) to the next leaf whose box, and every box above it
// that the walk meets, passes under tf: its node index, or 0. Depth first,
// left to right: the leaves come in index order.
__host__ __device__ inline uint32_t walk_next(const TNode *nodes, uint32_t P, uint32_t n, float ox, float oy, float oz,
                                              float ix, float iy, float iz, float tn, float tf) {
  while (n != 0u) {
    if (box_pass_inv(nodes[n].b, ox, oy, oz, ix, iy, iz, tn, tf)) {
      if (n >= P) return n;
      n = 2u * n;
    } else {
      n = walk_skip(n);
    }
  }
  return 0u;
}

// The walk of one ray on host arrays: the candidates in the order the kernel
// meets them. The c-th candidate (c = 0, 1, ...) is searched under
// tf_seq[min(c, ntf - 1)], which stands for tf_i = min(best, tFar) as best
// improves. Writes at most cap indices; returns the number found.
inline int32_t candidates_host(const TNode *nodes, int32_t P, const float o[3], const float d[3], float tn,
                               const float *tf_seq, int32_t ntf, int32_t *out, int32_t cap) {
  const float ix = 1.0f / d[0], iy = 1.0f / d[1], iz = 1.0f / d[2];
  int32_t c = 0;
  uint32_t n = 1u;
  while (n != 0u) {
    const float tf = tf_seq[c < ntf ? c : ntf - 1];
    n = walk_next(nodes, (uint32_t)P, n, o[0], o[1], o[2], ix, iy, iz, tn, tf);
    if (n == 0u) break;
    if (c < cap) out[c] = (int32_t)(n - (uint32_t)P);
    ++c;
    n = walk_skip(n);
  }
  return c;
}

}  // namespace rtt
