// rt_points.hip -- closest-point / signed-distance queries for points that
// are already on the GPU (rt_sdf_mesh_points_device).
//
// One point per lane, one 64-lane workgroup, and the walk of rt_sdfgen.hip's
// sdf_query: the BVH8 nearest-box-first with a lane-interleaved LDS stack of
// (box distance^2, child word). What is new here is chosen at compile time:
// which of the winner's values are carried through the walk (the closest
// point and the Voronoi feature only where an output or the sign needs them),
// whether a search radius seeds the walk, and whether the distance is signed
// (the only reader of the pseudonormals). The triangle id is carried always,
// it breaks the ties; whether it is stored is a wave-uniform branch on a
// kernel argument.
//
// A radius r seeds the acceptance bound with r*r and the prune bound with
// prune_bound(r*r), so the first triangle within r is accepted as any later
// improvement is, and a box farther than r (plus the slack) is never pushed: a
// lane whose point is farther than r from every root child is done after one
// node. A lane without a valid radius (negative, NaN) walks nothing.
#include <hip/hip_runtime.h>

#include <atomic>
#include <string>

#include "../../include/rtamd.h"
#include "rt_error.h"
#include "rt_layout.h"
#include "rt_math.h"
#include "rt_points.h"

using namespace rtd;
using namespace rtsdf;

namespace {

// a launch's global size is a 32-bit count of work-items (as for ray batches)
constexpr int64_t kMaxPointBlocks = (int64_t)(0xFFFFFFFFu / (uint32_t)kWave);

enum { kDistNone = 0, kDistUnsigned = 1, kDistSigned = 2 };

// Measurement switch (rtx_set_points_lds_pad): unused LDS bytes added to every
// launch's stack allocation, which lowers the workgroups a CU holds and
// nothing else (tools/points_time.py --lds-pad).
std::atomic<int32_t> g_lds_pad{0};
constexpr int32_t kMaxLds = 64 * 1024;

// Dynamic LDS: cap x 64 floats (box distances) then cap x 64 child words.
template <int DIST, bool CLOSEST, bool FEAT, bool BOUNDED>
__global__ __launch_bounds__(kWave) void points_kernel(SdfDev m, rt_point_batch b, int cap) {
  constexpr bool kKeepQ = CLOSEST || DIST == kDistSigned;
  constexpr bool kKeepFeat = FEAT || DIST == kDistSigned;
  extern __shared__ uint32_t lds[];
  float *st_d = reinterpret_cast<float *>(lds) + threadIdx.x;
  uint32_t *st_w = lds + (size_t)cap * kWave + threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * kWave + threadIdx.x;
  if (i >= b.n) return;
  const f3 p{b.d_point[3 * i], b.d_point[3 * i + 1], b.d_point[3 * i + 2]};
  // best: a triangle is accepted at d2 < best, or at d2 == best below the best
  // id; no id yet = above every id, so the seed r*r itself is within the radius
  float best = kInf;
  bool live = true;
  if (BOUNDED) {
    const float r = b.d_radius ? b.d_radius[i] : b.radius;
    live = r >= 0.0f;
    best = r * r;
  }
  float bound = prune_bound(best);
  uint32_t best_id = 0xFFFFFFFFu;
  int best_feat = -1;
  f3 best_q = p;
  int sp = 0;
  uint32_t word = live ? m.root : rtl::kInvalidChild;
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
          if (kKeepFeat) best_feat = feat;
          if (kKeepQ) best_q = q;
          bound = prune_bound(best);
        }
      }
    } else {
      const rtl::GNode &nd = m.nodes[word];
      float bx[48];
      const float4 *b4 = reinterpret_cast<const float4 *>(nd.box);
#pragma unroll
      for (int j = 0; j < 12; ++j) {
        const float4 v = b4[j];
        bx[4 * j] = v.x; bx[4 * j + 1] = v.y; bx[4 * j + 2] = v.z; bx[4 * j + 3] = v.w;
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
  const bool won = best_id != 0xFFFFFFFFu;
  if (DIST != kDistNone) {
    float d = kInf;
    if (won) {
      d = __builtin_sqrtf(best);
      if (DIST == kDistSigned) {
        const float4 N = m.pn[7u * best_id + (uint32_t)best_feat];
        const f3 e = p - best_q;
        const float s = e.x * N.x + e.y * N.y + e.z * N.z;
        d = s < 0.0f ? -d : d;
      }
    }
    b.d_dist[i] = d;
  }
  if (CLOSEST) {
    // (a point without a winner still holds its own bits in best_q)
    b.d_closest[3 * i] = best_q.x;
    b.d_closest[3 * i + 1] = best_q.y;
    b.d_closest[3 * i + 2] = best_q.z;
  }
  if (b.d_prim) b.d_prim[i] = won ? (int64_t)best_id : -1;
  if (FEAT) b.d_feature[i] = best_feat;
}

template <int DIST, bool CLOSEST, bool FEAT, bool BOUNDED>
void launch_t(const rt_sdf_mesh *m, const rt_point_batch &b, hipStream_t stream) {
  const uint32_t blocks = (uint32_t)((b.n + kWave - 1) / kWave);
  hipLaunchKernelGGL((points_kernel<DIST, CLOSEST, FEAT, BOUNDED>), dim3(blocks), dim3(kWave),
                     lds_bytes(m) + (size_t)g_lds_pad.load(std::memory_order_relaxed), stream, dev_of(m), b,
                     m->stack_cap);
}
template <int DIST, bool CLOSEST, bool FEAT>
void launch_b(const rt_sdf_mesh *m, const rt_point_batch &b, bool bounded, hipStream_t stream) {
  bounded ? launch_t<DIST, CLOSEST, FEAT, true>(m, b, stream) : launch_t<DIST, CLOSEST, FEAT, false>(m, b, stream);
}
template <int DIST, bool CLOSEST>
void launch_f(const rt_sdf_mesh *m, const rt_point_batch &b, bool bounded, hipStream_t stream) {
  b.d_feature ? launch_b<DIST, CLOSEST, true>(m, b, bounded, stream)
              : launch_b<DIST, CLOSEST, false>(m, b, bounded, stream);
}
template <int DIST>
void launch_c(const rt_sdf_mesh *m, const rt_point_batch &b, bool bounded, hipStream_t stream) {
  b.d_closest ? launch_f<DIST, true>(m, b, bounded, stream) : launch_f<DIST, false>(m, b, bounded, stream);
}

}  // namespace

extern "C" {

int rt_sdf_mesh_points_device(rt_sdf_mesh *m, const rt_point_batch *b, uint32_t flags, void *stream) {
  if (!m) return rterr::set(RT_E_INVALID, "SDF mesh is NULL");
  if (!b) return rterr::set(RT_E_INVALID, "point batch is NULL");
  if (flags & ~RT_POINTS_UNSIGNED) return rterr::set(RT_E_INVALID, "unknown point-query flag");
  if (b->n < 0) return rterr::set(RT_E_INVALID, "negative point count");
  if (!b->d_point && b->n > 0) return rterr::set(RT_E_INVALID, "NULL points");
  if (!b->d_dist && !b->d_closest && !b->d_prim && !b->d_feature)
    return rterr::set(RT_E_INVALID, "no output buffer");
  if (!b->d_radius && !(b->radius >= 0.0f))
    return rterr::set(RT_E_INVALID, "the search radius is negative or NaN");
  if (b->n / kWave + (b->n % kWave != 0) > kMaxPointBlocks)
    return rterr::set(RT_E_INVALID, "point count exceeds one launch (" + std::to_string(kMaxPointBlocks * kWave) +
                                        " points): split the batch");
  if (b->n == 0) return RT_OK;
  if (lds_bytes(m) + (size_t)g_lds_pad.load(std::memory_order_relaxed) > 160 * 1024)
    return rterr::set(RT_E_INVALID, "LDS pad beyond the workgroup's 160 KiB");
  const bool bounded = b->d_radius || b->radius < kInf;
  const hipStream_t s = (hipStream_t)stream;
  if (!b->d_dist)
    launch_c<kDistNone>(m, *b, bounded, s);
  else if (flags & RT_POINTS_UNSIGNED)
    launch_c<kDistUnsigned>(m, *b, bounded, s);
  else
    launch_c<kDistSigned>(m, *b, bounded, s);
  HIP_TRY(hipGetLastError());
  return RT_OK;
}

// Test / measurement hook: pad every later launch's LDS allocation by `bytes`
// (0 = none, at most 64 KiB); a launch whose padded allocation would pass the
// workgroup's 160 KiB is refused.
int rtx_set_points_lds_pad(int32_t bytes) {
  if (bytes < 0 || bytes > kMaxLds) return rterr::set(RT_E_INVALID, "LDS pad outside [0, 65536]");
  g_lds_pad.store(bytes, std::memory_order_relaxed);
  return RT_OK;
}

// The LDS bytes of a query launch of this handle without the pad (its stack).
int64_t rtx_sdf_mesh_lds_bytes(const rt_sdf_mesh *m) { return m ? (int64_t)lds_bytes(m) : RT_E_INVALID; }

}  // extern "C"
