// rt_tlas.hip -- instanced scenes with a top-level tree (RT_INSTANCED_TLAS,
// include/rtamd.h): the trace kernel that walks the
// implicit tree of world boxes per lane, the box kernel and the bottom-up
// refit that maintain the tree, and the host entries of the definition
// (rt_instance_world_box, rtx_tlas_candidates). The definition itself is
// rt_tlas.h.
//
// A translation unit of its own, as rt_instances.hip: nothing instantiated
// here moves a block of a kernel that existed before.
//
// Each lane owns a cursor into the heap-ordered tree and walks it without a
// stack (rtt::walk_next / walk_skip), so the only LDS is the mesh stacks. A
// lane's candidates come in index order, the order the definition prescribes.
// A round of the wave loop handles either the lowest candidate of the wave for
// the lanes that hold it (instance record and MeshDev through wave-uniform
// addresses, the wave-level traversal mesh_primary_wave: the flat kernel's
// loop body) or every lane's own candidate (record and MeshDev per lane, the
// per-lane traversal); both give the same bits, the choice is a matter of
// speed (`umin`). All stores are plain vector stores; there is no inline
// assembly here and no device-scope waiting.
#include <hip/hip_runtime.h>

#include <atomic>

#include "rt_dispatch.h"
#include "rt_error.h"
#include "rt_instances.h"
#include "rt_layout.h"
#include "rt_math.h"
#include "rt_scenes.h"
#include "rt_tlas.h"

using namespace rtd;

namespace {

constexpr int kTBlock = 64;  // one wave, as trace_instances_kernel

// A round takes the shared path when at least this many lanes hold the wave's
// lowest candidate (1: always, 65: never). Chosen by tools/tlas_time.py
// (profiles/r18/README.md); rtx_set_tlas_uniform_min overrides it.
constexpr int kUniformMinDefault = 16;
std::atomic<int> g_umin{kUniformMinDefault};
// diagnostic: BLAS traversals per ray of the next traces (rtx_set_tlas_count)
std::atomic<uint32_t *> g_count{nullptr};

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

template <int SLOTS, int MODE>
__global__ __launch_bounds__(kTBlock) void trace_tlas_kernel(const rti::InstRec *__restrict__ inst,
                                                             const MeshDev *__restrict__ tab,
                                                             const rtt::TNode *__restrict__ nodes, uint32_t P,
                                                             int32_t umin, uint32_t *count, PlaneDev pl,
                                                             rt_ray_batch b) {
  __shared__ uint32_t stk[SLOTS * MeshS::kFields * kTBlock];
  const int64_t i = (int64_t)blockIdx.x * kTBlock + threadIdx.x;
  // a partial last wave keeps its lanes without a ray (the wave-level steps
  // need the whole wave): their cursor starts at 0 and they touch no memory
  const bool active = i < b.n;
  LdsStack<kTBlock, MeshS::kFields> st{stk + threadIdx.x};
  f3 o{0.0f, 0.0f, 0.0f}, d{0.0f, 0.0f, 1.0f};
  float tn = b.tnear, tf = b.tfar;
  if (active) {
    o = f3{b.d_origin[3 * i], b.d_origin[3 * i + 1], b.d_origin[3 * i + 2]};
    d = f3{b.d_dir[3 * i], b.d_dir[3 * i + 1], b.d_dir[3 * i + 2]};
    if (b.d_tnear) tn = b.d_tnear[i];
    if (b.d_tfar) tf = b.d_tfar[i];
  }
  const f3 inv{1.0f / d.x, 1.0f / d.y, 1.0f / d.z};  // of the WORLD ray: the tree's test
  NoCnt cnt;
  constexpr bool kAny = MODE == kRaysAny;
  // mesh_primary_wave takes one tNear for the wave (tFar is per ray): a batch
  // with a d_tnear array has no wave-level traversal to share an instance
  // for, and takes the per-lane path in every round
  const bool can_share = kAny || !b.d_tnear;
  uint32_t n = active ? 1u : 0u;  // the cursor; 0: the walk is over
  bool have = false;              // n rests on a leaf that passed and is not handled yet
  uint32_t ntrav = 0;
  float best = kInf;
  int32_t wi = -1;  // winning instance
  uint32_t wk = 0;  // its triangle slot
  bool occ = false;
  for (;;) {
    // closest hit: tf_i = best < tFar ? best : tFar; any hit: the full tFar
    const float tfi = kAny ? tf : (best < tf ? best : tf);
    if (!have) {
      n = lane_next(nodes, P, n, o, inv, tn, tfi);
      have = n != 0u;
    }
    if (__ballot(have) == 0) break;
    const uint32_t cand = have ? n - P : 0xFFFFFFFFu;
    const uint32_t low = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave_min(cand));
    const bool mine = have && cand == low;
    const bool share = can_share && (int)__popcll(__ballot(mine)) >= umin;
    bool handled;
    if (share) {
      // the flat kernel's loop body on instance `low` for the lanes that hold it
      handled = mine;
      const rti::InstRec r = inst[low];
      const MeshDev md = tab[r.blas];
      if (!((r.flags & RT_INSTANCE_DISABLED) || r.skipped || md.root == rtl::kInvalidChild)) {
        const f3 oo = xf_point(r.m, o), dd = xf_dir(r.m, d);
        const bool go = mine && root_passes(md, oo, dd, tn, tfi);
        if constexpr (kAny) {
          if (go && mesh_occluded<kTBlock>(md, oo, dd, tn, tfi, st, cnt)) occ = true;
        } else {
          if (__ballot(go) != 0) {
            float t = kInf;
            uint32_t tri = 0;
            const bool h = mesh_primary_wave<kTBlock, MeshS::kFields>(md, oo, dd, tn, tfi, go, stk, t, tri) && go;
            if (h && t < best) {  // ties keep the lower index
              best = t;
              wi = (int32_t)low;
              wk = tri;
            }
          }
        }
      }
    } else {
      // every lane's own candidate: its record and its MeshDev per lane. (Not
      // through mesh_primary_wave: its shared node fetch assumes one mesh.)
      handled = have;
      if (have) {
        const rti::InstRec *rp = inst + cand;
        const uint32_t off = (rp->flags & RT_INSTANCE_DISABLED) | rp->skipped;
        const MeshDev md = load_md(tab + rp->blas);
        if (!off && md.root != rtl::kInvalidChild) {
          float m[12];
          load_m(rp, m);
          const f3 oo = xf_point(m, o), dd = xf_dir(m, d);
          if constexpr (kAny) {
            if (mesh_occluded<kTBlock>(md, oo, dd, tn, tfi, st, cnt)) occ = true;
          } else {
            float t = kInf;
            uint32_t tri = 0;
            if (mesh_trace<kTBlock, false>(md, oo, dd, tn, tfi, st, t, tri, cnt) && t < best) {
              best = t;
              wi = (int32_t)cand;
              wk = tri;
            }
          }
        }
      }
    }
    if (handled) {
      ++ntrav;
      // any hit: a lane that has its hit is done
      n = (kAny && occ) ? 0u : rtt::walk_skip(n);
      have = false;
    }
  }
  if (!active) return;
  if (count) count[i] = ntrav;
  if constexpr (kAny) {
    if (!occ && pl.on) {  // HitInfo::hitten of the union: the OR of both
      float tp, ap;
      occ = plane_hit(pl, o, d, tn, tf, tp, ap);
    }
    b.d_hit[i] = occ ? 1 : 0;
  } else {
    Hit h = miss_hit();
    if (wi >= 0) {
      // the winner's record and triangle, per lane (lanes differ in wi)
      const float *m = inst[wi].m;
      const rtl::GTri *tris = tab[inst[wi].blas].tris;
      h.hit = true;
      h.t = best;
      if constexpr (MODE == kRaysNormal) {
        const f3 nn = tri_normal(tris, wk);  // object space
        // the inverse transpose of the object-to-world map: M^T n
        h.n = normalize(f3{(m[0] * nn.x + m[4] * nn.y) + m[8] * nn.z, (m[1] * nn.x + m[5] * nn.y) + m[9] * nn.z,
                           (m[2] * nn.x + m[6] * nn.y) + m[10] * nn.z});
      }
      if (b.d_prim) h.prim = (int64_t)(((uint64_t)(uint32_t)wi << 32) | (uint64_t)tris[wk].orig_id);
    }
    if (pl.on) {  // SceneUnion::intersect, as trace_rays_kernel
      float tp = kInf, ap = 1.0f;
      const bool ph = plane_hit(pl, o, d, tn, tf, tp, ap);
      if (!(h.t < (ph ? tp : kInf))) h = ph ? Hit{true, tp, pl.n, -2} : miss_hit();
    }
    if (b.d_hit) b.d_hit[i] = h.hit ? 1 : 0;
    if (b.d_t) b.d_t[i] = h.t;
    if constexpr (MODE == kRaysNormal) {
      b.d_normal[3 * i] = h.n.x;
      b.d_normal[3 * i + 1] = h.n.y;
      b.d_normal[3 * i + 2] = h.n.z;
    }
    if (b.d_prim) b.d_prim[i] = h.hit ? h.prim : -1;
  }
}

// Leaves first .. first + count - 1 (< P), one per lane. A leaf of an instance
// (index < ninst): with xsrc, its object-to-world matrix is first taken over
// from xsrc[12 j ..] into the scene's own array; then the box is world_box of
// the matrix and the BLAS's root box as the table holds it, the unbounded box
// for a leaf-root BLAS, the empty box for a disabled or skipped instance or an
// empty BLAS. only_blas >= 0: the instances of other BLAS are left alone. A
// leaf past the instances is the empty box.
__global__ __launch_bounds__(64) void tlas_box_kernel(rtt::TNode *nodes, uint32_t P, int32_t ninst,
                                                      const rti::InstRec *__restrict__ inst, float *xform,
                                                      const MeshDev *__restrict__ tab, int32_t first, int32_t count,
                                                      const float *__restrict__ xsrc, int32_t only_blas) {
  const int32_t j = (int32_t)(blockIdx.x * 64u + threadIdx.x);
  if (j >= count) return;
  const int32_t i = first + j;
  if ((uint32_t)i >= P) return;
  float wb[6];
  rtt::empty_box(wb);
  if (i < ninst) {
    float x[12];
    const float *src = xsrc ? xsrc + 12 * (int64_t)j : xform + 12 * (int64_t)i;
#pragma unroll
    for (int k = 0; k < 12; ++k) x[k] = src[k];
    if (xsrc) {
#pragma unroll
      for (int k = 0; k < 12; ++k) xform[12 * (int64_t)i + k] = x[k];
    }
    const rti::InstRec *r = inst + i;
    if (only_blas >= 0 && r->blas != only_blas) return;
    if (!((r->flags & RT_INSTANCE_DISABLED) || r->skipped)) {
      const MeshDev *e = tab + r->blas;
      const uint32_t root = e->root;
      if (root != rtl::kInvalidChild) {
        if (root & rtl::kLeafBit) {
          rtt::unbounded_box(wb);
        } else {
          float ob[6];
#pragma unroll
          for (int k = 0; k < 6; ++k) ob[k] = e->rbox[k];
          rtt::world_box(x, ob, wb);
        }
      }
    }
  }
  float4 *q = reinterpret_cast<float4 *>(nodes + P + (uint32_t)i);
  q[0] = make_float4(wb[0], wb[1], wb[2], wb[3]);
  q[1] = make_float4(wb[4], wb[5], 0.0f, 0.0f);
}

__device__ __forceinline__ void refit_node(rtt::TNode *nodes, uint32_t n) {
  const float4 *l = reinterpret_cast<const float4 *>(nodes + 2u * n);
  const float4 *r = reinterpret_cast<const float4 *>(nodes + 2u * n + 1u);
  const float4 a0 = l[0], a1 = l[1], c0 = r[0], c1 = r[1];
  const float a[6] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y}, c[6] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y};
  float u[6];
  rtt::box_union(a, c, u);
  float4 *q = reinterpret_cast<float4 *>(nodes + n);
  q[0] = make_float4(u[0], u[1], u[2], u[3]);
  q[1] = make_float4(u[4], u[5], 0.0f, 0.0f);
}

// one level of `w` inner nodes (w .. 2w - 1), one node per lane: the levels
// too wide for one workgroup, one launch each
__global__ __launch_bounds__(256) void tlas_level_kernel(rtt::TNode *nodes, uint32_t w) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t < w) refit_node(nodes, w + t);
}

// the levels of width w, w / 2, .. 1 by ONE workgroup, a barrier between two
// levels (a workgroup's stores are visible to it behind __syncthreads)
constexpr uint32_t kRefitBlock = 256;
constexpr uint32_t kRefitTopWidth = 1024;
__global__ __launch_bounds__(kRefitBlock) void tlas_top_kernel(rtt::TNode *nodes, uint32_t w) {
  for (; w >= 1u; w >>= 1) {
    for (uint32_t t = threadIdx.x; t < w; t += kRefitBlock) refit_node(nodes, w + t);
    __syncthreads();
  }
}

template <int SLOTS>
void launch_t(const rti::InstArgs &a, const PlaneDev &pl, const rt_ray_batch &b, int mode, hipStream_t st) {
  const unsigned blocks = (unsigned)((b.n + kTBlock - 1) / kTBlock);
  const int32_t umin = g_umin.load();
  uint32_t *count = g_count.load();
  const uint32_t P = (uint32_t)a.tlas_leaves;
  switch (mode) {
    case kRaysAny:
      trace_tlas_kernel<SLOTS, kRaysAny><<<blocks, kTBlock, 0, st>>>(a.inst, a.blas, a.tlas, P, umin, count, pl, b);
      break;
    case kRaysClosest:
      trace_tlas_kernel<SLOTS, kRaysClosest><<<blocks, kTBlock, 0, st>>>(a.inst, a.blas, a.tlas, P, umin, count, pl, b);
      break;
    default:
      trace_tlas_kernel<SLOTS, kRaysNormal><<<blocks, kTBlock, 0, st>>>(a.inst, a.blas, a.tlas, P, umin, count, pl, b);
      break;
  }
}

}  // namespace

namespace rti {

int trace_tlas_launch(const InstArgs &a, const PlaneDev &pl, const rt_ray_batch &b, int mode, hipStream_t st) {
  with_slots(a.maxd, [&](auto slots) { launch_t<decltype(slots)::value>(a, pl, b, mode, st); });
  HIP_TRY(hipGetLastError());
  return RT_OK;
}

int tlas_boxes_launch(const TlasArgs &t, int32_t first, int32_t count, const float *d_xsrc, int32_t only_blas,
                      hipStream_t st) {
  if (count <= 0) return RT_OK;
  tlas_box_kernel<<<(unsigned)((count + 63) / 64), 64, 0, st>>>(t.nodes, (uint32_t)t.leaves, t.ninst, t.inst, t.xform,
                                                              t.blas, first, count, d_xsrc, only_blas);
  HIP_TRY(hipGetLastError());
  return RT_OK;
}

int tlas_refit_launch(const TlasArgs &t, hipStream_t st) {
  uint32_t w = (uint32_t)t.leaves / 2u;
  for (; w > kRefitTopWidth; w >>= 1) tlas_level_kernel<<<(w + 255u) / 256u, 256, 0, st>>>(t.nodes, w);
  if (w >= 1u) tlas_top_kernel<<<1, kRefitBlock, 0, st>>>(t.nodes, w);
  HIP_TRY(hipGetLastError());
  return RT_OK;
}

}  // namespace rti

extern "C" {

int rt_instance_world_box(const float xform[12], const float obox[6], float wbox[6]) {
  if (!xform || !obox || !wbox) return set_err(RT_E_INVALID, "rt_instance_world_box: NULL argument");
  float w[6];
  rtt::world_box(xform, obox, w);
  for (int k = 0; k < 6; ++k) wbox[k] = w[k];
  return RT_OK;
}

// Diagnostic (not part of include/rtamd.h): the shared path's threshold of the
// traces launched from now on, 1 (always) .. 65 (never); any other value
// restores the shipped default.
int rtx_set_tlas_uniform_min(int lanes) {
  g_umin.store((lanes >= 1 && lanes <= 65) ? lanes : kUniformMinDefault);
  return RT_OK;
}

// Diagnostic: the traces of top-level-tree scenes launched from now on store
// each ray's number of BLAS traversals into d_count[ray] (uint32, at least as
// many as the largest batch; NULL turns it off).
int rtx_set_tlas_count(void *d_count) {
  g_count.store((uint32_t *)d_count);
  return RT_OK;
}

// Diagnostic, host only: rtt::box_pass on host values (1: passes).
int rtx_tlas_box_pass(const float box[6], const float o[3], const float d[3], float tn, float tf) {
  if (!box || !o || !d) return set_err(RT_E_INVALID, "rtx_tlas_box_pass: NULL argument");
  return rtt::box_pass(box, o, d, tn, tf) ? 1 : 0;
}

// Diagnostic, host only: the tree over leaf boxes leaf6[6 K] as the device
// builds it, nodes8[8 * 2P] (32-byte records, node 0 and the pad words zero).
int rtx_tlas_build_host(const float *leaf6, int32_t k, float *nodes8) {
  if (!leaf6 || !nodes8 || k < 1) return set_err(RT_E_INVALID, "rtx_tlas_build_host: bad argument");
  const int32_t P = rtt::leaf_count(k);
  rtt::TNode *nd = reinterpret_cast<rtt::TNode *>(nodes8);
  for (int32_t n = 0; n < 2 * P; ++n) nd[n] = rtt::TNode{{0, 0, 0, 0, 0, 0}, {0, 0}};
  for (int32_t i = 0; i < P; ++i) {
    if (i < k)
      for (int c = 0; c < 6; ++c) nd[P + i].b[c] = leaf6[6 * (size_t)i + c];
    else
      rtt::empty_box(nd[P + i].b);
  }
  for (int32_t n = P - 1; n >= 1; --n) rtt::box_union(nd[2 * n].b, nd[2 * n + 1].b, nd[n].b);
  return RT_OK;
}

// Diagnostic, host only: the kernel's cursor walk for one ray on a host copy of
// the tree (rtt::candidates_host): the candidates in the order met, the c-th
// searched under tf_seq[min(c, ntf - 1)]. Returns their number (at most cap
// are written), or a negative error.
int rtx_tlas_candidates(const float *nodes8, int32_t leaves, const float o[3], const float d[3], float tn,
                        const float *tf_seq, int32_t ntf, int32_t *out, int32_t cap) {
  if (!nodes8 || !o || !d || !tf_seq || ntf < 1 || (cap > 0 && !out) || leaves < 1 || (leaves & (leaves - 1)))
    return set_err(RT_E_INVALID, "rtx_tlas_candidates: bad argument");
  return rtt::candidates_host(reinterpret_cast<const rtt::TNode *>(nodes8), leaves, o, d, tn, tf_seq, ntf, out,
                              cap < 0 ? 0 : cap);
}

}  // extern "C"
