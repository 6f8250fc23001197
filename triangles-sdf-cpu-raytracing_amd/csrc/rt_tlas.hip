// rt_tlas.hip -- instanced scenes with a top-level tree (RT_INSTANCED_TLAS,
// include/rtamd.h): the trace kernel that walks the
// implicit tree of world boxes per lane, the box kernel and the bottom-up
// refit that maintain the tree, and the host entries of the definition
// (rt_instance_world_box, rtx_tlas_candidates). The definition itself is
// rt_tlas.h.
//
// A translation unit of its own, as rt_instances.hip, whose shared pieces
// (rt_instance_dev.h, rt_ray_io.h, rt_dispatch.h) it uses as well.
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
#include "rt_instance_dev.h"
#include "rt_ray_io.h"

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
  const RayIn ray = load_ray(b, i, active);
  const f3 o = ray.o, d = ray.d;
  const float tn = ray.tn, tf = ray.tf;
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
  if constexpr (kAny)
    store_any(b, i, pl, ray, occ);
  else
    store_closest<MODE>(b, i, pl, ray, mesh_winner_hit<MODE == kRaysNormal>(inst, tab, best, wi, wk, b.d_prim));
}

// The object box of one table entry: what kind it is and, for kBoxObject, the
// box itself. A mesh: its root box as the table holds it, unbounded for a
// leaf root (no root box to test), empty for an empty mesh. A grid or an
// octree of the mixed table: the cube (-1,-1,-1, 1,1,1).
enum { kBoxEmpty = 0, kBoxUnbounded = 1, kBoxObject = 2 };
__device__ __forceinline__ int object_box(const MeshDev *e, float ob[6]) {
  const uint32_t root = e->root;
  if (root == rtl::kInvalidChild) return kBoxEmpty;
  if (root & rtl::kLeafBit) return kBoxUnbounded;
#pragma unroll
  for (int k = 0; k < 6; ++k) ob[k] = e->rbox[k];
  return kBoxObject;
}
__device__ __forceinline__ int object_box(const rti::BlasRec *e, float ob[6]) {
  ob[0] = ob[1] = ob[2] = -1.0f;
  ob[3] = ob[4] = ob[5] = 1.0f;
  return e->kind == (uint32_t)RT_SCENE_MESH ? object_box(&e->mesh, ob) : kBoxObject;
}

// Leaves first .. first + count - 1 (< P), one per lane, over a table of
// MeshDev or of BlasRec. A leaf of an instance (index < ninst): with xsrc, its
// object-to-world matrix is first taken over from xsrc[12 j ..] into the
// scene's own array; then the box is world_box of the matrix and object_box
// of the instance's table entry (the unbounded box for an unbounded one), the
// empty box for a disabled or skipped instance or an empty entry.
// only_blas >= 0: the instances of other BLAS are left alone. A leaf past the
// instances is the empty box.
template <class Rec>
__global__ __launch_bounds__(64) void tlas_box_kernel(rtt::TNode *nodes, uint32_t P, int32_t ninst,
                                                      const rti::InstRec *__restrict__ inst, float *xform,
                                                      const Rec *__restrict__ tab, int32_t first, int32_t count,
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
      float ob[6];
      const int kind = object_box(tab + r->blas, ob);
      if (kind == kBoxUnbounded)
        rtt::unbounded_box(wb);
      else if (kind == kBoxObject)
        rtt::world_box(x, ob, wb);
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
  with_mode(mode, [&](auto m) {
    trace_tlas_kernel<SLOTS, decltype(m)::value><<<blocks, kTBlock, 0, st>>>(a.inst, a.blas, a.tlas, P, umin, count, pl, b);
  });
}

template <class Rec>
int boxes_launch(const rti::TlasArgs &t, const Rec *tab, int32_t first, int32_t count, const float *d_xsrc,
                 int32_t only_blas, hipStream_t st) {
  if (count <= 0) return RT_OK;
  tlas_box_kernel<Rec><<<(unsigned)((count + 63) / 64), 64, 0, st>>>(t.nodes, (uint32_t)t.leaves, t.ninst, t.inst,
                                                                   t.xform, tab, first, count, d_xsrc, only_blas);
  HIP_TRY(hipGetLastError());
  return RT_OK;
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
  return boxes_launch(t, t.blas, first, count, d_xsrc, only_blas, st);
}

int mixed_boxes_launch(const TlasArgs &t, const BlasRec *tab, int32_t first, int32_t count, const float *d_xsrc,
                       int32_t only_blas, hipStream_t st) {
  return boxes_launch(t, tab, first, count, d_xsrc, only_blas, st);
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
