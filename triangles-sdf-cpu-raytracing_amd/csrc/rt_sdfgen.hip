// rt_sdfgen.hip -- mesh -> signed distance construction on the GPU (SURVEY.md
// 8(f) rank 1): the deterministic generator of the large grid / octree
// stand-ins for BASELINE configs 3 and 4 (example_grid_large.grid and
// example_octree_large.octree are not in the reference, .MISSING_LARGE_BLOBS).
//
// One thread per query point. A closest-point query walks the renderer's own
// BVH8 (rt_layout.h GNode) nearest-box-first with a lane-interleaved LDS
// stack of (box distance^2, child word), pruning boxes farther than the best
// distance plus an absolute slack of 1e-5 (>> the f32 rounding of points in
// [-1,1]^3), so the result equals the brute-force minimum over all triangles
// bit for bit, ties included (lexicographic (d^2, triangle id)). The closest
// point and its region follow Ericson (RTCD 5.1.5) op for op; the sign comes
// from the host-computed pseudonormal of the closest feature (rt_meshops.cpp).
// Lattice queries map a 4x4x4 brick of samples to each 64-lane wave.
// The handle and the pieces of the walk that the point queries on device
// buffers share (rt_points.hip) are in rt_points.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rtamd.h"
#include "rt_error.h"
#include "rt_host.h"
#include "rt_layout.h"
#include "rt_math.h"
#include "rt_points.h"
#include "rt_sdf_refit.h"

using namespace rtd;
using namespace rtsdf;

namespace {

thread_local std::string g_stale_seen;  // the last stale error a query found (rtx_sdf_last_stale)

// Signed distance at p. st_d / st_w: this lane's LDS stack columns (stride 64).
__device__ float sdf_query(const SdfDev &m, f3 p, float *st_d, uint32_t *st_w) {
  float best = kInf, bound = kInf;
  uint32_t best_id = 0xFFFFFFFFu;
  int best_feat = 0;
  f3 best_q{0.0f, 0.0f, 0.0f};
  int sp = 0;
  uint32_t word = m.root;
  while (true) {
    if (word != rtl::kInvalidChild) {
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
        // push farthest first so the nearest is popped next
#pragma unroll
        for (int c = 7; c >= 0; --c) {
          if (id[c] != rtl::kInvalidChild && t[c] <= bound) {
            st_d[sp * kWave] = t[c];
            st_w[sp * kWave] = id[c];
            ++sp;
          }
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
    if (word == rtl::kInvalidChild) break;
  }
  if (best_id == 0xFFFFFFFFu) return kInf;
  const float4 N = m.pn[7u * best_id + (uint32_t)best_feat];
  const f3 e = p - best_q;
  const float s = e.x * N.x + e.y * N.y + e.z * N.z;
  const float d = __builtin_sqrtf(best);
  return s < 0.0f ? -d : d;
}

// LATTICE: sample (i,j,k) of an n0 x n1 x n2 lattice over [-1,1]^3,
// p = 2*i/(n-1) - 1 per axis (the inverse of SDFGrid::sdf's
// q = (p+1)/2*(size-1), grid_raytracing.cpp:7-62), out[(i*n1+j)*n2+k].
// Dynamic LDS: cap x 64 floats (box distances) then cap x 64 child words.
template <bool LATTICE>
__global__ __launch_bounds__(kWave) void sdf_kernel(SdfDev m, const float *p3, int64_t n, uint32_t n0,
                                                   uint32_t n1, uint32_t n2, int cap, float *out) {
  extern __shared__ uint32_t lds[];
  float *st_d = reinterpret_cast<float *>(lds) + threadIdx.x;
  uint32_t *st_w = lds + (size_t)cap * kWave + threadIdx.x;
  f3 p;
  int64_t o;
  if (LATTICE) {
    const uint32_t by = (n1 + 3) / 4, bz = (n2 + 3) / 4;
    const uint64_t b = blockIdx.x;
    const uint32_t ib = (uint32_t)(b / ((uint64_t)by * bz));
    const uint32_t rem = (uint32_t)(b % ((uint64_t)by * bz));
    const uint32_t jb = rem / bz, kb = rem % bz;
    const uint32_t i = ib * 4 + (threadIdx.x >> 4), j = jb * 4 + ((threadIdx.x >> 2) & 3),
                   k = kb * 4 + (threadIdx.x & 3);
    if (i >= n0 || j >= n1 || k >= n2) return;
    p = f3{2.0f * (float)i / (float)(n0 - 1) - 1.0f, 2.0f * (float)j / (float)(n1 - 1) - 1.0f,
           2.0f * (float)k / (float)(n2 - 1) - 1.0f};
    o = ((int64_t)i * n1 + j) * n2 + k;
  } else {
    o = (int64_t)blockIdx.x * kWave + threadIdx.x;
    if (o >= n) return;
    p = f3{p3[3 * o], p3[3 * o + 1], p3[3 * o + 2]};
  }
  out[o] = sdf_query(m, p, st_d, st_w);
}

// What an RT_MESH_DYNAMIC handle adds (rt_points.h): the creation topology,
// the vertex staging buffer, scratch, and the event of the updates.
int upload_dynamic(rt_sdf_mesh *m, const rth::SdfTopo &t, const uint32_t *idx, int64_t nidx) {
  const size_t ntri = (size_t)m->ntri, nv = (size_t)m->nverts;
  m->n_wverts = t.n_wverts;
  m->n_wedges = t.n_wedges;
  m->level_first = rth::bvh_level_first(m->host.bvh.nodes);
  if (int rc = m->d_idx.upload(idx, (size_t)nidx)) return rc;
  if (int rc = m->d_weld.upload(t.weld.data(), t.weld.size())) return rc;
  if (int rc = m->d_tri_edge.upload(t.tri_edge.data(), t.tri_edge.size())) return rc;
  if (int rc = m->d_v_off.upload(t.v_off.data(), t.v_off.size())) return rc;
  if (int rc = m->d_v_inc.upload(t.v_inc.data(), t.v_inc.size())) return rc;
  if (int rc = m->d_e_off.upload(t.e_off.data(), t.e_off.size())) return rc;
  if (int rc = m->d_e_inc.upload(t.e_inc.data(), t.e_inc.size())) return rc;
  if (int rc = m->d_vstage.alloc(std::max<size_t>(nv, 1))) return rc;
  if (int rc = m->d_fn.alloc(ntri)) return rc;
  if (int rc = m->d_ang.alloc(3 * ntri)) return rc;
  if (int rc = m->d_vn.alloc(t.n_wverts)) return rc;
  if (int rc = m->d_en.alloc(t.n_wedges)) return rc;
  if (int rc = m->updated.create(hipEventDisableTiming)) return rc;
  m->dev_bytes += (int64_t)(4 * (size_t)nidx + 16 * nv + 4 * nv + 12 * ntri + 4 * ((size_t)t.n_wverts + 1) + 12 * ntri +
                            4 * ((size_t)t.n_wedges + 1) + 12 * ntri + 16 * ntri + 24 * ntri +
                            16 * (size_t)t.n_wverts + 16 * (size_t)t.n_wedges);
  // after an update only the device arrays are current: no stale host copy is kept
  std::vector<float>().swap(m->host.tri);
  std::vector<float>().swap(m->host.pn);
  return RT_OK;
}

int check_update(const rt_sdf_mesh *m, const float *vpos4, int64_t nverts, const char *who) {
  if (!m) return rterr::set(RT_E_INVALID, std::string(who) + ": handle is NULL");
  if (!m->dynamic) return rterr::set(RT_E_STATE, std::string(who) + ": the handle was not created with RT_MESH_DYNAMIC");
  if (!vpos4) return rterr::set(RT_E_INVALID, std::string(who) + ": vertex pointer is NULL");
  if (nverts != m->nverts)
    return rterr::set(RT_E_INVALID, std::string(who) + ": nverts " + std::to_string(nverts) + ", created with " +
                                        std::to_string(m->nverts));
  return RT_OK;
}

// Queues one refit on `st` and records the handle's event behind it. Only launches.
int update_device(rt_sdf_mesh *m, const float *d_vpos4, hipStream_t st) {
  SdfRefitArgs a{};
  a.nodes = m->d_nodes.p;
  a.tri = m->d_tri.p;
  a.pn = m->d_pn.p;
  a.root = m->root;
  a.vpos4 = d_vpos4;
  a.idx = m->d_idx.p;
  a.weld = m->d_weld.p;
  a.tri_edge = m->d_tri_edge.p;
  a.v_off = m->d_v_off.p;
  a.v_inc = m->d_v_inc.p;
  a.e_off = m->d_e_off.p;
  a.e_inc = m->d_e_inc.p;
  a.fn = m->d_fn.p;
  a.ang = m->d_ang.p;
  a.vn = m->d_vn.p;
  a.en = m->d_en.p;
  a.ntri = (uint32_t)m->ntri;
  a.n_wverts = m->n_wverts;
  a.n_wedges = m->n_wedges;
  a.level_first = m->level_first.data();
  a.levels = m->level_first.empty() ? 0 : (int32_t)m->level_first.size() - 1;
  m->oct_depth = -1;  // the octree cache is of the mesh before
  std::vector<uint8_t>().swap(m->oct_nodes);
  const int rc = sdf_refit_launch(a, st);
  HIP_TRY(hipEventRecord(m->updated.e, st));  // (also behind a partly queued refit)
  return rc;
}

// The handle's own host entries read behind the last update (its event).
int wait_updated(const rt_sdf_mesh *m, hipStream_t st) {
  if (m->updated.e) HIP_TRY(hipStreamWaitEvent(st, m->updated.e, 0));
  return RT_OK;
}

// The size checks of a lattice query, and its launch's workgroups: one 4x4x4
// brick of samples per wave.
int grid_blocks(const uint32_t size[3], uint32_t &blocks) {
  for (int a = 0; a < 3; ++a)
    if (size[a] < 2 || size[a] > 4096) return rterr::set(RT_E_INVALID, "grid size must be in [2, 4096]");
  const uint64_t b = (uint64_t)((size[0] + 3) / 4) * ((size[1] + 3) / 4) * ((size[2] + 3) / 4);
  if (b > 0x7FFFFFFFull) return rterr::set(RT_E_INVALID, "grid too large");
  blocks = (uint32_t)b;
  return RT_OK;
}

// Points per staged batch of a host query (16 MiB of pinned staging at most).
constexpr int64_t kQueryBatch = 1 << 20;

// The handle's query stream and staging for batches of up to `n` points.
int query_staging(rt_sdf_mesh *m, int64_t n) {
  if (int rc = m->qs.create(m->device, "SDF query stream")) return rc;
  rterr::stream_mark(m->qs.s, "rt_sdf_mesh_points");
  const int64_t want = std::min(n, kQueryBatch);
  if (want <= m->q_cap) return RT_OK;
  HIP_TRY(hipStreamSynchronize(m->qs.s));
  m->q_cap = 0;
  const int64_t cap = std::max<int64_t>(want, 4096);
  if (int rc = m->h_stage.alloc((size_t)cap * 4, hipHostMallocDefault)) return rc;
  if (int rc = m->d_p3.alloc((size_t)cap * 3)) return rc;
  if (int rc = m->d_out.alloc((size_t)cap)) return rc;
  m->q_cap = cap;
  return RT_OK;
}

// Signed distances of n host points. Every copy goes between the handle's
// pinned staging and device buffers on its own stream, so no pageable
// transfer (HIP's internal staging or on-the-fly pinning of caller memory)
// is on this path; each step reports its own failure, and an error that was
// already pending before the first copy is reported as such
// (rterr::take_stale) -- round 4 saw one "hipMemcpy H2D failed" here that
// carried no HIP error string.
int query_host(rt_sdf_mesh *m, const float *p3, int64_t n, float *out) {
  if (n <= 0) return RT_OK;
  const std::string stale = rterr::take_stale();  // before any call of ours can overwrite it
  g_stale_seen = stale;
  HIP_TRY(hipSetDevice(m->device));
  if (const hipError_t e = hipStreamQuery(m->qs.s ? m->qs.s : nullptr); e != hipSuccess && e != hipErrorNotReady)
    return rterr::set(RT_E_DEVICE, std::string("device already in error before the SDF query: ") +
                                       hipGetErrorString(e) + (stale.empty() ? "" : "; " + stale));
  int rc = query_staging(m, n);
  if (rc != RT_OK) return rc;
  if ((rc = wait_updated(m, m->qs.s)) != RT_OK) return rc;
  for (int64_t i0 = 0; i0 < n; i0 += m->q_cap) {
    const int64_t k = std::min(m->q_cap, n - i0);
    std::memcpy(m->h_stage.h, p3 + 3 * i0, (size_t)k * 12);
    hipError_t e = hipMemcpyAsync(m->d_p3.p, m->h_stage.h, (size_t)k * 12, hipMemcpyHostToDevice, m->qs.s);
    const char *step = "hipMemcpyAsync H2D of the points";
    if (e == hipSuccess) {
      hipLaunchKernelGGL(sdf_kernel<false>, dim3((uint32_t)((k + kWave - 1) / kWave)), dim3(kWave), lds_bytes(m),
                         m->qs.s, dev_of(m), m->d_p3.p, k, 0u, 0u, 0u, m->stack_cap, m->d_out.p);
      e = hipGetLastError();
      step = "sdf_kernel launch";
    }
    float *h_out = m->h_stage.h + 3 * m->q_cap;
    if (e == hipSuccess) {
      e = hipMemcpyAsync(h_out, m->d_out.p, (size_t)k * 4, hipMemcpyDeviceToHost, m->qs.s);
      step = "hipMemcpyAsync D2H of the distances";
    }
    if (e == hipSuccess) {
      e = hipStreamSynchronize(m->qs.s);
      step = "hipStreamSynchronize after the query";
    }
    if (e != hipSuccess) {
      HIP_NOTE(hipStreamSynchronize(m->qs.s));
      return rterr::set(RT_E_DEVICE, std::string("SDF query of ") + std::to_string(k) + " points: " + step +
                                         ": " + hipGetErrorString(e) + (stale.empty() ? "" : "; " + stale));
    }
    std::memcpy(out + i0, h_out, (size_t)k * 4);
  }
  return RT_OK;
}

bool octree_query(void *ctx, const float *p3, int64_t n, float *out, std::string &err) {
  if (query_host(static_cast<rt_sdf_mesh *>(ctx), p3, n, out) != RT_OK) {
    err = rterr::get();
    return false;
  }
  return true;
}

}  // namespace

extern "C" {

int rt_sdf_mesh_create(const float *vpos4, int64_t nverts, const uint32_t *idx, int64_t nidx,
                       rt_sdf_mesh **out) {
  return rt_sdf_mesh_create_ex(vpos4, nverts, idx, nidx, 0u, out);
}

int rt_sdf_mesh_create_ex(const float *vpos4, int64_t nverts, const uint32_t *idx, int64_t nidx, uint32_t flags,
                          rt_sdf_mesh **out) {
  if (!out || (!vpos4 && nverts) || (!idx && nidx) || nverts < 0 || nidx < 0)
    return rterr::set(RT_E_INVALID, "bad mesh arguments");
  *out = nullptr;
  if (flags & ~RT_MESH_DYNAMIC) return rterr::set(RT_E_INVALID, "rt_sdf_mesh_create_ex: unknown flag bits");
  rt_sdf_mesh *m = new rt_sdf_mesh();
  m->dynamic = (flags & RT_MESH_DYNAMIC) != 0;
  std::string err;
  rth::SdfTopo topo;
  if (!rth::prep_sdf_mesh(vpos4, nverts, idx, nidx, m->host, err, m->dynamic ? &topo : nullptr)) {
    delete m;
    return rterr::set(RT_E_INVALID, err);
  }
  m->nverts = nverts;
  m->ntri = nidx / 3;
  const rth::BVHGpu &b = m->host.bvh;
  m->root = b.root_word;
  m->stack_cap = 7 * std::max(b.max_depth, 1) + 1;
  if ((size_t)m->stack_cap * kWave * 8 > 160 * 1024) {
    delete m;
    return rterr::set(RT_E_INVALID, "BVH too deep for the SDF query stack");
  }
  int rc = hipGetDevice(&m->device) == hipSuccess ? RT_OK : rterr::set(RT_E_DEVICE, "no HIP device");
  if (rc == RT_OK) rc = m->d_nodes.upload(b.nodes.data(), b.nodes.size());
  if (rc == RT_OK) rc = m->d_tri.upload(reinterpret_cast<const float4 *>(m->host.tri.data()), m->host.tri.size() / 4);
  if (rc == RT_OK) rc = m->d_pn.upload(reinterpret_cast<const float4 *>(m->host.pn.data()), m->host.pn.size() / 4);
  m->dev_bytes = (int64_t)(b.nodes.size() * sizeof(rtl::GNode) + m->host.tri.size() * 4 + m->host.pn.size() * 4);
  if (rc == RT_OK && m->dynamic) rc = upload_dynamic(m, topo, idx, nidx);
  if (rc != RT_OK) {
    rt_sdf_mesh_destroy(m);
    return rc;
  }
  *out = m;
  return RT_OK;
}

int rt_sdf_mesh_update_vertices_device(rt_sdf_mesh *m, const float *d_vpos4, int64_t nverts, void *stream) {
  if (int rc = check_update(m, d_vpos4, nverts, "rt_sdf_mesh_update_vertices_device")) return rc;
  return update_device(m, d_vpos4, (hipStream_t)stream);
}

int rt_sdf_mesh_update_vertices(rt_sdf_mesh *m, const float *vpos4, int64_t nverts) {
  if (int rc = check_update(m, vpos4, nverts, "rt_sdf_mesh_update_vertices")) return rc;
  int prev = 0;
  HIP_TRY(hipGetDevice(&prev));
  HIP_TRY(hipSetDevice(m->device));
  int rc = RT_OK;
  // (the staging buffer may still be read by an earlier update's kernels)
  hipError_t e = hipEventSynchronize(m->updated.e);
  if (e == hipSuccess) e = rtdma::h2d(m->d_vstage.p, vpos4, 16 * (size_t)nverts, nullptr);
  if (e != hipSuccess) rc = rterr::set(RT_E_DEVICE, rterr::hip_fail("rt_sdf_mesh_update_vertices: vertex upload", e));
  if (!rc) rc = update_device(m, reinterpret_cast<const float *>(m->d_vstage.p), nullptr);
  if (!rc) {
    e = hipEventSynchronize(m->updated.e);
    if (e != hipSuccess) rc = rterr::set(RT_E_DEVICE, rterr::hip_fail("rt_sdf_mesh_update_vertices: wait", e));
  }
  HIP_NOTE(hipSetDevice(prev));
  return rc;
}

int rt_sdf_mesh_get_pseudonormals(const rt_sdf_mesh *m, float *pn28, int64_t ntri) {
  if (!m || !pn28) return rterr::set(RT_E_INVALID, "rt_sdf_mesh_get_pseudonormals: NULL argument");
  if (ntri != m->ntri) return rterr::set(RT_E_INVALID, "rt_sdf_mesh_get_pseudonormals: ntri is not the handle's");
  int prev = 0;
  HIP_TRY(hipGetDevice(&prev));
  HIP_TRY(hipSetDevice(m->device));
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess) e = rtdma::d2h(pn28, m->d_pn.p, (size_t)ntri * 28 * 4, nullptr);
  HIP_NOTE(hipSetDevice(prev));
  if (e != hipSuccess) return rterr::set(RT_E_DEVICE, rterr::hip_fail("rt_sdf_mesh_get_pseudonormals", e));
  return RT_OK;
}

int64_t rt_sdf_mesh_device_bytes(const rt_sdf_mesh *m) {
  if (!m) return rterr::set(RT_E_INVALID, "rt_sdf_mesh_device_bytes: handle is NULL");
  return m->dev_bytes;
}

// Diagnostic (not part of include/rtamd.h): the handle's device tree, as it is
// now: n_inner GNode records (224 bytes each) and n_tri triangle records (48
// bytes each: a.xyz, id | b.xyz, 0 | c.xyz, 0). Two-call protocol: with
// nodes224 = tri48 = NULL only the counts are returned; else *n_inner / *n_tri
// are the buffers' capacities.
int rtx_sdf_mesh_download(const rt_sdf_mesh *m, void *nodes224, int64_t *n_inner, void *tri48, int64_t *n_tri) {
  if (!m || !n_inner || !n_tri) return rterr::set(RT_E_INVALID, "rtx_sdf_mesh_download: NULL argument");
  const int64_t ni = (int64_t)m->host.bvh.nodes.size(), nt = (int64_t)m->host.bvh.tris.size();
  if (nodes224 || tri48) {
    if (!nodes224 || !tri48 || *n_inner < ni || *n_tri < nt)
      return rterr::set(RT_E_INVALID, "rtx_sdf_mesh_download: buffers too small");
    int prev = 0;
    HIP_TRY(hipGetDevice(&prev));
    HIP_TRY(hipSetDevice(m->device));
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess && ni) e = rtdma::d2h(nodes224, m->d_nodes.p, (size_t)ni * sizeof(rtl::GNode), nullptr);
    if (e == hipSuccess && nt) e = rtdma::d2h(tri48, m->d_tri.p, (size_t)nt * 48, nullptr);
    HIP_NOTE(hipSetDevice(prev));
    if (e != hipSuccess) return rterr::set(RT_E_DEVICE, rterr::hip_fail("rtx_sdf_mesh_download", e));
  }
  *n_inner = ni;
  *n_tri = nt;
  return RT_OK;
}

int rt_sdf_mesh_points(rt_sdf_mesh *m, const float *p3, int64_t n, float *dist) {
  if (!m || n < 0 || (n && (!p3 || !dist))) return rterr::set(RT_E_INVALID, "bad arguments");
  return query_host(m, p3, n, dist);
}

int rt_sdf_mesh_grid(rt_sdf_mesh *m, const uint32_t size[3], float *values) {
  if (!m || !size || !values) return rterr::set(RT_E_INVALID, "bad arguments");
  uint32_t blocks = 0;
  if (int rc = grid_blocks(size, blocks)) return rc;
  const int64_t n = (int64_t)size[0] * size[1] * size[2];
  g_stale_seen = rterr::take_stale();
  HIP_TRY(hipSetDevice(m->device));
  if (int rc = wait_updated(m, nullptr)) return rc;
  rtmem::DevArray<float> d;
  if (int rc = d.alloc((size_t)n)) return rc;
  hipLaunchKernelGGL(sdf_kernel<true>, dim3(blocks), dim3(kWave), lds_bytes(m), 0, dev_of(m), nullptr,
                     n, size[0], size[1], size[2], m->stack_cap, d.p);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = rtdma::d2h(values, d.p, (size_t)n * 4, nullptr);
  if (e != hipSuccess) return rterr::set(RT_E_DEVICE, std::string("sdf grid: ") + hipGetErrorString(e));
  return RT_OK;
}

int rt_sdf_mesh_grid_device(rt_sdf_mesh *m, const uint32_t size[3], float *d_values, void *stream) {
  if (!m || !size || !d_values) return rterr::set(RT_E_INVALID, "bad arguments");
  uint32_t blocks = 0;
  if (int rc = grid_blocks(size, blocks)) return rc;
  hipLaunchKernelGGL(sdf_kernel<true>, dim3(blocks), dim3(kWave), lds_bytes(m), (hipStream_t)stream, dev_of(m),
                     nullptr, (int64_t)size[0] * size[1] * size[2], size[0], size[1], size[2], m->stack_cap,
                     d_values);
  HIP_TRY(hipGetLastError());
  return RT_OK;
}

int rt_sdf_mesh_device(const rt_sdf_mesh *m) { return m ? m->device : RT_E_INVALID; }

int rt_sdf_mesh_octree(rt_sdf_mesh *m, int32_t depth, int64_t *count, void *nodes36) {
  if (!m || !count) return rterr::set(RT_E_INVALID, "bad arguments");
  if (m->oct_depth != depth) {
    std::string err;
    std::vector<uint8_t> nodes;
    if (!rth::build_sdf_octree(octree_query, m, depth, nodes, err))
      return rterr::set(err.rfind("octree", 0) == 0 ? RT_E_INVALID : RT_E_DEVICE, err);
    m->oct_nodes.swap(nodes);
    m->oct_depth = depth;
  }
  const int64_t n = (int64_t)(m->oct_nodes.size() / 36);
  if (nodes36) {
    if (*count < n) return rterr::set(RT_E_INVALID, "node buffer too small");
    std::memcpy(nodes36, m->oct_nodes.data(), m->oct_nodes.size());
  }
  *count = n;
  return RT_OK;
}

int rt_sdf_mesh_destroy(rt_sdf_mesh *m) {
  if (!m) return RT_OK;
  HIP_NOTE(hipSetDevice(m->device));
  if (m->qs.s) HIP_NOTE(hipStreamSynchronize(m->qs.s));
  delete m;
  return RT_OK;
}

int rt_mesh_subdivide(const float *vpos4, int64_t nverts, const uint32_t *idx, int64_t nidx, int32_t levels,
                      float *out_vpos4, int64_t *out_nverts, uint32_t *out_idx, int64_t *out_nidx) {
  if ((!vpos4 && nverts) || (!idx && nidx) || nverts < 0 || !out_nverts || !out_nidx)
    return rterr::set(RT_E_INVALID, "bad arguments");
  rth::Mesh r;
  std::string err;
  if (!rth::subdivide_mesh(vpos4, nverts, idx, nidx, levels, r, err)) return rterr::set(RT_E_INVALID, err);
  const int64_t nv = (int64_t)(r.vpos4.size() / 4), ni = (int64_t)r.idx.size();
  if (out_vpos4 || out_idx) {
    if (!out_vpos4 || !out_idx || *out_nverts < nv || *out_nidx < ni)
      return rterr::set(RT_E_INVALID, "output buffers too small");
    std::memcpy(out_vpos4, r.vpos4.data(), r.vpos4.size() * 4);
    std::memcpy(out_idx, r.idx.data(), r.idx.size() * 4);
  }
  *out_nverts = nv;
  *out_nidx = ni;
  return RT_OK;
}

// Test hooks: leave a HIP error pending on this thread through a librtamd
// call (hipSetDevice(-1)), and read the stale error the last SDF call of this
// thread found before its first copy ("" if none).
int rtx_inject_stale_error(void) {
  HIP_NOTE(hipSetDevice(-1));
  return RT_OK;
}
const char *rtx_sdf_last_stale(void) { return g_stale_seen.c_str(); }

}  // extern "C"
