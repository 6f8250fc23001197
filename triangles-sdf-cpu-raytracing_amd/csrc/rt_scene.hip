// rt_scene.hip -- scenes: creation from meshes (with the BVH builder choice),
// grids and octrees, replication to another device, vertex updates of dynamic
// meshes, instanced scenes, destruction, the plane and the getters of
// include/rtamd.h, and the device views of a scene that the kernel launchers
// take (mesh_dev, grid_dev, grid_mode; rt_scene.h). Its kernels are those
// that prepare scene data (brick_kernel, grid_copy_kernel,
// tri_edge_bound_kernel).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../include/rtamd.h"
#include "rt_dispatch.h"
#include "rt_error.h"
#include "rt_host.h"
#include "rt_refit.h"
#include "rt_scene.h"
#include "rt_sdf_octree.h"
#include "rt_shade.h"

using namespace rtd;
using namespace rti;

namespace {

// bricked sample count of a grid (rt_scenes.h GridDev)
uint64_t grid_bricked_samples(const uint32_t size[3]) {
  return (uint64_t)grid_bricks(size[0]) * grid_bricks(size[1]) * grid_bricks(size[2]) * 64u;
}

// device samples of a grid scene (s->grid.bricked picks the layout)
uint64_t grid_samples(const rt_scene *s) {
  return s->grid.bricked ? grid_bricked_samples(s->grid.size) : (uint64_t)s->grid.size[0] * s->grid.size[1] * s->grid.size[2];
}

// diagnostic (rtx_set_grid_force): bit 0 = grids created from now on take the
// bricked layout whatever their size, bit 1 = every grid launch takes the 64-bit
// address path (no buffer loads); tests reach each grid_mode branch with it
int g_grid_force = 0;

}  // namespace

namespace rti {

GridDev grid_dev(const rt_scene *s) {
  const uint64_t n = grid_samples(s);
  // buffer loads: 32-bit byte offsets and num_records, so only grids below
  // 4 GiB (a grid of exactly 2^32 bytes would put its last sample past a
  // saturated num_records) -- larger ones take the 64-bit address path
  const uint32_t bytes = 4 * n < (1ull << 32) ? (uint32_t)(4 * n) : 0u;
  if (!s->grid.bricked) return GridDev{s->geo.vals.p, s->grid.size[0], s->grid.size[1], s->grid.size[2], s->grid.size[2],
                                       s->grid.size[1] * s->grid.size[2], bytes};
  const uint32_t ys = grid_bricks(s->grid.size[2]) * 64u;
  return GridDev{s->geo.vals.p, s->grid.size[0], s->grid.size[1], s->grid.size[2], ys, grid_bricks(s->grid.size[1]) * ys, bytes};
}

int grid_mode(const rt_scene *s, const GridDev &gd) {
  // buffer mode: 32-bit byte offsets and 24-bit stride multiplies (grid_mul)
  const bool buf = gd.bytes != 0 && gd.xs < (1u << 24) && gd.ys < (1u << 24) && !(g_grid_force & 2);
  return (buf ? kGridBuf : 0) | (s->grid.bricked ? kGridBricked : 0);
}

}  // namespace rti

namespace {

// reference x-major values -> 4x4x4 bricks; one thread per bricked sample
// (padding samples get 0 and are never read)
__global__ __launch_bounds__(256) void brick_kernel(const float *__restrict__ src, float *__restrict__ dst,
                                                    uint32_t sx, uint32_t sy, uint32_t sz, uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t nby = grid_bricks(sy), nbz = grid_bricks(sz);
  const uint32_t l = (uint32_t)(i & 63u);
  const uint64_t b = i >> 6;
  const uint32_t bz = (uint32_t)(b % nbz), by = (uint32_t)((b / nbz) % nby), bx = (uint32_t)(b / nbz / nby);
  const uint32_t x = bx * 4 + (l >> 4), y = by * 4 + ((l >> 2) & 3u), z = bz * 4 + (l & 3u);
  dst[i] = (x < sx && y < sy && z < sz) ? src[((uint64_t)x * sy + y) * sz + z] : 0.0f;
}

// new values of a linear grid scene (rt_scene_update_grid_device): one sample per thread
__global__ __launch_bounds__(256) void grid_copy_kernel(const float *__restrict__ src, float *__restrict__ dst, uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) dst[i] = src[i];
}

}  // namespace

namespace rti {

MeshDev mesh_dev(const rt_scene *s) {
  MeshDev m{s->geo.nodes.p, s->geo.tris.p, s->mesh.root, {}, s->info.coop, s->mesh.dmax2};
  for (int k = 0; k < 6; ++k) m.rbox[k] = s->mesh.root_box[k];
  return m;
}

// the entries that render frames or copy a scene take no instanced scene
int no_instanced(const rt_scene *s, const char *who) {
  if (s && s->info.kind == RT_SCENE_INSTANCED)
    return set_err(RT_E_STATE, std::string(who) + ": not available for an instanced scene");
  return RT_OK;
}

int instanced_sync(rt_scene *s, hipStream_t stream) {
  for (size_t j = 0; j < s->inst.blas.size(); ++j) {
    // (only a dynamic mesh's version ever moves: an SDF scene that takes new
    // values keeps its arrays, so its table entry stays right as it is)
    if (s->inst.blas[j]->info.version == s->inst.blas_seen[j]) continue;
    // (a mixed table: the mesh view of the record; kind and variant stay)
    rtd::MeshDev *entry = s->inst.mixed.p ? &(s->inst.mixed.p + j)->mesh : s->inst.tab.p + j;
    if (int rc = rti::blas_entry_launch(entry, mesh_dev(s->inst.blas[j]), stream)) return rc;
    s->inst.blas_seen[j] = s->inst.blas[j]->info.version;
    if (!s->inst.tlas.p) continue;
    // its root box moved: that BLAS's leaves of the top-level tree and the
    // tree above them, behind the entry
    const rti::TlasArgs t = rti::tlas_args(s);
    if (int rc = s->inst.mixed.p ? rti::mixed_boxes_launch(t, s->inst.mixed.p, 0, s->inst.n, nullptr, (int32_t)j, stream)
                            : rti::tlas_boxes_launch(t, 0, s->inst.n, nullptr, (int32_t)j, stream))
      return rc;
    if (int rc = rti::tlas_refit_launch(t, stream)) return rc;
  }
  return RT_OK;
}

rti::TlasArgs tlas_args(const rt_scene *s) {
  return rti::TlasArgs{s->inst.tlas.p, s->inst.tlas_leaves, s->inst.n, s->inst.recs.p, s->inst.xform.p, s->inst.tab.p};
}

}  // namespace rti

namespace {

// LDS frame slots per lane for a tree with `depth` inner levels: the top frame
// lives in registers, so depth-1 slots. Sized to the tree (not a worst case)
// so the stack does not cap occupancy: 4 slots x 12 B x 256 lanes = 12 KiB.
int pick_maxd(int depth, int32_t &maxd) {
  const int need = depth > 1 ? depth - 1 : 1;
  const int options[] = {4, 7, 15, 31};
  for (int m : options)
    if (need <= m) { maxd = m; return RT_OK; }
  return set_err(RT_E_INVALID, "tree deeper than 32 levels");
}

}  // namespace

namespace {
// BVH8 builder selection (rt_set_bvh_builder): both builders give the same tree
int g_bvh_mode = RT_BVH_AUTO;
constexpr int64_t kBvhDeviceMinTris = 32768;  // auto: the device builder from this many triangles

// which builder produced this thread's last tree (rtx_bvh_last_builder):
// 1 host, 2 device, 3 host after a failed device build (AUTO)
thread_local int t_bvh_last = 0;

int build_bvh(const float *vpos4, int64_t nverts, const uint32_t *idx, int64_t nidx, rth::BVHGpu &b,
              unsigned want) {
  std::string err;
  int ndev = 0;
  const bool dev = g_bvh_mode == RT_BVH_DEVICE ||
                   (g_bvh_mode == RT_BVH_AUTO && nidx / 3 >= kBvhDeviceMinTris &&
                    hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0);
  bool fell_back = false;
  if (dev) {
    if (rth::build_bvh8_gpu(vpos4, nverts, idx, nidx, b, err, want)) {
      t_bvh_last = 2;
      return RT_OK;
    }
    if (err.rfind("GPU BVH builder bound", 0) == 0) return set_err(RT_E_DEVICE, err);
    const bool device_failure = err.rfind("GPU BVH build:", 0) == 0;
    if (!device_failure) return set_err(RT_E_INVALID, err);
    if (g_bvh_mode == RT_BVH_DEVICE) return set_err(RT_E_DEVICE, err);
    // AUTO: the host builder gives the identical tree, unless
    // the device is left in a sticky fault state: then every later call on it
    // fails too, so the failure is reported here instead of at the upload
    if (const hipError_t e = hipDeviceSynchronize(); e != hipSuccess)
      return set_err(RT_E_DEVICE, err + "; device unusable afterwards: " + hipGetErrorString(e));
    (void)hipGetLastError();  // the builder's failure was reported above: clear it
    std::fprintf(stderr, "rtamd: %s; building the BVH on the host instead\n", err.c_str());
    fell_back = true;
    err.clear();
  }
  if (!rth::build_bvh8(vpos4, nverts, idx, nidx, b, err, want)) return set_err(RT_E_INVALID, err);
  t_bvh_last = fell_back ? 3 : 1;
  return RT_OK;
}

int new_scene(rt_scene **out) {
  if (!out) return set_err(RT_E_INVALID, "out is NULL");
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  rt_scene *s = new rt_scene();
  s->device = dev;
  s->info.plane.on = 0;
  s->info.plane.n = f3{0.0f, 1.0f, 0.0f};
  *out = s;
  return RT_OK;
}

}  // namespace

extern "C" {

int rt_set_bvh_builder(int mode) {
  if (mode < RT_BVH_AUTO || mode > RT_BVH_DEVICE) return set_err(RT_E_INVALID, "bad BVH builder mode");
  g_bvh_mode = mode;
  return RT_OK;
}

int rt_bvh_export(const float *vpos4, int64_t nverts, const uint32_t *idx, int64_t nidx,
                  uint32_t *canon, int64_t *nnodes, uint32_t *perm_tri, int32_t *max_depth) {
  if (!vpos4 || !idx || !nnodes || nverts <= 0 || nidx <= 0) return set_err(RT_E_INVALID, "bad mesh");
  rth::BVHGpu b;
  const unsigned want = (canon ? rth::kBvhCanon : 0u) | (perm_tri ? rth::kBvhPerm : 0u);
  if (int rc = build_bvh(vpos4, nverts, idx, nidx, b, want)) return rc;
  const int64_t n = canon ? (int64_t)b.canon.size() / 52 : b.host_nodes;
  if (canon) {
    if (*nnodes < n) return set_err(RT_E_INVALID, "buffer too small");
    std::memcpy(canon, b.canon.data(), b.canon.size() * 4);
  }
  if (perm_tri) std::memcpy(perm_tri, b.perm_tri.data(), b.perm_tri.size() * 4);
  if (max_depth) *max_depth = b.max_depth;
  *nnodes = n;
  return RT_OK;
}

// max over triangle slots of |e1| |e2| (float bits: the values are >= 0, so
// their bit patterns order like them; NaN counts as +inf)
__global__ void tri_edge_bound_kernel(const rtl::GTri *__restrict__ tris, uint32_t n, uint32_t *out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  float m = 0.0f;
  if (i < n) {
    const float4 *q = reinterpret_cast<const float4 *>(tris + i);
    const float4 b = q[1], c = q[2];
    const float v = __builtin_sqrtf(b.x * b.x + b.y * b.y + b.z * b.z) *
                    __builtin_sqrtf(c.x * c.x + c.y * c.y + c.z * c.z);
    m = __builtin_isnan(v) ? kInf : v;
  }
  for (int off = 32; off > 0; off >>= 1) m = __builtin_fmaxf(m, __shfl_xor(m, off, 64));
  if ((threadIdx.x & 63) == 0 && m > 0.0f) atomicMax(out, __float_as_uint(m));
}

// MeshDev::dmax2 of a mesh scene: (2^124 / (2 M))^2, M = max |e1| |e2| over its
// triangles. A ray with dot(d, d) <= dmax2 has |d| <= 2^124 / (2 M) (up to a
// few ulps), and tri_t's float det = e1 . (d x e2) is at most sqrt(2) |e1|
// |e2| |d| (1 + 2^-24)^5 < 1.5 M |d| <= 0.75 x 2^124 in magnitude: inside the
// range where rtm::rcp_rn is the division. M = 0 (no triangle with both edges)
// leaves every direction; M = inf or NaN leaves none.
float dmax2_of(uint32_t edge_bits) {
  float M;
  std::memcpy(&M, &edge_bits, 4);
  if (M == 0.0f) return std::numeric_limits<float>::max();
  if (!std::isfinite(M)) return 0.0f;
  const double r = std::ldexp(1.0, 124) / (2.0 * (double)M * (1.0 + 1e-6));
  const double r2 = r * r;
  return r2 >= (double)std::numeric_limits<float>::max() ? std::numeric_limits<float>::max()
                                                          : std::nextafter((float)r2, 0.0f);
}
int mesh_dmax2(rt_scene *s, uint32_t n_tris) {
  s->mesh.dmax2 = 0.0f;
  if (n_tris == 0) return RT_OK;
  rtmem::DevArray<uint32_t> d;
  uint32_t h = 0;
  if (int rc = d.alloc(1)) return rc;
  hipError_t e = hipMemset(d.p, 0, 4);
  if (e == hipSuccess) {
    tri_edge_bound_kernel<<<(n_tris + 255) / 256, 256>>>(s->geo.tris.p, n_tris, d.p);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(&h, d.p, 4, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return set_err(RT_E_DEVICE, std::string("triangle edge bound: ") + hipGetErrorString(e));
  s->mesh.dmax2 = dmax2_of(h);
  return RT_OK;
}

int rt_scene_create_mesh(const float *vpos4, int64_t nverts, const uint32_t *idx, int64_t nidx,
                         rt_scene **out) {
  return rt_scene_create_mesh_ex(vpos4, nverts, idx, nidx, 0u, out);
}

int rt_scene_create_mesh_ex(const float *vpos4, int64_t nverts, const uint32_t *idx, int64_t nidx,
                            uint32_t flags, rt_scene **out) {
  if (!vpos4 || !idx || nverts <= 0 || nidx <= 0) return set_err(RT_E_INVALID, "empty mesh");
  if (flags & ~RT_MESH_DYNAMIC) return set_err(RT_E_INVALID, "rt_scene_create_mesh_ex: unknown flags");
  rth::BVHGpu b;
  if (int rc = build_bvh(vpos4, nverts, idx, nidx, b, rth::kBvhTris | rth::kBvhDeviceTris)) return rc;
  int32_t maxd = 8;
  int rc = pick_maxd(b.max_depth, maxd);
  if (rc) return rc;
  rt_scene *s;
  if ((rc = new_scene(&s))) return rc;
  s->info.kind = RT_SCENE_MESH;
  s->info.maxd = maxd;
  s->mesh.root = b.root_word;
  std::memcpy(s->mesh.root_box, b.root_box, sizeof(s->mesh.root_box));
  if (!(b.root_word & rtl::kLeafBit) && b.root_word < b.nodes.size())
    std::memcpy(s->mesh.root_child, b.nodes[b.root_word].box, sizeof(s->mesh.root_child));
  s->mesh.host_nodes = b.host_nodes;
  s->mesh.host_inner = b.host_inner;
  s->mesh.depth = b.max_depth;
  s->mesh.n_inner = (uint32_t)b.nodes.size();
  if (b.dev_tris.p) {  // the device builder left the triangles on the device (with the zero pad)
    s->info.dev_bytes += (int64_t)b.dev_tris.bytes;
    s->geo.tris.adopt(b.dev_tris);
  }
  if ((rc = s->geo.nodes.upload(b.nodes.data(), b.nodes.size(), s->info.dev_bytes)) ||
      (!s->geo.tris.p && (rc = s->geo.tris.upload_padded(b.tris.data(), b.tris.size(), 8, s->info.dev_bytes))) ||
      (rc = mesh_dmax2(s, b.n_tris))) {
    rt_scene_destroy(s);
    return rc;
  }
  s->mesh.n_tris = b.n_tris;
  if (!b.nodes.empty())
    for (uint32_t w : b.nodes[0].child) s->mesh.root_nchild += w != rtl::kInvalidChild;
  if (flags & RT_MESH_DYNAMIC) {
    const int64_t before = s->info.dev_bytes;
    s->dyn.nverts = nverts;
    s->dyn.level_first = rth::bvh_level_first(b.nodes);
    if ((rc = s->dyn.idx.upload(idx, (size_t)nidx, s->info.dev_bytes)) ||
        (rc = s->dyn.vstage.upload(nullptr, 4 * (size_t)nverts, s->info.dev_bytes)) ||
        (rc = s->dyn.edge.upload(nullptr, 1, s->info.dev_bytes)) ||
        (rc = s->dyn.h_refit.alloc(64, hipHostMallocDefault))) {
      rt_scene_destroy(s);
      return rc;
    }
    s->dyn.bytes = s->info.dev_bytes - before;
    s->dyn.on = true;
  }
  *out = s;
  return RT_OK;
}

// The refit behind both update entries: d_vpos4 (device, on the scene's
// device) is read in stream order on `stream`; returns after the constants
// are back on the host.
static int update_vertices_device(rt_scene *s, const float *d_vpos4, hipStream_t st) {
  const rti::RefitArgs a{s->geo.nodes.p, s->geo.tris.p, s->mesh.root, d_vpos4, s->dyn.idx.p, s->dyn.level_first.data(),
                         s->dyn.level_first.empty() ? 0 : (int32_t)s->dyn.level_first.size() - 1};
  if (int rc = rti::refit_launch(a, st)) return rc;
  // the constants the host keeps: the triangles' edge bound (dmax2) and, for
  // an inner root, its eight child boxes (root_child, root_box)
  const bool inner = a.levels > 0;
  HIP_TRY(hipMemsetAsync(s->dyn.edge.p, 0, 4, st));
  if (s->mesh.n_tris) {
    tri_edge_bound_kernel<<<(s->mesh.n_tris + 255) / 256, 256, 0, st>>>(s->geo.tris.p, s->mesh.n_tris, s->dyn.edge.p);
    HIP_TRY(hipGetLastError());
  }
  if (inner) HIP_TRY(hipMemcpyAsync(s->dyn.h_refit.h, s->geo.nodes.p[0].box, 192, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(s->dyn.h_refit.h + 48, s->dyn.edge.p, 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (inner) {
    std::memcpy(s->mesh.root_child, s->dyn.h_refit.h, 192);
    const float inf = std::numeric_limits<float>::infinity();
    float mn[3] = {inf, inf, inf}, mx[3] = {-inf, -inf, -inf};
    for (uint32_t c = 0; c < s->mesh.root_nchild; ++c) {  // bvh_layout's root box: the union over c = 0 .. nchild-1
      for (int k = 0; k < 3; ++k) {
        mn[k] = std::min(mn[k], s->mesh.root_child[6 * c + 2 * k]);
        mx[k] = std::max(mx[k], s->mesh.root_child[6 * c + 2 * k + 1]);
      }
    }
    for (int k = 0; k < 3; ++k) { s->mesh.root_box[k] = mn[k]; s->mesh.root_box[3 + k] = mx[k]; }
  }
  s->mesh.dmax2 = s->mesh.n_tris ? dmax2_of(s->dyn.h_refit.h[48]) : 0.0f;
  ++s->info.version;
  return RT_OK;
}

int rt_scene_create_grid(const uint32_t size[3], const float *values, rt_scene **out) {
  if (!size || !values) return set_err(RT_E_INVALID, "NULL argument");
  const uint64_t n = (uint64_t)size[0] * size[1] * size[2];
  if (size[0] < 1 || size[1] < 1 || size[2] < 1 || n > (1ull << 32))
    return set_err(RT_E_INVALID, "bad grid size");
  rt_scene *s;
  int rc = new_scene(&s);
  if (rc) return rc;
  s->info.kind = RT_SCENE_GRID;
  s->grid.size[0] = size[0]; s->grid.size[1] = size[1]; s->grid.size[2] = size[2];
  if ((uint64_t)n * 4 <= kGridLinearMaxBytes && !(g_grid_force & 1)) {  // fits one XCD's L2: the reference layout
    if ((rc = s->geo.vals.upload(values, (size_t)n, s->info.dev_bytes))) {
      rt_scene_destroy(s);
      return rc;
    }
    *out = s;
    return RT_OK;
  }
  const uint64_t nb = grid_bricked_samples(size);
  if (nb >= (1ull << 32)) {
    rt_scene_destroy(s);
    return set_err(RT_E_INVALID, "bad grid size");
  }
  s->grid.bricked = true;
  rtmem::DevArray<float> ref;  // the reference array, staged for the device-side bricking
  int64_t staged = 0;          // (not part of the scene's device bytes)
  if ((rc = ref.upload(values, (size_t)n, staged)) ||
      (rc = s->geo.vals.upload(nullptr, (size_t)nb, s->info.dev_bytes))) {
    rt_scene_destroy(s);
    return rc;
  }
  brick_kernel<<<(unsigned)((nb + 255) / 256), 256>>>(ref.p, s->geo.vals.p, size[0], size[1], size[2], nb);
  const hipError_t e1 = hipGetLastError(), e2 = hipDeviceSynchronize();
  if (e1 != hipSuccess || e2 != hipSuccess) {
    rt_scene_destroy(s);
    return set_err(RT_E_DEVICE, std::string("grid bricking: ") + hipGetErrorString(e1 != hipSuccess ? e1 : e2));
  }
  *out = s;
  return RT_OK;
}

int rt_scene_create_octree(const void *nodes36, int64_t count, rt_scene **out) {
  if (!nodes36 || count <= 0) return set_err(RT_E_INVALID, "empty octree");
  rth::OctGpu g;
  std::string err;
  if (!rth::flatten_octree((const uint8_t *)nodes36, count, g, err)) return set_err(RT_E_INVALID, err);
  int32_t maxd = 8;
  int rc = pick_maxd(g.max_depth, maxd);
  if (rc) return rc;
  rt_scene *s;
  if ((rc = new_scene(&s))) return rc;
  s->info.kind = RT_SCENE_OCTREE;
  s->info.maxd = maxd;
  s->oct.depth = g.max_depth;
  if ((rc = s->geo.child.upload(g.child.data(), g.child.size(), s->info.dev_bytes)) ||
      (rc = s->geo.ovals.upload(g.vals.data(), g.vals.size(), s->info.dev_bytes))) {
    rt_scene_destroy(s);
    return rc;
  }
  *out = s;
  return RT_OK;
}

int rt_scene_update_grid_device(rt_scene *s, const float *d_values, void *stream) {
  if (!s) return set_err(RT_E_INVALID, "rt_scene_update_grid_device: scene is NULL");
  if (!d_values) return set_err(RT_E_INVALID, "rt_scene_update_grid_device: values are NULL");
  if (s->info.kind != RT_SCENE_GRID) return set_err(RT_E_STATE, "rt_scene_update_grid_device: not a grid scene");
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (s->device != dev)
    return set_err(RT_E_INVALID, "rt_scene_update_grid_device: the scene lives on device " + std::to_string(s->device) +
                                     ", the current one is " + std::to_string(dev));
  const hipStream_t st = (hipStream_t)stream;
  const uint64_t n = grid_samples(s);  // (below 2^32 bricked, at most 2^32 linear)
  const unsigned blocks = (unsigned)((n + 255) / 256);
  if (s->grid.bricked)
    brick_kernel<<<blocks, 256, 0, st>>>(d_values, s->geo.vals.p, s->grid.size[0], s->grid.size[1], s->grid.size[2], n);
  else
    grid_copy_kernel<<<blocks, 256, 0, st>>>(d_values, s->geo.vals.p, n);
  HIP_TRY(hipGetLastError());
  return RT_OK;
}

int rt_scene_create_octree_dynamic(int32_t depth, int64_t max_nodes, rt_scene **out) {
  if (!out) return set_err(RT_E_INVALID, "rt_scene_create_octree_dynamic: out is NULL");
  if (depth < 0 || depth > 12) return set_err(RT_E_INVALID, "rt_scene_create_octree_dynamic: depth must be in [0, 12]");
  if (max_nodes < 1 || max_nodes > 0xFFFFFFFFll)
    return set_err(RT_E_INVALID, "rt_scene_create_octree_dynamic: max_nodes must be in [1, 2^32 - 1]");
  int32_t maxd = 8;
  int rc = pick_maxd(depth, maxd);
  if (rc) return rc;
  rt_scene *s;
  if ((rc = new_scene(&s))) return rc;
  s->info.kind = RT_SCENE_OCTREE;
  s->info.maxd = maxd;
  s->oct.depth = depth;
  rts::OctDynamic &od = s->octdyn;
  od.on = true;
  od.max_nodes = (uint32_t)max_nodes;
  const size_t C = (size_t)max_nodes;
  // the initial tree: a root that is an empty leaf
  rtl::OctWord w0{rtl::kOctNeverHits, 0u};
  rtl::OctVals v0;
  std::fill(v0.v, v0.v + 8, 1000.0f);
  const uint32_t st0[2] = {1u, 0u};
  hipError_t e = hipSuccess;
  auto put = [&](void *d, const void *h, size_t bytes) {
    if (rc == RT_OK && e == hipSuccess) e = rtdma::h2d(d, h, bytes, nullptr);
  };
  if ((rc = s->geo.child.alloc(C)) == RT_OK && (rc = s->geo.ovals.alloc(C)) == RT_OK) {
    s->info.dev_bytes += (int64_t)(s->geo.child.bytes() + s->geo.ovals.bytes());
    put(s->geo.child.p, &w0, sizeof w0);
    put(s->geo.ovals.p, &v0, sizeof v0);
  }
  if (rc == RT_OK) rc = od.status.alloc(2);
  put(od.status.p, st0, sizeof st0);
  if (rc == RT_OK) rc = od.s_child.alloc(C);
  if (rc == RT_OK) rc = od.s_vals.alloc(C);
  if (rc == RT_OK) rc = od.cells.alloc(C);
  if (rc == RT_OK) rc = od.flag.alloc(rtsdf::oct_flag_count(od.max_nodes));
  if (rc == RT_OK) rc = od.bsum.alloc(rtsdf::oct_bsum_count(od.max_nodes));
  if (rc == RT_OK) rc = od.lvl.alloc(rtsdf::kOctLvlWords);
  if (rc == RT_OK) rc = od.top.alloc(std::max<size_t>(rtsdf::oct_top_first(rtsdf::oct_top_levels(depth)), 1));
  if (rc == RT_OK && e != hipSuccess)
    rc = set_err(RT_E_DEVICE, rterr::hip_fail("rt_scene_create_octree_dynamic: upload of the initial tree", e));
  if (rc != RT_OK) {
    rt_scene_destroy(s);
    return rc;
  }
  od.bytes = (int64_t)(od.status.bytes() + od.s_child.bytes() + od.s_vals.bytes() + od.cells.bytes() + od.flag.bytes() +
                       od.bsum.bytes() + od.lvl.bytes() + od.top.bytes());
  s->info.dev_bytes += od.bytes;
  *out = s;
  return RT_OK;
}

// What an octree scene holds on the device after a wait for it: the node
// count and the dropped-build flag (a plain octree: its size, 0).
static int octree_check(const rt_scene *s, const char *who) {
  if (!s) return set_err(RT_E_INVALID, std::string(who) + ": scene is NULL");
  if (s->info.kind != RT_SCENE_OCTREE) return set_err(RT_E_STATE, std::string(who) + ": not an octree scene");
  return RT_OK;
}
static int octree_status(rt_scene *s, const char *who, uint32_t st[2]) {
  if (int rc = octree_check(s, who)) return rc;
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipDeviceSynchronize());
  st[0] = (uint32_t)s->geo.child.n;
  st[1] = 0u;
  if (s->octdyn.on) HIP_TRY(rtdma::d2h(st, s->octdyn.status.p, 8, nullptr));
  return RT_OK;
}

// The scene's device arrays, words and values of its first st[0] nodes.
static int octree_download(rt_scene *s, const char *who, uint32_t st[2], std::vector<rtl::OctWord> &w,
                           std::vector<rtl::OctVals> *v) {
  if (int rc = octree_check(s, who)) return rc;
  int prev = 0;
  HIP_TRY(hipGetDevice(&prev));
  int rc = octree_status(s, who, st);
  if (rc == RT_OK) {
    w.resize(st[0]);
    hipError_t e = rtdma::d2h(w.data(), s->geo.child.p, (size_t)st[0] * sizeof(rtl::OctWord), nullptr);
    if (e == hipSuccess && v) {
      v->resize(st[0]);
      e = rtdma::d2h(v->data(), s->geo.ovals.p, (size_t)st[0] * sizeof(rtl::OctVals), nullptr);
    }
    if (e != hipSuccess) rc = set_err(RT_E_DEVICE, rterr::hip_fail(who, e));
  }
  HIP_NOTE(hipSetDevice(prev));
  return rc;
}

int rt_scene_octree_status(rt_scene *s, int64_t *count, int32_t *overflow) {
  if (int rc = octree_check(s, "rt_scene_octree_status")) return rc;
  int prev = 0;
  HIP_TRY(hipGetDevice(&prev));
  uint32_t st[2];
  const int rc = octree_status(s, "rt_scene_octree_status", st);
  HIP_NOTE(hipSetDevice(prev));
  if (rc) return rc;
  if (count) *count = (int64_t)st[0];
  if (overflow) *overflow = (int32_t)st[1];
  return RT_OK;
}

int rt_scene_get_octree(rt_scene *s, int64_t *count, void *nodes36) {
  if (!count) return set_err(RT_E_INVALID, "rt_scene_get_octree: count is NULL");
  if (int rc = octree_check(s, "rt_scene_get_octree")) return rc;
  uint32_t st[2];
  if (!nodes36) {
    int prev = 0;
    HIP_TRY(hipGetDevice(&prev));
    const int rc = octree_status(s, "rt_scene_get_octree", st);
    HIP_NOTE(hipSetDevice(prev));
    if (rc == RT_OK) *count = (int64_t)st[0];
    return rc;
  }
  std::vector<rtl::OctWord> w;
  std::vector<rtl::OctVals> v;
  if (int rc = octree_download(s, "rt_scene_get_octree", st, w, &v)) return rc;
  if (*count < (int64_t)st[0]) return set_err(RT_E_INVALID, "rt_scene_get_octree: node buffer too small");
  uint8_t *o = static_cast<uint8_t *>(nodes36);
  for (size_t i = 0; i < w.size(); ++i) {
    // (both leaf words are offset 0 in the 36-byte format)
    const uint32_t off = w[i].child == rtl::kOctNeverHits ? 0u : w[i].child;
    std::memcpy(o + 36 * i, v[i].v, 32);
    std::memcpy(o + 36 * i + 32, &off, 4);
  }
  *count = (int64_t)st[0];
  return RT_OK;
}

int rt_scene_replicate(const rt_scene *src, int device, rt_scene **out) {
  if (!src || !out) return set_err(RT_E_INVALID, "bad arguments");
  if (int rc = no_instanced(src, "rt_scene_replicate")) return rc;
  *out = nullptr;
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return set_err(RT_E_INVALID, "rt_scene_replicate: no such device");
  int prev = 0;
  HIP_TRY(hipGetDevice(&prev));
  HIP_TRY(hipSetDevice(device));
  rt_scene *s = new rt_scene();
  // the scene's description (kind, tree shape, plane, kernel instantiation, switches)
  s->device = device;
  s->info = src->info;
  s->mesh = src->mesh;
  s->grid = src->grid;
  s->oct = src->oct;
  s->info.dev_bytes = src->info.dev_bytes - src->dyn.bytes - src->octdyn.bytes;  // (a plain snapshot: not dynamic)
  // the device arrays, copied device to device (over xGMI between GPUs) at the
  // size their owner holds (the triangles with their zero pad)
  hipError_t e = hipSuccess;
  const char *step = "";
  auto copy = [&](auto &to, const auto &from) {
    if (!from.p || e != hipSuccess) return;
    if ((e = to.alloc_e(from.n)) != hipSuccess) { step = "hipMalloc"; return; }
    if ((e = hipMemcpyPeer(to.p, device, from.p, src->device, from.bytes())) != hipSuccess) step = "hipMemcpyPeer";
  };
  copy(s->geo.nodes, src->geo.nodes);
  copy(s->geo.tris, src->geo.tris);
  copy(s->geo.vals, src->geo.vals);
  copy(s->geo.child, src->geo.child);
  copy(s->geo.ovals, src->geo.ovals);
  HIP_NOTE(hipSetDevice(prev));
  if (e != hipSuccess) {
    rt_scene_destroy(s);
    return set_err(RT_E_DEVICE, std::string("rt_scene_replicate: ") + step + ": " + hipGetErrorString(e));
  }
  *out = s;
  return RT_OK;
}

int rt_scene_device(const rt_scene *s) { return s ? s->device : RT_E_INVALID; }

static int check_update(const rt_scene *s, const float *vpos4, int64_t nverts, const char *who) {
  if (!s) return set_err(RT_E_INVALID, std::string(who) + ": scene is NULL");
  if (!vpos4) return set_err(RT_E_INVALID, std::string(who) + ": vertex pointer is NULL");
  if (nverts <= 0) return set_err(RT_E_INVALID, std::string(who) + ": nverts must be positive");
  if (s->info.kind != RT_SCENE_MESH) return set_err(RT_E_STATE, std::string(who) + ": not a mesh scene");
  if (!s->dyn.on)
    return set_err(RT_E_STATE, std::string(who) + ": the mesh was not created with RT_MESH_DYNAMIC");
  if (nverts != s->dyn.nverts)
    return set_err(RT_E_INVALID, std::string(who) + ": nverts is " + std::to_string(nverts) + ", the mesh was created with " +
                                     std::to_string(s->dyn.nverts));
  return RT_OK;
}

// ---- instanced scenes (include/rtamd.h; kernels in rt_instances.hip) -------
namespace {
// one rt_instance -> its device record; `who` names the entry in the message
int instance_record(const rt_instance &in, int32_t nblas, int64_t index, const char *who, rti::InstRec &r) {
  const std::string at = std::string(who) + ": instance " + std::to_string(index);
  if (in.blas < 0 || in.blas >= nblas) return set_err(RT_E_INVALID, at + ": blas index out of range");
  if (in.flags & ~RT_INSTANCE_DISABLED) return set_err(RT_E_INVALID, at + ": unknown flag bits");
  if (!rti::affine_inverse(in.xform, r.m))
    return set_err(RT_E_INVALID, at + ": the matrix is singular or has a non-finite entry");
  r.blas = in.blas;
  r.flags = in.flags;
  r.skipped = 0;
  r.pad = 0;
  return RT_OK;
}

int instance_range(const rt_scene *s, int32_t first, int32_t count, const char *who) {
  if (!s) return set_err(RT_E_INVALID, std::string(who) + ": scene is NULL");
  if (s->info.kind != RT_SCENE_INSTANCED) return set_err(RT_E_STATE, std::string(who) + ": not an instanced scene");
  if (first < 0 || count < 0 || (int64_t)first + count > s->inst.n)
    return set_err(RT_E_INVALID, std::string(who) + ": range outside the scene's " + std::to_string(s->inst.n) +
                                     " instances");
  return RT_OK;
}
}  // namespace

// the tree of a scene created with RT_INSTANCED_TLAS, from the records, the
// matrices and the table as the device holds them: leaves first .. first +
// count - 1 (d_xsrc, only_blas: rti::tlas_boxes_launch), then every inner node
static int tlas_update(const rt_scene *s, int32_t first, int32_t count, const float *d_xsrc, int32_t only_blas,
                       hipStream_t st) {
  const rti::TlasArgs t = rti::tlas_args(s);
  if (int rc = s->inst.mixed.p ? rti::mixed_boxes_launch(t, s->inst.mixed.p, first, count, d_xsrc, only_blas, st)
                          : rti::tlas_boxes_launch(t, first, count, d_xsrc, only_blas, st))
    return rc;
  return rti::tlas_refit_launch(t, st);
}

// the record of the mixed table for one bottom-level scene (rt_instances.h)
static rti::BlasRec blas_rec(const rt_scene *bl) {
  rti::BlasRec e{};
  e.kind = (uint32_t)bl->info.kind;
  if (bl->info.kind == RT_SCENE_MESH) {
    e.mesh = mesh_dev(bl);
  } else if (bl->info.kind == RT_SCENE_GRID) {
    e.grid = grid_dev(bl);
    e.var = (uint32_t)grid_mode(bl, e.grid);
  } else {
    e.oct = OctDev{bl->geo.child.p, bl->geo.ovals.p};
    e.var = bl->info.maxd <= 7 ? 1u : 0u;  // rt_dispatch.h: packed node coordinates for trees of up to 7 slots
  }
  return e;
}

// any: rt_scene_create_instanced_any, which also takes grids and octrees; with
// one of them among the BLAS the scene gets the mixed table instead of d_blas
static int create_instanced(const char *who, rt_scene *const *blas, int32_t nblas, const rt_instance *inst,
                            int32_t ninst, uint32_t flags, rt_scene **out, bool any = false) {
  if (!blas || !inst || !out) return set_err(RT_E_INVALID, std::string(who) + ": NULL argument");
  *out = nullptr;
  if (flags & ~RT_INSTANCED_TLAS) return set_err(RT_E_INVALID, std::string(who) + ": unknown flag bits");
  if (nblas < 1 || ninst < 1) return set_err(RT_E_INVALID, std::string(who) + ": nblas and ninst must be at least 1");
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  int32_t maxd = 1;
  bool mixed = false;
  for (int32_t j = 0; j < nblas; ++j) {
    if (!blas[j]) return set_err(RT_E_INVALID, std::string(who) + ": BLAS " + std::to_string(j) + " is NULL");
    const int kind = blas[j]->info.kind;
    if (any && (kind == RT_SCENE_GRID || kind == RT_SCENE_OCTREE))
      mixed = true;
    else if (kind != RT_SCENE_MESH)
      return set_err(RT_E_STATE, std::string(who) + ": BLAS " + std::to_string(j) +
                                     (any ? " is not a mesh, grid or octree scene" : " is not a mesh scene"));
    if (blas[j]->device != dev)
      return set_err(RT_E_INVALID, std::string(who) + ": BLAS " + std::to_string(j) + " lives on device " +
                                       std::to_string(blas[j]->device) + ", the current device is " + std::to_string(dev));
    maxd = std::max(maxd, blas[j]->info.maxd);  // (a grid keeps the default 1: it has no stack)
  }
  if (mixed) maxd = std::max(maxd, 4);  // the smallest slot option (rt_dispatch.h) when only grids are there
  std::vector<rti::InstRec> recs((size_t)ninst);
  for (int32_t i = 0; i < ninst; ++i)
    if (int rc = instance_record(inst[i], nblas, i, who, recs[(size_t)i])) return rc;
  std::vector<MeshDev> tab;
  std::vector<rti::BlasRec> mtab;
  for (int32_t j = 0; j < nblas; ++j) {
    if (mixed)
      mtab.push_back(blas_rec(blas[j]));
    else
      tab.push_back(mesh_dev(blas[j]));
  }
  rt_scene *s = nullptr;
  if (int rc = new_scene(&s)) return rc;
  s->info.kind = RT_SCENE_INSTANCED;
  s->info.maxd = maxd;  // the LDS stack of the deepest bottom-level tree
  s->inst.n = ninst;
  s->inst.blas.assign(blas, blas + nblas);
  for (int32_t j = 0; j < nblas; ++j) s->inst.blas_seen.push_back(blas[j]->info.version);
  int rc = s->inst.recs.upload(recs.data(), recs.size(), s->info.dev_bytes);
  if (!rc) rc = mixed ? s->inst.mixed.upload(mtab.data(), mtab.size(), s->info.dev_bytes)
                      : s->inst.tab.upload(tab.data(), tab.size(), s->info.dev_bytes);
  if (!rc && (flags & RT_INSTANCED_TLAS)) {
    // the matrices as given, the node array zeroed (node 0 and the pad words
    // stay zero), every leaf (the empty ones past ninst too) and the inner
    // nodes by the kernels that also serve the updates; done when this returns
    std::vector<float> xf(12 * (size_t)ninst);
    for (int32_t i = 0; i < ninst; ++i) std::memcpy(&xf[12 * (size_t)i], inst[i].xform, sizeof inst[i].xform);
    s->inst.tlas_leaves = rtt::leaf_count(ninst);
    rc = s->inst.xform.upload(xf.data(), xf.size(), s->info.dev_bytes);
    if (!rc) rc = s->inst.tlas.upload(nullptr, 2 * (size_t)s->inst.tlas_leaves, s->info.dev_bytes);
    if (!rc) {
      hipError_t e = hipMemset(s->inst.tlas.p, 0, 2 * (size_t)s->inst.tlas_leaves * sizeof(rtt::TNode));
      if (e == hipSuccess) rc = tlas_update(s, 0, s->inst.tlas_leaves, nullptr, -1, nullptr);
      if (e == hipSuccess && !rc) e = hipStreamSynchronize(nullptr);
      if (e != hipSuccess) rc = set_err(RT_E_DEVICE, rterr::hip_fail((std::string(who) + ": top-level tree").c_str(), e));
    }
  }
  if (rc) {
    rt_scene_destroy(s);
    return rc;
  }
  *out = s;
  return RT_OK;
}

int rt_scene_create_instanced(rt_scene *const *blas, int32_t nblas, const rt_instance *inst, int32_t ninst,
                              rt_scene **out) {
  return create_instanced("rt_scene_create_instanced", blas, nblas, inst, ninst, 0u, out);
}

int rt_scene_create_instanced_ex(rt_scene *const *blas, int32_t nblas, const rt_instance *inst, int32_t ninst,
                                 uint32_t flags, rt_scene **out) {
  return create_instanced("rt_scene_create_instanced_ex", blas, nblas, inst, ninst, flags, out);
}

int rt_scene_create_instanced_any(rt_scene *const *blas, int32_t nblas, const rt_instance *inst, int32_t ninst,
                                  uint32_t flags, rt_scene **out) {
  return create_instanced("rt_scene_create_instanced_any", blas, nblas, inst, ninst, flags, out, true);
}

int rt_scene_update_instances(rt_scene *s, int32_t first, int32_t count, const rt_instance *inst) {
  const char *who = "rt_scene_update_instances";
  if (int rc = instance_range(s, first, count, who)) return rc;
  if (!inst) return set_err(RT_E_INVALID, std::string(who) + ": instance pointer is NULL");
  if (count == 0) return RT_OK;
  std::vector<rti::InstRec> recs((size_t)count);
  for (int32_t i = 0; i < count; ++i)
    if (int rc = instance_record(inst[i], (int32_t)s->inst.blas.size(), (int64_t)first + i, who, recs[(size_t)i])) return rc;
  int prev = 0;
  HIP_TRY(hipGetDevice(&prev));
  HIP_TRY(hipSetDevice(s->device));
  hipError_t e = rtdma::h2d(s->inst.recs.p + first, recs.data(), recs.size() * sizeof(rti::InstRec), nullptr);
  int rc = RT_OK;
  if (e == hipSuccess && s->inst.tlas.p) {  // the matrices as given, then the leaves and the tree; done on return
    std::vector<float> xf(12 * (size_t)count);
    for (int32_t i = 0; i < count; ++i) std::memcpy(&xf[12 * (size_t)i], inst[i].xform, sizeof inst[i].xform);
    e = rtdma::h2d(s->inst.xform.p + 12 * (size_t)first, xf.data(), xf.size() * sizeof(float), nullptr);
    if (e == hipSuccess) rc = tlas_update(s, first, count, nullptr, -1, nullptr);
    if (e == hipSuccess && !rc) e = hipStreamSynchronize(nullptr);
  }
  HIP_NOTE(hipSetDevice(prev));
  if (e != hipSuccess) return set_err(RT_E_DEVICE, rterr::hip_fail("rt_scene_update_instances: upload", e));
  return rc;
}

int rt_scene_update_instances_device(rt_scene *s, int32_t first, int32_t count, const float *d_xform12,
                                     void *stream) {
  const char *who = "rt_scene_update_instances_device";
  if (int rc = instance_range(s, first, count, who)) return rc;
  if (!d_xform12) return set_err(RT_E_INVALID, std::string(who) + ": matrix pointer is NULL");
  if (count == 0) return RT_OK;
  if (int rc = rti::pose_launch(s->inst.recs.p, first, count, d_xform12, (hipStream_t)stream)) return rc;
  // a top-level tree: the box kernel takes the matrices over and redoes these
  // leaves behind the pose kernel, then the refit; still only launches
  return s->inst.tlas.p ? tlas_update(s, first, count, d_xform12, -1, (hipStream_t)stream) : RT_OK;
}

int rt_scene_get_tlas(const rt_scene *s, float *leaf_boxes, float *node_boxes, int32_t *leaves) {
  const char *who = "rt_scene_get_tlas";
  if (!s) return set_err(RT_E_INVALID, std::string(who) + ": scene is NULL");
  if (s->info.kind != RT_SCENE_INSTANCED || !s->inst.tlas.p)
    return set_err(RT_E_STATE, std::string(who) + ": not an instanced scene created with RT_INSTANCED_TLAS");
  const int32_t P = s->inst.tlas_leaves;
  if (leaves) *leaves = P;
  if (!leaf_boxes && !node_boxes) return RT_OK;
  std::vector<rtt::TNode> nd(2 * (size_t)P);
  int prev = 0;
  HIP_TRY(hipGetDevice(&prev));
  HIP_TRY(hipSetDevice(s->device));
  hipError_t e = hipDeviceSynchronize();  // updates queued on any stream
  if (e == hipSuccess) e = rtdma::d2h(nd.data(), s->inst.tlas.p, nd.size() * sizeof(rtt::TNode), nullptr);
  HIP_NOTE(hipSetDevice(prev));
  if (e != hipSuccess) return set_err(RT_E_DEVICE, rterr::hip_fail(who, e));
  if (leaf_boxes)
    for (int32_t i = 0; i < s->inst.n; ++i) std::memcpy(leaf_boxes + 6 * (size_t)i, nd[(size_t)P + i].b, 6 * sizeof(float));
  if (node_boxes)
    for (int32_t n = 0; n < 2 * P; ++n) std::memcpy(node_boxes + 6 * (size_t)n, nd[(size_t)n].b, 6 * sizeof(float));
  return RT_OK;
}

int rt_scene_get_instances(const rt_scene *s, int32_t first, int32_t count, rt_instance *inst, float *inv12,
                           uint32_t *skipped) {
  if (int rc = instance_range(s, first, count, "rt_scene_get_instances")) return rc;
  if (count == 0) return RT_OK;
  std::vector<rti::InstRec> recs((size_t)count);
  int prev = 0;
  HIP_TRY(hipGetDevice(&prev));
  HIP_TRY(hipSetDevice(s->device));
  hipError_t e = hipDeviceSynchronize();  // pose updates queued on any stream
  if (e == hipSuccess) e = rtdma::d2h(recs.data(), s->inst.recs.p + first, recs.size() * sizeof(rti::InstRec), nullptr);
  HIP_NOTE(hipSetDevice(prev));
  if (e != hipSuccess) return set_err(RT_E_DEVICE, rterr::hip_fail("rt_scene_get_instances", e));
  for (int32_t i = 0; i < count; ++i) {
    const rti::InstRec &r = recs[(size_t)i];
    if (inst) {
      inst[i].blas = r.blas;
      inst[i].flags = r.flags;
      for (float &x : inst[i].xform) x = 0.0f;
      if (!r.skipped) (void)rti::affine_inverse(r.m, inst[i].xform);
    }
    if (inv12) std::memcpy(inv12 + 12 * (size_t)i, r.m, sizeof r.m);
    if (skipped) skipped[i] = r.skipped;
  }
  return RT_OK;
}

int rt_scene_update_vertices_device(rt_scene *s, const float *d_vpos4, int64_t nverts, void *stream) {
  if (int rc = check_update(s, d_vpos4, nverts, "rt_scene_update_vertices_device")) return rc;
  return update_vertices_device(s, d_vpos4, (hipStream_t)stream);
}

int rt_scene_update_vertices(rt_scene *s, const float *vpos4, int64_t nverts) {
  if (int rc = check_update(s, vpos4, nverts, "rt_scene_update_vertices")) return rc;
  int prev = 0;
  HIP_TRY(hipGetDevice(&prev));
  HIP_TRY(hipSetDevice(s->device));
  int rc = RT_OK;
  if (const hipError_t e = rtdma::h2d(s->dyn.vstage.p, vpos4, 16 * (size_t)nverts, nullptr))
    rc = set_err(RT_E_DEVICE, rterr::hip_fail("rt_scene_update_vertices: vertex upload", e));
  if (!rc) rc = update_vertices_device(s, s->dyn.vstage.p, nullptr);
  HIP_NOTE(hipSetDevice(prev));
  return rc;
}

// Diagnostic (not part of include/rtamd.h): a mesh scene's device tree, as it
// is now: n_inner GNode records (224 bytes each) and n_tris GTri records (48
// bytes each). Two-call protocol: with nodes224 = tris48 = NULL only the counts
// are returned; else *n_inner / *n_tris are the buffers' capacities.
int rtx_scene_mesh_download(rt_scene *s, void *nodes224, int64_t *n_inner, void *tris48, int64_t *n_tris) {
  if (!s || !n_inner || !n_tris) return set_err(RT_E_INVALID, "rtx_scene_mesh_download: NULL argument");
  if (s->info.kind != RT_SCENE_MESH) return set_err(RT_E_STATE, "rtx_scene_mesh_download: not a mesh scene");
  if (nodes224 || tris48) {
    if (!nodes224 || !tris48 || *n_inner < (int64_t)s->mesh.n_inner || *n_tris < (int64_t)s->mesh.n_tris)
      return set_err(RT_E_INVALID, "rtx_scene_mesh_download: buffers too small");
    int prev = 0;
    HIP_TRY(hipGetDevice(&prev));
    HIP_TRY(hipSetDevice(s->device));
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess) e = rtdma::d2h(nodes224, s->geo.nodes.p, (size_t)s->mesh.n_inner * sizeof(rtl::GNode), nullptr);
    if (e == hipSuccess) e = rtdma::d2h(tris48, s->geo.tris.p, (size_t)s->mesh.n_tris * sizeof(rtl::GTri), nullptr);
    HIP_NOTE(hipSetDevice(prev));
    if (e != hipSuccess) return set_err(RT_E_DEVICE, rterr::hip_fail("rtx_scene_mesh_download", e));
  }
  *n_inner = s->mesh.n_inner;
  *n_tris = s->mesh.n_tris;
  return RT_OK;
}

// Diagnostic (not part of include/rtamd.h): the constants the host keeps of a
// mesh scene: root_box[6], the root's child boxes root_child[48], dmax2.
int rtx_scene_mesh_constants(const rt_scene *s, float root_box[6], float root_child[48], float *dmax2) {
  if (!s) return set_err(RT_E_INVALID, "rtx_scene_mesh_constants: scene is NULL");
  if (s->info.kind != RT_SCENE_MESH) return set_err(RT_E_STATE, "rtx_scene_mesh_constants: not a mesh scene");
  if (root_box) std::memcpy(root_box, s->mesh.root_box, sizeof s->mesh.root_box);
  if (root_child) std::memcpy(root_child, s->mesh.root_child, sizeof s->mesh.root_child);
  if (dmax2) *dmax2 = s->mesh.dmax2;
  return RT_OK;
}

int rt_scene_get_plane(const rt_scene *s, int *enabled, float normal[3], float *offset) {
  if (!s) return set_err(RT_E_INVALID, "scene is NULL");
  if (enabled) *enabled = s->info.plane.on;
  if (normal) { normal[0] = s->info.plane.n.x; normal[1] = s->info.plane.n.y; normal[2] = s->info.plane.n.z; }
  if (offset) *offset = s->info.plane.off;
  return RT_OK;
}

int rt_scene_set_plane(rt_scene *s, int enabled, const float normal[3], float offset) {
  if (!s) return set_err(RT_E_INVALID, "scene is NULL");
  PlaneDev &p = s->info.plane;
  p.on = enabled ? 1 : 0;
  if (!enabled) return RT_OK;
  if (!normal) return set_err(RT_E_INVALID, "normal is NULL");
  // Plane(normal, offset) + recalcBasis (raytracing.hpp:121-124, 169-179)
  const float n[3] = {normal[0], normal[1], normal[2]};
  const float a[3] = {std::fabs(n[0]), std::fabs(n[1]), std::fabs(n[2])};
  float b1[3];
  if (a[0] > a[1] && a[0] > a[2]) { b1[0] = n[1]; b1[1] = -n[0]; b1[2] = 0; }
  else { b1[0] = 0; b1[1] = n[2]; b1[2] = -n[1]; }
  auto nrm = [](float v[3]) {
    const float l = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    v[0] = v[0] / l; v[1] = v[1] / l; v[2] = v[2] / l;
  };
  nrm(b1);
  float b2[3] = {b1[1] * n[2] - b1[2] * n[1], b1[2] * n[0] - b1[0] * n[2], b1[0] * n[1] - b1[1] * n[0]};
  nrm(b2);
  p.n = f3{n[0], n[1], n[2]};
  p.off = offset;
  p.b1 = f3{b1[0], b1[1], b1[2]};
  p.b2 = f3{b2[0], b2[1], b2[2]};
  return RT_OK;
}

int rt_scene_kind(const rt_scene *s) { return s ? s->info.kind : RT_E_INVALID; }
int64_t rt_scene_device_bytes(const rt_scene *s) { return s ? s->info.dev_bytes : 0; }

int rt_scene_bvh_stats(const rt_scene *s, int64_t *nodes, int64_t *inner, int32_t *max_depth) {
  if (!s) return set_err(RT_E_INVALID, "scene is NULL");
  if (s->info.kind != RT_SCENE_MESH && s->info.kind != RT_SCENE_OCTREE) return set_err(RT_E_STATE, "not a tree scene");
  if (nodes) *nodes = s->mesh.host_nodes;
  if (inner) *inner = s->mesh.host_inner;
  if (max_depth) *max_depth = s->info.kind == RT_SCENE_MESH ? s->mesh.depth : s->oct.depth;
  return RT_OK;
}

int rt_scene_destroy(rt_scene *s) {
  if (!s) return RT_OK;
  int prev = 0;
  HIP_NOTE(hipGetDevice(&prev));
  HIP_NOTE(hipSetDevice(s->device));
  // the scene's own copy/render streams drain before anything they may still
  // read or write is freed (rt_render returns only after both, but a failed
  // call or a caller-stream launch may not have)
  for (const rtmem::Stream &x : s->drop.xs)
    if (x.s) HIP_NOTE(hipStreamSynchronize(x.s));
  if (s->sched.os.s) HIP_NOTE(hipStreamSynchronize(s->sched.os.s));
  delete s;
  HIP_NOTE(hipSetDevice(prev));
  return RT_OK;
}

// Diagnostic (not part of include/rtamd.h): the live owners of rt_mem.h, in
// the order device arrays, pinned host blocks, events, streams.
int rtx_live_resources(int64_t out[4]) {
  if (!out) return set_err(RT_E_INVALID, "rtx_live_resources: out is NULL");
  for (int k = 0; k < 4; ++k) out[k] = rtmem::g_live[k].load(std::memory_order_relaxed);
  return RT_OK;
}

// Builder of this thread's last BVH: 1 host, 2 device, 3 host after a failed
// device build (AUTO mode falls back; see rtx_bvh_inject_failure)
int rtx_bvh_last_builder(void) { return t_bvh_last; }

// Diagnostic: force grid layouts / address paths (g_grid_force bits). Not part
// of include/rtamd.h.
int rtx_set_grid_force(int flags) {
  if (flags < 0 || flags > 3) return set_err(RT_E_INVALID, "grid force flags must be 0..3");
  g_grid_force = flags;
  return RT_OK;
}

// Diagnostic (not part of include/rtamd.h; host only, touches no device): the
// kernel template arguments the scene dispatch (rt_dispatch.h) picks for a
// scene of `kind` with `maxd` stack slots and, for a grid, the launch mode
// `gmode`: out[0] = the adapter's scene kind, out[1] = the slot count N,
// out[2] = the adapter's variant (GridS: kMode, OctS: PACK, MeshS: 0).
// RT_E_STATE for a kind without an adapter (an unknown one, or an instanced
// scene, whose entries branch off ahead of the dispatch).
int rtx_dispatch_probe(int kind, int maxd, int gmode, int out[3]) {
  if (!out) return set_err(RT_E_INVALID, "rtx_dispatch_probe: out is NULL");
  if (!dispatch_types(kind, maxd, gmode, [&](auto adapter, auto slots) {
        using A = typename decltype(adapter)::type;
        out[0] = AdapterInfo<A>::kKind;
        out[1] = decltype(slots)::value;
        out[2] = AdapterInfo<A>::kVariant;
      }))
    return set_err(RT_E_STATE, "rtx_dispatch_probe: no scene adapter for this scene kind");
  return RT_OK;
}

// Diagnostic (not part of include/rtamd.h; host only, touches no device): what
// rt_scene_create_octree makes of `count` 36-byte nodes before it uploads
// anything. rth::flatten_octree's verdict is the return value (RT_E_INVALID
// with its message); on success *max_depth is the tree's depth, *maxd the
// stack slot count pick_maxd grants it (what the scene would carry into the
// dispatch), and words, if given, receives the count rtl::OctWord {child,
// masks} pairs as 2 * count uint32.
int rtx_octree_flatten(const void *nodes36, int64_t count, int32_t *max_depth, int32_t *maxd, uint32_t *words) {
  if (!nodes36 || count <= 0) return set_err(RT_E_INVALID, "empty octree");
  rth::OctGpu g;
  std::string err;
  if (!rth::flatten_octree((const uint8_t *)nodes36, count, g, err)) return set_err(RT_E_INVALID, err);
  int32_t m = 0;
  if (int rc = pick_maxd(g.max_depth, m)) return rc;
  if (max_depth) *max_depth = g.max_depth;
  if (maxd) *maxd = m;
  if (words)
    for (int64_t i = 0; i < count; ++i) {
      words[2 * i] = g.child[(size_t)i].child;
      words[2 * i + 1] = g.child[(size_t)i].masks;
    }
  return RT_OK;
}

// Diagnostic (not part of include/rtamd.h): the {child, masks} pairs of an
// octree scene as the device holds them now, after a wait for it, as 2 uint32
// per node for the scene's first `count` nodes; count must not pass what the
// scene holds (rt_scene_octree_status).
int rtx_scene_octree_words(rt_scene *s, uint32_t *words, int64_t count) {
  if (!words || count < 0) return set_err(RT_E_INVALID, "rtx_scene_octree_words: bad arguments");
  uint32_t st[2];
  std::vector<rtl::OctWord> w;
  if (int rc = octree_download(s, "rtx_scene_octree_words", st, w, nullptr)) return rc;
  if (count > (int64_t)st[0]) return set_err(RT_E_INVALID, "rtx_scene_octree_words: count passes the scene's nodes");
  for (int64_t i = 0; i < count; ++i) {
    words[2 * i] = w[(size_t)i].child;
    words[2 * i + 1] = w[(size_t)i].masks;
  }
  return RT_OK;
}

}  // extern "C"

namespace rti {

uint64_t scene_version(const rt_scene *s) { return s ? s->info.version : 0; }

// A replica (rt_scene_replicate) of mesh scene `src` brought up to src's last
// update: nodes and triangles copied device to device (the sizes never
// change), the three host constants taken over. Blocking; the caller has
// drained the streams that use the replica.
int scene_refresh_replica(rt_scene *rep, const rt_scene *src) {
  if (!rep || !src || rep->info.kind != src->info.kind) return set_err(RT_E_INVALID, "scene_refresh_replica: bad arguments");
  if (rep->info.version == src->info.version || src->info.kind != RT_SCENE_MESH) return RT_OK;
  if (rep->mesh.n_inner != src->mesh.n_inner || rep->mesh.n_tris != src->mesh.n_tris)
    return set_err(RT_E_STATE, "scene_refresh_replica: the replica is not of this scene");
  if (src->mesh.n_inner)
    HIP_TRY(hipMemcpyPeer(rep->geo.nodes.p, rep->device, src->geo.nodes.p, src->device, (size_t)src->mesh.n_inner * sizeof(rtl::GNode)));
  if (src->mesh.n_tris)
    HIP_TRY(hipMemcpyPeer(rep->geo.tris.p, rep->device, src->geo.tris.p, src->device, (size_t)src->mesh.n_tris * sizeof(rtl::GTri)));
  std::memcpy(rep->mesh.root_box, src->mesh.root_box, sizeof rep->mesh.root_box);
  std::memcpy(rep->mesh.root_child, src->mesh.root_child, sizeof rep->mesh.root_child);
  rep->mesh.dmax2 = src->mesh.dmax2;
  rep->info.version = src->info.version;
  return RT_OK;
}

}  // namespace rti
