// rt_abi_host.hip -- the entry points of include/rtamd.h that only check their
// arguments and forward to the host code (rth::, rt_host.cpp): loaders, the
// camera, image and mesh output, tile arithmetic. No kernel, no rt_scene.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rtamd.h"
#include "rt_error.h"
#include "rt_host.h"

extern "C" {

int rt_load_obj(const char *path, int scale, float *vpos4, int64_t *nverts, uint32_t *idx,
                int64_t *nidx) {
  if (!path || !nverts || !nidx) return set_err(RT_E_INVALID, "NULL argument");
  rth::Mesh m;
  std::string err;
  if (!rth::load_obj(path, scale != 0, m, err)) return set_err(RT_E_IO, err);
  const int64_t nv = (int64_t)m.vpos4.size() / 4, ni = (int64_t)m.idx.size();
  if (vpos4 || idx) {
    if (*nverts < nv || *nidx < ni) return set_err(RT_E_INVALID, "buffers too small");
    if (vpos4) std::memcpy(vpos4, m.vpos4.data(), m.vpos4.size() * 4);
    if (idx) std::memcpy(idx, m.idx.data(), m.idx.size() * 4);
  }
  *nverts = nv;
  *nidx = ni;
  return RT_OK;
}

int rt_load_grid(const char *path, uint32_t size[3], float *values) {
  if (!path || !size) return set_err(RT_E_INVALID, "NULL argument");
  std::vector<float> v;
  uint32_t sz[3];
  std::string err;
  if (!rth::load_grid(path, sz, v, err)) return set_err(RT_E_IO, err);
  if (values) {
    if ((uint64_t)size[0] * size[1] * size[2] < v.size()) return set_err(RT_E_INVALID, "buffer too small");
    std::memcpy(values, v.data(), v.size() * 4);
  }
  size[0] = sz[0]; size[1] = sz[1]; size[2] = sz[2];
  return RT_OK;
}

int rt_load_octree(const char *path, int64_t *count, void *nodes36) {
  if (!path || !count) return set_err(RT_E_INVALID, "NULL argument");
  std::vector<uint8_t> v;
  std::string err;
  if (!rth::load_octree(path, v, err)) return set_err(RT_E_IO, err);
  const int64_t n = (int64_t)v.size() / 36;
  if (nodes36) {
    if (*count < n) return set_err(RT_E_INVALID, "buffer too small");
    std::memcpy(nodes36, v.data(), v.size());
  }
  *count = n;
  return RT_OK;
}

int rt_camera(const float pos[3], const float target[3], const float up[3], float fovy_deg,
              float aspect, float znear, float zfar, float view_inv[16], float proj_inv[16]) {
  if (!pos || !target || !up || !view_inv || !proj_inv) return set_err(RT_E_INVALID, "NULL argument");
  rth::camera_matrices(pos, target, up, fovy_deg, aspect, znear, zfar, view_inv, proj_inv);
  return RT_OK;
}

int64_t rt_tile_pixels(int32_t W, int32_t H, const rt_tile *tile) {
  if (W <= 0 || H <= 0) return 0;
  if (!tile || tile->num_ranks <= 1) return (int64_t)W * H;
  if (tile->band_rows <= 0) return 0;
  int64_t rows = 0;
  const int32_t nb = (H + tile->band_rows - 1) / tile->band_rows;
  for (int32_t b = tile->rank; b < nb; b += tile->num_ranks)
    rows += std::min(tile->band_rows, H - b * tile->band_rows);
  return rows * W;
}

// ---- orbit camera + image output (host-only; rt_host.cpp) ----------------
static_assert(sizeof(rt_camera_state) == sizeof(rth::CamState), "camera state layout");
#define CAM(c) (*reinterpret_cast<rth::CamState *>(c))
int rt_camera_init(const float pos[3], const float target[3], const float up[3], rt_camera_state *c) {
  if (!pos || !target || !up || !c) return set_err(RT_E_INVALID, "bad arguments");
  rth::cam_init(CAM(c), pos, target, up);
  return RT_OK;
}
int rt_camera_rotate(rt_camera_state *c, float dx, float dy) {
  if (!c) return set_err(RT_E_INVALID, "camera is NULL");
  rth::cam_rotate(CAM(c), dx, dy);
  return RT_OK;
}
int rt_camera_reset_position(rt_camera_state *c, const float pos[3]) {
  if (!c || !pos) return set_err(RT_E_INVALID, "bad arguments");
  rth::cam_reset_position(CAM(c), pos);
  return RT_OK;
}
int rt_camera_reset_target(rt_camera_state *c, const float target[3]) {
  if (!c || !target) return set_err(RT_E_INVALID, "bad arguments");
  rth::cam_reset_target(CAM(c), target);
  return RT_OK;
}
int rt_camera_set_lock_up(rt_camera_state *c, int on) {
  if (!c) return set_err(RT_E_INVALID, "camera is NULL");
  rth::cam_set_lock_up(CAM(c), on != 0);
  return RT_OK;
}
int rt_camera_zoom(rt_camera_state *c, float wheel) {
  if (!c) return set_err(RT_E_INVALID, "camera is NULL");
  rth::cam_zoom(CAM(c), wheel);
  return RT_OK;
}
int rt_camera_basis(const rt_camera_state *c, float up[3], float right[3], float forward[3]) {
  if (!c) return set_err(RT_E_INVALID, "camera is NULL");
  rth::cam_basis(*reinterpret_cast<const rth::CamState *>(c), up, right, forward);
  return RT_OK;
}
int rt_camera_view_inverse(const rt_camera_state *c, float view_inv[16]) {
  if (!c || !view_inv) return set_err(RT_E_INVALID, "bad arguments");
  rth::cam_view_inverse(*reinterpret_cast<const rth::CamState *>(c), view_inv);
  return RT_OK;
}
#undef CAM
int rt_write_png(const char *path, const uint32_t *color, int32_t W, int32_t H) {
  std::string err;
  if (!rth::write_png(path, color, W, H, err)) return set_err(RT_E_IO, err);
  return RT_OK;
}

int rt_save_obj(const char *path, const float *vpos4, int64_t nverts, const uint32_t *idx, int64_t nidx,
                const float *vnorm4, const float *vtex2) {
  std::string err;
  if (nverts < 0 || nidx < 0) return set_err(RT_E_INVALID, "bad counts");
  if (!rth::save_obj(path, vpos4, nverts, idx, nidx, vnorm4, vtex2, err))
    return set_err(err.rfind("cannot", 0) == 0 || err == "short write" ? RT_E_IO : RT_E_INVALID, err);
  return RT_OK;
}

// The host restatement of the refit, no GPU: the host builder's tree of the
// mesh (rth::build_bvh8) in device layout -- n_inner GNode records of 224 bytes,
// n_tris GTri records of 48 bytes -- refitted to new_vpos4 (rth::refit_bvh8),
// or as built when new_vpos4 is NULL. Two-call protocol: with nodes224 =
// tris48 = NULL only the counts are returned; else *n_inner / *n_tris are the
// buffers' capacities. Not part of include/rtamd.h.
int rtx_bvh_refit_host(const float *vpos4, int64_t nverts, const uint32_t *idx, int64_t nidx, const float *new_vpos4,
                       void *nodes224, int64_t *n_inner, void *tris48, int64_t *n_tris) {
  if (!vpos4 || !idx || !n_inner || !n_tris || nverts <= 0 || nidx <= 0) return set_err(RT_E_INVALID, "bad mesh");
  rth::BVHGpu b;
  std::string err;
  if (!rth::build_bvh8(vpos4, nverts, idx, nidx, b, err, rth::kBvhTris)) return set_err(RT_E_INVALID, err);
  if (nodes224 || tris48) {
    if (!nodes224 || !tris48 || *n_inner < (int64_t)b.nodes.size() || *n_tris < (int64_t)b.tris.size())
      return set_err(RT_E_INVALID, "buffers too small");
    if (new_vpos4) rth::refit_bvh8(b, new_vpos4, idx);
    if (!b.nodes.empty()) std::memcpy(nodes224, b.nodes.data(), b.nodes.size() * sizeof(rtl::GNode));
    if (!b.tris.empty()) std::memcpy(tris48, b.tris.data(), b.tris.size() * sizeof(rtl::GTri));
  }
  *n_inner = (int64_t)b.nodes.size();
  *n_tris = (int64_t)b.tris.size();
  return RT_OK;
}

// The host restatement of the SDF-mesh refit, no GPU: rth::prep_sdf_mesh of
// the mesh -- n_inner GNode records of 224 bytes, n_tri triangle records of 48
// bytes (a.xyz, id | b.xyz, 0 | c.xyz, 0) and 28 floats of pseudonormals per
// ORIGINAL triangle (pn28: nidx / 3 * 28 floats) -- moved to new_vpos4
// (rth::refit_sdf_mesh), or as built when new_vpos4 is NULL. Two-call protocol
// on the counts, as rtx_bvh_refit_host. Not part of include/rtamd.h.
int rtx_sdf_mesh_refit_host(const float *vpos4, int64_t nverts, const uint32_t *idx, int64_t nidx,
                            const float *new_vpos4, void *nodes224, int64_t *n_inner, void *tri48, int64_t *n_tri,
                            float *pn28) {
  if (!vpos4 || !idx || !n_inner || !n_tri || nverts <= 0 || nidx <= 0) return set_err(RT_E_INVALID, "bad mesh");
  rth::SdfMeshHost m;
  rth::SdfTopo topo;
  std::string err;
  if (!rth::prep_sdf_mesh(vpos4, nverts, idx, nidx, m, err, &topo)) return set_err(RT_E_INVALID, err);
  const int64_t ni = (int64_t)m.bvh.nodes.size(), nt = (int64_t)m.bvh.tris.size();
  if (nodes224 || tri48 || pn28) {
    if (!nodes224 || !tri48 || !pn28 || *n_inner < ni || *n_tri < nt) return set_err(RT_E_INVALID, "buffers too small");
    if (new_vpos4) rth::refit_sdf_mesh(m, topo, idx, nidx, new_vpos4);
    if (ni) std::memcpy(nodes224, m.bvh.nodes.data(), (size_t)ni * sizeof(rtl::GNode));
    std::memcpy(tri48, m.tri.data(), m.tri.size() * 4);
    std::memcpy(pn28, m.pn.data(), m.pn.size() * 4);
  }
  *n_inner = ni;
  *n_tri = nt;
  return RT_OK;
}

// The pageable drop-in's host copy (rth::copy_spans) on caller arrays, no GPU:
// span[2y] = first stored column of row y, span[2y+1] = -last (INT32_MAX,
// INT32_MAX: none); threads 0 = the library's default; clear_src != 0: the
// copied spans of the source reset to (0, +inf). Not part of include/rtamd.h.
int rtx_copy_spans(uint32_t *dc, float *dt, uint32_t *sc, float *st, int64_t W, int32_t H, const int32_t *span,
                   int32_t threads, int32_t clear_src) {
  if (!dc || !dt || !sc || !st || !span || W <= 0 || H <= 0) return set_err(RT_E_INVALID, "bad arguments");
  rth::copy_spans(dc, dt, sc, st, W, H, span, threads, clear_src != 0);
  return RT_OK;
}

}  // extern "C"
