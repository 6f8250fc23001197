// rt_scene.h -- struct rt_scene (the opaque scene of include/rtamd.h) and what
// the units behind the scene entries need from one another: rt_scene.hip
// (creation, update, destruction, the device views of a scene), rt_device.hip
// (the renderer and the ray queries) and rt_dropin.hip (rt_render on host
// buffers).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/rtamd.h"
#include "rt_error.h"
#include "rt_frame.h"
#include "rt_instances.h"
#include "rt_layout.h"
#include "rt_scenes.h"

struct rt_scene {
  int kind = 0;
  int device = 0;
  int32_t maxd = 1;  // LDS stack frames the kernel is instantiated for
  // mesh
  rtl::GNode *d_nodes = nullptr;
  rtl::GTri *d_tris = nullptr;
  uint32_t root = rtl::kInvalidChild;
  float root_box[6] = {0, 0, 0, 0, 0, 0};
  // the root node's eight child boxes (xMin xMax yMin yMax zMin zMax each; an
  // empty slot is all +inf): the bounds a camera must not sit on (cull_rect)
  float root_child[48] = {};
  int64_t host_nodes = 0, host_inner = 0;
  uint32_t n_inner = 0;  // inner nodes on the device
  float dmax2 = 0.0f;    // MeshDev::dmax2 (mesh_dmax2; 0: every ray takes the division)
  int32_t bvh_depth = 0;
  uint32_t n_tris = 0;   // triangle slots in d_tris (8 zero triangles follow)
  uint32_t root_nchild = 0;  // children of an inner root (slots 0 .. root_nchild-1)
  // a mesh created with RT_MESH_DYNAMIC (rt_scene_update_vertices*): the
  // creation index array and a vertex staging buffer on the device, the first
  // node index of every depth level (+ the node count), the edge-bound word of
  // tri_edge_bound_kernel and the pinned host words the update reads back
  // (48 root child box floats, then the edge bound)
  bool dynamic = false;
  int64_t nverts = 0;
  uint32_t *d_idx = nullptr;
  float *d_vstage = nullptr;
  uint32_t *d_edge = nullptr;
  uint32_t *h_refit = nullptr;
  std::vector<uint32_t> level_first;
  int64_t dyn_bytes = 0;  // what `dynamic` added to dev_bytes
  uint64_t version = 0;   // counts the updates (rt_multi re-copies its replicas when it moves)
  // grid
  float *d_vals = nullptr;
  uint32_t size[3] = {0, 0, 0};
  bool grid_bricked = false;  // device layout (rt_scenes.h GridDev): bricked, or the reference's linear
  // octree
  rtl::OctWord *d_child = nullptr;
  rtl::OctVals *d_ovals = nullptr;
  int32_t oct_depth = 0;
  // instanced (RT_SCENE_INSTANCED): the instance records and the table of the
  // bottom-level scenes' MeshDev on the device; the scenes themselves (not
  // owned) and the update counter each table entry was written from. Nothing
  // here depends on a pose.
  rti::InstRec *d_inst = nullptr;
  rtd::MeshDev *d_blas = nullptr;
  int32_t ninst = 0;
  std::vector<rt_scene *> blas;
  std::vector<uint64_t> blas_seen;
  // a mixed scene (rt_scene_create_instanced_any with a grid or an octree among
  // its bottom-level scenes): the table of tagged records instead of d_blas,
  // which stays NULL (rt_instances_mixed.hip)
  rti::BlasRec *d_mixed = nullptr;
  // created with RT_INSTANCED_TLAS: the top-level tree (2 * tlas_leaves nodes,
  // rt_tlas.h) and the object-to-world matrices (12 floats per instance) its
  // leaves are recomputed from when a BLAS's root box moves. Both live on the
  // device only: the host keeps nothing that depends on a pose.
  rtt::TNode *d_tlas = nullptr;
  float *d_xform = nullptr;
  int32_t tlas_leaves = 0;
  rtd::PlaneDev plane{};
  int64_t dev_bytes = 0;
  // cached buffers for host-buffer entry points
  uint32_t *d_color = nullptr;
  float *d_t = nullptr;
  size_t fb_cap = 0;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  hipEvent_t ev_host = nullptr;  // rt_render's pageable cleared frame: the spans are on the host
  hipStream_t xs[2] = {nullptr, nullptr};  // rt_render: colour / t copy streams (render on xs[0])
  hipEvent_t xev = nullptr;
  // rt_render: FrameArgs::hit_box of its frame (4 words) and a pinned,
  // mapped host copy (h_hit_box_dev: its device address, box_out_kernel)
  int32_t *d_hit_box = nullptr;
  int32_t *h_hit_box = nullptr;
  int32_t *h_hit_box_dev = nullptr;
  // the pageable zero-copy path: FrameArgs::row_span (2 words per row) and its
  // pinned, mapped host copy, for span_cap rows
  int32_t *d_row_span = nullptr;
  int32_t *h_row_span = nullptr;
  int32_t *h_row_span_dev = nullptr;
  int32_t span_cap = 0;
  // rt_render's staging frame for a cleared frame on pageable buffers: pinned
  // host memory the kernel stores its hits into (zero-copy), kept cleared
  rtdma::HostStage stage{hipHostMallocDefault};
  // cost-ordered block schedule (see launch_render), double-buffered: frame k
  // of the scene's one-frame kernel records its tiles' costs into d_cost[k & 1]
  // and dispatches in the order d_order[k & 1] that frame k - 2's costs gave;
  // frame k's own order is computed by order_kernel on the side stream
  // sched_os as soon as frame k is done (frame_ev), beside frame k + 1, and
  // ord_ev[k & 1] marks it done. sched_key[b] = the grid (gx << 16 | gy) whose
  // order d_order[b] holds (0: none). sched_on = false renders in plain
  // blockIdx order
  uint32_t *d_cost[2] = {nullptr, nullptr};
  uint32_t *d_order[2] = {nullptr, nullptr};
  uint32_t sched_key[2] = {0, 0};
  bool ord_rec[2] = {false, false};
  int sched_par = 0;
  uint32_t sched_cap = 0;
  bool sched_on = true;
  bool coop = true;  // mesh primary rays: cooperative tail (rtx_set_coop)
  hipStream_t last_stream = nullptr;   // stream of the previous frame (scheduled or not)
  hipStream_t sched_os = nullptr;      // side stream of the order kernels
  hipEvent_t ord_ev[2] = {nullptr, nullptr};
  hipEvent_t frame_ev = nullptr;
  bool pump_on = false;  // primary-ray batches on the ray pump (rtx_set_pump)
};

namespace rti {

// ---- rt_scene.hip: the device views of a scene ------------------------------
rtd::MeshDev mesh_dev(const rt_scene *s);
rtd::GridDev grid_dev(const rt_scene *s);
// kGridBuf / kGridBricked bits of a grid scene's launches (rt_scenes.h)
int grid_mode(const rt_scene *s, const rtd::GridDev &gd);
// the entries that render frames or copy a scene take no instanced scene
int no_instanced(const rt_scene *s, const char *who);
// what maintains the top-level tree of an instanced scene that has one
rti::TlasArgs tlas_args(const rt_scene *s);
// What every ray query of an instanced scene queues ahead of its kernel
// (rt_trace_rays_device, rt_shade_rays_device): the table entry of a
// bottom-level scene refitted since the entry was written is rewritten in
// stream order, and with a top-level tree that BLAS's leaf boxes and the tree
// above them follow. Only launches; no host wait.
int instanced_sync(rt_scene *s, hipStream_t stream);

// ---- rt_device.hip: the renderer --------------------------------------------
// the scene's cached device frame for px pixels / its timing events
int ensure_fb(rt_scene *s, size_t px);
int ensure_events(rt_scene *s);
// one frame's arguments from the C ABI's (checks flags and tile; sets the tile
// cull's rectangle and the fast eye-ray flag)
int fill_frame(FrameArgs &fa, const rt_scene *s, const rt_render_params *p, uint32_t *c, float *t, int32_t W,
               int32_t H, uint32_t flags, const rt_tile *tile);
// the one-frame kernel (diag 1 / 2: its counting / stamping variant into
// `counters`; sched: the cost-ordered block schedule may apply)
int launch_render(rt_scene *s, const FrameArgs &fa, hipStream_t stream, unsigned long long *counters = nullptr,
                  int diag = 0, bool sched = true);
// one launch for n <= kMaxBatch frames of equal size / tile
int launch_batch(rt_scene *s, FrameBatch &fb, int n, hipStream_t stream);


}  // namespace rti
