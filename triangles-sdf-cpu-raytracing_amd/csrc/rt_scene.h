// rt_scene.h -- struct rt_scene (the opaque scene of include/rtamd.h) and what
// the units behind the scene entries need from one another: rt_scene.hip
// (creation, update, destruction, the device views of a scene), rt_device.hip
// (the renderer and the ray queries) and rt_dropin.hip (rt_render on host
// buffers).
//
// A scene is grouped by what owns what. Its description is plain data
// (rts::Common and one struct per geometry kind): rt_scene_replicate assigns
// it. Everything on the device, in pinned host memory, every event and every
// stream sits in an owner of rt_mem.h inside one of the owning parts below,
// each next to the state that says what it holds. No part lists what it has
// to free: rt_scene_destroy drains the scene's own streams and deletes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/rtamd.h"
#include "rt_error.h"
#include "rt_frame.h"
#include "rt_instances.h"
#include "rt_layout.h"
#include "rt_mem.h"
#include "rt_scenes.h"

namespace rts {

// ---- the description: plain, assignable ------------------------------------
struct Common {
  int kind = 0;
  int32_t maxd = 1;  // LDS stack frames the kernel is instantiated for
  rtd::PlaneDev plane{};
  uint64_t version = 0;   // counts the updates (rt_multi re-copies its replicas when it moves)
  int64_t dev_bytes = 0;  // rt_scene_device_bytes: the geometry, the dynamic part and the instanced tables
  // diagnostic switches
  bool sched_on = true;  // false renders in plain blockIdx order (rts::Schedule)
  bool coop = true;      // mesh primary rays: cooperative tail (rtx_set_coop)
  bool pump_on = false;  // primary-ray batches on the ray pump (rtx_set_pump)
};

struct MeshDesc {
  uint32_t root = rtl::kInvalidChild;
  float root_box[6] = {0, 0, 0, 0, 0, 0};
  // the root node's eight child boxes (xMin xMax yMin yMax zMin zMax each; an
  // empty slot is all +inf): the bounds a camera must not sit on (cull_rect)
  float root_child[48] = {};
  int64_t host_nodes = 0, host_inner = 0;
  uint32_t n_inner = 0;  // inner nodes on the device
  float dmax2 = 0.0f;    // MeshDev::dmax2 (mesh_dmax2; 0: every ray takes the division)
  int32_t depth = 0;
  uint32_t n_tris = 0;       // triangle slots in Geometry::tris (8 zero triangles follow)
  uint32_t root_nchild = 0;  // children of an inner root (slots 0 .. root_nchild-1)
};

struct GridDesc {
  uint32_t size[3] = {0, 0, 0};
  bool bricked = false;  // device layout (rt_scenes.h GridDev): bricked, or the reference's linear
};

struct OctDesc {
  int32_t depth = 0;
};

// ---- the owning parts -------------------------------------------------------
// The arrays of the scene's kind; the others stay empty. Each remembers its
// size (with the triangles' zero pad), which is what a replica copies.
struct Geometry {
  rtmem::DevArray<rtl::GNode> nodes;  // mesh
  rtmem::DevArray<rtl::GTri> tris;
  rtmem::DevArray<float> vals;  // grid
  rtmem::DevArray<rtl::OctWord> child;  // octree
  rtmem::DevArray<rtl::OctVals> ovals;
};

// A mesh created with RT_MESH_DYNAMIC (rt_scene_update_vertices*): the
// creation index array and a vertex staging buffer on the device, the first
// node index of every depth level (+ the node count), the edge-bound word of
// tri_edge_bound_kernel and the pinned host words the update reads back
// (48 root child box floats, then the edge bound).
struct Dynamic {
  bool on = false;
  int64_t nverts = 0;
  rtmem::DevArray<uint32_t> idx;
  rtmem::DevArray<float> vstage;
  rtmem::DevArray<uint32_t> edge;
  rtmem::Pinned<uint32_t> h_refit;
  std::vector<uint32_t> level_first;
  int64_t bytes = 0;  // what this part added to Common::dev_bytes
};

// An octree made by rt_scene_create_octree_dynamic: Geometry::child / ovals
// hold max_nodes entries, of which status[0] are the tree, and the scratch of
// the device build (rt_sdf_octree.h OctBuildArgs) sits here, allocated once.
// A plain octree scene and a replica leave all of it empty.
struct OctDynamic {
  bool on = false;
  uint32_t max_nodes = 0;
  rtmem::DevArray<uint32_t> status;  // {nodes the scene holds, the last build was dropped}
  rtmem::DevArray<rtl::OctWord> s_child;
  rtmem::DevArray<rtl::OctVals> s_vals;
  rtmem::DevArray<uint64_t> cells;
  rtmem::DevArray<uint32_t> flag, bsum, lvl;
  rtmem::DevArray<float> top;
  int64_t bytes = 0;  // what this part added to Common::dev_bytes
};

// RT_SCENE_INSTANCED: the instance records and the table of the bottom-level
// scenes' MeshDev on the device; the scenes themselves (not owned) and the
// update counter each table entry was written from. Nothing here depends on a
// pose.
struct Instanced {
  rtmem::DevArray<rti::InstRec> recs;
  rtmem::DevArray<rtd::MeshDev> tab;
  int32_t n = 0;
  std::vector<rt_scene *> blas;
  std::vector<uint64_t> blas_seen;
  // a mixed scene (rt_scene_create_instanced_any with a grid or an octree among
  // its bottom-level scenes): the table of tagged records instead of tab,
  // which stays empty (rt_instances_mixed.hip)
  rtmem::DevArray<rti::BlasRec> mixed;
  // created with RT_INSTANCED_TLAS: the top-level tree (2 * tlas_leaves nodes,
  // rt_tlas.h) and the object-to-world matrices (12 floats per instance) its
  // leaves are recomputed from when a BLAS's root box moves. Both live on the
  // device only: the host keeps nothing that depends on a pose.
  rtmem::DevArray<rtt::TNode> tlas;
  rtmem::DevArray<float> xform;
  int32_t tlas_leaves = 0;
};

// The cached device frame of the host-buffer entry points, for cap pixels,
// and their timing events.
struct Frame {
  rtmem::DevArray<uint32_t> color;
  rtmem::DevArray<float> t;
  size_t cap = 0;
  rtmem::Event ev0, ev1;
};

// Cost-ordered block schedule (see launch_render), double-buffered: frame k
// of the scene's one-frame kernel records its tiles' costs into cost[k & 1]
// and dispatches in the order order[k & 1] that frame k - 2's costs gave;
// frame k's own order is computed by order_kernel on the side stream os as
// soon as frame k is done (frame_ev), beside frame k + 1, and ord_ev[k & 1]
// marks it done. key[b] = the grid (gx << 16 | gy) whose order order[b] holds
// (0: none).
struct Schedule {
  rtmem::DevArray<uint32_t> cost[2], order[2];
  uint32_t key[2] = {0, 0};
  bool rec[2] = {false, false};
  int par = 0;
  uint32_t cap = 0;
  hipStream_t last_stream = nullptr;  // stream of the previous frame (scheduled or not)
  rtmem::Stream os;                   // side stream of the order kernels
  rtmem::Event ord_ev[2], frame_ev;
};

// rt_render on host buffers (rt_dropin.hip).
struct Dropin {
  rtmem::Stream xs[2];  // colour / t copy streams (render on xs[0])
  rtmem::Event xev;
  rtmem::Event ev_host;  // the pageable cleared frame: the spans are on the host
  // FrameArgs::hit_box of its frame (4 words) and a pinned, mapped host copy
  // (box_out_kernel)
  rtmem::DevArray<int32_t> hit_box;
  rtmem::Pinned<int32_t> h_hit_box;
  // the pageable zero-copy path: FrameArgs::row_span (2 words per row) and its
  // pinned, mapped host copy, for span_cap rows
  rtmem::DevArray<int32_t> row_span;
  rtmem::Pinned<int32_t> h_row_span;
  int32_t span_cap = 0;
  // the staging frame for a cleared frame on pageable buffers: pinned host
  // memory the kernel stores its hits into (zero-copy), kept cleared
  rtdma::HostStage stage{hipHostMallocDefault};
};

}  // namespace rts

// rt_scene_destroy makes `device` current and drains drop.xs and sched.os
// before it deletes; after that nothing of the scene is in use, so the order
// in which the members below release is immaterial.
struct rt_scene {
  int device = 0;
  rts::Common info;
  rts::MeshDesc mesh;
  rts::GridDesc grid;
  rts::OctDesc oct;
  rts::Geometry geo;
  rts::Dynamic dyn;
  rts::OctDynamic octdyn;
  rts::Instanced inst;
  rts::Frame fb;
  rts::Schedule sched;
  rts::Dropin drop;
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
