// rt_instances.h -- instanced scenes (RT_SCENE_INSTANCED, include/rtamd.h):
// the device records, the one function that defines an instance's
// world-to-object matrix, and the launches of rt_instances.hip as rt_device.hip
// (traces) and rt_scene.hip (pose updates) queue them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rtamd.h"
#include "rt_scenes.h"
#include "rt_tlas.h"

namespace rti {

// One instance on the device: 64 bytes, read by the trace kernel through a
// wave-uniform address. m is the world-to-object map M (row-major 3x4, the
// inverse of rt_instance::xform); skipped is set by the device pose update for
// a matrix affine_inverse refuses and cleared by every accepted update.
struct InstRec {
  float m[12];
  int32_t blas;
  uint32_t flags;
  uint32_t skipped;
  uint32_t pad;
};
static_assert(sizeof(InstRec) == 64, "instance record: 64 bytes");

// inv = the inverse of the affine map x (row-major 3x4), by cofactors: nine
// 2x2 minors, the determinant along the first row, nine divisions, then
// -(inv3 * translation) summed left to right. Plain float operations in this
// order on both sides (-ffp-contract=off, correctly rounded division), so the
// host entry rt_affine_inverse and the device pose kernel give the same bits.
// Exact for the identity, translations, power-of-two scales and signed axis
// permutations (every product and quotient is then exact). False, with inv
// untouched, when an entry is not finite or the determinant is zero or not
// finite.
__host__ __device__ inline bool affine_inverse(const float x[12], float inv[12]) {
  for (int k = 0; k < 12; ++k)
    if (!__builtin_isfinite(x[k])) return false;
  const float a = x[0], b = x[1], c = x[2], d = x[4], e = x[5], f = x[6], g = x[8], h = x[9], i = x[10];
  const float c00 = e * i - f * h, c01 = f * g - d * i, c02 = d * h - e * g;
  const float det = (a * c00 + b * c01) + c * c02;
  if (det == 0.0f || !__builtin_isfinite(det)) return false;
  const float r[9] = {c00 / det, (c * h - b * i) / det, (b * f - c * e) / det,
                      c01 / det, (a * i - c * g) / det, (c * d - a * f) / det,
                      c02 / det, (b * g - a * h) / det, (a * e - b * d) / det};
  for (int k = 0; k < 3; ++k) {
    inv[4 * k] = r[3 * k];
    inv[4 * k + 1] = r[3 * k + 1];
    inv[4 * k + 2] = r[3 * k + 2];
    inv[4 * k + 3] = -((r[3 * k] * x[3] + r[3 * k + 1] * x[7]) + r[3 * k + 2] * x[11]);
  }
  return true;
}

// What one trace of an instanced scene needs: the instance records, the table
// of its bottom-level scenes (one MeshDev each, in device memory) and the LDS
// stack slots of the deepest of them (4, 7, 15 or 31).
struct InstArgs {
  const InstRec *inst;
  const rtd::MeshDev *blas;
  int32_t ninst;
  int32_t maxd;
  // a scene created with RT_INSTANCED_TLAS: its tree (rt_tlas.h) and the
  // tree's leaf count P; NULL / 0 for the flat list
  const rtt::TNode *tlas = nullptr;
  int32_t tlas_leaves = 0;
};
// mode: kRaysAny / kRaysClosest / kRaysNormal (rt_shade.h). Only launches.
int trace_instances_launch(const InstArgs &a, const rtd::PlaneDev &pl, const rt_ray_batch &b, int mode,
                           hipStream_t st);
// Writes one table entry in stream order (the entry travels as a kernel
// argument: no host mirror that a later update could overwrite under a copy).
int blas_entry_launch(rtd::MeshDev *entry, const rtd::MeshDev &md, hipStream_t st);
// inst[first + j].m = affine_inverse(d_xform12 + 12 j) for j < count, one
// matrix per lane; blas and flags stay. Only launches.
int pose_launch(InstRec *inst, int32_t first, int32_t count, const float *d_xform12, hipStream_t st);

// ---- rt_shade_instances.hip: rt_shade_rays_device of an instanced scene ------
// shade_one (rt_shade.h) over the flat list or, with a.tlas set, the top-level
// tree; d_color and flags as rt_shade_rays_device takes them. Only launches.
int shade_instances_launch(const InstArgs &a, const rtd::PlaneDev &pl, const rt_render_params &p,
                           const rt_ray_batch &b, uint32_t *d_color, uint32_t flags, hipStream_t st);

// ---- rt_tlas.hip: scenes created with RT_INSTANCED_TLAS ---------------------
// the trace through the top-level tree (a.tlas set); as trace_instances_launch
int trace_tlas_launch(const InstArgs &a, const rtd::PlaneDev &pl, const rt_ray_batch &b, int mode, hipStream_t st);
// What maintains the tree: its nodes (2 * leaves records), the scene's
// object-to-world matrices (12 floats per instance) and the two tables.
struct TlasArgs {
  rtt::TNode *nodes;
  int32_t leaves;
  int32_t ninst;
  const InstRec *inst;
  float *xform;
  const rtd::MeshDev *blas;
};
// Leaves first .. first + count - 1 (first + count <= leaves) from the records
// and the table as they are in stream order. d_xsrc (or NULL): count matrices
// that are first taken over into t.xform. only_blas >= 0: only that BLAS's
// instances. Only launches.
int tlas_boxes_launch(const TlasArgs &t, int32_t first, int32_t count, const float *d_xsrc, int32_t only_blas,
                      hipStream_t st);
// every inner node from the leaves, bottom-up. Only launches.
int tlas_refit_launch(const TlasArgs &t, hipStream_t st);

// ---- rt_instances_mixed.hip: scenes of rt_scene_create_instanced_any whose ----
// bottom-level scenes are not all meshes. One table record per BLAS, 112
// bytes: the kind (RT_SCENE_MESH / _GRID / _OCTREE), the kind's variant (a
// grid's launch mode, kGridBuf | kGridBricked as rti::grid_mode gives it; an
// octree's PACK bit, rt_dispatch.h's rule on the BLAS's own depth) and the
// three device views, of which the kind's own is filled. The flat list reads a
// record through a wave-uniform address (scalar loads, the view stays in
// SGPRs); the tree's mesh phase reads it per lane. InstRec is unchanged.
struct BlasRec {
  uint32_t kind;
  uint32_t var;
  rtd::MeshDev mesh;
  rtd::GridDev grid;
  rtd::OctDev oct;
};
static_assert(sizeof(BlasRec) == 112, "mixed table record: 112 bytes");

// InstArgs of a mixed scene: its table instead of InstArgs::blas (left NULL)
struct MixedArgs {
  InstArgs a;
  const BlasRec *tab;
};
// as trace_instances_launch / trace_tlas_launch (a.a.tlas picks the tree)
int trace_mixed_launch(const MixedArgs &a, const rtd::PlaneDev &pl, const rt_ray_batch &b, int mode, hipStream_t st);
// as shade_instances_launch
int shade_mixed_launch(const MixedArgs &a, const rtd::PlaneDev &pl, const rt_render_params &p, const rt_ray_batch &b,
                       uint32_t *d_color, uint32_t flags, hipStream_t st);
// (the mesh view of a record of kind RT_SCENE_MESH is rewritten by
// blas_entry_launch on &record->mesh; kind and variant stay)
// rt_tlas.hip: as tlas_boxes_launch with the object boxes of the mixed table
// (t.blas is not read): a mesh's rbox, the cube (-1,-1,-1, 1,1,1) for both SDF kinds
int mixed_boxes_launch(const TlasArgs &t, const BlasRec *tab, int32_t first, int32_t count, const float *d_xsrc,
                       int32_t only_blas, hipStream_t st);

}  // namespace rti
