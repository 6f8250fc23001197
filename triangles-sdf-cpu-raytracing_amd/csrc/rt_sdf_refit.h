// rt_sdf_refit.h -- the device refit of an SDF-mesh handle (rt_sdf_refit.hip),
// as rt_sdf_mesh_update_vertices_device (rt_sdfgen.hip) queues it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_layout.h"

namespace rtsdf {
// The handle's arrays and the inputs of one refit, all on the current device
// except level_first (host: rth::bvh_level_first, levels + 1 entries). The
// topology arrays are those of rth::SdfTopo, uploaded at creation.
struct SdfRefitArgs {
  rtl::GNode *nodes;          // inner nodes (BFS order): child boxes rewritten
  float4 *tri;                // 3 per triangle slot: a.w (the original id) is read, the rest rewritten
  float4 *pn;                 // 7 per original triangle: rewritten
  uint32_t root;              // the root's child word (a leaf word when levels == 0)
  const float *vpos4;         // new positions, 4 floats per vertex
  const uint32_t *idx;        // the creation index array, 3 per original triangle
  const uint32_t *weld;       // per vertex
  const uint32_t *tri_edge;   // 3 per triangle
  const uint32_t *v_off, *v_inc, *e_off, *e_inc;
  float4 *fn;                 // scratch, per triangle: the face normal
  double *ang;                // scratch, 3 per triangle: the corner angles
  float4 *vn, *en;            // per welded vertex / edge: its pseudonormal
  uint32_t ntri, n_wverts, n_wedges;
  const uint32_t *level_first;
  int32_t levels;
};
// Queues the refit on `st`: the per-triangle terms, the tree (one launch per
// depth level, deepest first, or one single-lane launch for a root-is-leaf
// tree), the welded vertex and edge sums and the scatter into pn. No
// allocation, no copy, no wait.
int sdf_refit_launch(const SdfRefitArgs &a, hipStream_t st);
}  // namespace rtsdf
