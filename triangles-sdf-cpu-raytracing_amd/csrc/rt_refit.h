// rt_refit.h -- the device refit of a mesh scene's BVH8 (rt_refit.hip), as
// rt_scene_update_vertices_device (rt_scene.hip) queues it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_layout.h"

namespace rti {
// The tree and the inputs of one refit, all on the current device except
// level_first (host: rth::bvh_level_first, levels + 1 entries).
struct RefitArgs {
  rtl::GNode *nodes;     // n_inner inner nodes (BFS order)
  rtl::GTri *tris;       // triangle slots; orig_id is read, the rest rewritten
  uint32_t root;         // the root's child word (a leaf word when levels == 0)
  const float *vpos4;    // new positions, 4 floats per vertex
  const uint32_t *idx;   // the creation index array, 3 per original triangle
  const uint32_t *level_first;
  int32_t levels;
};
// Queues the refit on `st`: one launch per depth level, deepest first (or one
// single-lane launch for a root-is-leaf tree). No allocation, no wait.
int refit_launch(const RefitArgs &a, hipStream_t st);
}  // namespace rti
