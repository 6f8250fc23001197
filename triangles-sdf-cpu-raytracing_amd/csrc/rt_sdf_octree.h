// rt_sdf_octree.h -- the device build of an SDF octree (rt_sdf_octree.hip):
// what rt_sdf_mesh_octree_device queues to rebuild a scene made by
// rt_scene_create_octree_dynamic (rt_scene.hip) from an SDF-mesh handle.
//
// A build is 5 * depth + 4 launches on one stream, and one more for depth > 0,
// whatever the mesh:
//   1          the level table: level 0 is the root, no overflow
//   1          (depth > 0) the SDF at the centre of every cell of the top
//              levels, min(depth, 6) of them, in or out of the tree
//   4 * depth  per level d < depth: the SDF at the level's centres and the
//              refine flags; the flags' block sums; one block over the sums
//              (the next level's first node and size, or the overflow); the
//              node records and the children's cells, ranked by the scan
//   2          the corner values of the level-`depth` leaves; their words
//   depth      the child masks, one level per launch, deepest first
//   1          publish: scratch -> scene, unless the build overflowed
// Every launch is sized by the scene's capacity (min(max_nodes, 8^d) nodes for
// level d) and reads its level's size from the level table on the device.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_layout.h"
#include "rt_points.h"

namespace rtsdf {

// words of the level table: first node and size of level d at 2d and 2d + 1
// (d = 0 .. 12), then the build's overflow flag
constexpr int kOctLvlOvf = 26, kOctLvlWords = 32;
// nodes per block of the flag scan (256 lanes x 4 consecutive flags)
constexpr uint32_t kOctScanTile = 1024;

// The top levels whose centre distances one launch computes for every cell,
// and where level d's start in that table: (8^d - 1) / 7 cells come before it.
constexpr int kOctTopLevels = 6;
constexpr int oct_top_levels(int depth) { return depth < kOctTopLevels ? depth : kOctTopLevels; }
__host__ __device__ constexpr uint32_t oct_top_first(int d) { return (uint32_t)(((1ull << (3 * d)) - 1) / 7); }

// Scratch entries a scene of capacity max_nodes holds per array below.
inline size_t oct_flag_count(uint32_t max_nodes) {
  return ((size_t)max_nodes + kOctScanTile - 1) / kOctScanTile * kOctScanTile;
}
inline size_t oct_bsum_count(uint32_t max_nodes) { return oct_flag_count(max_nodes) / kOctScanTile; }

// The scene's arrays and the build's scratch, all on the current device and
// all allocated at creation for max_nodes nodes.
struct OctBuildArgs {
  int32_t depth;
  uint32_t max_nodes;
  rtl::OctWord *child;  // the scene: written by the publish kernel only
  rtl::OctVals *ovals;
  uint32_t *status;     // {nodes the scene holds, the last build was dropped}
  rtl::OctWord *s_child;  // the build, max_nodes each
  rtl::OctVals *s_vals;
  uint64_t *cells;      // per node: x | y << 16 | z << 32, its cell at its level
  uint32_t *flag;       // oct_flag_count: refine flags of the level in work
  uint32_t *bsum;       // oct_bsum_count: the flags' block sums, then their exclusive scan
  uint32_t *lvl;        // kOctLvlWords
  float *top;           // oct_top_first(oct_top_levels(depth)) centre distances (one entry at depth 0)
};

// Launches of one build of a tree of `depth` levels.
constexpr int oct_build_launches(int depth) { return 5 * depth + 4 + (depth > 0 ? 1 : 0); }

// Queues the build on `st`. No allocation, no copy, no wait.
int octree_build_launch(const rt_sdf_mesh *m, const OctBuildArgs &a, hipStream_t st);

}  // namespace rtsdf
