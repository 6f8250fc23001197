// rt_frame.h -- what one frame of a render launch carries from the host to the
// kernels: FrameArgs, the batch of them that travels in one kernel-argument
// segment, and the library's internal frame flags. Shared by the renderer
// (rt_device.hip, which fills and launches frames) and the entries that hand it
// frames of their own (rt_dropin.hip).
#pragma once
#include <stdint.h>

#include "../../include/rtamd.h"

namespace rti {

struct FrameArgs {
  rt_render_params P;
  uint32_t *color;
  float *t;
  int32_t W, H;
  uint32_t flags;
  int32_t band_rows, rank, nranks, rows_local;
  // screen rectangle outside which no ray of this frame can store a hit
  // (cull_rect, mesh primary rays), in 8-pixel tiles of image columns: first
  // tile | (last tile + 1) << 16. Its image rows travel the same way in
  // P.reserved (this copy of the parameters is the library's own), so the
  // batch keeps its size. kCullWhole: no rectangle, every tile is traced
  uint32_t cull_x;
  const uint32_t *order;  // block -> tile schedule (NULL: blockIdx order)
  uint32_t *cost;         // per-tile cost of this frame (shader cycles, max over waves), or NULL
  // one-frame kernel: bounding box of the pixels a hit was stored to, as
  // (min x, -max x, min y, -max y) in buffer coordinates (four atomicMin
  // words, initialised to INT32_MAX), or NULL (rt_render's partial download).
  // With kFlagRowSpan in flags: per buffer row instead, the span of those
  // pixels as (min x, -max x), two such words per row (rt_render's zero-copy
  // cleared frames on pageable buffers: the host copies just these spans)
  int32_t *hit_box;
};

// At most 16 frames per launch (3.7 KiB of kernel arguments): row-band ranks
// of a multi-GPU split render 1/N of each frame, so they take 16 frames per
// launch to keep a launch's bulk long against its tail (bench.py --group;
// rank compute at N = 8: 0.0170 -> 0.0133 ms/frame); whole frames stay at 8.
#ifndef RT_MAX_BATCH
#define RT_MAX_BATCH 16
#endif
constexpr int kMaxBatch = RT_MAX_BATCH;
struct FrameBatch {
  FrameArgs f[kMaxBatch];
};
// the whole batch travels in the kernarg segment next to the scene, plane and queue words
static_assert(sizeof(FrameBatch) + 256 <= 4096, "FrameBatch exceeds the 4 KiB kernel-argument budget");

// Internal flag (never passed through the C ABI; fill_frame rejects it): the
// frame lives in host memory (rt_render's zero-copy cleared frames) and takes
// system-scope stores, which write through this GPU's L2, with no per-wave
// fence. Agent-scope stores leave the lines dirty in L2 for the end-of-kernel
// release to write back over PCIe after the last wave; RTAMD_HOST_STORES=agent
// keeps those (A/B switch).
constexpr uint32_t kFlagHostFrame = 1u << 30;
// Internal flag: FrameArgs::hit_box holds per-row spans (see FrameArgs).
constexpr uint32_t kFlagRowSpan = 1u << 29;
// Internal flag: the frame's eye rays take eye_ray_fast (fill_frame sets it
// when fast_eye_ok holds for its projection and size).
constexpr uint32_t kFlagFastEye = 1u << 28;
// Internal flag: a row-band tile's rows are stored at their own rows of a full
// W x H frame (as RT_FLAG_TILE_NATURAL) but with the frame's plain stores and
// no peer fence: rt_multi_render's zero-copy slots, whose frame is one host
// frame shared by every slot (the kernels' end-of-dispatch release before the
// host's stream synchronisation covers their stores, as for rt_render's).
constexpr uint32_t kFlagNatural = 1u << 27;
// FrameArgs::cull_x / P.reserved of a frame without a rectangle: tiles [0, 65535)
constexpr uint32_t kCullWhole = 0xFFFF0000u;

}  // namespace rti
