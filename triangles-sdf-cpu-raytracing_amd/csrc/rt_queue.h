// Item order of the sharded work queue (render_persist_kernel, the ray pump's
// ItemStream and the host's rtx_queue_item / rtx_queue_cap share it, so the two
// kernels and the test cannot drift apart).
//
// A launch's `items` are dealt over `heads` counters: item i belongs to head
// i % heads, as its slot i / heads. A wave claims slots of one head (an atomic
// increment) until the slot it gets is past the head's cap, then moves to the
// next head that still has items. `heads` is 8 (the XCDs) times a power of two
// of sub-heads per XCD, at most 64: a wave scans every head with one lane each.
//
// Below the item order: the item rectangle of a launch (grid, host side), the
// part of the frame's item grid a launch of culled frames deals its items over.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RTQ_HD __host__ __device__ __forceinline__ constexpr
#else
#define RTQ_HD inline constexpr
#endif

namespace rtq {

constexpr uint32_t kXcds = 8;
constexpr uint32_t kMaxHeads = 64;
constexpr uint32_t kNone = 0xFFFFFFFFu;  // "past the end"

RTQ_HD bool heads_ok(uint32_t heads) {
  return heads >= kXcds && heads <= kMaxHeads && (heads & (heads - 1u)) == 0u;
}

// slots of `head` that hold an item: slot k < cap <=> k * heads + head < items
RTQ_HD uint32_t cap(uint32_t items, uint32_t heads, uint32_t head) {
  return (items + heads - 1u - head) >> __builtin_ctz(heads);
}

// slot k of `head` -> item, kNone past the head's cap. (k is a claimed ticket:
// at most cap + one over-claim per wave and visit, far from 2^32 / heads)
RTQ_HD uint32_t item(uint32_t items, uint32_t heads, uint32_t head, uint32_t k) {
  const uint32_t i = k * heads + head;
  return i < items ? i : kNone;
}

// the head a wave starts on: its XCD's, sub-head `seed % (heads / 8)`. Any
// wave may start on any head; this only spreads an XCD's waves evenly.
RTQ_HD uint32_t home(uint32_t xcc, uint32_t seed, uint32_t heads) {
  return (xcc & (kXcds - 1u)) + kXcds * (seed & ((heads >> 3) - 1u));
}

// left != 0, bit i: head i still has items. -> the first such head after
// `own` (own itself last): a rotate of the `heads`-bit mask by own + 1
RTQ_HD uint32_t next(uint64_t left, uint32_t own, uint32_t heads) {
  const uint32_t s = own + 1u;  // 1..heads
  uint64_t rot = left;
  if (s < heads) rot = (left >> s) | (left << (heads - s));
  if (heads < 64u) rot &= (1ull << heads) - 1ull;
  return (s + (uint32_t)__builtin_ctzll(rot)) & (heads - 1u);
}

// Item rectangle of a launch (host side; make_queue and rtx_queue_grid): the
// part of the frame's item grid that holds the union of the frames' cull
// rectangles, so a launch queues no items that every frame would cull.
// A frame's rectangle travels as two words of 8-pixel tiles, columns in cx and
// rows in cy: first tile | (last tile + 1) << 16 (FrameArgs::cull_x and
// P.reserved). first >= last + 1 is an empty rectangle and contributes
// nothing; kWhole in either word (rti::kCullWhole) makes the result the whole
// frame. Items are gx x gy tiles; the origin is rounded down and the end up to
// whole items and clipped to the frame's item grid (W x rows pixels), so no
// item straddles the edge. All frames empty: tiles_x = tiles_y = 0.
constexpr uint32_t kWhole = 0xFFFF0000u;
struct Grid {
  uint32_t ox, oy;            // first item column / row of the rectangle
  uint32_t tiles_x, tiles_y;  // its size in items
};
inline constexpr Grid grid(const uint32_t *cx, const uint32_t *cy, uint32_t n, uint32_t W, uint32_t rows,
                           uint32_t gx, uint32_t gy) {
  const uint32_t fx = (W + 8u * gx - 1u) / (8u * gx), fy = (rows + 8u * gy - 1u) / (8u * gy);  // the frame, in items
  const uint32_t tw = (W + 7u) / 8u, th = (rows + 7u) / 8u;                                    // and in tiles
  uint32_t x0 = tw, x1 = 0u, y0 = th, y1 = 0u;
  for (uint32_t i = 0; i < n; ++i) {
    if (cx[i] == kWhole || cy[i] == kWhole) return Grid{0u, 0u, fx, fy};
    const uint32_t a = cx[i] & 0xFFFFu, b = (cx[i] >> 16) < tw ? (cx[i] >> 16) : tw;
    const uint32_t c = cy[i] & 0xFFFFu, d = (cy[i] >> 16) < th ? (cy[i] >> 16) : th;
    if (a >= b || c >= d) continue;  // empty, or past the frame
    x0 = a < x0 ? a : x0;
    x1 = b > x1 ? b : x1;
    y0 = c < y0 ? c : y0;
    y1 = d > y1 ? d : y1;
  }
  if (x0 >= x1 || y0 >= y1) return Grid{0u, 0u, 0u, 0u};
  const uint32_t ox = x0 / gx, oy = y0 / gy;
  const uint32_t ex = (x1 + gx - 1u) / gx < fx ? (x1 + gx - 1u) / gx : fx;
  const uint32_t ey = (y1 + gy - 1u) / gy < fy ? (y1 + gy - 1u) / gy : fy;
  return Grid{ox, oy, ex - ox, ey - oy};
}

}  // namespace rtq
