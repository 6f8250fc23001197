// Item order of the sharded work queue (render_persist_kernel, the ray pump's
// ItemStream and the host's rtx_queue_item / rtx_queue_cap share it, so the two
// kernels and the test cannot drift apart).
//
// A launch's `items` are dealt over `heads` counters: item i belongs to head
// i % heads, as its slot i / heads. A wave claims slots of one head (an atomic
// increment) until the slot it gets is past the head's cap, then moves to the
// next head that still has items. `heads` is 8 (the XCDs) times a power of two
// of sub-heads per XCD, at most 64: a wave scans every head with one lane each.
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

}  // namespace rtq
