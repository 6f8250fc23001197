// rt_device.hip -- the renderer: the HIP kernels (gfx950) that render frames
// (one frame, a batch of frames by block dispatch, the persistent work-queue
// form and the ray pump), the launchers and schedules that instantiate them,
// the frame set-up with the tile cull, and the entry points of include/rtamd.h
// that reach them (rt_render_device*, rt_clear_device, rt_stream_*,
// rt_count_work, rt_bench_frames, the rtx_set_* switches of the launchers);
// at the end of the file the ray queries (rt_intersect_rays,
// rt_trace_rays_device), whose kernels share the render kernels' traversal
// code. Scenes are made in rt_scene.hip, rt_render on host buffers is
// rt_dropin.hip; rt_dispatch.h maps a scene to the kernel template
// arguments. The rest of the C ABI is in rt_runtime.hip (errors,
// streams, host memory, devices), rt_abi_host.hip (loaders, camera, output)
// and rt_diag.hip (device self-checks).
//
// One thread per pixel; a 256-thread workgroup renders a 16x16 pixel block as
// four 8x8 wave tiles (coherent rays share BVH / octree nodes and grid
// voxels in L1/L2). Framebuffer stores are row-major, so a wave writes 8 rows
// x 32 B per buffer. Per-lane traversal stacks live in LDS, lane-interleaved.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <limits>
#include <map>
#include <mutex>
#include <string>
#include <type_traits>
#include <utility>

#include "../../include/rtamd.h"
#include "rt_dispatch.h"
#include "rt_error.h"
#include "rt_host.h"
#include "rt_queue.h"
#include "rt_ray_io.h"
#include "rt_scene.h"
#include "rt_shade.h"

using namespace rtd;
using namespace rti;

namespace {

// Workgroup of the persistent multi-frame kernel (render_persist_kernel), in
// threads. Its waves are independent (each pulls its own items), so the block
// only sets the granularity at which a launch's resources are handed back:
// the next launch on the other stream gets a workgroup slot only when every
// wave of a finished workgroup has left. One wave per workgroup lets the next
// launch replace the draining one wave by wave (128 and
// 256, the block-dispatch size, are A/B settings).
#ifndef RT_PERSIST_BLOCK
#define RT_PERSIST_BLOCK 64
#endif
constexpr int kPBlock = RT_PERSIST_BLOCK;
static_assert(kPBlock % 64 == 0 && kPBlock >= 64 && kPBlock <= 1024, "persistent block: whole waves");
constexpr int kTile = 16;

// Framebuffer stores. The frame (8 B/pixel, 16.6 MB at 1080p) is written once
// and never re-read by the kernel; plain stores keep every written line in the
// XCD's 4 MiB L2 and push scene data out. Agent-scope relaxed atomic stores
// lower to `global_store ... sc1`, which the MI355X L2 drops after writing.
// A peer's frame mapped over xGMI (RT_FLAG_TILE_NATURAL, the row-split p2p
// exchange) takes system-scope stores: they write through this GPU's L2 to the
// owner's memory whatever caching the IPC mapping got, so the kernel's
// completion (before the stream-ordered RCCL signal) covers them.
template <class T>
__device__ __forceinline__ void fb_store(T *p, T v, bool peer) {
  if (peer) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    return;
  }
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Peer frames (RT_FLAG_TILE_NATURAL, the row-split p2p exchange): a system-
// scope release after the wave's last peer store. The stores above are relaxed;
// the fence waits for them to complete and makes them visible at system scope
// before the wave ends, so the RCCL completion signal the host enqueues after
// this kernel on the same stream cannot overtake them over xGMI, whatever the
// end-of-kernel release of the dispatch covers. Once per wave (A/B switch
// RT_PEER_RELEASE=0 drops it).
#ifndef RT_PEER_RELEASE
#define RT_PEER_RELEASE 1
#endif
// (A frame in HOST memory -- rt_render's zero-copy cleared frames -- takes the
// device frame's stores: the dispatch's end-of-kernel system-scope release,
// before rt_render's stream synchronisation, makes them visible to the host.
// A per-wave system-scope fence there costs an L2 write-back per wave: the
// one-frame kernel's 32 k waves took the frame from 0.19 to ~0.38 ms.)
constexpr uint32_t kSysStoreFlags = RT_FLAG_TILE_NATURAL;
__device__ __forceinline__ void peer_release(uint32_t flags) {
#if RT_PEER_RELEASE
  if (flags & kSysStoreFlags) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
#endif
}

__device__ __forceinline__ int image_row(int yl, const FrameArgs &fa) {
  if (fa.nranks <= 1) return yl;
  // unsigned (yl, band_rows > 0): no sign fix-ups around the division
  const uint32_t br = (uint32_t)fa.band_rows, k = (uint32_t)yl / br, r = (uint32_t)yl - k * br;
  return (int)((k * (uint32_t)fa.nranks + (uint32_t)fa.rank) * br + r);
}

// Renderer::draw (raytracing.cpp:67-102). GENERAL=false is the primary-ray
// path (Normal shading, no plane, no secondary rays) used by the headline
// benchmark; GENERAL=true runs intersectionColor in full.
// DIAG selects diagnostic variants of the same kernel (the timed kernels use 0):
//   1: accumulate the work counters (algorithmic-bytes model) into diag[C_NUM];
//   2: per-wave timestamps: diag[4*w .. 4*w+3] = start, end (s_memrealtime,
//      100 MHz), (sum << 32 | max) over lanes of work units, XCC_ID register;
//      w = linear block * 4 + wave.
template <int DIAG>
struct CntSel { using T = NoCnt; };
template <>
struct CntSel<1> { using T = LaneCnt; };
template <>
struct CntSel<2> { using T = LaneCnt; };

__device__ __forceinline__ void flush_counts(NoCnt &, unsigned long long *) {}
__device__ __forceinline__ void flush_counts(LaneCnt &c, unsigned long long *out) {
#pragma unroll
  for (int i = 0; i < C_ALL; ++i) {
    unsigned long long v = c.v[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(out + i, v);
  }
}

// Block -> tile map: plain 2-D dispatch (tiles dealt round-robin over the 8
// XCDs in blockIdx order). Measured and rejected: one contiguous band of tiles
// per XCD (GEMM-style XCD swizzle: the XCD owning the model's band becomes the
// tail; bunny 0.356 -> 0.378 ms, octree 4K default 1.72 -> 2.30 ms) and a
// centre-out order that dispatches the model tiles first (octree 4K primary
// 1.15 -> 1.29 ms: the heavy tiles then compete for the same CUs at once).

// Diagnostic switch (never in a shipping build): 1 drops the stores into host
// frames, 2 keeps only their colour stores, to time what the traversal costs
// without them
#ifndef RT_DIAG_HOST_NOSTORE
#define RT_DIAG_HOST_NOSTORE 0
#endif

// Host-frame pair flush (one-frame kernel, 16x16 tiles of 4 waves). The
// stores of a cleared frame in host memory (rt_render's and rt_multi_render's
// zero-copy frames) cross the host link, where their number, not their bytes,
// is what costs: an 8x8 wave tile's rows are 32-byte pieces, and the stores
// were 45-95 us of the one-frame kernel's ~0.19 ms (dropping only the t
// stores took ~3/4 of that, profiles/r06/dropin_host_store_cost.txt). The two
// waves side by side in a tile (one 16-pixel row band of 8 rows) therefore
// leave their pixels in LDS -- a miss as the cleared frame's words, which the
// host frame already holds -- and the second of the two to finish writes the
// band's 8 rows of colour and t as 64-byte pieces (one 16-byte store per
// lane), or nothing when neither wave stored a hit. Taken for whole bands
// inside the frame with 16-byte aligned rows (W % 4 == 0, aligned buffers);
// other bands store per pixel as before. RT_PAIR_FLUSH=0: off (A/B switch).
#ifndef RT_PAIR_FLUSH
#define RT_PAIR_FLUSH 1
#endif
constexpr int kPairWords = 2 * 8 * 16;  // per buffer: 2 bands x 8 rows x 16 pixels

// One pixel per lane of the wave's 8x8 tile: column xo, rank-local row yl.
// Returns true iff this lane stored a hit (its pixel differs from a cleared
// frame's or from tPrev).
// defer (host-frame pair flush, render_body): this lane's colour and t words
// go to defer[0] and defer[kPairWords] in LDS instead of the frame
template <class S, int SLOTS, bool GENERAL, int DIAG, int B = kBlock, class CT>
__device__ __forceinline__ bool render_pixels(const S &sc, const PlaneDev &pl, const FrameArgs &fa,
                                              CT &cnt, uint32_t *stk, int xo, int yl,
                                              uint32_t *defer = nullptr) {
  const bool active = xo < fa.W && yl < fa.rows_local;
  // wave-cooperative primary path: every lane of the wave takes part
  constexpr bool kWaveCoop = DIAG == 0 && !GENERAL && S::kCoop;
  // the counting variant of that path: the same waves, so that its wave-level
  // counters (C_BVH_SHARED) are those of the timed kernels
  constexpr bool kWaveCount = DIAG == 1 && !GENERAL && S::kCoop;
  if (DIAG == 0 && !kWaveCoop && !active) return false;
  if (active || kWaveCoop || kWaveCount) {  // (the counting variant keeps every lane for its wave reduction)
    StackOf<S, B> st{stk + threadIdx.x};
    if constexpr (kWaveCoop) {
      const int yo = image_row(active ? yl : 0, fa);
      // Tile cull (cull_rect): no pixel of this wave lies in the frame's screen
      // rectangle, so none of its rays can store a hit. The wave does what a
      // wave of misses does, before any ray arithmetic. Each lane tests its own
      // pixel (image row: right for bands whose tiles straddle two bands); the
      // decision is wave-uniform, as mesh_primary_wave needs.
      const uint32_t cx = fa.cull_x, cy = (uint32_t)fa.P.reserved;
      const uint32_t px = (uint32_t)xo >> 3, py = (uint32_t)yo >> 3;
      const bool inside = active && px >= (cx & 0xFFFFu) && px < (cx >> 16) && py >= (cy & 0xFFFFu) && py < (cy >> 16);
      if (__ballot(inside) == 0) {
        const bool natural = (fa.flags & (kSysStoreFlags | kFlagNatural)) != 0;
        const uint32_t idx = (uint32_t)(natural ? yo : yl) * (uint32_t)fa.W + (uint32_t)xo;
        if (defer) {
          defer[0] = 0u;
          defer[kPairWords] = __float_as_uint(kInf);
        } else if (RT_DIAG_HOST_NOSTORE != 0 && (fa.flags & kFlagHostFrame)) {
          // diagnostic build only (see below)
        } else if (active && (fa.flags & RT_FLAG_CLEAR) && !(fa.flags & RT_FLAG_HITS_ONLY)) {
          const bool sys = (fa.flags & (kSysStoreFlags | kFlagHostFrame)) != 0;
          fb_store(fa.color + idx, 0u, sys);
          fb_store(fa.t + idx, kInf, sys);
        }
        return false;
      }
      // The pixel is made opaque here, so that what follows computes its
      // values from it afresh (the image row above all) and shares none with
      // the test. With them shared the register allocation came out worse:
      // at the 96-VGPR floor 12-16 B more scratch per lane in every 4- and
      // 7-slot kernel, and a wave per SIMD less in the 15-slot batch kernel
      // (profiles/r08/README.md). Like this the kernels' registers, scratch
      // and occupancy are what they were without the test.
      asm volatile("" : "+v"(xo), "+v"(yl));
    }
    const int yo = image_row(active ? yl : 0, fa);
    const int y = fa.H - yo - 1;  // loop row y is stored to image row H-y-1 (raytracing.cpp:82)
    const f3 o{fa.P.camera_pos[0], fa.P.camera_pos[1], fa.P.camera_pos[2]};
    f3 d;
    if (fa.flags & kFlagFastEye)
      d = eye_ray_fast(active ? xo : 0, y, fa.W, fa.H, fa.P.proj_inv, fa.P.view_inv);
    else
      d = eye_ray(active ? xo : 0, y, fa.W, fa.H, fa.P.proj_inv, fa.P.view_inv);
    // packed band layout (rank-local row yl) or, with RT_FLAG_TILE_NATURAL, the
    // full frame's own row (a peer's frame mapped over xGMI)
    const bool natural = (fa.flags & (kSysStoreFlags | kFlagNatural)) != 0;
    const bool sys = (fa.flags & (kSysStoreFlags | kFlagHostFrame)) != 0;
    const int yb = natural ? yo : yl;
    // 32-bit pixel index (check_params caps W*H at 2^31): one register live
    // across the traversal instead of two
    const uint32_t idx = active ? (uint32_t)yb * (uint32_t)fa.W + (uint32_t)xo : 0u;
    const bool clear = (fa.flags & RT_FLAG_CLEAR) != 0;
    const bool hits_only = (fa.flags & RT_FLAG_HITS_ONLY) != 0;
    const float tPrev = (clear || !active) ? kInf : fa.t[idx];
    const float tFarEff = std_min(100.0f, tPrev);  // std::min(tFar, tPrev)
    bool hit;
    float t;
    f4 c;
    if (!GENERAL) {
      if (active) cnt.add(C_RAYS, 1);
      Hit h;
      if constexpr (kWaveCoop)
        h = sc.template primary<B>(o, d, 0.01f, tFarEff, active, stk);
      else if constexpr (kWaveCount)
        h = sc.template primary_counted<B>(o, d, 0.01f, tFarEff, active, stk, cnt);
      else
        h = sc.template intersect<B>(o, d, 0.01f, tFarEff, st, cnt);
      hit = h.hit;
      t = h.t;
      f3 n = h.n;
      if (dot(n, d) > 0) n = n * -1.0f;
      c = f4{(n.x + 1.0f) / 2.0f, (n.y + 1.0f) / 2.0f, (n.z + 1.0f) / 2.0f, (1.0f + 1.0f) / 2.0f};
    } else {
      c = shade_one<S, B>(sc, pl, fa.P, o, d, tFarEff, true, hit, t, st, nullptr, cnt);
    }
    // the reference stores only when !isinf(tNew) (raytracing.cpp:91-94)
    const bool store = hit && !__builtin_isinf(t);
    if (defer) {
      // a cleared host frame's pixel, hit or not: the pair flush writes whole
      // rows (a miss's words are the cleared frame's own)
      defer[0] = store ? pack_rgba(c) : 0u;
      defer[kPairWords] = __float_as_uint(store ? t : kInf);
    } else if (RT_DIAG_HOST_NOSTORE == 1 && (fa.flags & kFlagHostFrame)) {
      // diagnostic build only: a host frame's stores dropped (wrong output)
    } else if (RT_DIAG_HOST_NOSTORE == 2 && (fa.flags & kFlagHostFrame)) {
      if (active && store) fb_store(fa.color + idx, pack_rgba(c), sys);  // (colour only)
    } else if (!active) {
      // helper lane of the cooperative path: no pixel of its own
    } else if (clear && !hits_only) {
      fb_store(fa.color + idx, store ? pack_rgba(c) : 0u, sys);
      fb_store(fa.t + idx, store ? t : kInf, sys);
    } else if (store) {
      fb_store(fa.color + idx, pack_rgba(c), sys);
      fb_store(fa.t + idx, t, sys);
    }
    return active && store;
  }
  return false;
}

// 16 bytes into a host frame, written through to memory at system scope (the
// 16-byte form of fb_store's system-scope relaxed store: global_store ... sc0 sc1)
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void host_store16(uint32_t *p, u32x4 v) {
  asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1" : : "v"(p), "v"(v) : "memory");
}

// hf: the pair-flush LDS (render_kernel; nullptr elsewhere): kPairWords colour
// words, kPairWords t words, then one arrival counter per band (zeroed by the
// kernel before any wave gets here)
template <class S, int SLOTS, bool GENERAL, int DIAG, int BT = kBlock>
__device__ __forceinline__ void render_body(const S &sc, const PlaneDev &pl, const FrameArgs &fa,
                                            unsigned long long *counters, uint32_t *stk,
                                            uint32_t *hf = nullptr) {
  typename CntSel<DIAG>::T cnt{};
  unsigned long long t_start = 0;
  if (DIAG == 2) t_start = __builtin_amdgcn_s_memrealtime();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t bx = blockIdx.x, by = blockIdx.y;
  if (DIAG == 0 && fa.order) {  // cost-ordered schedule: this block renders tile order[b]
    const uint32_t tl = fa.order[blockIdx.y * gridDim.x + blockIdx.x];
    bx = tl % gridDim.x;
    by = tl / gridDim.x;
  }
  const uint64_t c0 = (DIAG == 0 && fa.cost) ? __builtin_amdgcn_s_memtime() : 0;
  const int xo = BT == 64 ? (int)bx * 8 + (lane & 7) : (int)bx * kTile + (wave & 1) * 8 + (lane & 7);
  const int yl = BT == 64 ? (int)by * 8 + (lane >> 3) : (int)by * kTile + (wave >> 1) * 8 + (lane >> 3);
  // host-frame pair flush: this wave's band of 8 rows x 16 pixels lies inside
  // the frame and its rows are 16-byte aligned (wave-uniform; the same for
  // both waves of the band)
  const int band = wave >> 1;
  const bool flush = RT_PAIR_FLUSH && DIAG == 0 && BT == kBlock && hf != nullptr &&
                     (fa.flags & kFlagHostFrame) && (fa.flags & RT_FLAG_CLEAR) && (fa.flags & RT_FLAG_HITS_ONLY) &&
                     (fa.W & 3) == 0 && (((uintptr_t)fa.color | (uintptr_t)fa.t) & 15u) == 0 &&
                     (int)bx * kTile + kTile <= fa.W && (int)by * kTile + band * 8 + 8 <= fa.rows_local;
  uint32_t *slot = flush ? hf + band * 128 + (lane >> 3) * 16 + (wave & 1) * 8 + (lane & 7) : nullptr;
  const bool stored = render_pixels<S, SLOTS, GENERAL, DIAG, BT>(sc, pl, fa, cnt, stk, xo, yl, slot);
  if (flush) {
    const uint32_t any = __ballot(stored) != 0 ? 1u : 0u;
    // this wave's LDS words are written before its arrival is counted, and the
    // band's second wave reads them only after counting its own
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    uint32_t old = 0;
    if (lane == 0) old = atomicAdd(hf + 2 * kPairWords + band, 1u | (any << 16));
    old = __builtin_amdgcn_readfirstlane(old);
    if ((old & 0xFFFFu) == 1u && (any | (old >> 16)) != 0u) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      // lanes 0-31 write the colour rows, 32-63 the t rows: row r, 4 pixels at 4 ch
      const int b = lane >> 5, r = (lane & 31) >> 2, ch = lane & 3;
      const u32x4 v = *reinterpret_cast<const u32x4 *>(hf + b * kPairWords + band * 128 + r * 16 + ch * 4);
      const int ylr = (int)by * kTile + band * 8 + r;
      const bool natural = (fa.flags & (kSysStoreFlags | kFlagNatural)) != 0;
      const uint32_t row = (uint32_t)(natural ? image_row(ylr, fa) : ylr);
      uint32_t *base = b ? reinterpret_cast<uint32_t *>(fa.t) : fa.color;
      host_store16(base + row * (uint32_t)fa.W + (uint32_t)bx * kTile + (uint32_t)ch * 4u, v);
    }
  }
  if constexpr (DIAG == 0) {
    if (fa.hit_box && !(fa.flags & kFlagRowSpan) && __ballot(stored)) {  // this wave's stored pixels into the frame's hit box
      int32_t v[4] = {stored ? xo : INT32_MAX, stored ? -xo : INT32_MAX, stored ? yl : INT32_MAX,
                      stored ? -yl : INT32_MAX};
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
          const int32_t o = __shfl_xor(v[i], off, 64);
          v[i] = o < v[i] ? o : v[i];
        }
      // one lane, and only the words this wave improves: ~30 k waves' atomics
      // on one cache line would queue behind each other at the L2
      if (lane == __ffsll((unsigned long long)__ballot(1)) - 1)
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (v[i] < __hip_atomic_load(fa.hit_box + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            atomicMin(fa.hit_box + i, v[i]);
    }
    if (fa.hit_box && (fa.flags & kFlagRowSpan) && __ballot(stored)) {  // per row of the tile: its stored pixels' span
      int32_t lo = stored ? xo : INT32_MAX, nhi = stored ? -xo : INT32_MAX;
#pragma unroll
      for (int off = 1; off < 8; off <<= 1) {  // the 8 lanes of one tile row
        const int32_t a = __shfl_xor(lo, off, 64), b = __shfl_xor(nhi, off, 64);
        lo = a < lo ? a : lo;
        nhi = b < nhi ? b : nhi;
      }
      if ((lane & 7) == 0 && lo != INT32_MAX) {
        int32_t *sp = fa.hit_box + 2 * yl;
        if (lo < __hip_atomic_load(sp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(sp, lo);
        if (nhi < __hip_atomic_load(sp + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(sp + 1, nhi);
      }
    }
  }
  if constexpr (DIAG == 0) {
    if (fa.cost) {  // this wave's duration; the tile keeps its slowest wave's
      const uint64_t dt = __builtin_amdgcn_s_memtime() - c0;
      if (lane == __ffsll((unsigned long long)__ballot(1)) - 1)
        atomicMax(fa.cost + by * gridDim.x + bx, dt > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)dt);
    }
  }
  if constexpr (DIAG == 1) flush_counts(cnt, counters);
  if constexpr (DIAG == 2) {
    const unsigned long long t_end = __builtin_amdgcn_s_memrealtime();
    // this lane's sequential work units (node/leaf visits, tests, steps, sdf evals)
    uint32_t units = 0;
#pragma unroll
    for (int i = 0; i < C_RAYS; ++i) units += cnt.v[i];
    uint32_t mx = units, sm = units;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const uint32_t om = __shfl_xor(mx, off, 64), os = __shfl_xor(sm, off, 64);
      mx = mx > om ? mx : om;
      sm += os;
    }
    // the 9th-largest lane's units: the work the wave does with more than 8 lanes busy
    uint32_t rest = units, u9 = 0;
    for (int r = 0; r < 9; ++r) {
      uint32_t m = rest;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const uint32_t om = __shfl_xor(m, off, 64);
        m = m > om ? m : om;
      }
      u9 = m;
      const uint64_t who = __ballot(rest == m);
      if ((threadIdx.x & 63) == (int)__builtin_ctzll(who)) rest = 0;
    }
    if ((threadIdx.x & 63) == 0) {
      const size_t w = ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (kBlock / 64) + (threadIdx.x >> 6);
      counters[4 * w] = t_start;
      counters[4 * w + 1] = t_end;
      counters[4 * w + 2] = ((unsigned long long)sm << 32) | mx;
      // HW_REG_XCC_ID (4 bits) | 9th-largest lane units << 8
      counters[4 * w + 3] = __builtin_amdgcn_s_getreg(0x1814) | ((unsigned long long)u9 << 8);
    }
  }
}

// Occupancy floor of the primary-ray kernels (waves per SIMD; 1 = the
// compiler's choice). The octree primary kernel is register-limited to 5 waves
// and gains ~5 % at 6 (a few spilled words outside the traversal loop); more
// (8) or the same on the grid (64 VGPRs, spills in the march) lose 5-25 %.
// Trees deeper than 7 slots are LDS-limited anyway.
template <class S, int SLOTS, bool GENERAL, int DIAG>
constexpr int min_waves() {
  return (DIAG != 0 || SLOTS > 7) ? 1 : GENERAL ? RT_GENERAL_WAVES : S::kMinWaves;
}

// Workgroup of the one-frame kernel (render_kernel, DIAG == 0): 64 = one 8x8
// wave tile per workgroup (the cost-ordered schedule then orders 8x8 tiles),
// 256 = 16x16 tiles of 4 waves (A/B switch). The counting and stamping
// variants (DIAG 1, 2) keep 16x16 tiles.
#ifndef RT_FRAME_BLOCK
#define RT_FRAME_BLOCK 256
#endif
constexpr int kFBlock = RT_FRAME_BLOCK;
constexpr int kFTile = kFBlock == 64 ? 8 : kTile;
static_assert(kFBlock == 64 || kFBlock == kBlock, "one-frame workgroup: one wave or the 16x16 tile");
template <int DIAG>
constexpr int frame_block() { return DIAG == 0 ? kFBlock : kBlock; }
template <int DIAG>
constexpr int frame_tile() { return DIAG == 0 ? kFTile : kTile; }

// one-frame kernel, mesh primary rays: wave priority after this many traversal
// iterations and the cooperative tail's ray threshold (A/B switches; the
// persistent kernel's are RT_HEAVY_PRIO and its own)
#ifndef RT_FRAME_PRIO
#define RT_FRAME_PRIO 0
#endif
#ifndef RT_FRAME_COOP
#define RT_FRAME_COOP RT_COOP_RAYS
#endif
template <class S, int SLOTS, bool GENERAL, int DIAG>
__global__ __launch_bounds__(frame_block<DIAG>()) __attribute__((amdgpu_waves_per_eu(min_waves<S, SLOTS, GENERAL, DIAG>())))
void render_kernel(S sc_arg, PlaneDev pl, FrameArgs fa,
                                                        unsigned long long *counters) {
  __shared__ uint32_t stk[stack_words<S, SLOTS>() * frame_block<DIAG>()];
  constexpr bool kPair = RT_PAIR_FLUSH && DIAG == 0 && frame_block<DIAG>() == kBlock;
  __shared__ __attribute__((aligned(16))) uint32_t hf[kPair ? 2 * kPairWords + 4 : 4];
  S sc = sc_arg;
  if constexpr (S::kCoop && !GENERAL && DIAG == 0) {
    sc.prio_iters = RT_FRAME_PRIO;
    sc.coop_rays = RT_FRAME_COOP;
  }
  // (grid-uniform condition: every wave of the block passes the barrier or none)
  if (kPair && (fa.flags & kFlagHostFrame) && (fa.flags & RT_FLAG_CLEAR) && (fa.flags & RT_FLAG_HITS_ONLY)) {
    if (threadIdx.x < 2) hf[2 * kPairWords + threadIdx.x] = 0u;
    __syncthreads();
  }
  render_body<S, SLOTS, GENERAL, DIAG, frame_block<DIAG>()>(sc, pl, fa, counters, stk, kPair ? hf : nullptr);
  peer_release(fa.flags);
}

// Several frames in one launch: blockIdx.z selects the frame. The tiles of
// frame z+1 fill the CUs while frame z's last tiles (grazing rays at the
// silhouette, the per-frame tail) finish, so only the batch's last frame
// leaves a tail. The per-frame arguments travel in the kernarg segment
// (uniform blockIdx.z index: scalar loads).
// Workgroup of the multi-frame block dispatch (render_batch_kernel; grids and
// the small row bands of N >= 4 ranks): one 8x8 wave tile per workgroup, so a
// finished wave frees its slot for the next tile at once instead of waiting for
// the slowest wave of a 16x16 tile (256^3 grid 0.0542 -> 0.0512, bunny rank
// bands at N = 4 0.0305 -> 0.0269 ms/frame). 256 = the
// 16x16 tile of 4 waves (A/B switch).
#ifndef RT_BATCH_BLOCK
#define RT_BATCH_BLOCK 64
#endif
constexpr int kBBlock = RT_BATCH_BLOCK;
// Multi-frame block dispatch, block b -> tile b / n of frame b % n: the
// batch's frames advance together, so the last blocks dispatched are every
// frame's last rows instead of the whole last frame (256^3 grid one stream
// 0.0537 / 0.0523 -> 0.0510 / 0.0501 ms/frame, two streams ~1 %; row bands
// level). 0: frame after frame (A/B switch).
#ifndef RT_BATCH_INTERLEAVE
#define RT_BATCH_INTERLEAVE 1
#endif
constexpr int kBTile = kBBlock == 64 ? 8 : kTile;
static_assert(kBBlock == 64 || kBBlock == kBlock, "batch workgroup: one wave or the 16x16 tile");

template <class S, int SLOTS, bool GENERAL>
__global__ __launch_bounds__(kBBlock) __attribute__((amdgpu_waves_per_eu(min_waves<S, SLOTS, GENERAL, 0>())))
void render_batch_kernel(S sc, PlaneDev pl, FrameBatch fb) {
  __shared__ uint32_t stk[stack_words<S, SLOTS>() * kBBlock];
  if constexpr (kBBlock == kBlock) {
    render_body<S, SLOTS, GENERAL, 0>(sc, pl, fb.f[blockIdx.z], nullptr, stk);
  } else {
    NoCnt cnt{};
    const int lane = threadIdx.x & 63;
#if RT_BATCH_INTERLEAVE
    const uint32_t n = gridDim.z, b = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    // heavy-first tile order of row bands (fb.f[0].order, from the previous
    // launch's recorded tile costs on this stream; band_sched)
    const uint32_t f = b % n, tl = fb.f[0].order ? fb.f[0].order[b / n] : b / n;
    const uint32_t tx = tl % gridDim.x, ty = tl / gridDim.x;
#else
    const uint32_t f = blockIdx.z, tl = blockIdx.y * gridDim.x + blockIdx.x, tx = blockIdx.x, ty = blockIdx.y;
#endif
    const uint64_t c0 = fb.f[0].cost ? __builtin_amdgcn_s_memtime() : 0;
    render_pixels<S, SLOTS, GENERAL, 0, kBBlock>(sc, pl, fb.f[f], cnt, stk, (int)tx * 8 + (lane & 7),
                                                 (int)ty * 8 + (lane >> 3));
    if (fb.f[0].cost && lane == 0) {  // this tile's cost: the slowest of its frames' waves
      const uint64_t dc = __builtin_amdgcn_s_memtime() - c0;
      atomicMax(fb.f[0].cost + tl, (uint32_t)(dc < 0xFFFFFFFFull ? dc : 0xFFFFFFFFull));
    }
  }
  peer_release(fb.f[0].flags);
}

// Persistent form of render_batch_kernel: a grid of just the resident blocks;
// every wave pulls 8x8 pixel tiles (items) from a work queue until the batch
// is drained, so a wave whose tile finishes early takes the next one at once
// instead of waiting for the in-order workgroup dispatcher (which stalls
// behind a full SE while other SEs have free slots). The queue is sharded per
// XCD, with `nheads` / 8 sub-heads each (rt_queue.h holds the item order): item
// i belongs to head i % nheads; a wave starts on a head of its own XCD
// (HW_REG_XCC_ID) and, once that is drained, moves on to the others, so the
// batch completes whatever XCDs the grid lands on. The next item is claimed
// before the current one is traced (its atomic's latency hides under the
// traversal). The last wave out resets the heads for the next launch on the
// stream.
struct PersistQ {
  uint32_t *heads;   // nheads heads `stride` words apart; heads[nheads * stride] = waves done
  uint32_t items;    // frames * per_frame
  uint32_t tiles_x, per_frame;  // items (groups of gx x gy wave tiles) per row / per frame
  uint32_t waves;    // waves in the grid
  uint32_t gx, gy;   // wave tiles (8x8 pixels) per item: 1x1, 2x1 or 2x2
  uint32_t stride;   // words between heads
  uint32_t nheads;   // 8, 16, 32 or 64 (rtq::heads_ok)
  // item order of a head: cpf == 0 interleaved (rt_queue.h: item i on head
  // i % nheads); cpf > 0 banded: head h takes tile rows [h cpf, (h+1) cpf) of
  // the row-major items of every frame, frame after frame (nper = frames x
  // cpf slots, slots past per_frame are empty). The banded order was measured
  // and rejected and no launch sets it; the branch
  // stays because the 4- and 7-slot mesh kernels come out with 28 B more
  // scratch per lane without it (profiles/r09/README.md)
  uint32_t cpf, nper;
  // diagnostic builds (-DRT_PERSIST_STAMPS, tools/build_variant.sh; see
  // rtx_set_persist_stamps): per wave w = blockIdx.x * (kPBlock / 64) + wave, 8 x u64 =
  // start, end (s_memrealtime, 100 MHz), items traced | XCD << 32, end of its
  // last item, start of its last item, last item, longest item's duration, longest item
  unsigned long long *stamps;
  // first item column / row: a launch of mesh primary frames queues items over
  // its item rectangle only (rtq::grid, make_queue; tiles_x and per_frame are
  // the rectangle's). 0, 0 with the whole frame's grid. Only the kernels that
  // read a frame's cull rectangle (kQueueOrigin) add it; the words come last,
  // so the other kernels' argument offsets and code are what they were
  uint32_t ox, oy;
};
template <class S, bool GENERAL>
constexpr bool kQueueOrigin = S::kCoop && !GENERAL;
// 4 KiB + 256 B apart: every head on its own memory channel's lines, so the
// memory-side atomics of different heads do not queue behind each other
// (RTAMD_QSTRIDE=<words> overrides it for A/B runs, at most kHeadStrideMax)
constexpr int kHeadStride = 1088;
constexpr int kHeadStrideMax = 4096;

__device__ __forceinline__ uint32_t q_claim(uint32_t *head) {
  uint32_t k = 0;
  if ((threadIdx.x & 63) == 0) k = __hip_atomic_fetch_add(head, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return __builtin_amdgcn_readfirstlane(k);
}
// RT_QUEUE_HEADS: 0 = PersistQ::nheads (a run-time setting), 8..64 = compiled in
#ifndef RT_QUEUE_HEADS
#define RT_QUEUE_HEADS 0
#endif
__device__ __forceinline__ uint32_t q_nheads(const PersistQ &q) { return RT_QUEUE_HEADS ? (uint32_t)RT_QUEUE_HEADS : q.nheads; }
// a wave's first head: its XCD's, the sub-head dealt over the XCD's waves
// (workgroups go to the XCDs round-robin, so blockIdx.x >> 3 counts an XCD's
// workgroups; nothing depends on that: any wave may start on any head)
__device__ __forceinline__ uint32_t q_home(uint32_t xcc, uint32_t nheads) {
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  return rtq::home(xcc, (blockIdx.x >> 3) + wave, nheads);
}
// head `own` is drained: every head read at once (one lane each, one round
// trip) -> the first head after `own` that still has items, rtq::kNone if none
__device__ __forceinline__ uint32_t q_scan(const PersistQ &q, uint32_t nh, uint32_t own, int lane) {
  uint32_t v = 0xFFFFFFFFu;
  const bool mine = (uint32_t)lane < nh;
  if (mine) v = __hip_atomic_load(q.heads + (uint32_t)lane * q.stride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const uint32_t cap = q.cpf ? q.nper : rtq::cap(q.items, nh, (uint32_t)lane);
  const uint64_t left = __ballot(mine && v < cap);
  return left ? rtq::next(left, own, nh) : rtq::kNone;
}
// a wave is done: the last one out resets the heads for the stream's next launch
__device__ __forceinline__ void q_leave(const PersistQ &q, uint32_t nh, int lane) {
  uint32_t *done = q.heads + nh * q.stride;
  uint32_t last = 0;
  if (lane == 0) last = __hip_atomic_fetch_add(done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == q.waves - 1;
  if (__builtin_amdgcn_readfirstlane(last)) {
    // every wave has left its claim loop: no claim is in flight any more
    if ((uint32_t)lane < nh)
      __hip_atomic_store(q.heads + (uint32_t)lane * q.stride, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (lane == 0) __hip_atomic_store(done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

template <class S, int SLOTS, bool GENERAL>
__global__ __launch_bounds__(kPBlock) __attribute__((amdgpu_waves_per_eu(min_waves<S, SLOTS, GENERAL, 0>())))
void render_persist_kernel(S sc_arg, PlaneDev pl, FrameBatch fb, PersistQ q) {
  __shared__ uint32_t stk[stack_words<S, SLOTS>() * kPBlock];
  S sc = sc_arg;
  if constexpr (S::kCoop && !GENERAL) sc.prio_iters = RT_HEAVY_PRIO;
  const int lane = threadIdx.x & 63;
  const uint32_t xcc = __builtin_amdgcn_s_getreg(0x1814) & 7;  // HW_REG_XCC_ID: this wave's XCD
#ifdef RT_PERSIST_STAMPS
  const unsigned long long t_start = __builtin_amdgcn_s_memrealtime();
  unsigned long long t_item = t_start, t_last = t_start, d_max = 0;
  uint32_t n_items = 0, last_item = 0, max_item = 0;
#endif
  uint32_t h = q_home(xcc, q_nheads(q));
  uint32_t k = q_claim(q.heads + h * q.stride);
  NoCnt cnt{};
  for (;;) {
    // slot k of head h -> item (frame f, row-major index r in the frame)
    uint32_t item, f, r;
    bool drained, empty = false;
    if (q.cpf == 0) {
      // rtq::item(q.items, nheads, h, k), spelled out beside the banded form
      item = k * q_nheads(q) + h;
      drained = item >= q.items;
      f = item / q.per_frame;
      r = item - f * q.per_frame;
    } else {
      drained = k >= q.nper;
      f = k / q.cpf;
      r = h * q.cpf + (k - f * q.cpf);
      empty = r >= q.per_frame;
      item = f * q.per_frame + r;
    }
    if (drained) {
      // head h drained: claim from the first head after it that still has
      // items; none left: done. A claim that loses the race to the last item
      // just comes back here.
      h = q_scan(q, q_nheads(q), h, lane);
      if (h == rtq::kNone) break;
      k = q_claim(q.heads + h * q.stride);
      continue;
    }
    const uint32_t knext = q_claim(q.heads + h * q.stride);
    if (empty) {
      k = knext;
      continue;
    }
    uint32_t ty = r / q.tiles_x, tx = r - ty * q.tiles_x;
    if constexpr (kQueueOrigin<S, GENERAL>) {  // (after tx: ty is still the rectangle's row there)
      tx += q.ox;
      ty += q.oy;
    }
#ifdef RT_PERSIST_STAMPS
    const unsigned long long t_begin = __builtin_amdgcn_s_memrealtime();
#endif
    for (uint32_t j = 0; j < q.gy; ++j)
      for (uint32_t i = 0; i < q.gx; ++i) {
        // the frame index is made opaque per tile, so the frame's arguments
        // (two 4x4 matrices among them) are re-read from the kernarg segment by
        // each tile instead of being hoisted out of the tile loop and kept
        // live across the traversal
        uint32_t fo = f;
        asm volatile("" : "+s"(fo));
        render_pixels<S, SLOTS, GENERAL, 0, kPBlock>(sc, pl, fb.f[fo], cnt, stk, (int)((tx * q.gx + i) * 8) + (lane & 7),
                                            (int)((ty * q.gy + j) * 8) + (lane >> 3));
      }
#ifdef RT_PERSIST_STAMPS
    ++n_items;
    t_item = __builtin_amdgcn_s_memrealtime();
    t_last = t_begin;
    last_item = item;
    if (t_item - t_begin > d_max) {
      d_max = t_item - t_begin;
      max_item = item;
    }
#endif
    k = knext;
  }
#ifdef RT_PERSIST_STAMPS
  if (q.stamps && lane == 0) {
    const size_t w = (size_t)blockIdx.x * (kPBlock / 64) + (threadIdx.x >> 6);
    unsigned long long *o = q.stamps + 8 * w;
    o[0] = t_start;
    o[1] = __builtin_amdgcn_s_memrealtime();
    o[2] = n_items | ((unsigned long long)xcc << 32);
    o[3] = t_item;
    o[4] = t_last;
    o[5] = last_item;
    o[6] = d_max;
    o[7] = max_item;
  }
#endif
  peer_release(fb.f[0].flags);
  q_leave(q, q_nheads(q), lane);
}

// ---------------------------------------------------------------- ray pump --
// render_pump_kernel: the persistent multi-frame kernel with wavefront
// active-ray compaction (north star: "ballot/prefix-sum active-ray compaction
// for the sphere-march and octree steps", replacing the 8-wide ISPC gangs of
// ray_pack.ispc:241-273 and the recursion of octree_raytracing.cpp:166-202).
// A wave does not own a fixed 8x8 tile: each lane owns ONE ray at a time, and
// the wave pulls pixels from a per-wave pixel stream (consecutive pixels of
// the work-queue items, 8x8 tiles in order, so a refill's rays are coherent).
// The traversal of every live lane runs until `refill_min` lanes have
// finished (__ballot of the lanes still in the loop); the wave then writes the
// finished lanes' pixels, hands each dead lane the next pixel of the stream
// (its rank in the dead-lane ballot, __mbcnt, is its offset in the stream) and
// resumes. Traversal state stays in the lane's registers and its own LDS stack
// column, so nothing moves. Once the queue is drained the remaining rays run
// to the end. Primary rays (Normal shading, no plane); every image is the
// same as render_kernel's, bit for bit.
struct PumpFrame {  // the per-frame arguments a lane needs, copied to LDS
  float o[3];
  float proj_inv[16];
  float view_inv[16];
  uint32_t *color;
  float *t;
};

// wave-uniform work-item stream over the sharded queue (render_persist_kernel's
// protocol): the ticket of the next item on head h is claimed one ahead
// The pump keeps one head per XCD (kPumpHeads): its refill loop has no
// registers to spare for a run-time head count (profiles/r09/README.md), and a
// stream's head set is all zero between launches, so each kernel may deal its
// items over a head count of its own.
constexpr uint32_t kPumpHeads = rtq::kXcds;
struct ItemStream {
  uint32_t h, k;
};
__device__ __forceinline__ uint32_t take_item(const PersistQ &q, ItemStream &s, uint32_t xcc, int lane) {
  for (;;) {
    const uint32_t item = rtq::item(q.items, kPumpHeads, s.h, s.k);
    if (item != rtq::kNone) {
      s.k = q_claim(q.heads + s.h * q.stride);
      return item;
    }
    // head s.h drained: render_persist_kernel's q_scan for the 8 heads, from
    // this XCD's own, spelled out (rtq::cap and rtq::next with the count folded
    // in; the shared form costs the octree pump 4-12 B of scratch per lane)
    static_assert(kPumpHeads == 8 && rtq::cap(45, 8, 3) == (45 + 7 - 3) / 8 && rtq::next(0x21, 5, 8) == 0, "take_item's scan");
    uint32_t v = 0xFFFFFFFFu;
    if (lane < 8) v = __hip_atomic_load(q.heads + lane * q.stride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint64_t m = __ballot(lane < 8 && v < (q.items + 7u - (uint32_t)lane) / 8u) & 0xFFull;
    if (m == 0) return 0xFFFFFFFFu;
    const uint32_t rot = (uint32_t)(((m >> (xcc + 1)) | (m << (7 - xcc))) & 0xFFull);
    s.h = (xcc + 1 + (uint32_t)__builtin_ctz(rot)) & 7u;
    s.k = q_claim(q.heads + s.h * q.stride);
  }
}

struct OctP {
  using Ray = OctRay;
  static constexpr int kFields = kOctFields;
  static constexpr int kMinWaves = RT_OCT_WAVES;
  OctDev d;
  template <bool FAST>
  __device__ __forceinline__ int start(f3 o, f3 dir, f3 inv, float tf, Ray &R, float &t, f3 &n) const {
    NoCnt c;
    OctHitPt hp;
    const int s = oct_start<FAST>(d, o, dir, inv, 0.01f, tf, R, t, hp, c);
    if (s == RAY_HIT) n = oct_normal_at(d, hp, c);
    return s;
  }
  template <bool FAST>
  __device__ __forceinline__ int run(f3 o, f3 dir, f3 inv, float tf, LdsStack<kBlock, kOctFields> st, Ray &R, int limit,
                                     float &t, f3 &n) const {
    NoCnt c;
    OctHitPt hp;
    const int s = oct_run<kBlock, FAST, true, false>(d, o, dir, inv, 0.01f, tf, st, R, limit, t, hp, c);
    if (s == RAY_HIT) n = oct_normal_at(d, hp, c);
    return s;
  }
};

// the grid's sphere march on the pump (grid_start / grid_run): a lane's state
// is (t, p), so a refill costs an eye ray and a box entry
template <int kMode>
struct GridP {
  using Ray = GridRay;
  static constexpr int kFields = 1;  // no traversal stack (one unused LDS word per lane)
  static constexpr int kMinWaves = RT_GRID_WAVES;
  GridDev d;
  template <bool FAST>
  __device__ __forceinline__ int start(f3 o, f3 dir, f3 inv, float tf, Ray &R, float &, f3 &) const {
    return grid_start(o, dir, inv, 0.01f, tf, R);
  }
  template <bool FAST>
  __device__ __forceinline__ int run(f3 o, f3 dir, f3, float, LdsStack<kBlock, kFields>, Ray &R, int limit,
                                     float &t, f3 &n) const {
    NoCnt c;
    f3 hp;
    const int s = grid_run<kMode, true>(d, o, dir, R, limit, t, hp, c);
    if (s == RAY_HIT) n = grid_normal<kMode>(d, hp, c);
    return s;
  }
};

#ifndef RT_REFILL_MIN
#define RT_REFILL_MIN 16  // dead lanes that trigger a refill (RTAMD_REFILL overrides)
#endif

#ifndef RT_PUMP_WAVES
#define RT_PUMP_WAVES 0  // occupancy floor of the pump kernel: 0 = the scene's kMinWaves, 1 = the compiler's
#endif
template <class P, int SLOTS>
__global__ __launch_bounds__(kBlock)
__attribute__((amdgpu_waves_per_eu(SLOTS > 7 ? 1 : (RT_PUMP_WAVES ? RT_PUMP_WAVES : P::kMinWaves))))
void render_pump_kernel(P sc, FrameBatch fb, PersistQ q, int32_t nframes, int32_t refill_min) {
  __shared__ uint32_t stk[SLOTS * P::kFields * kBlock];
  __shared__ PumpFrame frames[kMaxBatch];
  if ((int)threadIdx.x < nframes) {
    const FrameArgs &fa = fb.f[threadIdx.x];
    PumpFrame &pf = frames[threadIdx.x];
    for (int i = 0; i < 3; ++i) pf.o[i] = fa.P.camera_pos[i];
    for (int i = 0; i < 16; ++i) {
      pf.proj_inv[i] = fa.P.proj_inv[i];
      pf.view_inv[i] = fa.P.view_inv[i];
    }
    pf.color = fa.color;
    pf.t = fa.t;
  }
  __syncthreads();
  const FrameArgs &F = fb.f[0];  // size, flags and tile are the same for every frame of a batch
  const int lane = threadIdx.x & 63;
  const uint32_t xcc = __builtin_amdgcn_s_getreg(0x1814) & 7;  // HW_REG_XCC_ID
  const bool clear = (F.flags & RT_FLAG_CLEAR) != 0, hits_only = (F.flags & RT_FLAG_HITS_ONLY) != 0;
  const bool peer = (F.flags & kSysStoreFlags) != 0;
  const uint32_t isz = 64u * q.gx * q.gy;  // pixels per item
  ItemStream is{xcc, 0u};
  is.k = q_claim(q.heads + is.h * q.stride);
  uint32_t cur = take_item(q, is, xcc, lane), off = 0;
  LdsStack<kBlock, P::kFields> st{stk + threadIdx.x};
  typename P::Ray R;
  bool live = false, fast = true;
  uint32_t f = 0;
  uint32_t idx = 0;
  f3 o{0.0f, 0.0f, 0.0f}, d{0.0f, 0.0f, 1.0f}, inv{kInf, kInf, 1.0f};
  float tfar = 100.0f;
  // Renderer::draw's store (raytracing.cpp:91-94) of a finished ray, Normal shading
  auto finish = [&](int status, float t, f3 n) {
    const bool hit = status == RAY_HIT;
    const bool store = hit && !__builtin_isinf(t);
    if (dot(n, d) > 0) n = n * -1.0f;
    const f4 c{(n.x + 1.0f) / 2.0f, (n.y + 1.0f) / 2.0f, (n.z + 1.0f) / 2.0f, (1.0f + 1.0f) / 2.0f};
    uint32_t *cp = frames[f].color + idx;
    float *tp = frames[f].t + idx;
    if (clear && !hits_only) {
      fb_store(cp, store ? pack_rgba(c) : 0u, peer);
      fb_store(tp, store ? t : kInf, peer);
    } else if (store) {
      fb_store(cp, pack_rgba(c), peer);
      fb_store(tp, t, peer);
    }
  };
  for (;;) {
    // refill: every dead lane takes the next pixel of the wave's stream
    while (cur != 0xFFFFFFFFu) {
      const uint64_t dead = __ballot(!live);
      const uint32_t ndead = (uint32_t)__popcll(dead);
      if ((int)ndead < refill_min) break;
      const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(dead >> 32),
                                                      __builtin_amdgcn_mbcnt_lo((uint32_t)dead, 0u));
      const uint32_t nxt = (off + ndead >= isz) ? take_item(q, is, xcc, lane) : 0xFFFFFFFFu;
      // (frame, tile row, tile column) of the two items, wave-uniform (scalar divisions)
      const uint32_t fc = cur / q.per_frame, rc = cur - fc * q.per_frame;
      const uint32_t tyc = rc / q.tiles_x, txc = rc - tyc * q.tiles_x;
      uint32_t fn = 0, txn = 0, tyn = 0;
      if (nxt != 0xFFFFFFFFu) {
        fn = nxt / q.per_frame;
        const uint32_t rn = nxt - fn * q.per_frame;
        tyn = rn / q.tiles_x;
        txn = rn - tyn * q.tiles_x;
      }
      bool got = false;
      uint32_t p = 0, tx = 0, ty = 0;
      if (!live) {
        if (off + rank < isz) { got = true; p = off + rank; f = fc; tx = txc; ty = tyc; }
        else if (nxt != 0xFFFFFFFFu) { got = true; p = off + rank - isz; f = fn; tx = txn; ty = tyn; }
      }
      off += ndead;
      if (off >= isz) { cur = nxt; off -= isz; }
      if (got) {
        const uint32_t tile = p >> 6;
        const uint32_t ti = q.gx == 1 ? 0u : (tile & 1u), tj = q.gx == 1 ? tile : (tile >> 1);
        const int x = (int)((tx * q.gx + ti) * 8 + (p & 7u));
        const int yl = (int)((ty * q.gy + tj) * 8 + ((p >> 3) & 7u));
        if (x < F.W && yl < F.rows_local) {
          const int yo = image_row(yl, F);
          const PumpFrame &pf = frames[f];
          idx = (uint32_t)(peer ? yo : yl) * (uint32_t)F.W + (uint32_t)x;
          o = f3{pf.o[0], pf.o[1], pf.o[2]};
          d = eye_ray(x, F.H - yo - 1, F.W, F.H, pf.proj_inv, pf.view_inv);
          inv = f3{1.0f / d.x, 1.0f / d.y, 1.0f / d.z};
          fast = __builtin_isfinite(inv.x) && __builtin_isfinite(inv.y) && __builtin_isfinite(inv.z);
          tfar = clear ? 100.0f : std_min(100.0f, pf.t[idx]);  // std::min(tFar, tPrev)
          float t = kInf;
          f3 n{0.0f, 1.0f, 0.0f};
          const int s = fast ? sc.template start<true>(o, d, inv, tfar, R, t, n)
                             : sc.template start<false>(o, d, inv, tfar, R, t, n);
          if (s == RAY_PENDING) live = true;
          else finish(s, t, n);
        }
      }
    }
    if (__ballot(live) == 0) {
      if (cur == 0xFFFFFFFFu) break;
      continue;
    }
    const int limit = cur == 0xFFFFFFFFu ? 0 : 64 - refill_min;
    float t = kInf;
    f3 n{0.0f, 1.0f, 0.0f};
    int s = RAY_PENDING;
    if (__ballot(live && !fast) == 0) {  // every live ray has finite 1/d: the fast slab form for all
      if (live) s = sc.template run<true>(o, d, inv, tfar, st, R, limit, t, n);
    } else {  // the exact ISPC form (the same bits for finite 1/d too)
      if (live) s = sc.template run<false>(o, d, inv, tfar, st, R, limit, t, n);
    }
    if (live && s != RAY_PENDING) {
      finish(s, t, n);
      live = false;
    }
  }
  peer_release(F.flags);
  q_leave(q, kPumpHeads, lane);
}

// FrameBuffer::clear() (raytracing.hpp:16-19): 16 B per lane per buffer.
__global__ void clear_kernel(uint32_t *c, float *t, int64_t n) {
  const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i + 4 <= n) {
    *reinterpret_cast<uint4 *>(c + i) = make_uint4(0u, 0u, 0u, 0u);
    *reinterpret_cast<float4 *>(t + i) = make_float4(kInf, kInf, kInf, kInf);
  } else {
    for (int64_t j = i; j < n; ++j) {
      c[j] = 0u;
      t[j] = kInf;
    }
  }
}

// The cleared background of a multi-frame launch outside its item rectangle
// (rtq::grid): the persistent launch that follows on the stream queues items
// over the rectangle only, and with RT_FLAG_CLEAR (without HITS_ONLY) the
// pixels outside it are a miss's words, colour 0 and t = +inf, written here.
// One wave per workgroup (it takes single wave slots beside the other stream's
// resident waves) writes 64 consecutive pixels of 8 rows: block x = 64-pixel
// column segment, y = 8-row band, z = frame. The rectangle [x0, x1) x [y0, y1)
// is in pixels, its edges multiples of 8: a lane inside it, or past W x H,
// stores nothing. fb_store's agent-scope stores: the lines do not stay in L2.
struct ClearOutside {
  uint32_t *color[kMaxBatch];
  float *t[kMaxBatch];
  uint32_t W, H;
  uint32_t x0, x1, y0, y1;
};
__global__ __launch_bounds__(64) void clear_outside_kernel(ClearOutside a) {
  const uint32_t x = blockIdx.x * 64u + threadIdx.x, yb = blockIdx.y * 8u;
  if (x >= a.W) return;
  const bool in_x = x >= a.x0 && x < a.x1;
  if (in_x && yb >= a.y0 && yb + 8u <= a.y1) return;  // (the rectangle's rows start and end on bands)
  uint32_t *c = a.color[blockIdx.z];
  float *t = a.t[blockIdx.z];
#pragma unroll
  for (uint32_t j = 0; j < 8u; ++j) {
    const uint32_t y = yb + j;
    if (y >= a.H || (in_x && y >= a.y0 && y < a.y1)) continue;
    const uint32_t idx = y * a.W + x;  // (check_params caps W * H at 2^31)
    fb_store(c + idx, 0u, false);
    fb_store(t + idx, kInf, false);
  }
}

// Block schedule for the next frame from this frame's per-tile costs:
// tiles in descending cost class (2 classes per octave of shader cycles), so
// the long-running tiles of a frame -- grazing rays at silhouettes, the tail
// that otherwise starts late and runs alone -- are dispatched first. Order
// within a class is arbitrary; the image does not depend on the order. Resets
// the costs for the next frame.
constexpr int kCostClasses = 66;
__device__ __forceinline__ uint32_t cost_class(uint32_t c) {
  if (c == 0) return 0;
  const uint32_t e = 32u - (uint32_t)__clz(c);
  return 2 * e + (e >= 2 ? (c >> (e - 2)) & 1u : 0u);
}
__global__ __launch_bounds__(1024) void order_kernel(uint32_t *cost, uint32_t *order, uint32_t n) {
  __shared__ uint32_t hist[kCostClasses];
  for (uint32_t i = threadIdx.x; i < kCostClasses; i += blockDim.x) hist[i] = 0;
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) atomicAdd(&hist[cost_class(cost[i])], 1u);
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t run = 0;
    for (int b = kCostClasses - 1; b >= 0; --b) {
      const uint32_t h = hist[b];
      hist[b] = run;
      run += h;
    }
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
    order[atomicAdd(&hist[cost_class(cost[i])], 1u)] = i;
    cost[i] = 0;
  }
}

}  // namespace

namespace rti {

int ensure_events(rt_scene *s) {
  if (int rc = s->fb.ev0.create_timing()) return rc;
  if (int rc = s->fb.ev1.create_timing()) return rc;
  return s->drop.ev_host.create(hipEventDisableTiming);
}

int ensure_fb(rt_scene *s, size_t px) {
  if (px <= s->fb.cap) return RT_OK;
  s->fb.cap = 0;
  if (int rc = s->fb.color.alloc(px)) return rc;
  if (int rc = s->fb.t.alloc(px)) return rc;
  s->fb.cap = px;
  return RT_OK;
}

}  // namespace rti

namespace {

template <class S, int MAXD>
void launch_render_t(const S &sc, const PlaneDev &pl, const FrameArgs &fa, bool general,
                     hipStream_t stream, unsigned long long *counters, int diag) {
  const dim3 grid((fa.W + kTile - 1) / kTile, (fa.rows_local + kTile - 1) / kTile);
  const dim3 fgrid((fa.W + kFTile - 1) / kFTile, (fa.rows_local + kFTile - 1) / kFTile);
  if (diag == 1) {
    if (general)
      render_kernel<S, MAXD, true, 1><<<grid, kBlock, 0, stream>>>(sc, pl, fa, counters);
    else
      render_kernel<S, MAXD, false, 1><<<grid, kBlock, 0, stream>>>(sc, pl, fa, counters);
  } else if (diag == 2) {
    if (general)
      render_kernel<S, MAXD, true, 2><<<grid, kBlock, 0, stream>>>(sc, pl, fa, counters);
    else
      render_kernel<S, MAXD, false, 2><<<grid, kBlock, 0, stream>>>(sc, pl, fa, counters);
  } else {
    if (general)
      render_kernel<S, MAXD, true, 0><<<fgrid, kFBlock, 0, stream>>>(sc, pl, fa, nullptr);
    else
      render_kernel<S, MAXD, false, 0><<<fgrid, kFBlock, 0, stream>>>(sc, pl, fa, nullptr);
  }
}

// Cost-ordered schedule state for a frame of grid gx x gy blocks on `stream`.
// Two cost / order buffer pairs alternate (rt_scene::d_cost): a frame waits
// for the order kernel of two frames before (ord_ev of its parity: its order
// is ready and its cost buffer zeroed), renders in that order, and its own
// order kernel runs on the side stream after it, concurrently with the next
// frame -- so back-to-back one-frame launches never queue behind an order
// kernel (~8 us at 1080p), at the price of an order two frames old.
#ifndef RT_SCHED_FRESH
#define RT_SCHED_FRESH 1  // A/B switch: 0 always renders in the order two frames old
#endif
int schedule_begin(rt_scene *s, FrameArgs &fa, uint32_t gx, uint32_t gy, hipStream_t stream) {
  fa.order = nullptr;
  fa.cost = nullptr;
  // Frames of this scene arriving on alternating streams are frames in flight:
  // each one's tail is filled by the next frame's tiles. Such frames render in
  // blockIdx order and leave the schedule state alone.
  const bool same_stream = stream == s->sched.last_stream;
  s->sched.last_stream = stream;
  if (!s->info.sched_on || !same_stream) return RT_OK;
  const uint32_t nb = gx * gy;
  if (!s->sched.os.s) {
    char label[64];
    std::snprintf(label, sizeof label, "scene %p schedule stream", (void *)s);
    if (int rc = s->sched.os.create(s->device, label)) return rc;
    for (rtmem::Event &e : s->sched.ord_ev)
      if (int rc = e.create(hipEventDisableTiming)) return rc;
    if (int rc = s->sched.frame_ev.create(hipEventDisableTiming)) return rc;
  }
  if (nb > s->sched.cap) {
    HIP_TRY(hipStreamSynchronize(s->sched.os.s));  // (no order kernel still reads the old buffers)
    s->sched.cap = 0;
    s->sched.key[0] = s->sched.key[1] = 0;
    for (int b = 0; b < 2; ++b) {
      if (int rc = s->sched.cost[b].alloc(nb)) return rc;
      if (int rc = s->sched.order[b].alloc(nb)) return rc;
      HIP_TRY(hipMemsetAsync(s->sched.cost[b].p, 0, (size_t)nb * 4, stream));  // (in the frame's stream order)
    }
    s->sched.cap = nb;
  }
  const int p = s->sched.par;
  if (s->sched.rec[p]) {
    // usually long done (it ran beside the previous frame): then no
    // cross-stream barrier goes into the frame's stream
    const hipError_t q = hipEventQuery(s->sched.ord_ev[p].e);
    if (q == hipErrorNotReady) {
      HIP_TRY(hipStreamWaitEvent(stream, s->sched.ord_ev[p].e, 0));
    } else if (q != hipSuccess) {
      HIP_TRY(q);
    }
  }
  const uint32_t key = (gx << 16) | gy;
  // The previous frame's order when its order kernel has already finished --
  // a frame issued after the host waited for the one before it (the drop-in's
  // Renderer::draw loop) -- else the one two frames old. The previous frame's
  // order buffer is rewritten only by the next frame's order kernel, which
  // runs after the next frame, so after this one.
  if (RT_SCHED_FRESH && s->sched.rec[p ^ 1] && s->sched.key[p ^ 1] == key &&
      hipEventQuery(s->sched.ord_ev[p ^ 1].e) == hipSuccess) {
    fa.order = s->sched.order[p ^ 1].p;
  } else if (s->sched.key[p] == key) {
    fa.order = s->sched.order[p].p;
  }
  fa.cost = s->sched.cost[p].p;
  return RT_OK;
}

// the frame's order kernel on the side stream, after the frame
int schedule_end(rt_scene *s, const FrameArgs &fa, uint32_t gx, uint32_t gy, hipStream_t stream) {
  if (!fa.cost) return RT_OK;
  const int p = s->sched.par;
  HIP_TRY(hipEventRecord(s->sched.frame_ev.e, stream));
  HIP_TRY(hipStreamWaitEvent(s->sched.os.s, s->sched.frame_ev.e, 0));
  order_kernel<<<1, 1024, 0, s->sched.os.s>>>(s->sched.cost[p].p, s->sched.order[p].p, gx * gy);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(s->sched.ord_ev[p].e, s->sched.os.s));
  s->sched.rec[p] = true;
  s->sched.key[p] = (gx << 16) | gy;
  s->sched.par = p ^ 1;
  return RT_OK;
}

}  // namespace

namespace rti {

int launch_render(rt_scene *s, const FrameArgs &fa_in, hipStream_t stream, unsigned long long *counters, int diag,
                  bool sched) {
  FrameArgs fa = fa_in;
  const bool general = s->info.plane.on || fa.P.shading_mode != RT_SHADING_NORMAL;
  const uint32_t gx = (fa.W + kFTile - 1) / kFTile, gy = (fa.rows_local + kFTile - 1) / kFTile;
  fa.order = nullptr;
  fa.cost = nullptr;
  if (diag == 0 && sched) {
    const int rc = schedule_begin(s, fa, gx, gy, stream);
    if (rc) return rc;
  }
  if (!dispatch_scene(s, [&](const auto &sc, auto slots) {
        launch_render_t<std::decay_t<decltype(sc)>, decltype(slots)::value>(sc, s->info.plane, fa, general, stream,
                                                                            counters, diag);
      }))
    return set_err(RT_E_STATE, "scene has no geometry");
  HIP_TRY(hipGetLastError());
  if (diag == 0 && sched) return schedule_end(s, fa, gx, gy, stream);
  return RT_OK;
}

}  // namespace rti

namespace {

// Work-queue heads of render_persist_kernel, one set per (device, stream):
// launches on one stream run in order, and each launch's last wave resets its
// heads, so consecutive launches on a stream reuse them; concurrent streams
// never share a set. The set is allocated and zeroed IN STREAM ORDER
// (hipMallocAsync + hipMemsetAsync on that stream): no device-wide sync, so a
// first launch on a new stream neither stalls the other streams nor breaks a
// graph capture. rt_stream_prepare() does it ahead of time (outside a timed
// region); rt_stream_release() frees the set, again in stream order.
// (the most heads at the default stride, then the waves-done counter; the
// widest RTAMD_QSTRIDE fits with 8 heads, make_queue checks every other pair)
constexpr size_t kQueueWords = (size_t)rtq::kMaxHeads * kHeadStride + 16;
constexpr size_t kQueueBytes = kQueueWords * sizeof(uint32_t);
static_assert((size_t)rtq::kXcds * kHeadStrideMax + 1 <= kQueueWords, "8 heads at the widest stride must fit");
std::mutex g_queue_mu;
std::map<std::pair<int, hipStream_t>, uint32_t *> g_queues;

int stream_queue(hipStream_t stream, uint32_t **out) {
  *out = nullptr;
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(g_queue_mu);
  auto it = g_queues.find({dev, stream});
  if (it != g_queues.end()) {
    *out = it->second;
    return RT_OK;
  }
  void *p = nullptr;
  HIP_TRY(hipMallocAsync(&p, kQueueBytes, stream));
  const hipError_t e = hipMemsetAsync(p, 0, kQueueBytes, stream);
  if (e != hipSuccess) {
    HIP_NOTE(hipFreeAsync(p, stream));
    return set_err(RT_E_DEVICE, std::string("work-queue init: ") + hipGetErrorString(e));
  }
  g_queues[{dev, stream}] = (uint32_t *)p;
  *out = (uint32_t *)p;
  return RT_OK;
}

// Heavy-first order of the block dispatch for row bands (a rank's 1/N of each
// frame at N > 1): with so little work per launch, a rank's time is its
// slowest tiles' chains (silhouette tiles) unless they start first. Each
// (device, stream) keeps the per-tile cost of its previous band launch (the
// slowest wave of each tile, any frame) and the order derived from it
// (order_kernel: half-octave cost classes, heaviest first); consecutive orbit
// frames keep their heavy tiles near the model's outline, so the last launch
// predicts the next. Output-neutral: only the dispatch order changes.
// Off by default: 8 ranks x 16 frames of bunny / the 1.1 M-triangle stand-in,
// two interleaved A/B rounds, came out level within the run-to-run spread
// (profiles/r05/band_order_ab.txt). RTAMD_BAND_ORDER=1 (or rtx_set_band_order)
// switches it on.
struct BandSched {
  uint32_t *cost = nullptr, *order = nullptr;
  uint32_t ntiles = 0;
  bool valid = false;
};
std::map<std::pair<int, hipStream_t>, BandSched> g_band_sched;  // (under g_queue_mu)

bool band_order_env() { return ab_on("RTAMD_BAND_ORDER"); }
std::atomic<bool> g_band_order{band_order_env()};
bool band_order_enabled() { return g_band_order.load(std::memory_order_relaxed); }

int band_sched(hipStream_t stream, uint32_t ntiles, BandSched **out) {
  *out = nullptr;
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(g_queue_mu);
  BandSched &b = g_band_sched[{dev, stream}];
  if (b.ntiles != ntiles) {  // new band geometry: fresh buffers in stream order, no order yet
    if (b.cost) HIP_NOTE(hipFreeAsync(b.cost, stream));
    if (b.order) HIP_NOTE(hipFreeAsync(b.order, stream));
    b = BandSched{};
    void *c = nullptr, *o = nullptr;
    HIP_TRY(hipMallocAsync(&c, (size_t)ntiles * 4, stream));
    HIP_TRY(hipMallocAsync(&o, (size_t)ntiles * 4, stream));
    HIP_TRY(hipMemsetAsync(c, 0, (size_t)ntiles * 4, stream));
    b.cost = (uint32_t *)c;
    b.order = (uint32_t *)o;
    b.ntiles = ntiles;
  }
  *out = &b;
  return RT_OK;
}

// diagnostic per-wave stamps of the persistent launches (rtx_set_persist_stamps)
unsigned long long *g_persist_stamps = nullptr;
int64_t g_persist_stamps_cap = 0;

// RTAMD_PERSIST=0 selects the one-block-per-16x16-tile dispatch (A/B switch).
bool persist_enabled() {
  static const bool on = !ab_off("RTAMD_PERSIST");
  return on;
}

// Which row-band launches take the work queue. A rank's share of a frame is
// 1/N of the pixels; below about a million pixels per frame the queue's drain
// (a wave probes all 8 heads before it exits) and its launch-to-launch
// hand-over cost more than its balancing gains. Bunny 1080p, max over ranks, 8
// frames x 2 streams (ms/frame, queue vs blocks): N = 2 (1.04 M px) 0.0595 vs
// 0.0607, N = 4 0.0425 vs 0.0342, N = 8 0.0379 vs 0.0218. The 1.1 M-triangle
// stand-in at 4K (2.07 M px per rank at N = 4) took 3.18x at N = 4 on the block
// dispatch against 1.93x at N = 2 on the queue (profiles/r03/split_mesh_large.txt).
// RTAMD_BAND_PERSIST=<N> (ranks) or RTAMD_BAND_PERSIST_PX=<pixels> override the
// rule (A/B switches).
// (rtx_set_band_queue_px sets the pixel threshold at run time, for tests)
std::atomic<int64_t> g_band_queue_px{ab_int("RTAMD_BAND_PERSIST_PX", 1000000, INT64_MIN, INT64_MAX)};
bool band_takes_queue(const FrameArgs &f) {
  if (f.nranks <= 1) return true;
  static const int max_ranks = (int)ab_int("RTAMD_BAND_PERSIST", -1, 0, INT32_MAX);
  if (max_ranks >= 0) return f.nranks <= max_ranks;
  return (int64_t)f.rows_local * f.W >= g_band_queue_px.load(std::memory_order_relaxed);
}

// wave tiles per queue item (0: block dispatch); RTAMD_PERSIST_G=1|2|4 overrides
// the scene's default (A/B switch)
int persist_group(int dflt) {
  static const int g = (int)ab_int("RTAMD_PERSIST_G", 0, 1, 4);
  return (g == 1 || g == 2 || g == 4) ? g : dflt;
}

// Resident workgroups of a persistent kernel on the current device (cached per
// kernel instantiation and device).
template <class K>
int resident_blocks(K kernel, int &blocks, int &dev_cached, int block = kBlock) {
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (blocks == 0 || dev != dev_cached) {
    int per_cu = 0, cus = 0;
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, block, 0));
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    // RTAMD_PERSIST_OVERSUB=k launches k x the resident workgroups (A/B
    // switch: extra waves start as resident ones leave and exit at once when
    // the queue is drained)
    static const int oversub = (int)ab_int("RTAMD_PERSIST_OVERSUB", 1, 1, 8);
    blocks = std::max(1, per_cu) * std::max(1, cus) * oversub;
    dev_cached = dev;
  }
  return RT_OK;
}

// Heads of the work queue: 8 (one per XCD) x RT_QUEUE_SUBHEADS sub-heads.
// RTAMD_QHEADS=8|16|32|64 overrides it (A/B switch); rtx_set_queue_heads
// switches inside one process. A stream's head set is all zero between
// launches whatever count the last one ran with, so the count may change from
// launch to launch.
#ifndef RT_QUEUE_SUBHEADS
#define RT_QUEUE_SUBHEADS 2
#endif
static_assert(rtq::heads_ok(rtq::kXcds * RT_QUEUE_SUBHEADS), "RT_QUEUE_SUBHEADS: 1, 2, 4 or 8");
int queue_heads_env() {
  static const int h = [] {
    const long long v = ab_int("RTAMD_QHEADS", rtq::kXcds * RT_QUEUE_SUBHEADS, rtq::kXcds, rtq::kMaxHeads);
    return rtq::heads_ok((uint32_t)v) ? (int)v : (int)(rtq::kXcds * RT_QUEUE_SUBHEADS);
  }();
  return h;
}
std::atomic<int> g_queue_heads{queue_heads_env()};

// Item rectangle (rtq::grid) on / off: RTAMD_QGRID=0 keeps every launch on the
// whole frame's item grid (A/B switch); rtx_set_queue_grid switches inside one
// process.
bool queue_grid_env() {
  static const bool on = !ab_off("RTAMD_QGRID");
  return on;
}
std::atomic<bool> g_queue_grid{queue_grid_env()};
static_assert(rtq::kWhole == kCullWhole, "rtq::grid's whole-frame word is FrameArgs'");
namespace grid_check {  // tile columns 3..6 and row 1 of a 250 x 131 frame, an empty frame, 2x1 items
constexpr uint32_t cx[2] = {3u | (7u << 16), 0u}, cy[2] = {1u | (2u << 16), 0u};
constexpr rtq::Grid g = rtq::grid(cx, cy, 2, 250, 131, 2, 1);
static_assert(g.ox == 1 && g.oy == 1 && g.tiles_x == 3 && g.tiles_y == 1, "rtq::grid");
}  // namespace grid_check

// Whether a launch's items may cover its item rectangle only: whole frames in
// device memory, rows stored at their own place. Row bands, peer and host
// frames keep the whole grid.
bool takes_queue_grid(const FrameBatch &fb, int n) {
  if (!g_queue_grid.load(std::memory_order_relaxed)) return false;
  for (int i = 0; i < n; ++i)
    if (fb.f[i].nranks != 1 || (fb.f[i].flags & (kSysStoreFlags | kFlagNatural | kFlagHostFrame)) != 0 ||
        fb.f[i].W != fb.f[0].W || fb.f[i].rows_local != fb.f[0].rows_local || fb.f[i].flags != fb.f[0].flags)
      return false;
  return true;
}

// Work queue of one multi-frame launch: items of `group` 8x8 wave tiles
// (1: 1x1, 2: 2x1, 4: 2x2) of n frames, the stream's head set; *grid = the
// launch's workgroups (the resident ones, fewer for a small batch; 0: the
// launch has no items). shrink: the items cover the launch's item rectangle
// (rtq::grid) instead of the whole frame.
int make_queue(const FrameBatch &fb, int n, int group, int blocks, hipStream_t stream, PersistQ &q,
               uint32_t &grid, int block = kBlock, bool shrink = false) {
  uint32_t *heads = nullptr;
  if (const int rc = stream_queue(stream, &heads)) return rc;
  q.heads = heads;
  static const uint32_t stride = (uint32_t)ab_int("RTAMD_QSTRIDE", kHeadStride, 1, kHeadStrideMax);
  q.stride = stride;
  q.nheads = (uint32_t)g_queue_heads.load(std::memory_order_relaxed);
  if ((size_t)q.stride * q.nheads + 1 > kQueueWords)
    return set_err(RT_E_INVALID, "work queue: RTAMD_QSTRIDE x the head count does not fit the stream's head set");
  q.gx = group >= 2 ? 2 : 1;
  q.gy = group >= 4 ? 2 : 1;
  uint32_t cx[kMaxBatch], cy[kMaxBatch];
  for (int i = 0; i < n; ++i) {
    cx[i] = shrink ? fb.f[i].cull_x : rtq::kWhole;
    cy[i] = shrink ? (uint32_t)fb.f[i].P.reserved : rtq::kWhole;
  }
  const rtq::Grid g = rtq::grid(cx, cy, (uint32_t)n, (uint32_t)fb.f[0].W, (uint32_t)fb.f[0].rows_local, q.gx, q.gy);
  q.ox = g.ox;
  q.oy = g.oy;
  q.tiles_x = g.tiles_x;
  q.per_frame = g.tiles_x * g.tiles_y;
  q.items = q.per_frame * (uint32_t)n;
  q.cpf = q.nper = 0;  // interleaved order (PersistQ::cpf)
  const uint32_t wpb = (uint32_t)block / 64;  // waves per workgroup
  grid = std::min<uint32_t>((uint32_t)blocks, (q.items + wpb - 1) / wpb);
  q.waves = grid * wpb;
  q.stamps = (g_persist_stamps && (int64_t)q.waves <= g_persist_stamps_cap) ? g_persist_stamps : nullptr;
  return RT_OK;
}

template <class S, int MAXD, bool GENERAL>
int launch_persist_t(rt_scene *s, const S &sc, const PlaneDev &pl, const FrameBatch &fb, int n, int group,
                     hipStream_t stream) {
  static int blocks = 0, dev_cached = -1;
  if (const int rc = resident_blocks(render_persist_kernel<S, MAXD, GENERAL>, blocks, dev_cached, kPBlock)) return rc;
  PersistQ q;
  uint32_t grid = 0;
  const bool shrink = kQueueOrigin<S, GENERAL> && takes_queue_grid(fb, n);
  if (const int rc = make_queue(fb, n, group, blocks, stream, q, grid, kPBlock, shrink)) return rc;
  // Items over the launch's item rectangle only: what lies outside it is every
  // frame's background, which a cleared frame gets from one fill launch ahead
  // of the queue (HITS_ONLY and tPrev frames already hold it)
  const uint32_t W = (uint32_t)fb.f[0].W, H = (uint32_t)fb.f[0].rows_local;
  ClearOutside co;
  co.W = W;
  co.H = H;
  co.x0 = std::min(W, q.ox * q.gx * 8u);
  co.x1 = std::min(W, (q.ox + q.tiles_x) * q.gx * 8u);
  co.y0 = std::min(H, q.oy * q.gy * 8u);
  co.y1 = q.tiles_x ? std::min(H, (q.oy + q.per_frame / q.tiles_x) * q.gy * 8u) : co.y0;
  const bool whole = co.x0 == 0 && co.y0 == 0 && co.x1 == W && co.y1 == H;
  if (!whole && (fb.f[0].flags & RT_FLAG_CLEAR) && !(fb.f[0].flags & RT_FLAG_HITS_ONLY)) {
    for (int i = 0; i < kMaxBatch; ++i) {
      co.color[i] = i < n ? fb.f[i].color : nullptr;
      co.t[i] = i < n ? fb.f[i].t : nullptr;
    }
    clear_outside_kernel<<<dim3((W + 63u) / 64u, (H + 7u) / 8u, (uint32_t)n), 64, 0, stream>>>(co);
  }
  if (grid == 0) return RT_OK;  // every frame's rectangle is empty: the heads stay zero
  render_persist_kernel<S, MAXD, GENERAL><<<grid, kPBlock, 0, stream>>>(sc, pl, fb, q);
  return RT_OK;
}

// The ray pump is measured slower than one tile per wave on every scene (DESIGN.md
// section 8: refills break the coherence of a wave's rays), so primary-ray batches
// take render_persist_kernel unless RTAMD_PUMP=1 or rtx_set_pump(scene, 1) asks
// for the pump; RTAMD_REFILL=<lanes> sets its refill threshold.
bool pump_env() {
  static const bool on = ab_on("RTAMD_PUMP");
  return on;
}
std::atomic<int> g_refill{(int)ab_int("RTAMD_REFILL", RT_REFILL_MIN, 1, 64)};
int refill_min() { return g_refill.load(std::memory_order_relaxed); }

// scenes with a ray-pump adapter (primary-ray batches)
template <class S>
struct PumpOf {
  static constexpr bool kHas = false;
};
template <bool PK>
struct PumpOf<OctS<PK>> {
  static constexpr bool kHas = true;
  using P = OctP;
  static P make(const OctS<PK> &s) { return P{s.d}; }
};
template <int kMode>
struct PumpOf<GridS<kMode>> {
  static constexpr bool kHas = true;
  using P = GridP<kMode>;
  static P make(const GridS<kMode> &s) { return P{s.d}; }
};
// work-queue item of the pump for scenes that otherwise take the block
// dispatch (the grid): 2x2 wave tiles, so a wave's pixel stream claims once per
// 256 pixels
constexpr int kPumpGroup = 4;

template <class P, int MAXD>
int launch_pump_t(const P &sc, const FrameBatch &fb, int n, int group, hipStream_t stream) {
  static int blocks = 0, dev_cached = -1;
  if (const int rc = resident_blocks(render_pump_kernel<P, MAXD>, blocks, dev_cached)) return rc;
  PersistQ q;
  uint32_t grid = 0;
  if (const int rc = make_queue(fb, n, group, blocks, stream, q, grid)) return rc;
  render_pump_kernel<P, MAXD><<<grid, kBlock, 0, stream>>>(sc, fb, q, n, refill_min());
  return RT_OK;
}

template <class S, int MAXD>
int launch_batch_t(rt_scene *s, const S &sc, const PlaneDev &pl, const FrameBatch &fb, int n, bool general,
                   hipStream_t stream) {
  // Row-band tiles (a rank's share of a multi-GPU frame) with fewer than about
  // a million pixels take the block dispatch (band_takes_queue).
  const int group = persist_group(S::kQueueGroup);
  if constexpr (PumpOf<S>::kHas) {
    if (!general && (pump_env() || (s && s->info.pump_on)) && persist_enabled() && band_takes_queue(fb.f[0]))
      return launch_pump_t<typename PumpOf<S>::P, MAXD>(PumpOf<S>::make(sc), fb, n,
                                                        persist_group(S::kQueueGroup ? S::kQueueGroup : kPumpGroup),
                                                        stream);
  }
  if (persist_enabled() && group > 0 && band_takes_queue(fb.f[0])) {
    return general ? launch_persist_t<S, MAXD, true>(s, sc, pl, fb, n, group, stream)
                   : launch_persist_t<S, MAXD, false>(s, sc, pl, fb, n, group, stream);
  }
  const dim3 grid((fb.f[0].W + kBTile - 1) / kBTile, (fb.f[0].rows_local + kBTile - 1) / kBTile, n);
  BandSched *bs = nullptr;
  if (kBBlock == 64 && RT_BATCH_INTERLEAVE && fb.f[0].nranks > 1 && band_order_enabled()) {
    if (const int rc = band_sched(stream, grid.x * grid.y, &bs)) return rc;
  }
  const FrameBatch *fbp = &fb;
  FrameBatch fbo;
  if (bs) {
    fbo = fb;
    fbo.f[0].order = bs->valid ? bs->order : nullptr;
    fbo.f[0].cost = bs->cost;
    fbp = &fbo;
  }
  if (general)
    render_batch_kernel<S, MAXD, true><<<grid, kBBlock, 0, stream>>>(sc, pl, *fbp);
  else
    render_batch_kernel<S, MAXD, false><<<grid, kBBlock, 0, stream>>>(sc, pl, *fbp);
  if (bs) {  // this launch's tile costs -> the next launch's order (and the costs cleared)
    // one wave: it takes the first wave slot the other stream's launch frees
    // (a 1024-thread block would wait for a whole CU and hold this stream's
    // next launch behind it)
    order_kernel<<<1, 64, 0, stream>>>(bs->cost, bs->order, bs->ntiles);
    HIP_TRY(hipGetLastError());
    bs->valid = true;
  }
  return RT_OK;
}

}  // namespace

namespace rti {

// One launch for n <= kMaxBatch frames of equal size / tile (blockIdx order).
int launch_batch(rt_scene *s, FrameBatch &fb, int n, hipStream_t stream) {
  const bool general = s->info.plane.on || fb.f[0].P.shading_mode != RT_SHADING_NORMAL;
  for (int i = 0; i < n; ++i) {
    if (general != (s->info.plane.on || fb.f[i].P.shading_mode != RT_SHADING_NORMAL))
      return set_err(RT_E_INVALID, "frames of one batch must share the shading path");
    fb.f[i].order = nullptr;
    fb.f[i].cost = nullptr;
  }
  int rc = RT_OK;
  if (!dispatch_scene(s, [&](const auto &sc, auto slots) {
        rc = launch_batch_t<std::decay_t<decltype(sc)>, decltype(slots)::value>(s, sc, s->info.plane, fb, n, general,
                                                                                stream);
      }))
    return set_err(RT_E_STATE, "scene has no geometry");
  if (rc) return rc;
  HIP_TRY(hipGetLastError());
  return RT_OK;
}

}  // namespace rti

namespace {

// Whether eye_ray_fast gives eye_ray's bits for every pixel of a W x H frame
// with this inverse projection: the operand ranges rtm::div_mk needs, bounded
// over the whole frame. Every entry zero or of magnitude in [2^-10, 2^10] (the
// z column, which meets z = 0, only finite), so a
// nonzero pos component (NDC steps >= 2^-24) is at least ~2^-60 and at most
// 3 x 2^10; |w| >= 2^-10 over [-1, 1]^2 (one sign); a component of pos whose
// constant term dominates keeps |p| >= 2^-20. Then pos / w, p and p / |p|
// stay in [2^-96, 2^44] (or are +-0). 2 fx / W: every W <= 32768 is checked.
// The reference's projection (perspectiveMatrix(45, W/H, 0.01, 100)) passes.
// RTAMD_FAST_EYE=0 keeps the divisions (A/B switch)
bool fast_eye_enabled() {
  static const bool on = !ab_off("RTAMD_FAST_EYE");
  return on;
}

bool fast_eye_ok(const float *m, int32_t W, int32_t H) {
  if (W > 32768 || H > 32768) return false;
  for (int i = 0; i < 16; ++i) {
    const float a = std::fabs(m[i]);
    if (i >= 8 && i < 12) {  // the z column meets z = 0: any finite entry adds +-0
      if (!std::isfinite(m[i])) return false;
    } else if (!(m[i] == 0.0f || (a >= 0x1p-10f && a <= 0x1p10f))) {
      return false;
    }
  }
  const double wc = std::fabs((double)m[15]), wr = std::fabs((double)m[3]) + std::fabs((double)m[7]);
  if (!(wc - wr >= 0x1p-10)) return false;
  const double wmax = wc + wr;
  double lmin = 0.0;
  for (int i = 0; i < 3; ++i)
    lmin = std::max(lmin, (std::fabs((double)m[12 + i]) - std::fabs((double)m[i]) - std::fabs((double)m[4 + i])) / wmax);
  return lmin >= 0x1p-20;
}

// Tile cull of the mesh primary path: the screen rectangle of a frame outside
// which no pixel can store a hit, so that the kernels skip the ray set-up and
// the traversal of the wave tiles outside it (render_pixels).
// RTAMD_TILE_CULL=0 renders every tile (A/B switch); rtx_set_tile_cull
// switches inside one process.
bool tile_cull_env() {
  static const bool on = !ab_off("RTAMD_TILE_CULL");
  return on;
}
std::atomic<bool> g_tile_cull{tile_cull_env()};

// cull_rect: the rectangle of pixels whose eye rays can reach `box` (xMin yMin
// zMin xMax yMax zMax), as out = {first tile column, last + 1, first tile row,
// last + 1} in 8-pixel tiles of IMAGE columns and rows, padded by 2 pixels and
// rounded outwards; first == last + 1 == 0 is the empty rectangle (the camera
// looks away). Returns false for "whole frame". All arithmetic in double.
// `guard`: n further boxes (xMin xMax yMin yMax zMin zMax each) whose bounds
// the camera must not sit on (the root node's child boxes; see step 3).
//
// The eye ray of pixel (x, loop row y) is d = V3 normalize(q.xyz / q.w) with
// q = proj_inv (nx, ny, 0, 1), nx = 2 (x + .5) / W - 1, ny likewise: z = 0
// drops proj_inv's third column, and the divisions by q.w and |p| only scale,
// so d = s M (nx, ny, 1) with the 3x3 M = V3 [P0 P1 P3] and sign(s) = sign(q.w).
// A point X = o + t d, t > 0, therefore has c = M^-1 (X - o) = t s (nx, ny, 1):
// c.z has the sign of q.w and (nx, ny) = (c.x, c.y) / c.z. With all eight
// corners strictly in front (c.z of that sign) the box is their convex hull
// and projects into the bounding rectangle of their projections. Loop row y is
// stored to image row H - 1 - y.
//
// Lemma: a pixel outside the rectangle stores no hit on the uncut path, for
// every ray the kernels generate.
//  1. A hit lies in the root box. A stored hit needs the root stage
//     (mesh_root) to enter a child, and every child box lies in the box given
//     here, MeshDev::rbox, their exact union. A scene whose root is a leaf has
//     no root stage (its triangles are tested unconditionally and keep
//     negative t): whole frame.
//  2. Finite 1/d. Float subtraction and multiplication are correctly rounded,
//     and b - o is the rounded exact difference of two floats, so each slab
//     distance carries a relative error of a few 2^-24 and a comparison of
//     tMin against tMax goes wrong only when the exact values are that close.
//     Outside the rectangle the ray's line passes the box's projection at 2
//     pixels or more, i.e. (tMin - tMax) / tMax exceeds 2 pixels' angle; frames
//     whose pixel subtends less than 2^-17 of the view vector (or with more
//     than 32768 columns or rows) are "whole frame", which leaves more than an
//     order of magnitude to the 2^-22 of the error. The float direction itself is within ~2^-21
//     of the exact one: a hundredth of such a pixel.
//  3. A zero direction component k: 1/d_k = +-inf, root_box_miss declines and
//     slab_ispc runs on the root's children. With o_k strictly inside a child's
//     range on k, (t1, t2) = (-+inf, +-inf): isp_min / isp_max give (-inf,
//     +inf), the axis drops out as it should. Strictly outside, both are the
//     same infinity: as tMin's operand +inf survives every isp_max (tMin = +inf
//     > tMax <= tFar), as tMax's operand -inf survives every isp_min (tMax < 0)
//     -- a miss, as it should be -- PROVIDED no other operand is NaN, because
//     isp_max(a, NaN) = NaN and isp_max(NaN, tNear) = tNear turn a NaN tMin
//     into tNear and a NaN tMax into tFar: the child would be entered whatever
//     the other axes say. A NaN needs (b - o_k) * inf with b == o_k (an empty
//     slot's +inf bounds give infinities, never NaN). So a camera with a
//     coordinate equal to a bound, on that axis, of the box or of a guard box
//     is "whole frame"; for every other camera the root stage is exact interval
//     logic on the nonzero axes, and step 2 applies to those.
//  4. The negative-t leaf quirk (leaf hits are kept without a range test).
//     Entering a root child needs tMax >= tNear > 0 on the ray's line inside
//     the box; the camera is outside the box (else "whole frame") and the box
//     is convex, so the line's whole stretch inside it has t > 0: every
//     triangle of the scene the line can meet lies ahead of the camera.
bool cull_rect(const rt_render_params *p, int32_t W, int32_t H, const float box[6], const float *guard,
               int n_guard, int32_t out[4]) {
  if (W <= 0 || H <= 0 || W > 32768 || H > 32768) return false;  // (16-bit tile indices; step 2)
  const float *pi = p->proj_inv, *vi = p->view_inv;
  double o[3], M[3][3];
  for (int k = 0; k < 3; ++k) {
    o[k] = (double)p->camera_pos[k];
    if (!std::isfinite(o[k]) || !std::isfinite((double)box[k]) || !std::isfinite((double)box[3 + k])) return false;
    if (!(box[k] <= box[3 + k])) return false;
  }
  // the camera inside or on the box, or on a bound of the box or of a guard box
  bool outside = false;
  for (int k = 0; k < 3; ++k) {
    if (o[k] < (double)box[k] || o[k] > (double)box[3 + k]) outside = true;
    if (o[k] == (double)box[k] || o[k] == (double)box[3 + k]) return false;
    for (int g = 0; g < n_guard; ++g)
      if (o[k] == (double)guard[6 * g + 2 * k] || o[k] == (double)guard[6 * g + 2 * k + 1]) return false;
  }
  if (!outside) return false;
  // q.w keeps one sign over the screen (else the rays flip direction across it)
  const double wc = (double)pi[15], wr = std::fabs((double)pi[3]) + std::fabs((double)pi[7]);
  if (!std::isfinite(wc) || !std::isfinite(wr) || !(std::fabs(wc) > wr * (1.0 + 0x1p-20))) return false;
  const double sgn = wc > 0 ? 1.0 : -1.0;
  const int cols[3] = {0, 1, 3};
  double scale = 0.0;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      double a = 0.0;
      for (int j = 0; j < 3; ++j) a += (double)vi[j * 4 + r] * (double)pi[cols[c] * 4 + j];  // V(r,j) P(j,col)
      if (!std::isfinite(a)) return false;
      M[r][c] = a;
      scale = std::max(scale, std::fabs(a));
    }
  // inverse by cofactors; near-singular: whole frame
  double C[3][3];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      const int r1 = (r + 1) % 3, r2 = (r + 2) % 3, c1 = (c + 1) % 3, c2 = (c + 2) % 3;
      C[r][c] = M[r1][c1] * M[r2][c2] - M[r1][c2] * M[r2][c1];
    }
  const double det = M[0][0] * C[0][0] + M[0][1] * C[0][1] + M[0][2] * C[0][2];
  if (!std::isfinite(det) || !(std::fabs(det) > 1e-9 * scale * scale * scale)) return false;
  // a pixel's share of the view vector (step 2)
  const double l0 = std::sqrt(M[0][0] * M[0][0] + M[1][0] * M[1][0] + M[2][0] * M[2][0]) * 2.0 / W;
  const double l1 = std::sqrt(M[0][1] * M[0][1] + M[1][1] * M[1][1] + M[2][1] * M[2][1]) * 2.0 / H;
  const double l2 = std::sqrt(M[0][2] * M[0][2] + M[1][2] * M[1][2] + M[2][2] * M[2][2]) +
                    std::sqrt(M[0][0] * M[0][0] + M[1][0] * M[1][0] + M[2][0] * M[2][0]) +
                    std::sqrt(M[0][1] * M[0][1] + M[1][1] * M[1][1] + M[2][1] * M[2][1]);
  if (!(l0 >= 0x1p-17 * l2) || !(l1 >= 0x1p-17 * l2)) return false;
  double lo[2] = {std::numeric_limits<double>::infinity(), std::numeric_limits<double>::infinity()};
  double hi[2] = {-lo[0], -lo[1]};
  int behind = 0;
  for (int i = 0; i < 8; ++i) {
    double v[3], c[3];
    for (int k = 0; k < 3; ++k) v[k] = (double)box[((i >> k) & 1) ? 3 + k : k] - o[k];
    for (int r = 0; r < 3; ++r) c[r] = (C[0][r] * v[0] + C[1][r] * v[1] + C[2][r] * v[2]) / det;  // M^-1 = C^T / det
    // strictly in front: c.z of q.w's sign, and not so small that nx, ny
    // leave double's comfort. Strictly behind (all eight: the camera looks
    // away, every t on a line through the box is negative): counted
    const double z = sgn * c[2], zb = 1e-9 * (std::fabs(c[0]) + std::fabs(c[1]));
    if (!std::isfinite(z) || !std::isfinite(zb)) return false;
    if (z < -zb && z < 0.0) {
      ++behind;
      continue;
    }
    if (behind != 0 || !(z > zb) || !(z > 0.0)) return false;
    for (int a = 0; a < 2; ++a) {
      const double n = c[a] / c[2];
      if (!std::isfinite(n)) return false;
      lo[a] = std::min(lo[a], n);
      hi[a] = std::max(hi[a], n);
    }
  }
  if (behind == 8) {
    out[0] = out[1] = out[2] = out[3] = 0;
    return true;
  }
  if (behind != 0) return false;
  // NDC -> pixel centres (n = 2 (x + .5) / W - 1), padded by 2 pixels; clamped
  // in double before the conversion
  const double dim[2] = {(double)W, (double)H};
  int64_t p0[2], p1[2];  // first and last pixel (column; LOOP row)
  for (int a = 0; a < 2; ++a) {
    const double f0 = std::floor((lo[a] + 1.0) * dim[a] * 0.5 - 0.5) - 2.0;
    const double f1 = std::ceil((hi[a] + 1.0) * dim[a] * 0.5 - 0.5) + 2.0;
    p0[a] = (int64_t)std::min(std::max(f0, 0.0), dim[a]);
    p1[a] = (int64_t)std::min(std::max(f1, -1.0), dim[a] - 1.0);
  }
  // loop row y -> image row H - 1 - y
  const int64_t r0 = (int64_t)H - 1 - p1[1], r1 = (int64_t)H - 1 - p0[1];
  if (p0[0] > p1[0] || r0 > r1) {
    out[0] = out[1] = out[2] = out[3] = 0;
    return true;
  }
  out[0] = (int32_t)(p0[0] >> 3);
  out[1] = (int32_t)(p1[0] >> 3) + 1;
  out[2] = (int32_t)(r0 >> 3);
  out[3] = (int32_t)(r1 >> 3) + 1;
  return true;
}

}  // namespace

namespace rti {

int fill_frame(FrameArgs &fa, const rt_scene *s, const rt_render_params *p, uint32_t *c, float *t, int32_t W,
               int32_t H, uint32_t flags, const rt_tile *tile) {
  fa.P = *p;
  // the rectangle: mesh primary rays only (no plane, Normal shading); the
  // shading kernels, the counting and stamping variants and the grids and
  // octrees never read it
  fa.cull_x = kCullWhole;
  fa.P.reserved = (int32_t)kCullWhole;
  if (g_tile_cull.load(std::memory_order_relaxed) && s && s->info.kind == RT_SCENE_MESH && !s->info.plane.on &&
      p->shading_mode == RT_SHADING_NORMAL && s->mesh.root != rtl::kInvalidChild && !(s->mesh.root & rtl::kLeafBit)) {
    int32_t r[4];
    if (cull_rect(p, W, H, s->mesh.root_box, s->mesh.root_child, 8, r)) {
      fa.cull_x = (uint32_t)r[0] | ((uint32_t)r[1] << 16);
      fa.P.reserved = (int32_t)((uint32_t)r[2] | ((uint32_t)r[3] << 16));
    }
  }
  fa.color = c;
  fa.t = t;
  fa.W = W;
  fa.H = H;
  fa.flags = flags;
  fa.band_rows = H;
  fa.rank = 0;
  fa.nranks = 1;
  fa.rows_local = H;
  fa.order = nullptr;
  fa.cost = nullptr;
  fa.hit_box = nullptr;
  if ((flags & RT_FLAG_HITS_ONLY) && !(flags & RT_FLAG_CLEAR))
    return set_err(RT_E_INVALID, "RT_FLAG_HITS_ONLY needs RT_FLAG_CLEAR (a cleared frame)");
  if (flags & ~(RT_FLAG_CLEAR | RT_FLAG_TILE_NATURAL | RT_FLAG_HITS_ONLY))
    return set_err(RT_E_INVALID, "unknown render flag");
  if (tile && tile->num_ranks > 1) {
    if (tile->band_rows <= 0 || tile->rank < 0 || tile->rank >= tile->num_ranks)
      return set_err(RT_E_INVALID, "bad tile");
    fa.band_rows = tile->band_rows;
    fa.rank = tile->rank;
    fa.nranks = tile->num_ranks;
    fa.rows_local = (int32_t)(rt_tile_pixels(W, H, tile) / W);
  }
  if (fast_eye_enabled() && fast_eye_ok(p->proj_inv, W, H)) fa.flags |= kFlagFastEye;
  return RT_OK;
}

}  // namespace rti

extern "C" {

int rt_render_device(rt_scene *s, const rt_render_params *p, uint32_t *d_color, float *d_t, int32_t W,
                     int32_t H, uint32_t flags, const rt_tile *tile, void *stream) {
  if (!s) return set_err(RT_E_INVALID, "scene is NULL");
  int rc = no_instanced(s, "rt_render_device");
  if (rc) return rc;
  if ((rc = check_params(p, W, H))) return rc;
  if (!d_color || !d_t) return set_err(RT_E_INVALID, "NULL framebuffer");
  FrameArgs fa;
  if ((rc = fill_frame(fa, s, p, d_color, d_t, W, H, flags, tile))) return rc;
  if (fa.rows_local <= 0) return RT_OK;
  return launch_render(s, fa, (hipStream_t)stream);
}

int rt_render_device_frames(rt_scene *s, const rt_render_params *params, int32_t frames,
                            uint32_t *const *d_color, float *const *d_t, int32_t W, int32_t H,
                            uint32_t flags, const rt_tile *tile, void *stream) {
  if (!s || !params || !d_color || !d_t || frames < 0) return set_err(RT_E_INVALID, "bad arguments");
  if (int rc = no_instanced(s, "rt_render_device_frames")) return rc;
  if (frames == 1) return rt_render_device(s, params, d_color[0], d_t[0], W, H, flags, tile, stream);
  FrameBatch fb;
  for (int32_t f0 = 0; f0 < frames; f0 += kMaxBatch) {
    const int n = std::min<int32_t>(kMaxBatch, frames - f0);
    for (int i = 0; i < n; ++i) {
      int rc = check_params(params + f0 + i, W, H);
      if (rc) return rc;
      if (!d_color[f0 + i] || !d_t[f0 + i]) return set_err(RT_E_INVALID, "NULL framebuffer");
      if ((rc = fill_frame(fb.f[i], s, params + f0 + i, d_color[f0 + i], d_t[f0 + i], W, H, flags, tile)))
        return rc;
    }
    if (fb.f[0].rows_local <= 0) return RT_OK;
    const int rc = launch_batch(s, fb, n, (hipStream_t)stream);
    if (rc) return rc;
  }
  return RT_OK;
}

int rt_clear_device(uint32_t *d_color, float *d_t, int64_t n, void *stream) {
  if (!d_color || !d_t || n < 0) return set_err(RT_E_INVALID, "bad arguments");
  if (((uintptr_t)d_color | (uintptr_t)d_t) & 15) return set_err(RT_E_INVALID, "buffers must be 16-byte aligned");
  if (n == 0) return RT_OK;
  const int64_t lanes = (n + 3) / 4;
  clear_kernel<<<(unsigned)((lanes + 255) / 256), 256, 0, (hipStream_t)stream>>>(d_color, d_t, n);
  HIP_TRY(hipGetLastError());
  return RT_OK;
}

int rt_stream_prepare(void *stream) {
  uint32_t *heads = nullptr;
  return stream_queue((hipStream_t)stream, &heads);
}

int rt_stream_release(void *stream) {
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  uint32_t *p = nullptr;
  {
    std::lock_guard<std::mutex> lk(g_queue_mu);
    auto b = g_band_sched.find({dev, (hipStream_t)stream});
    if (b != g_band_sched.end()) {  // the band order state (band_sched), freed in stream order too
      if (b->second.cost) HIP_NOTE(hipFreeAsync(b->second.cost, (hipStream_t)stream));
      if (b->second.order) HIP_NOTE(hipFreeAsync(b->second.order, (hipStream_t)stream));
      g_band_sched.erase(b);
    }
    auto it = g_queues.find({dev, (hipStream_t)stream});
    if (it == g_queues.end()) return RT_OK;
    p = it->second;
    g_queues.erase(it);
  }
  HIP_TRY(hipFreeAsync(p, (hipStream_t)stream));
  return RT_OK;
}

// the counting kernel over `frames` frames: all C_ALL counters
static int count_frames(rt_scene *s, const rt_render_params *params, int32_t frames, int32_t W, int32_t H,
                        uint32_t flags, const rt_tile *tile, unsigned long long (&h)[C_ALL]) {
  if (!s || !params || frames <= 0) return set_err(RT_E_INVALID, "bad arguments");
  int rc = no_instanced(s, "rt_count_work");
  if (rc) return rc;
  if ((rc = check_params(params, W, H))) return rc;
  const size_t px = (size_t)W * H;
  if ((rc = ensure_fb(s, px))) return rc;
  rtmem::DevArray<unsigned long long> d;
  if ((rc = d.alloc(C_ALL))) return rc;
  hipError_t e = hipMemset(d.p, 0, d.bytes());
  if (e == hipSuccess) HIP_NOTE(hipMemset(s->fb.t.p, 0x7f, px * 4));
  for (int32_t f = 0; f < frames && e == hipSuccess && rc == RT_OK; ++f) {
    FrameArgs fa;
    if (!(rc = check_params(params + f, W, H)) &&
        !(rc = fill_frame(fa, s, params + f, s->fb.color.p, s->fb.t.p, W, H, flags, tile)))
      rc = launch_render(s, fa, 0, d.p, 1);
  }
  if (e == hipSuccess && rc == RT_OK) e = hipMemcpy(h, d.p, sizeof(h), hipMemcpyDeviceToHost);
  if (rc) return rc;
  if (e != hipSuccess) return set_err(RT_E_DEVICE, std::string("rt_count_work: ") + hipGetErrorString(e));
  return RT_OK;
}

int rt_count_work(rt_scene *s, const rt_render_params *params, int32_t frames, int32_t W, int32_t H,
                  uint32_t flags, const rt_tile *tile, int64_t counters[9]) {
  if (!counters) return set_err(RT_E_INVALID, "bad arguments");
  unsigned long long h[C_ALL] = {};
  const int rc = count_frames(s, params, frames, W, H, flags, tile, h);
  if (rc) return rc;
  for (int i = 0; i < C_NUM; ++i) counters[i] = (int64_t)h[i];
  return RT_OK;
}

// Diagnostic (not part of include/rtamd.h): the wave-level counters of the
// primary mesh path over the same frames as rt_count_work. out[0] = expansions
// that took the shared fetch (C_BVH_SHARED), out[1] = wave-level expansions of
// either form below the root (C_BVH_WAVE_EXP). Zero for scenes and shading
// modes that do not take that path.
int rtx_count_share(rt_scene *s, const rt_render_params *params, int32_t frames, int32_t W, int32_t H,
                    uint32_t flags, int64_t out[2]) {
  if (!out) return set_err(RT_E_INVALID, "bad arguments");
  unsigned long long h[C_ALL] = {};
  const int rc = count_frames(s, params, frames, W, H, flags, nullptr, h);
  if (rc) return rc;
  out[0] = (int64_t)h[C_BVH_SHARED];
  out[1] = (int64_t)h[C_BVH_WAVE_EXP];
  return RT_OK;
}

// Diagnostic (not part of include/rtamd.h): per-wave timestamps of one frame.
// out: 4 x u64 per wave (see DIAG == 2); *nwaves in/out: capacity / written.
int rtx_wave_stamps(rt_scene *s, const rt_render_params *params, int32_t W, int32_t H, uint32_t flags,
                    uint64_t *out, int64_t *nwaves) {
  if (!s || !params || !out || !nwaves) return set_err(RT_E_INVALID, "bad arguments");
  int rc = check_params(params, W, H);
  if (rc) return rc;
  const int64_t nb = (int64_t)((W + kTile - 1) / kTile) * ((H + kTile - 1) / kTile);
  const int64_t nw = nb * (kBlock / 64);
  if (*nwaves < nw) { *nwaves = nw; return set_err(RT_E_INVALID, "buffer too small"); }
  const size_t px = (size_t)W * H;
  if ((rc = ensure_fb(s, px))) return rc;
  rtmem::DevArray<unsigned long long> d;
  if ((rc = d.alloc((size_t)nw * 4))) return rc;
  FrameArgs fa;
  if (!(rc = fill_frame(fa, s, params, s->fb.color.p, s->fb.t.p, W, H, flags, nullptr)))
    rc = launch_render(s, fa, 0, d.p, 2);
  hipError_t e = rc ? hipSuccess : hipMemcpy(out, d.p, d.bytes(), hipMemcpyDeviceToHost);
  if (rc) return rc;
  if (e != hipSuccess) return set_err(RT_E_DEVICE, hipGetErrorString(e));
  *nwaves = nw;
  return RT_OK;
}

// Row bands with at least this many pixels per frame take the work queue
// (band_takes_queue); < 0 restores the default threshold.
int rtx_set_band_queue_px(int64_t px) {
  g_band_queue_px.store(px < 0 ? (int64_t)1000000 : px);
  return RT_OK;
}

// fast_eye_ok for tests (host only): 1 when a W x H frame with this inverse
// projection takes eye_ray_fast. Not part of include/rtamd.h.
int rtx_fast_eye_ok(const float *proj_inv, int32_t W, int32_t H) {
  return proj_inv && fast_eye_ok(proj_inv, W, H) ? 1 : 0;
}

// cull_rect for tests (host only): the tile rectangle of a W x H frame for a
// scene box (xMin yMin zMin xMax yMax zMax) into out[4] = first tile column,
// last + 1, first tile row, last + 1 (image rows, 8-pixel tiles; all zero:
// empty). Returns 1 with a rectangle, 0 for "whole frame" (out untouched).
// Not part of include/rtamd.h.
int rtx_cull_rect(const rt_render_params *p, int32_t W, int32_t H, const float box[6], int32_t out[4]) {
  return p && box && out && cull_rect(p, W, H, box, nullptr, 0, out) ? 1 : 0;
}

// Tile cull of the mesh primary path on (1) / off (0) for the frames filled
// from now on; < 0 restores the RTAMD_TILE_CULL setting. Not part of
// include/rtamd.h.
int rtx_set_tile_cull(int on) {
  g_tile_cull.store(on < 0 ? tile_cull_env() : (on != 0));
  return RT_OK;
}

// Heads of the work queue (8, 16, 32 or 64) for the launches from now on;
// < 0 restores the RTAMD_QHEADS setting. Not part of include/rtamd.h.
int rtx_set_queue_heads(int heads) {
  if (heads >= 0 && !rtq::heads_ok((uint32_t)heads)) return set_err(RT_E_INVALID, "queue heads: 8, 16, 32 or 64");
  g_queue_heads.store(heads < 0 ? queue_heads_env() : heads);
  return RT_OK;
}

// The work queue's item order for tests (host only, rt_queue.h): slot k of
// `head` -> *item (0xFFFFFFFF past the head's last item), and the number of
// slots of `head` that hold an item. rtx_queue_cap returns -1 for a head count
// the queue does not take. Not part of include/rtamd.h.
int rtx_queue_item(uint32_t items, uint32_t heads, uint32_t head, uint32_t k, uint32_t *item) {
  if (!item || !rtq::heads_ok(heads) || head >= heads) return set_err(RT_E_INVALID, "bad queue head");
  *item = rtq::item(items, heads, head, k);
  return RT_OK;
}
int64_t rtx_queue_cap(uint32_t items, uint32_t heads, uint32_t head) {
  if (!rtq::heads_ok(heads) || head >= heads) return -1;
  return (int64_t)rtq::cap(items, heads, head);
}

// The item rectangle of a launch for tests (host only, rtq::grid): `frames`
// pairs of cull words (tile columns in cull_x, tile rows in cull_y, as
// FrameArgs::cull_x and P.reserved), a W x rows frame, items of gx x gy tiles
// -> out[4] = first item column, first item row, columns, rows (in items).
// Not part of include/rtamd.h.
int rtx_queue_grid(const uint32_t *cull_x, const uint32_t *cull_y, int32_t frames, int32_t W, int32_t rows,
                   uint32_t gx, uint32_t gy, uint32_t out[4]) {
  if (!cull_x || !cull_y || !out || frames < 0 || W <= 0 || rows <= 0 || gx < 1 || gx > 2 || gy < 1 || gy > 2)
    return set_err(RT_E_INVALID, "bad queue grid");
  const rtq::Grid g = rtq::grid(cull_x, cull_y, (uint32_t)frames, (uint32_t)W, (uint32_t)rows, gx, gy);
  out[0] = g.ox;
  out[1] = g.oy;
  out[2] = g.tiles_x;
  out[3] = g.tiles_y;
  return RT_OK;
}

// Item rectangle of the persistent launches on (1) / off (0: the whole frame's
// item grid) from now on; < 0 restores the RTAMD_QGRID setting. Not part of
// include/rtamd.h.
int rtx_set_queue_grid(int on) {
  g_queue_grid.store(on < 0 ? queue_grid_env() : (on != 0));
  return RT_OK;
}

// Heavy-first band order on (1) / off (0) from now on; < 0 restores the
// RTAMD_BAND_ORDER setting. Not part of include/rtamd.h.
int rtx_set_band_order(int on) {
  g_band_order.store(on < 0 ? band_order_env() : (on != 0));
  return RT_OK;
}

// Diagnostic: persistent launches from now on write per-wave stamps (see
// PersistQ::stamps) into the device buffer d_buf of cap_waves x 8 u64
// (d_buf = NULL turns it off). Not part of include/rtamd.h.
int rtx_set_persist_stamps(void *d_buf, int64_t cap_waves) {
  g_persist_stamps = (unsigned long long *)d_buf;
  g_persist_stamps_cap = d_buf ? cap_waves : 0;
  return RT_OK;
}

// Diagnostic A/B switch: cooperative tail of the mesh primary path on (default) / off.
int rtx_set_coop(rt_scene *s, int on) {
  if (!s) return set_err(RT_E_INVALID, "scene is NULL");
  s->info.coop = on != 0;
  return RT_OK;
}

// Diagnostic switch: primary-ray batches of this scene on the ray pump
// (render_pump_kernel) instead of one tile per wave (default off).

// the ray pump's refill threshold in lanes (1..64; other values: the default)
int rtx_set_refill(int32_t lanes) {
  g_refill.store((lanes >= 1 && lanes <= 64) ? lanes : RT_REFILL_MIN);
  return RT_OK;
}

int rtx_set_pump(rt_scene *s, int on) {
  if (!s) return set_err(RT_E_INVALID, "scene is NULL");
  s->info.pump_on = on != 0;
  return RT_OK;
}

// Diagnostic A/B switch: cost-ordered block schedule on (default) / off.
int rtx_set_schedule(rt_scene *s, int on) {
  if (!s) return set_err(RT_E_INVALID, "scene is NULL");
  s->info.sched_on = on != 0;
  s->sched.key[0] = s->sched.key[1] = 0;
  return RT_OK;
}

int rt_bench_frames(rt_scene *s, const rt_render_params *params, int32_t frames, int32_t W, int32_t H,
                    uint32_t flags, float *mean_ms, float *total_ms) {
  if (!s || !params || frames <= 0) return set_err(RT_E_INVALID, "bad arguments");
  int rc = no_instanced(s, "rt_bench_frames");
  if (rc) return rc;
  if ((rc = check_params(params, W, H))) return rc;
  const size_t px = (size_t)W * H;
  if ((rc = ensure_fb(s, px)) || (rc = ensure_events(s))) return rc;
  HIP_TRY(hipMemset(s->fb.t.p, 0x7f, px * 4));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipEventRecord(s->fb.ev0.e, 0));
  for (int32_t f = 0; f < frames; ++f) {
    FrameArgs fa;
    if ((rc = check_params(params + f, W, H)) ||
        (rc = fill_frame(fa, s, params + f, s->fb.color.p, s->fb.t.p, W, H, flags, nullptr)) ||
        (rc = launch_render(s, fa, 0)))
      return rc;
  }
  HIP_TRY(hipEventRecord(s->fb.ev1.e, 0));
  HIP_TRY(hipEventSynchronize(s->fb.ev1.e));
  float ms = 0.0f;
  HIP_TRY(hipEventElapsedTime(&ms, s->fb.ev0.e, s->fb.ev1.e));
  if (total_ms) *total_ms = ms;
  if (mean_ms) *mean_ms = ms / (float)frames;
  return RT_OK;
}

}  // extern "C"

// ============================================================ ray queries ==
// rays_kernel behind rt_intersect_rays (host buffers; the shading path's
// per-lane S::intersect on arbitrary rays) and trace_rays_kernel behind
// rt_trace_rays_device (device buffers, closest and any hit, on a stream). An
// instanced scene's rays go on to rt_instances.hip. They are compiled in this
// unit, beside the render kernels whose traversal instantiations they share:
// in a unit of their own, the render kernels come out with other code
// (profiles/r17/README.md).
namespace {

template <class S, int SLOTS>
__global__ __launch_bounds__(kBlock) void rays_kernel(S sc, PlaneDev pl, const float *o3,
                                                       const float *d3, int64_t n, float tn,
                                                       float tf, int32_t *hit, float *t,
                                                       float *nrm, int64_t *prim) {
  __shared__ uint32_t stk[stack_words<S, SLOTS>() * kBlock];
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  StackOf<S, kBlock> st{stk + threadIdx.x};
  const f3 o{o3[3 * i], o3[3 * i + 1], o3[3 * i + 2]};
  const f3 d{d3[3 * i], d3[3 * i + 1], d3[3 * i + 2]};
  NoCnt cnt;
  const SurfHit sh = union_intersect<S, kBlock>(sc, pl, o, d, tn, tf, st, cnt);
  hit[i] = sh.h.hit ? 1 : 0;
  t[i] = sh.h.t;
  nrm[3 * i] = sh.h.n.x;
  nrm[3 * i + 1] = sh.h.n.y;
  nrm[3 * i + 2] = sh.h.n.z;
  prim[i] = sh.h.hit ? sh.h.prim : -1;
}

// ---- rt_trace_rays_device: IScene::intersect on device buffers -------------
// One ray per lane, like rays_kernel, with the work chosen at compile time:
// kRaysAny (S::occluded, one word per ray), kRaysClosest (no normal is
// computed: no tri_normal triangle reload, no grid_normal, oct_trace without
// NEED_NORMAL) and kRaysNormal. The outputs the caller left NULL and the
// per-ray tNear / tFar arrays are wave-uniform branches on kernel arguments.
// The mesh's closest hit is mesh_primary_wave (a wave's last rays finish in
// 8-lane groups), the other traversals are per lane (DESIGN.md section 4;
// what was measured against them is in section 8).
// Workgroup of trace_rays_kernel: one wave. A ray batch has no tile that needs
// four waves together, and a workgroup keeps its LDS stacks until its slowest
// wave ends.
constexpr int kRBlock = 64;
// a launch's global size is a 32-bit count of work-items
constexpr int64_t kMaxRayBlocks = (int64_t)(0xFFFFFFFFu / (uint32_t)kRBlock);

// S::intersect with the normal (and the primitive id's load) optional
template <int B, bool NORMAL, class CT>
__device__ __forceinline__ Hit rays_closest(const MeshS &sc, f3 o, f3 d, float tn, float tf,
                                            LdsStack<B, MeshS::kFields> st, bool want_prim, CT &cnt) {
  float t;
  uint32_t k;
  Hit h = miss_hit();
  if (mesh_trace<B, false>(sc.d, o, d, tn, tf, st, t, k, cnt)) {
    h.hit = true;
    h.t = t;
    if constexpr (NORMAL) h.n = tri_normal(sc.d.tris, k);
    if (want_prim) h.prim = (int64_t)sc.d.tris[k].orig_id;
  }
  return h;
}
template <int B, bool NORMAL, int kMode, class CT>
__device__ __forceinline__ Hit rays_closest(const GridS<kMode> &sc, f3 o, f3 d, float tn, float tf,
                                            LdsStack<B, GridS<kMode>::kFields>, bool, CT &cnt) {
  Hit h = miss_hit();
  f3 p;
  uint32_t cell;
  if (grid_march<kMode>(sc.d, o, d, tn, tf, h.t, p, cell, cnt)) {
    h.hit = true;
    if constexpr (NORMAL) h.n = grid_normal<kMode>(sc.d, p, cnt);
    h.prim = (int64_t)cell;
  } else {
    h.t = kInf;
  }
  return h;
}
template <int B, bool NORMAL, bool PACK, class CT>
__device__ __forceinline__ Hit rays_closest(const OctS<PACK> &sc, f3 o, f3 d, float tn, float tf,
                                            LdsStack<B, kOctFields> st, bool, CT &cnt) {
  Hit h = miss_hit();
  uint32_t node;
  if (oct_trace<B, NORMAL, PACK>(sc.d, o, d, tn, tf, st, h.t, h.n, node, cnt)) {
    h.hit = true;
    h.prim = (int64_t)node;
  } else {
    h.t = kInf;
  }
  return h;
}

// Occupancy floor of the mesh's closest-hit query at 4 and 7 slots: the
// primary kernels' 5 waves per SIMD. Left to itself the compiler took 94 VGPRs
// there before the shared node fetch and 118 (4 waves) with it.
template <class S, int SLOTS, int MODE>
constexpr int trace_min_waves() {
  return (S::kCoop && SLOTS <= 7 && MODE != kRaysAny) ? S::kMinWaves : 1;
}
template <class S, int SLOTS, int MODE>
__global__ __launch_bounds__(kRBlock) __attribute__((amdgpu_waves_per_eu(trace_min_waves<S, SLOTS, MODE>())))
void trace_rays_kernel(S sc, PlaneDev pl, rt_ray_batch b) {
  __shared__ uint32_t stk[stack_words<S, SLOTS>() * kRBlock];
  const int64_t i = (int64_t)blockIdx.x * kRBlock + threadIdx.x;
  // a partial last wave keeps its lanes without a ray: mesh_primary_wave needs
  // the whole wave, so they carry active = false and touch no memory
  const bool active = i < b.n;
  StackOf<S, kRBlock> st{stk + threadIdx.x};
  f3 o{0.0f, 0.0f, 0.0f}, d{0.0f, 0.0f, 1.0f};
  float tn = b.tnear, tf = b.tfar;
  if (active) {
    o = f3{b.d_origin[3 * i], b.d_origin[3 * i + 1], b.d_origin[3 * i + 2]};
    d = f3{b.d_dir[3 * i], b.d_dir[3 * i + 1], b.d_dir[3 * i + 2]};
    if (b.d_tnear) tn = b.d_tnear[i];
    if (b.d_tfar) tf = b.d_tfar[i];
  }
  NoCnt cnt;
  if constexpr (MODE == kRaysAny) {
    if (active) b.d_hit[i] = union_occluded<S, kRBlock>(sc, pl, o, d, tn, tf, st, cnt) ? 1 : 0;
  } else {
    Hit h = miss_hit();
    bool traced = false;
    if constexpr (std::is_same_v<S, MeshS>) {
      // mesh_primary_wave takes one tNear for the wave (tFar is per ray):
      // batches with a d_tnear array take the per-lane traversal below
      if (!b.d_tnear) {
        float t;
        uint32_t k;
        if (mesh_primary_wave<kRBlock, MeshS::kFields>(sc.d, o, d, tn, tf, active, stk, t, k) && active) {
          h.hit = true;
          h.t = t;
          if constexpr (MODE == kRaysNormal) h.n = tri_normal(sc.d.tris, k);
          if (b.d_prim) h.prim = (int64_t)sc.d.tris[k].orig_id;
        }
        traced = true;
      }
    }
    if (!active) return;
    if (!traced) h = rays_closest<kRBlock, MODE == kRaysNormal>(sc, o, d, tn, tf, st, b.d_prim != nullptr, cnt);
    store_closest<MODE>(b, i, pl, RayIn{o, d, tn, tf}, h);
  }
}

template <class S, int MAXD>
void launch_rays_t(const S &sc, const PlaneDev &pl, const float *o, const float *d, int64_t n,
                   float tn, float tf, int32_t *hit, float *t, float *nrm, int64_t *prim) {
  const int64_t blocks = (n + kBlock - 1) / kBlock;
  rays_kernel<S, MAXD><<<(unsigned)blocks, kBlock>>>(sc, pl, o, d, n, tn, tf, hit, t, nrm, prim);
}

template <class S, int MAXD>
void launch_trace_t(const S &sc, const PlaneDev &pl, const rt_ray_batch &b, int mode, hipStream_t stream) {
  const unsigned blocks = (unsigned)((b.n + kRBlock - 1) / kRBlock);
  with_mode(mode, [&](auto m) {
    trace_rays_kernel<S, MAXD, decltype(m)::value><<<blocks, kRBlock, 0, stream>>>(sc, pl, b);
  });
}

// rt_trace_rays_device's launch: an instanced scene goes to rt_instances.hip,
// every other one through the scene dispatch
int launch_trace(rt_scene *s, const rt_ray_batch &b, int mode, hipStream_t stream) {
  if (s->info.kind == RT_SCENE_INSTANCED) {
    // a bottom-level scene refitted since its table entry was written: the
    // entry (and a top-level tree) catch up in stream order ahead of the trace
    if (int rc = rti::instanced_sync(s, stream)) return rc;
    const rti::InstArgs a{s->inst.recs.p, s->inst.tab.p, s->inst.n, s->info.maxd, s->inst.tlas.p, s->inst.tlas_leaves};
    if (s->inst.mixed.p) return rti::trace_mixed_launch(rti::MixedArgs{a, s->inst.mixed.p}, s->info.plane, b, mode, stream);
    return s->inst.tlas.p ? rti::trace_tlas_launch(a, s->info.plane, b, mode, stream)
                     : rti::trace_instances_launch(a, s->info.plane, b, mode, stream);
  }
  if (!dispatch_scene(s, [&](const auto &sc, auto slots) {
        launch_trace_t<std::decay_t<decltype(sc)>, decltype(slots)::value>(sc, s->info.plane, b, mode, stream);
      }))
    return set_err(RT_E_STATE, "scene has no geometry");
  HIP_TRY(hipGetLastError());
  return RT_OK;
}

}  // namespace

extern "C" {

int rt_intersect_rays(rt_scene *s, const float *o, const float *d, int64_t n, float tnear, float tfar,
                      int32_t *hit, float *t, float *normal, int64_t *prim) {
  if (!s || !o || !d || !hit || !t || !normal || !prim) return set_err(RT_E_INVALID, "NULL argument");
  if (n <= 0) return RT_OK;
  const size_t m = (size_t)n;
  rtmem::DevArray<float> aO, aD, aT, aN;
  rtmem::DevArray<int32_t> aH;
  rtmem::DevArray<int64_t> aP;
  hipError_t e = hipSuccess;
  do {
    if ((e = aO.alloc_e(3 * m)) || (e = aD.alloc_e(3 * m)) || (e = aT.alloc_e(m)) || (e = aN.alloc_e(3 * m)) ||
        (e = aH.alloc_e(m)) || (e = aP.alloc_e(m)))
      break;
    float *const dO = aO.p, *const dD = aD.p, *const dT = aT.p, *const dN = aN.p;
    int32_t *const dH = aH.p;
    int64_t *const dP = aP.p;
    if ((e = rtdma::h2d(dO, o, n * 12, nullptr)) || (e = rtdma::h2d(dD, d, n * 12, nullptr))) break;
    if (s->info.kind == RT_SCENE_INSTANCED) {
      // the device entry's kernel on the staged buffers (the same values)
      const rt_ray_batch b{n, dO, dD, nullptr, nullptr, tnear, tfar, dH, dT, dN, dP};
      if (const int rc = launch_trace(s, b, kRaysNormal, nullptr)) return rc;
    } else if (!dispatch_scene(s, [&](const auto &sc, auto slots) {
                 launch_rays_t<std::decay_t<decltype(sc)>, decltype(slots)::value>(sc, s->info.plane, dO, dD, n, tnear,
                                                                                   tfar, dH, dT, dN, dP);
               })) {
      return set_err(RT_E_STATE, "rt_intersect_rays: scene has no geometry");
    }
    if ((e = hipGetLastError())) break;
    if ((e = rtdma::d2h(hit, dH, n * 4, nullptr)) || (e = rtdma::d2h(t, dT, n * 4, nullptr)) ||
        (e = rtdma::d2h(normal, dN, n * 12, nullptr)) || (e = rtdma::d2h(prim, dP, n * 8, nullptr)))
      break;
  } while (0);
  if (e != hipSuccess) return set_err(RT_E_DEVICE, std::string("rt_intersect_rays: ") + hipGetErrorString(e));
  return RT_OK;
}

int rt_trace_rays_device(rt_scene *s, const rt_ray_batch *b, uint32_t flags, void *stream) {
  if (!s) return set_err(RT_E_INVALID, "scene is NULL");
  if (!b) return set_err(RT_E_INVALID, "ray batch is NULL");
  if (flags & ~RT_RAYS_ANY_HIT) return set_err(RT_E_INVALID, "unknown ray flag");
  if (b->n < 0) return set_err(RT_E_INVALID, "negative ray count");
  if (!b->d_origin || !b->d_dir) return set_err(RT_E_INVALID, "NULL ray origins or directions");
  if (!b->d_hit && !b->d_t && !b->d_normal && !b->d_prim) return set_err(RT_E_INVALID, "no output buffer");
  const bool any = (flags & RT_RAYS_ANY_HIT) != 0;
  if (any && (!b->d_hit || b->d_t || b->d_normal || b->d_prim))
    return set_err(RT_E_INVALID, "RT_RAYS_ANY_HIT writes d_hit only: d_t, d_normal and d_prim must be NULL");
  if (b->n / kRBlock + (b->n % kRBlock != 0) > kMaxRayBlocks)
    return set_err(RT_E_INVALID, "ray count exceeds one launch (" + std::to_string(kMaxRayBlocks * kRBlock) +
                                     " rays): split the batch");
  if (b->n == 0) return RT_OK;
  return launch_trace(s, *b, any ? kRaysAny : b->d_normal ? kRaysNormal : kRaysClosest, (hipStream_t)stream);
}

}  // extern "C"
