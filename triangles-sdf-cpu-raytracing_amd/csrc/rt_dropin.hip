// rt_dropin.hip -- rt_render, the drop-in for the reference's Renderer::draw on
// HOST buffers: the copy streams and the staging frame, the zero-copy path of
// cleared frames with its span copies, the boxed download of the others, and
// the small kernels that move their bookkeeping (box_out_kernel,
// clear_spans_kernel). Also rt_untile_device (untile_kernel) and the band of a
// multi-GPU host frame (rti::render_band_host). The frames themselves are
// rendered by rt_device.hip (rti::fill_frame, rti::launch_render).
#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../include/rtamd.h"
#include "rt_error.h"
#include "rt_host.h"
#include "rt_scene.h"

using namespace rtd;
using namespace rti;

namespace {

// rt_render's hit box / row spans (n words) to their pinned, mapped host
// copy: system-scope stores, which the host reads after synchronising the
// stream (a kernel in stream order instead of a small DMA copy)
__global__ void box_out_kernel(const int32_t *d_box, int32_t *h_box, int n) {
  for (int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); i < n; i += (int)(gridDim.x * blockDim.x))
    __hip_atomic_store(h_box + i, d_box[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// the staging frame's stored spans (the row spans of its last frame) cleared
// again, and the span words reset for the next frame: block y clears row y's
// span. A row without hits holds (INT32_MAX, INT32_MAX): it returns before
// any index is formed from them.
__global__ void clear_spans_kernel(uint32_t *c, float *t, int32_t *span, int32_t W) {
  const int32_t y = (int32_t)blockIdx.x, lo = span[2 * y], hi = -span[2 * y + 1];
  __syncthreads();  // (every thread has read the row's span)
  if (threadIdx.x == 0) {
    span[2 * y] = INT32_MAX;
    span[2 * y + 1] = INT32_MAX;
  }
  if (lo > hi || lo < 0 || hi >= W) return;
  for (int32_t x = lo + (int32_t)threadIdx.x; x <= hi; x += (int32_t)blockDim.x) {
    const size_t i = (size_t)y * (size_t)W + (size_t)x;
    c[i] = 0u;
    t[i] = kInf;
  }
}

__global__ void untile_kernel(const uint32_t *pc, const float *pt, int64_t per_rank, uint32_t *c,
                              float *t, int W, int H, int band_rows, int nranks) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)W * H) return;
  const int yo = (int)(i / W), x = (int)(i - (int64_t)yo * W);
  const int b = yo / band_rows, r = b % nranks, k = b / nranks;
  const int64_t src = (int64_t)r * per_rank + ((int64_t)k * band_rows + (yo - b * band_rows)) * W + x;
  if (c) c[i] = pc[src];
  if (t) t[i] = pt[src];
}

// rt_render's two copy/render streams (non-blocking: no implicit sync with
// the null stream) and the event that orders the uploads before the kernel
int ensure_copy_streams(rt_scene *s) {
  for (int k = 0; k < 2; ++k)
    if (!s->drop.xs[k].s) {
      char label[64];
      std::snprintf(label, sizeof label, "scene %p stream %s", (void *)s, k ? "t" : "render/colour");
      if (int rc = s->drop.xs[k].create(s->device, label)) return rc;
    }
  if (int rc = s->drop.xev.create(hipEventDisableTiming)) return rc;
  if (!s->drop.hit_box.p)
    if (int rc = s->drop.hit_box.alloc(4)) return rc;
  if (!s->drop.h_hit_box.dev) return s->drop.h_hit_box.alloc(4, hipHostMallocMapped);
  return RT_OK;
}

// The scene's staging frame (rtdma::HostStage) for px pixels, used by
// rt_render on pageable caller buffers (host copies on one side, DMA on the
// other). Its streams are synchronised before a smaller frame is replaced.
int ensure_stage(rt_scene *s, size_t px) {
  if (px <= s->drop.stage.cap) return RT_OK;
  if (s->drop.xs[0].s) HIP_TRY(hipStreamSynchronize(s->drop.xs[0].s));  // (the previous frame's work on the old frame)
  if (s->drop.xs[1].s) HIP_TRY(hipStreamSynchronize(s->drop.xs[1].s));
  if (const hipError_t e = s->drop.stage.ensure(px))
    return set_err(RT_E_DEVICE, std::string("staging frame: ") + hipGetErrorString(e));
  return RT_OK;
}

// rt_render's failure injection (rtx_render_inject_failure): the next n calls
// fail after their uploads were issued; g_render_drains counts the returns that
// waited for both copy streams (rtx_render_drain_count)
std::atomic<int> g_render_fault{0};
std::atomic<int64_t> g_render_drains{0};

using rtdma::pinned_device_ptr;

// RTAMD_DROPIN_ZC=0: rt_render's cleared frames take the device frame + boxed
// download instead of the zero-copy path (A/B switch)
bool dropin_zero_copy() {
  static const bool on = !ab_off("RTAMD_DROPIN_ZC");
  return on;
}

bool dropin_trace() {
  static const bool on = ab_on("RTAMD_DROPIN_TRACE");
  return on;
}

// The pageable drop-in's staging spans reset by the host threads that copy
// them; RTAMD_HOST_CLEAR=0: by clear_spans_kernel instead (A/B switch).
bool host_clears_stage() {
  static const bool on = !ab_off("RTAMD_HOST_CLEAR");
  return on;
}

// System-scope stores into host frames (kFlagHostFrame); RTAMD_HOST_STORES=agent
// turns them off (A/B switch).
bool host_sys_stores() {
  static const bool on = [] {
    const char *e = ab_env("RTAMD_HOST_STORES");
    return !(e && std::strcmp(e, "agent") == 0);
  }();
  return on;
}

// rt_render of a cleared frame (RT_FLAG_CLEAR | RT_FLAG_HITS_ONLY: the app's
// frameBuf.clear() + draw, src/main.cpp:197,203): only hit pixels differ from
// the caller's buffers (raytracing.cpp:91-94), and the kernel stores exactly
// those -- into HOST memory (zero-copy), so no download follows the kernel:
//  * buffers pinned by rt_host_pin: the hits go straight into them;
//  * pageable buffers: into the scene's pinned staging frame, which is kept
//    cleared. The kernel records, per row, the span of the pixels it stored
//    (kFlagRowSpan); box_out_kernel moves the spans to mapped host memory, the
//    host copies just those spans to the caller's buffers (OpenMP rows) and
//    resets them in the staging frame as it goes (RTAMD_HOST_CLEAR=0: the
//    GPU does, clear_spans_kernel, in stream order before the next frame).
int render_cleared_zero_copy(rt_scene *s, FrameArgs fa, uint32_t *color, float *t, int32_t W, int32_t H,
                             float *ms) {
  const size_t px = (size_t)W * H;
  hipStream_t a = s->drop.xs[0].s;
  rterr::stream_mark(a, "rt_render (zero-copy cleared frame)");
  // every return waits for stream a while it may still touch the caller's
  // buffers; the span-word reset (below) is the library's own and
  // is left running when the call returns
  struct Drain {
    hipStream_t a;
    bool on = true;
    ~Drain() {
      if (on && hipStreamSynchronize(a) == hipSuccess) g_render_drains.fetch_add(1);
    }
  } drain{a};
  void *dc = pinned_device_ptr(color, px * 4), *dt = pinned_device_ptr(t, px * 4);
  fa.flags |= RT_FLAG_HITS_ONLY | (host_sys_stores() ? kFlagHostFrame : 0u);
  fa.hit_box = nullptr;
  if (dc && dt) {
    fa.color = (uint32_t *)dc;
    fa.t = (float *)dt;
    if (g_render_fault.load() > 0) {
      g_render_fault.fetch_sub(1);
      return set_err(RT_E_DEVICE, "injected rt_render failure (rtx_render_inject_failure)");
    }
    HIP_TRY(hipEventRecord(s->fb.ev0.e, a));
    // (the frame's tile-order kernel runs on the schedule's side stream: not waited for)
    if (int rc = launch_render(s, fa, a)) return rc;
    HIP_TRY(hipEventRecord(s->fb.ev1.e, a));
    HIP_TRY(hipEventSynchronize(s->fb.ev1.e));
    drain.on = false;
    if (ms) HIP_TRY(hipEventElapsedTime(ms, s->fb.ev0.e, s->fb.ev1.e));
    return RT_OK;
  }
  if (int rc = ensure_stage(s, px)) return rc;
  void *sc = nullptr, *st = nullptr;
  HIP_TRY(hipHostGetDevicePointer(&sc, s->drop.stage.c, 0));
  HIP_TRY(hipHostGetDevicePointer(&st, s->drop.stage.t, 0));
  if (H > s->drop.span_cap) {
    HIP_TRY(hipStreamSynchronize(a));  // (the previous frame's span clear reads d_row_span)
    s->drop.span_cap = 0;
    if (int rc = s->drop.row_span.alloc((size_t)H * 2)) return rc;
    if (int rc = s->drop.h_row_span.alloc((size_t)H * 2, hipHostMallocMapped)) return rc;
    s->drop.span_cap = H;
    s->drop.stage.mark_dirty();  // (the spans of the frame in the staging frame are gone)
  }
  // (otherwise the previous frame's span reset left both the staging
  // frame and the span words reset)
  if (s->drop.stage.clear_for(W, H)) {
    s->drop.stage.mark_dirty();  // (a failed reset of the span words leaves the next frame to redo both)
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)s->drop.row_span.p, 0x7FFFFFFF, (size_t)H * 2, a));
    s->drop.stage.mark_clean();
  }
  fa.color = (uint32_t *)sc;
  fa.t = (float *)st;
  fa.hit_box = s->drop.row_span.p;
  fa.flags |= kFlagRowSpan;
  if (g_render_fault.load() > 0) {
    g_render_fault.fetch_sub(1);
    return set_err(RT_E_DEVICE, "injected rt_render failure (rtx_render_inject_failure)");
  }
  const auto h0 = std::chrono::steady_clock::now();
  HIP_TRY(hipEventRecord(s->fb.ev0.e, a));
  s->drop.stage.mark_dirty();  // until its spans are cleared again below
  if (int rc = launch_render(s, fa, a)) return rc;
  HIP_TRY(hipEventRecord(s->fb.ev1.e, a));
  box_out_kernel<<<(unsigned)((2 * H + 255) / 256), 256, 0, a>>>(s->drop.row_span.p, s->drop.h_row_span.dev, 2 * H);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(s->drop.ev_host.e, a));
  const auto h1 = std::chrono::steady_clock::now();
  HIP_TRY(hipEventSynchronize(s->drop.ev_host.e));
  const auto h2 = std::chrono::steady_clock::now();
  if (ms) HIP_TRY(hipEventElapsedTime(ms, s->fb.ev0.e, s->fb.ev1.e));
  // the stored spans to the caller (host threads; every other pixel of the
  // caller's cleared frame already holds the staging frame's 0 / +inf); the
  // host resets the same spans of the staging frame as it goes (the GPU only
  // stores into it, from the next call on), and the span words are reset in
  // stream order before the next frame's kernel; the call does not wait for that
  const bool host_clear = host_clears_stage();
  rth::copy_spans(color, t, s->drop.stage.c, s->drop.stage.t, W, H, s->drop.h_row_span.h, 0, host_clear);
  const auto h3 = std::chrono::steady_clock::now();
  drain.on = false;
  if (host_clear) {
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)s->drop.row_span.p, 0x7FFFFFFF, (size_t)H * 2, a));
  } else {
    clear_spans_kernel<<<(unsigned)H, 256, 0, a>>>((uint32_t *)sc, (float *)st, s->drop.row_span.p, W);
    HIP_TRY(hipGetLastError());
  }
  s->drop.stage.mark_clean();
  if (dropin_trace()) {  // RTAMD_DROPIN_TRACE=1: host-side phases of this call (dev switch)
    const auto h4 = std::chrono::steady_clock::now();
    auto us = [](auto x, auto y) { return std::chrono::duration<double, std::micro>(y - x).count(); };
    int64_t pxs = 0;
    for (int32_t y = 0; y < H; ++y)
      if (s->drop.h_row_span.h[2 * y] <= -s->drop.h_row_span.h[2 * y + 1]) pxs += -s->drop.h_row_span.h[2 * y + 1] - s->drop.h_row_span.h[2 * y] + 1;
    std::fprintf(stderr, "dropin: issue %.1f, wait %.1f, copy %.1f (%lld px), clear issue %.1f us; kernel %.1f us\n",
                 us(h0, h1), us(h1, h2), us(h2, h3), (long long)pxs, us(h3, h4), ms ? *ms * 1e3 : -1.0);
  }
  return RT_OK;
}

}  // namespace

extern "C" {

int rt_render(rt_scene *s, const rt_render_params *p, uint32_t *color, float *t, int32_t W, int32_t H,
              uint32_t flags, float *ms) {
  if (!s) return set_err(RT_E_INVALID, "scene is NULL");
  int rc = no_instanced(s, "rt_render");
  if (rc) return rc;
  if ((rc = check_params(p, W, H))) return rc;
  if (!color || !t) return set_err(RT_E_INVALID, "NULL framebuffer");
  if (flags & RT_FLAG_TILE_NATURAL) return set_err(RT_E_INVALID, "rt_render renders whole frames (no tile)");
  // every argument is checked before the first copy is queued
  FrameArgs fa;
  if ((rc = fill_frame(fa, s, p, nullptr, nullptr, W, H, flags & ~RT_FLAG_HITS_ONLY, nullptr))) return rc;
  const size_t px = (size_t)W * H;
  if (flags == (RT_FLAG_CLEAR | RT_FLAG_HITS_ONLY) && dropin_zero_copy()) {
    if ((rc = ensure_events(s)) || (rc = ensure_copy_streams(s))) return rc;
    return render_cleared_zero_copy(s, fa, color, t, W, H, ms);
  }
  if ((rc = ensure_fb(s, px)) || (rc = ensure_events(s)) || (rc = ensure_copy_streams(s))) return rc;
  fa.color = s->fb.color.p;
  fa.t = s->fb.t.p;
  // The DMA engines only ever see pinned memory (rtdma):
  // buffers pinned by rt_host_pin are copied directly; pageable ones go through
  // the scene's staging frame, host threads copying between it and the caller's
  // buffers on the host side of each DMA (hc / ht: where the DMAs read / write).
  const bool direct = rtdma::pinned(color, px * 4) && rtdma::pinned(t, px * 4);
  if (!direct && (rc = ensure_stage(s, px))) return rc;
  uint32_t *hc = direct ? color : s->drop.stage.c;
  float *ht = direct ? t : s->drop.stage.t;
  // colour and t move on two streams (two DMA engines, concurrent). Once a copy
  // is queued, every return -- an error included -- first waits for both
  // streams, so the caller may unpin or free its buffers as soon as the call
  // returns.
  hipStream_t a = s->drop.xs[0].s, b = s->drop.xs[1].s;
  rterr::stream_mark(a, "rt_render (render + colour copies)");
  rterr::stream_mark(b, "rt_render (t copies)");
  struct Drain {
    hipStream_t a, b;
    ~Drain() {
      const hipError_t ea = hipStreamSynchronize(a), eb = hipStreamSynchronize(b);
      if (ea == hipSuccess && eb == hipSuccess) g_render_drains.fetch_add(1);
    }
  } drain{a, b};
  // Which pixels can differ from the caller's buffers after the frame:
  //  * RT_FLAG_CLEAR: every pixel (misses become 0 / +inf), so all are copied back;
  //  * RT_FLAG_CLEAR | RT_FLAG_HITS_ONLY: the caller's buffers already hold a
  //    cleared frame (the app's frameBuf.clear() + draw, src/main.cpp:197,203),
  //    so only stored hits differ (raytracing.cpp:91-94);
  //  * no flag (tPrev frame): colour and t are written only on hit, so again
  //    only stored hits differ.
  // In the last two cases the kernel records the bounding box of its stored
  // pixels and only that box is copied back. The device frame is always
  // written whole (a cleared frame) or uploaded whole (tPrev), so the box
  // holds exactly the caller's values outside the hits.
  const bool boxed = !(flags & RT_FLAG_CLEAR) || (flags & RT_FLAG_HITS_ONLY);
  if (!direct) s->drop.stage.mark_dirty();  // (the zero-copy path's cleared staging frame is overwritten)
  if (!(flags & RT_FLAG_CLEAR)) {
    if (!direct) rth::copy_rect(hc, ht, color, t, W, 0, W - 1, 0, H - 1, 0);
    HIP_TRY(hipMemcpyAsync(s->fb.color.p, hc, px * 4, hipMemcpyHostToDevice, a));
    HIP_TRY(hipMemcpyAsync(s->fb.t.p, ht, px * 4, hipMemcpyHostToDevice, b));
    HIP_TRY(hipEventRecord(s->drop.xev.e, b));
    HIP_TRY(hipStreamWaitEvent(a, s->drop.xev.e, 0));
  }
  if (g_render_fault.load() > 0) {
    g_render_fault.fetch_sub(1);
    return set_err(RT_E_DEVICE, "injected rt_render failure (rtx_render_inject_failure)");
  }
  if (boxed) {
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)s->drop.hit_box.p, 0x7FFFFFFF, 4, a));
    fa.hit_box = s->drop.hit_box.p;
  }
  HIP_TRY(hipEventRecord(s->fb.ev0.e, a));
  if ((rc = launch_render(s, fa, a))) return rc;
  HIP_TRY(hipEventRecord(s->fb.ev1.e, a));
  int32_t x0 = 0, x1 = W - 1, y0 = 0, y1 = H - 1;  // the region copied back
  if (!boxed) {
    HIP_TRY(hipStreamWaitEvent(b, s->fb.ev1.e, 0));
    HIP_TRY(hipMemcpyAsync(ht, s->fb.t.p, px * 4, hipMemcpyDeviceToHost, b));
    HIP_TRY(hipMemcpyAsync(hc, s->fb.color.p, px * 4, hipMemcpyDeviceToHost, a));
  } else {
    box_out_kernel<<<1, 64, 0, a>>>(s->drop.hit_box.p, s->drop.h_hit_box.dev, 4);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(a));
    x0 = s->drop.h_hit_box.h[0], x1 = -s->drop.h_hit_box.h[1], y0 = s->drop.h_hit_box.h[2], y1 = -s->drop.h_hit_box.h[3];
    if (x0 <= x1 && y0 <= y1) {  // else: no hit, nothing changed
      HIP_TRY(hipStreamWaitEvent(b, s->fb.ev1.e, 0));
      const size_t off = (size_t)y0 * W + x0, rows = (size_t)(y1 - y0 + 1), w = (size_t)(x1 - x0 + 1);
      if (w * 2 > (size_t)W) {  // wide box: whole rows, one contiguous copy per buffer
        x0 = 0;
        x1 = W - 1;
        HIP_TRY(hipMemcpyAsync(ht + (size_t)y0 * W, s->fb.t.p + (size_t)y0 * W, rows * W * 4, hipMemcpyDeviceToHost, b));
        HIP_TRY(hipMemcpyAsync(hc + (size_t)y0 * W, s->fb.color.p + (size_t)y0 * W, rows * W * 4,
                               hipMemcpyDeviceToHost, a));
      } else {
        HIP_TRY(hipMemcpy2DAsync(ht + off, (size_t)W * 4, s->fb.t.p + off, (size_t)W * 4, w * 4, rows,
                                 hipMemcpyDeviceToHost, b));
        HIP_TRY(hipMemcpy2DAsync(hc + off, (size_t)W * 4, s->fb.color.p + off, (size_t)W * 4, w * 4, rows,
                                 hipMemcpyDeviceToHost, a));
      }
    }
  }
  HIP_TRY(hipStreamSynchronize(a));
  HIP_TRY(hipStreamSynchronize(b));
  if (!direct && x0 <= x1 && y0 <= y1) rth::copy_rect(color, t, hc, ht, W, x0, x1, y0, y1, 0);
  if (ms) HIP_TRY(hipEventElapsedTime(ms, s->fb.ev0.e, s->fb.ev1.e));
  return RT_OK;
}

// test hooks: fail the next n rt_render calls after their uploads; how many
// rt_render returns have waited for both copy streams
int rtx_render_inject_failure(int32_t n) {
  g_render_fault.store(n);
  return RT_OK;
}
int64_t rtx_render_drain_count(void) { return g_render_drains.load(); }

int rt_untile_device(const uint32_t *d_packed_color, const float *d_packed_t, int64_t per_rank_pixels,
                     uint32_t *d_color, float *d_t, int32_t W, int32_t H, const rt_tile *tile,
                     void *stream) {
  if (!tile || tile->num_ranks < 1 || tile->band_rows <= 0 || W <= 0 || H <= 0)
    return set_err(RT_E_INVALID, "bad tile");
  const int64_t n = (int64_t)W * H;
  untile_kernel<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(
      d_packed_color, d_packed_t, per_rank_pixels, d_color, d_t, W, H, tile->band_rows, tile->num_ranks);
  HIP_TRY(hipGetLastError());
  return RT_OK;
}

}  // extern "C"

// ------------------------------------------------ rt_multi_render internals --
namespace rti {
// One slot of rt_multi_render's zero-copy cleared frame (RT_FLAG_CLEAR |
// RT_FLAG_HITS_ONLY over a cleared host frame): the slot's bands of `tile` go
// through the one-frame kernel on `stream`, storing only their hits, at their
// own rows of the W x H host frame whose device addresses (on the scene's
// device) are dc / dt (kFlagNatural: one frame shared by every slot). With
// d_span != NULL the kernel records per LOCAL row (tile->rank's rows in
// increasing order) the span of the pixels it stored (kFlagRowSpan, 2 words per
// row, pre-set to INT32_MAX by the caller).
int render_band_host(rt_scene *s, const rt_render_params *p, uint32_t *dc, float *dt, int32_t W, int32_t H,
                     const rt_tile *tile, int32_t *d_span, hipStream_t stream) {
  if (!s) return set_err(RT_E_INVALID, "scene is NULL");
  if (int rc = check_params(p, W, H)) return rc;
  FrameArgs fa;
  if (int rc = fill_frame(fa, s, p, dc, dt, W, H, RT_FLAG_CLEAR | RT_FLAG_HITS_ONLY, tile)) return rc;
  if (fa.rows_local <= 0) return RT_OK;
  fa.flags |= kFlagHostFrame | kFlagNatural | (d_span ? kFlagRowSpan : 0u);
  fa.hit_box = d_span;
  return launch_render(s, fa, stream);
}

}  // namespace rti
