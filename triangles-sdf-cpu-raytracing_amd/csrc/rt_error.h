// rt_error.h -- the library's error slot behind rt_last_error() (one per host
// thread), the HIP error check used by every C entry point, the registry of the
// library's own HIP streams and the copies between the device and caller host
// memory with their staging frame (rtdma).
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/rtamd.h"

namespace rterr {
int set(int code, const std::string &msg);  // stores msg, returns code
const char *get();
// A HIP call whose failure librtamd does not return (destroy paths, best-effort
// cleanup) goes through HIP_NOTE: its name and error are remembered (per host
// thread), because HIP keeps the failure as the thread's pending last error,
// and a later hipGetLastError() -- or a synchronous call that reports it --
// would otherwise blame whatever call comes next.
hipError_t note(const char *call, hipError_t e);
// The pending HIP last error of this thread, read and cleared: "" when none,
// else a message naming the librtamd call that raised it (or "outside
// librtamd": torch, the caller). Entry points call it before their first
// copy, so a stale error is reported as such and not as the copy's failure.
std::string take_stale();

// Streams the library creates (scene copy/render streams, rt_multi slots, the
// SDF query stream), each with a label and the last library call that queued
// work on it (stream_mark). rt_host_unpin drains them all before it
// unregisters a range, and a sticky device error (a kernel or DMA fault, which
// HIP reports on whatever call comes next) is attributed: the message lists the
// library streams whose hipStreamQuery reports an error and what was last
// queued on each.
void stream_add(hipStream_t s, int device, const std::string &label);
void stream_remove(hipStream_t s);
void stream_mark(hipStream_t s, const char *what);
hipError_t streams_sync();     // every registered stream on its device; the first failure
std::string stream_faults();   // "" or "; library streams reporting errors: ..."
// The message of a failed HIP call: "expr: error", plus stream_faults() when
// the error is a sticky device fault.
std::string hip_fail(const char *expr, hipError_t e);
}  // namespace rterr
static inline int set_err(int code, const std::string &msg) { return rterr::set(code, msg); }
static inline int check_params(const rt_render_params *p, int32_t W, int32_t H) {
  if (!p) return set_err(RT_E_INVALID, "params is NULL");
  if (W <= 0 || H <= 0 || (int64_t)W * H > (int64_t)1 << 31) return set_err(RT_E_INVALID, "bad frame size");
  if (p->shading_mode < 0 || p->shading_mode > 2) return set_err(RT_E_INVALID, "bad shading mode");
  return RT_OK;
}

// Copies between device memory and CALLER host memory. The runtime's DMA only
// ever sees pinned memory: host ranges the caller pinned with rt_host_pin are
// copied directly, any other (pageable) host memory goes through a
// process-wide pinned bounce buffer (hipHostMalloc), with a host memcpy on one
// side of the DMA. Both return when the host range may be reused (they
// synchronise `st`). DESIGN.md section 0e: the round-5 GPU-suite stop was a
// runtime DMA from a caller's pageable buffer.
namespace rtdma {
// the device address of host range [p, p + bytes) when it lies inside one range
// pinned by rt_host_pin (on the current device), else nullptr
void *pinned_device_ptr(const void *p, size_t bytes);
bool pinned(const void *p, size_t bytes);
hipError_t h2d(void *d, const void *h, size_t n, hipStream_t st);
hipError_t d2h(void *h, const void *d, size_t n, hipStream_t st);

// The pinned host frame (colour + t) behind rt_render and rt_multi_render on
// pageable caller buffers: the zero-copy cleared frame stores its hits into it
// and the other frames' uploads / downloads go through it. The runtime owns the
// memory (hipHostMalloc with `flags`), never handed back to the process heap,
// so no caller buffer can later land on pages this library registered and
// unregistered (aligned_alloc + hipHostRegister did that in round 5). It stays
// cleared (0 / +inf) between cleared frames of one size: the host resets each
// span it copies out.
struct HostStage {
  uint32_t *c = nullptr;
  float *t = nullptr;
  size_t cap = 0;  // pixels
  explicit HostStage(unsigned flags) : flags_(flags) {}
  // room for px pixels; the owner drains the streams that use the frame before
  // it grows (px > cap)
  hipError_t ensure(size_t px);
  void mark_dirty() { dirty_ = true; }
  void mark_clean() { dirty_ = false; }  // every span stored since clear_for is reset again
  // a cleared W x H frame: cleared here when it is dirty or was last cleared
  // for another size (returns true), else left as the span resets kept it
  bool clear_for(int32_t W, int32_t H);
  void release();  // the owner has synchronised the streams that use it
  // (so has whoever destroys it: a handle's destroy entry drains, then deletes)
  ~HostStage() { release(); }
  HostStage(const HostStage &) = delete;
  HostStage &operator=(const HostStage &) = delete;

 private:
  unsigned flags_;
  int32_t W_ = 0, H_ = 0;
  bool dirty_ = true;
};
}  // namespace rtdma

namespace rti {  // librtamd-internal entry points shared between its translation units
int render_band_host(rt_scene *s, const rt_render_params *p, uint32_t *dc, float *dt, int32_t W, int32_t H,
                     const rt_tile *tile, int32_t *d_span, hipStream_t stream);
// A scene's update counter (rt_scene_update_vertices*), and a replica of it
// brought up to date: rt_multi re-copies its replicas when the root has moved.
uint64_t scene_version(const rt_scene *s);
int scene_refresh_replica(rt_scene *rep, const rt_scene *src);
}  // namespace rti

#define HIP_NOTE(expr) ((void)rterr::note(#expr, (expr)))

#define HIP_TRY(expr)                                                   \
  do {                                                                  \
    hipError_t e_ = (expr);                                             \
    if (e_ != hipSuccess) return rterr::set(RT_E_DEVICE, rterr::hip_fail(#expr, e_)); \
  } while (0)
