// rt_runtime.hip -- what rt_error.h declares (the error slot, the registry of
// the library's streams, the copies to and from caller host memory, the
// staging frame) and the entry points about the process and its memory:
// devices, pinned host ranges, exchange slots, IPC handles. Host code only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../include/rtamd.h"
#include "rt_error.h"
#include "rt_host.h"

namespace rterr {
thread_local std::string g_err;
int set(int code, const std::string &msg) {
  g_err = msg;
  return code;
}
const char *get() { return g_err.c_str(); }
thread_local std::string g_noted;
thread_local hipError_t g_noted_err = hipSuccess;
hipError_t note(const char *call, hipError_t e) {
  if (e != hipSuccess) {
    g_noted = call;
    g_noted_err = e;
  }
  return e;
}
std::string take_stale() {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return {};
  std::string m = std::string("stale HIP error ") + hipGetErrorName(e) + " (" + hipGetErrorString(e) +
                  ") was pending from an earlier call: ";
  m += e == g_noted_err ? "librtamd's " + g_noted : std::string("a HIP call outside librtamd");
  g_noted.clear();
  g_noted_err = hipSuccess;
  return m;
}

namespace {
struct StreamInfo {
  int device;
  std::string label;
  const char *last;  // the last library call that queued work on it (static strings)
};
std::mutex g_stream_mu;
std::map<hipStream_t, StreamInfo> g_streams;

// errors HIP keeps for the context once raised (a faulting kernel or copy):
// every later call may report them, whichever work raised them
bool sticky(hipError_t e) {
  return e == hipErrorIllegalAddress || e == hipErrorLaunchFailure || e == hipErrorLaunchTimeOut ||
         e == hipErrorAssert || e == hipErrorIllegalState || e == hipErrorUnknown;
}
}  // namespace

void stream_add(hipStream_t s, int device, const std::string &label) {
  std::lock_guard<std::mutex> lk(g_stream_mu);
  g_streams[s] = StreamInfo{device, label, "(nothing queued yet)"};
}
void stream_remove(hipStream_t s) {
  std::lock_guard<std::mutex> lk(g_stream_mu);
  g_streams.erase(s);
}
void stream_mark(hipStream_t s, const char *what) {
  std::lock_guard<std::mutex> lk(g_stream_mu);
  auto it = g_streams.find(s);
  if (it != g_streams.end()) it->second.last = what;
}
hipError_t streams_sync() {
  std::vector<std::pair<hipStream_t, int>> all;
  {
    std::lock_guard<std::mutex> lk(g_stream_mu);
    for (const auto &kv : g_streams) all.emplace_back(kv.first, kv.second.device);
  }
  int prev = 0;
  if (const hipError_t e = hipGetDevice(&prev)) return e;
  hipError_t first = hipSuccess;
  for (const auto &[s, dev] : all) {
    hipError_t e = hipSetDevice(dev);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess && first == hipSuccess) first = e;
  }
  (void)hipSetDevice(prev);
  return first;
}
std::string stream_faults() {
  std::vector<std::pair<hipStream_t, StreamInfo>> all;
  {
    std::lock_guard<std::mutex> lk(g_stream_mu);
    for (const auto &kv : g_streams) all.emplace_back(kv.first, kv.second);
  }
  int prev = 0;
  (void)hipGetDevice(&prev);
  std::string m;
  for (const auto &[s, info] : all) {
    if (hipSetDevice(info.device) != hipSuccess) continue;
    const hipError_t e = hipStreamQuery(s);
    if (e == hipSuccess || e == hipErrorNotReady) continue;
    m += (m.empty() ? "" : "; ") + info.label + " (device " + std::to_string(info.device) + ", last queued: " +
         info.last + "): " + hipGetErrorName(e);
  }
  (void)hipSetDevice(prev);
  (void)hipGetLastError();  // (the queries' errors are reported here, not left pending)
  return m.empty() ? std::string("; no librtamd stream reports an error (the fault came from work queued "
                                 "by this call itself or outside librtamd)")
                   : "; librtamd streams reporting errors: " + m;
}
std::string hip_fail(const char *expr, hipError_t e) {
  std::string m = std::string(expr) + ": " + hipGetErrorString(e);
  if (sticky(e)) m += stream_faults();
  return m;
}
}  // namespace rterr

// ------------------------------------------------ caller host memory (rtdma) --
namespace {
// Host ranges pinned through rt_host_pin (base -> bytes): rt_render writes a
// cleared frame's hits straight into such buffers, and rtdma DMAs them directly.
std::mutex g_pin_mu;
std::map<uintptr_t, size_t> g_pins;

// The process-wide bounce buffer of rtdma: two halves of kBounce bytes of
// pinned host memory (allocated on first use, kept for the process).
constexpr size_t kBounce = 8u << 20;
std::mutex g_bounce_mu;
char *g_bounce[2] = {nullptr, nullptr};

hipError_t bounce_ready() {
  for (char *&b : g_bounce)
    if (!b)
      if (const hipError_t e = hipHostMalloc((void **)&b, kBounce, hipHostMallocPortable)) {
        b = nullptr;
        return e;
      }
  return hipSuccess;
}
}  // namespace

namespace rtdma {
void *pinned_device_ptr(const void *p, size_t bytes) {
  const uintptr_t a = (uintptr_t)p;
  uintptr_t base = 0;
  {
    std::lock_guard<std::mutex> lk(g_pin_mu);
    auto it = g_pins.upper_bound(a);
    if (it == g_pins.begin()) return nullptr;
    --it;
    if (a < it->first || a + bytes > it->first + it->second) return nullptr;
    base = it->first;
  }
  void *d = nullptr;
  if (hipHostGetDevicePointer(&d, (void *)base, 0) != hipSuccess || !d) {
    (void)hipGetLastError();  // (not mapped: take the staged path)
    return nullptr;
  }
  return (char *)d + (a - base);
}
bool pinned(const void *p, size_t bytes) {
  const uintptr_t a = (uintptr_t)p;
  std::lock_guard<std::mutex> lk(g_pin_mu);
  auto it = g_pins.upper_bound(a);
  if (it == g_pins.begin()) return false;
  --it;
  return a >= it->first && a + bytes <= it->first + it->second;
}
hipError_t h2d(void *d, const void *h, size_t n, hipStream_t st) {
  if (n == 0) return hipSuccess;
  if (pinned(h, n)) {
    hipError_t e = hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    return e;
  }
  std::lock_guard<std::mutex> lk(g_bounce_mu);
  if (const hipError_t e = bounce_ready()) return e;
  // chunk k fills half k & 1 while the DMA of chunk k - 1 runs from the other
  for (size_t off = 0, k = 0; off < n; off += kBounce, ++k) {
    const size_t m = std::min(kBounce, n - off);
    if (k >= 2)
      if (const hipError_t e = hipStreamSynchronize(st)) return e;
    std::memcpy(g_bounce[k & 1], (const char *)h + off, m);
    if (const hipError_t e = hipMemcpyAsync((char *)d + off, g_bounce[k & 1], m, hipMemcpyHostToDevice, st)) {
      (void)hipStreamSynchronize(st);
      return e;
    }
  }
  return hipStreamSynchronize(st);
}
hipError_t d2h(void *h, const void *d, size_t n, hipStream_t st) {
  if (n == 0) return hipSuccess;
  if (pinned(h, n)) {
    hipError_t e = hipMemcpyAsync(h, d, n, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    return e;
  }
  std::lock_guard<std::mutex> lk(g_bounce_mu);
  if (const hipError_t e = bounce_ready()) return e;
  // two chunks per round trip: both DMAs queued, then both copied out
  for (size_t off = 0; off < n; off += 2 * kBounce) {
    size_t m[2] = {0, 0};
    for (int k = 0; k < 2 && off + k * kBounce < n; ++k) {
      m[k] = std::min(kBounce, n - off - k * kBounce);
      if (const hipError_t e = hipMemcpyAsync(g_bounce[k], (const char *)d + off + k * kBounce, m[k],
                                              hipMemcpyDeviceToHost, st)) {
        (void)hipStreamSynchronize(st);
        return e;
      }
    }
    if (const hipError_t e = hipStreamSynchronize(st)) return e;
    for (int k = 0; k < 2; ++k)
      if (m[k]) std::memcpy((char *)h + off + k * kBounce, g_bounce[k], m[k]);
  }
  return hipSuccess;
}
hipError_t HostStage::ensure(size_t px) {
  if (px <= cap) return hipSuccess;
  release();
  for (void **q : {(void **)&c, (void **)&t})
    if (const hipError_t e = hipHostMalloc(q, px * 4, flags_)) {
      *q = nullptr;
      release();
      return e;
    }
  cap = px;
  dirty_ = true;
  return hipSuccess;
}
bool HostStage::clear_for(int32_t W, int32_t H) {
  if (!dirty_ && W_ == W && H_ == H) return false;
  rth::clear_frame(c, t, (int64_t)W * H, 8);
  W_ = W;
  H_ = H;
  dirty_ = false;
  return true;
}
void HostStage::release() {
  if (c) HIP_NOTE(hipHostFree(c));
  if (t) HIP_NOTE(hipHostFree(t));
  c = nullptr;
  t = nullptr;
  cap = 0;
}
}  // namespace rtdma

extern "C" {

const char *rt_last_error(void) { return rterr::get(); }
int rt_abi_version(void) { return RTAMD_ABI_VERSION; }

int rt_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int rt_set_device(int device) {
  HIP_TRY(hipSetDevice(device));
  return RT_OK;
}

// Exchange slots: uncached device memory, so stores arriving from a peer GPU
// over xGMI are never shadowed by stale lines in this GPU's L2.
int rt_exchange_alloc(int64_t bytes, void **d_ptr) {
  if (!d_ptr || bytes <= 0) return set_err(RT_E_INVALID, "bad arguments");
  *d_ptr = nullptr;
  HIP_TRY(hipExtMallocWithFlags(d_ptr, (size_t)bytes, hipDeviceMallocUncached));
  return RT_OK;
}

int rt_exchange_free(void *d_ptr) {
  if (d_ptr) HIP_TRY(hipFree(d_ptr));
  return RT_OK;
}

int rt_ipc_get_handle(void *d_ptr, uint8_t handle[RT_IPC_HANDLE_BYTES]) {
  static_assert(sizeof(hipIpcMemHandle_t) == RT_IPC_HANDLE_BYTES, "IPC handle size");
  if (!d_ptr || !handle) return set_err(RT_E_INVALID, "bad arguments");
  hipIpcMemHandle_t h;
  HIP_TRY(hipIpcGetMemHandle(&h, d_ptr));
  std::memcpy(handle, &h, sizeof h);
  return RT_OK;
}

int rt_ipc_open(const uint8_t handle[RT_IPC_HANDLE_BYTES], void **d_ptr) {
  if (!d_ptr || !handle) return set_err(RT_E_INVALID, "bad arguments");
  *d_ptr = nullptr;
  hipIpcMemHandle_t h;
  std::memcpy(&h, handle, sizeof h);
  HIP_TRY(hipIpcOpenMemHandle(d_ptr, h, hipIpcMemLazyEnablePeerAccess));
  return RT_OK;
}

int rt_ipc_close(void *d_ptr) {
  if (d_ptr) HIP_TRY(hipIpcCloseMemHandle(d_ptr));
  return RT_OK;
}

#ifndef RT_PIN_COARSE
#define RT_PIN_COARSE 1  // A/B switch: 0 registers caller ranges fine-grained (the HIP default)
#endif
int rt_host_pin(void *ptr, int64_t bytes) {
  if (!ptr || bytes <= 0) return set_err(RT_E_INVALID, "bad host range");
  {
    std::lock_guard<std::mutex> lk(g_pin_mu);
    auto it = g_pins.upper_bound((uintptr_t)ptr + (size_t)bytes - 1);
    if (it != g_pins.begin() && (--it)->first + it->second > (uintptr_t)ptr)
      return set_err(RT_E_INVALID, "rt_host_pin: the range overlaps a range pinned earlier and not unpinned "
                                   "(a buffer freed without rt_host_unpin?)");
  }
  // portable: mapped on every device (rt_multi_render's slots store into it).
  // Coarse-grained (RT_PIN_COARSE): the range is coherent with the host at
  // kernel and copy boundaries only -- which is all the library relies on: the
  // host reads or writes a pinned frame only after the stream that used it is
  // synchronised, and a dispatch's end-of-kernel release covers its stores --
  // so the GPU's stores into it are not snooped by the host's caches: the
  // zero-copy cleared frame's kernel (hits stored into the caller's pinned
  // buffers) ran 0.19-0.24 ms into a fine-grained registration against
  // ~0.18 into the library's own (coarse-grained) hipHostMalloc staging frame
  // (profiles/r06/pin_coarse_ab.txt)
  hipError_t e = hipHostRegister(ptr, (size_t)bytes,
                                 hipHostRegisterMapped | hipHostRegisterPortable | (RT_PIN_COARSE ? hipExtHostRegisterCoarseGrained : 0u));
  if (RT_PIN_COARSE && e == hipErrorInvalidValue) {  // (a runtime without the flag)
    (void)hipGetLastError();
    e = hipHostRegister(ptr, (size_t)bytes, hipHostRegisterMapped | hipHostRegisterPortable);
  }
  if (e == hipErrorHostMemoryAlreadyRegistered) {
    (void)hipGetLastError();
    return set_err(RT_E_INVALID, "rt_host_pin: the HIP runtime already holds a registration over this range "
                                 "(registered outside librtamd, or freed without unregistering)");
  }
  HIP_TRY(e);
  std::lock_guard<std::mutex> lk(g_pin_mu);
  g_pins[(uintptr_t)ptr] = (size_t)bytes;
  return RT_OK;
}

int rt_host_unpin(void *ptr) {
  if (!ptr) return set_err(RT_E_INVALID, "NULL pointer");
  {
    std::lock_guard<std::mutex> lk(g_pin_mu);
    if (!g_pins.erase((uintptr_t)ptr)) return set_err(RT_E_INVALID, "rt_host_unpin: not a range pinned by rt_host_pin");
  }
  // no library stream may still read or write the range when it is unregistered
  // (every entry point drains its streams before returning; a failed call or a
  // stream-ordered launch may not have)
  if (const hipError_t e = rterr::streams_sync())
    return set_err(RT_E_DEVICE, rterr::hip_fail("rt_host_unpin: draining the library's streams", e));
  HIP_TRY(hipHostUnregister(ptr));
  return RT_OK;
}

}  // extern "C"
