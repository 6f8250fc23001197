// rt_mem.h -- the owners of what a handle (rt_scene, rt_sdf_mesh) or a call
// holds on the device and in pinned host memory: a typed device array, a
// pinned host block, an event and a library stream. Host only. Every type is
// move-only and frees in its destructor; a failed free is logged (HIP_NOTE),
// never returned. The device current at destruction must be the one the
// object was made on: the handles' destroy entries see to that.
//
// live(k) counts the objects of each type that hold something (rtmem::Kind;
// rtx_live_resources). It moves only where one is created or freed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <string>
#include <utility>

#include "rt_error.h"
#include "rt_host.h"

namespace rtmem {

enum Kind { kArrays = 0, kPinned = 1, kEvents = 2, kStreams = 3 };
inline std::atomic<int64_t> g_live[4];
inline void live(Kind k, int64_t d) { g_live[k].fetch_add(d, std::memory_order_relaxed); }

// n elements of T on the device. p is there for kernel arguments and copies.
template <class T>
struct DevArray {
  T *p = nullptr;
  size_t n = 0;

  DevArray() = default;
  DevArray(const DevArray &) = delete;
  DevArray &operator=(const DevArray &) = delete;
  DevArray(DevArray &&o) noexcept : p(std::exchange(o.p, nullptr)), n(std::exchange(o.n, 0)) {}
  DevArray &operator=(DevArray &&o) noexcept {
    if (this != &o) {
      reset();
      p = std::exchange(o.p, nullptr);
      n = std::exchange(o.n, 0);
    }
    return *this;
  }
  ~DevArray() { reset(); }

  size_t bytes() const { return n * sizeof(T); }
  void reset() {
    if (p) {
      HIP_NOTE(hipFree(p));
      live(kArrays, -1);
    }
    p = nullptr;
    n = 0;
  }
  // what it held is freed, then `count` elements allocated (uninitialised)
  hipError_t alloc_e(size_t count) {
    reset();
    const hipError_t e = hipMalloc(&p, count * sizeof(T));
    if (e != hipSuccess) {
      p = nullptr;
      return e;
    }
    n = count;
    if (p) live(kArrays, 1);
    return hipSuccess;
  }
  int alloc(size_t count) {
    HIP_TRY(alloc_e(count));
    return RT_OK;
  }
  // `count` elements from the host (src == NULL: left uninitialised); an empty
  // array still gets one element, so that p is a valid pointer.
  int upload(const T *src, size_t count) {
    if (int rc = alloc(count ? count : 1)) return rc;
    if (src && count) HIP_TRY(rtdma::h2d(p, src, count * sizeof(T), nullptr));
    return RT_OK;
  }
  // the same; `total` grows by what was allocated
  int upload(const T *src, size_t count, int64_t &total) {
    if (int rc = upload(src, count)) return rc;
    total += (int64_t)bytes();
    return RT_OK;
  }
  // upload + `pad` zeroed trailing elements (kernels may read past the end)
  int upload_padded(const T *src, size_t count, size_t pad, int64_t &total) {
    if (int rc = alloc(count + pad)) return rc;
    HIP_TRY(hipMemset(p, 0, bytes()));
    if (count) HIP_TRY(rtdma::h2d(p, src, count * sizeof(T), nullptr));
    total += (int64_t)bytes();
    return RT_OK;
  }
  // takes over a hipMalloc'ed buffer the builder left on the device
  void adopt(rth::DevBuffer &b) {
    reset();
    n = b.bytes / sizeof(T);
    p = static_cast<T *>(b.take());
    if (p) live(kArrays, 1);
  }
};

// n elements of T in pinned host memory (hipHostMalloc with `flags`); with
// hipHostMallocMapped, dev is the block's device address.
template <class T>
struct Pinned {
  T *h = nullptr;
  T *dev = nullptr;
  size_t n = 0;
  unsigned flags = 0;

  Pinned() = default;
  Pinned(const Pinned &) = delete;
  Pinned &operator=(const Pinned &) = delete;
  Pinned(Pinned &&o) noexcept
      : h(std::exchange(o.h, nullptr)), dev(std::exchange(o.dev, nullptr)), n(std::exchange(o.n, 0)), flags(o.flags) {}
  Pinned &operator=(Pinned &&o) noexcept {
    if (this != &o) {
      reset();
      h = std::exchange(o.h, nullptr);
      dev = std::exchange(o.dev, nullptr);
      n = std::exchange(o.n, 0);
      flags = o.flags;
    }
    return *this;
  }
  ~Pinned() { reset(); }

  void reset() {
    if (h) {
      HIP_NOTE(hipHostFree(h));
      live(kPinned, -1);
    }
    h = dev = nullptr;
    n = 0;
  }
  int alloc(size_t count, unsigned host_flags) {
    reset();
    flags = host_flags;
    HIP_TRY(hipHostMalloc((void **)&h, count * sizeof(T), flags));
    n = count;
    live(kPinned, 1);
    if (flags & hipHostMallocMapped) {
      const hipError_t e = hipHostGetDevicePointer((void **)&dev, h, 0);
      if (e != hipSuccess) {
        reset();  // (the next call tries again)
        HIP_TRY(e);
      }
    }
    return RT_OK;
  }
};

struct Event {
  hipEvent_t e = nullptr;

  Event() = default;
  Event(const Event &) = delete;
  Event &operator=(const Event &) = delete;
  Event(Event &&o) noexcept : e(std::exchange(o.e, nullptr)) {}
  Event &operator=(Event &&o) noexcept {
    if (this != &o) {
      reset();
      e = std::exchange(o.e, nullptr);
    }
    return *this;
  }
  ~Event() { reset(); }

  void reset() {
    if (e) {
      HIP_NOTE(hipEventDestroy(e));
      live(kEvents, -1);
    }
    e = nullptr;
  }
  // made once: a second call leaves the event as it is
  int create(unsigned flags) {
    if (e) return RT_OK;
    HIP_TRY(hipEventCreateWithFlags(&e, flags));
    live(kEvents, 1);
    return RT_OK;
  }
  int create_timing() {
    if (e) return RT_OK;
    HIP_TRY(hipEventCreate(&e));
    live(kEvents, 1);
    return RT_OK;
  }
};

// A non-blocking stream of the library's own, registered with the stream
// registry (rterr::stream_add) under its label for as long as it lives.
struct Stream {
  hipStream_t s = nullptr;

  Stream() = default;
  Stream(const Stream &) = delete;
  Stream &operator=(const Stream &) = delete;
  Stream(Stream &&o) noexcept : s(std::exchange(o.s, nullptr)) {}
  Stream &operator=(Stream &&o) noexcept {
    if (this != &o) {
      reset();
      s = std::exchange(o.s, nullptr);
    }
    return *this;
  }
  ~Stream() { reset(); }

  void reset() {
    if (s) {
      rterr::stream_remove(s);
      HIP_NOTE(hipStreamDestroy(s));
      live(kStreams, -1);
    }
    s = nullptr;
  }
  // made once: a second call leaves the stream as it is
  int create(int device, const std::string &label) {
    if (s) return RT_OK;
    HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    live(kStreams, 1);
    rterr::stream_add(s, device, label);
    return RT_OK;
  }
};

}  // namespace rtmem
