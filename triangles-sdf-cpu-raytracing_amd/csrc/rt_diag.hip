// rt_diag.hip -- the device self-checks behind the rtx_* diagnostics: the
// reciprocal and division of rt_rcp.h against the IEEE division, the 8-lane
// group primitives of the cooperative tail, the primary rays as the render
// kernels compute them, and the read pass that calibrates the cache counters.
// None of them takes a scene. (rtx_fast_eye_ok stays with fill_frame in
// rt_device.hip: it forwards to the check every frame makes there.)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "../../include/rtamd.h"
#include "rt_error.h"
#include "rt_math.h"
#include "rt_scenes.h"

using namespace rtd;

namespace {

// rtx_rcp_check: out[0] += floats checked, out[1] += mismatches, out[2] = bits
// of a mismatching x
// rtx_calib_read: a grid-stride pass, each element loaded once; the xor of
// everything is stored only if it equals a value a zeroed buffer never gives
// (the loads cannot be dropped, and no store lands)
__device__ __forceinline__ uint32_t fold(uint32_t v) { return v; }
__device__ __forceinline__ uint32_t fold(uint4 v) { return v.x ^ v.y ^ v.z ^ v.w; }
template <class T>
__global__ __launch_bounds__(256) void calib_read_kernel(const T *__restrict__ p, int64_t n, uint32_t *out) {
  uint32_t acc = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) acc ^= fold(p[i]);
  if (acc == 0x9E3779B9u) out[0] = acc;
}

// rtx_l1_rate: how fast one CU's vector L1, and its LDS, answer loads that
// always hit -- the two ways a wave can get a BVH node all its lanes share
// (expand_node's per-lane loads against the shared fetch, rt_scenes.h).
// Every wave runs `iters` rounds of kRateLoads 16-byte loads and waits for
// each round, then leaves its shader cycles (s_memtime) and its 100 MHz ticks
// (s_memrealtime). The loads are asm volatile so that none is merged or hoisted.
//   mode 0: global_load_dwordx4, all 64 lanes on the same 16 bytes;
//   mode 1: global_load_dwordx4, every lane on its own 16 bytes, the rounds'
//           loads walking a 4 KiB set (L1-resident after the first round);
//   mode 2: ds_read_b128 at 14 constant offsets of the wave's 224-byte pad,
//           one address for all lanes (broadcast); a round is 14 reads.
typedef unsigned int rate_u4 __attribute__((ext_vector_type(4)));
constexpr int kRateLoads = 8, kRateLds = 14, kRateBlock = 1024;
template <int OFF>
__device__ __forceinline__ rate_u4 rate_lds_read(uint32_t l) {
  rate_u4 v;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=&v"(v) : "v"(l), "n"(OFF));
  return v;
}
template <int OFF>
__device__ __forceinline__ rate_u4 rate_global_read(const char *g) {
  rate_u4 v;
  asm volatile("global_load_dwordx4 %0, %1, off offset:%2" : "=&v"(v) : "v"(g), "n"(OFF));
  return v;
}
template <int... K>
__device__ __forceinline__ void rate_lds_round(uint32_t l, rate_u4 (&v)[kRateLds], std::integer_sequence<int, K...>) {
  ((v[K] = rate_lds_read<16 * K>(l)), ...);
}
template <int... K>
__device__ __forceinline__ void rate_global_round(const char *g, rate_u4 (&v)[kRateLoads],
                                                  std::integer_sequence<int, K...>) {
  ((v[K] = rate_global_read<1024 * (K & 3)>(g)), ...);  // mode 1: 4 x 1 KiB, twice
}
__global__ __launch_bounds__(kRateBlock) void l1_rate_kernel(int mode, int iters, const char *buf,
                                                             unsigned long long *out) {
  __shared__ __attribute__((aligned(16))) uint32_t pad[(kRateBlock / 64) * 56];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = lane; i < 56; i += 64) pad[wave * 56 + i] = (uint32_t)i;
  __syncthreads();
  const char *g = buf + (mode == 1 ? lane * 16 : 0);  // within buf's first 4 KiB
  const uint32_t l = (uint32_t)(uintptr_t)(pad + wave * 56);  // LDS byte address of the wave's pad
  rate_u4 acc = {0u, 0u, 0u, 0u};
  const unsigned long long c0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
  for (int it = 0; it < iters; ++it) {
    if (mode == 2) {
      rate_u4 v[kRateLds];
      rate_lds_round(l, v, std::make_integer_sequence<int, kRateLds>{});
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int k = 0; k < kRateLds; ++k) {
        asm volatile("" : "+v"(v[k]));
        acc ^= v[k];
      }
    } else {
      rate_u4 v[kRateLoads];
      rate_global_round(g, v, std::make_integer_sequence<int, kRateLoads>{});
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
      for (int k = 0; k < kRateLoads; ++k) {
        asm volatile("" : "+v"(v[k]));
        acc ^= v[k];
      }
    }
  }
  const unsigned long long c1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
  const uint32_t f = acc.x ^ acc.y ^ acc.z ^ acc.w;
  const size_t w = (size_t)blockIdx.x * (kRateBlock / 64) + wave;
  if (lane == 0) {
    out[2 * w] = c1 - c0;
    out[2 * w + 1] = (r1 - r0) | (f == 0x9E3779B9u ? 1ull << 63 : 0ull);  // (keeps acc alive; the buffer is zero)
  }
}

__global__ void rcp_check_kernel(uint32_t base, unsigned long long *out) {
  const uint32_t bits = base + blockIdx.x * blockDim.x + threadIdx.x;
  const float x = __uint_as_float(bits);
  const float ax = __builtin_fabsf(x);
  const bool in = ax >= 1e-8f && ax < 0x1p126f;
  const bool bad = in && __float_as_uint(1.0f / x) != __float_as_uint(rtm::rcp_rn(x));
  const unsigned long long nin = __popcll(__ballot(in)), nbad = __popcll(__ballot(bad));
  if ((threadIdx.x & 63) == 0) {
    if (nin) atomicAdd(out, nin);
    if (nbad) atomicAdd(out + 1, nbad);
  }
  if (bad) out[2] = bits;
}

// rtx_div_check: rtm::div_mk against the division. mode 0: 2 (x + 1/2) / W for
// every W in [1, 32768] and x < W (blockIdx.y = W - 1); mode 1: random pairs in
// the eye ray's ranges (|a| in [2^-72, 2^24] or +-0, |b| in [2^-20, 2^24],
// random signs and mantissas). out[0] += checked, out[1] += mismatches,
// out[2] = a mismatching pair (a's bits | b's bits << 32)
__device__ __forceinline__ uint64_t mix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__global__ void div_check_kernel(int mode, uint64_t base, uint64_t seed, unsigned long long *out) {
  uint64_t n_in = 0, n_bad = 0, bad_ab = 0;
  if (mode == 0) {
    const int W = (int)blockIdx.y + 1;
    for (int x = (int)threadIdx.x; x < W; x += (int)blockDim.x) {
      const float a = 2.0f * ((float)x + 0.5f), b = (float)W;
      ++n_in;
      if (__float_as_uint(rtm::div_mk(a, b)) != __float_as_uint(a / b)) {
        ++n_bad;
        bad_ab = __float_as_uint(a) | ((uint64_t)__float_as_uint(b) << 32);
      }
    }
  } else {
    const uint64_t i = base + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t h = mix64(i ^ (seed << 40)), g = mix64(h);
    const uint32_t ea = 127 - 72 + (uint32_t)(g % 97), eb = 127 - 20 + (uint32_t)((g >> 16) % 45);
    uint32_t ua = ((uint32_t)h & 0x807FFFFFu) | (ea << 23);
    const uint32_t ub = ((uint32_t)(h >> 32) & 0x807FFFFFu) | (eb << 23);
    if (((g >> 32) & 63) == 0) ua &= 0x80000000u;  // +-0 numerators
    const float a = __uint_as_float(ua), b = __uint_as_float(ub);
    n_in = 1;
    if (__float_as_uint(rtm::div_mk(a, b)) != __float_as_uint(a / b)) {
      n_bad = 1;
      bad_ab = ua | ((uint64_t)ub << 32);
    }
  }
  if (n_in) atomicAdd(out, (unsigned long long)n_in);
  if (n_bad) {
    atomicAdd(out + 1, (unsigned long long)n_bad);
    out[2] = bad_ab;
  }
}

// Diagnostic: the world-space primary ray of every pixel, as render_kernel
// computes it (image row yo, loop row y = H - yo - 1).
__global__ void eye_rays_kernel(rt_render_params P, int W, int H, float *out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= W * H) return;
  const int yo = i / W, x = i - yo * W;
  const f3 d = eye_ray(x, H - yo - 1, W, H, P.proj_inv, P.view_inv);
  out[3 * i] = d.x;
  out[3 * i + 1] = d.y;
  out[3 * i + 2] = d.z;
}

// Diagnostic: the 8-lane group primitives of the cooperative tail on test
// vectors (one 8-lane group per vector of 8 keys): sort8 across lanes, the
// first-wins min, the OR reduction. Checked against the scalar forms in tests.
__global__ void grp_test_kernel(const float *keys, int n, float *st, uint32_t *sid, float *mt,
                                uint32_t *mk, uint32_t *orv) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;  // blockDim = 64: 8 groups per wave
  const int g = i >> 3, k = i & 7;
  const bool ok = g < n;
  float t = ok ? keys[8 * g + k] : 0.0f;
  uint32_t id = (uint32_t)k;
  grp_sort8(t, id, k);
  float m = ok ? keys[8 * g + k] : 0.0f;
  uint32_t kk = (uint32_t)k;
  grp_min_first(m, kk, k);
  const uint32_t o = grp_or(1u << (3 * k), k);
  if (ok) {
    st[8 * g + k] = t;
    sid[8 * g + k] = id;
    if (k == 0) { mt[g] = m; mk[g] = kk; orv[g] = o; }
  }
}

}  // namespace

extern "C" {

// Diagnostic: primary ray directions as the render kernel computes them (host buffer [H][W][3]).
int rtx_eye_rays(const rt_render_params *p, int32_t W, int32_t H, float *out) {
  int rc = check_params(p, W, H);
  if (rc) return rc;
  float *d = nullptr;
  HIP_TRY(hipMalloc(&d, (size_t)W * H * 12));
  eye_rays_kernel<<<(W * H + 255) / 256, 256>>>(*p, W, H, d);
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, d, (size_t)W * H * 12, hipMemcpyDeviceToHost);
  HIP_NOTE(hipFree(d));
  if (e != hipSuccess) return set_err(RT_E_DEVICE, hipGetErrorString(e));
  return RT_OK;
}

// Diagnostic: run the 8-lane group primitives on n vectors of 8 keys (host buffers).
int rtx_grp_test(const float *keys, int32_t n, float *st, uint32_t *sid, float *mt, uint32_t *mk,
                 uint32_t *orv) {
  if (n <= 0) return set_err(RT_E_INVALID, "n must be positive");
  float *dk = nullptr, *dst = nullptr, *dmt = nullptr;
  uint32_t *dsid = nullptr, *dmk = nullptr, *dor = nullptr;
  const size_t n8 = (size_t)n * 8;
  HIP_TRY(hipMalloc(&dk, n8 * 4));
  HIP_TRY(hipMalloc(&dst, n8 * 4));
  HIP_TRY(hipMalloc(&dsid, n8 * 4));
  HIP_TRY(hipMalloc(&dmt, (size_t)n * 4));
  HIP_TRY(hipMalloc(&dmk, (size_t)n * 4));
  HIP_TRY(hipMalloc(&dor, (size_t)n * 4));
  HIP_TRY(hipMemcpy(dk, keys, n8 * 4, hipMemcpyHostToDevice));
  grp_test_kernel<<<(unsigned)((n8 + 63) / 64), 64>>>(dk, n, dst, dsid, dmt, dmk, dor);
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(st, dst, n8 * 4, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(sid, dsid, n8 * 4, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(mt, dmt, (size_t)n * 4, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(mk, dmk, (size_t)n * 4, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(orv, dor, (size_t)n * 4, hipMemcpyDeviceToHost);
  for (void *q : {(void *)dk, (void *)dst, (void *)dsid, (void *)dmt, (void *)dmk, (void *)dor}) HIP_NOTE(hipFree(q));
  if (e != hipSuccess) return set_err(RT_E_DEVICE, hipGetErrorString(e));
  return RT_OK;
}

// key_order (rt_math.h, the keyed expansion's visit order) for tests, host
// only: n vectors of 8 entry distances as slab_key hands them over (t < 0: a
// miss, which takes its slot's miss constant) -> per vector the packed list,
// the count, the bits of the first child's t and the tie flag. Not part of
// include/rtamd.h.
int rtx_expand_order(const float *t, int64_t n, uint32_t *list, uint32_t *cnt, uint32_t *tfirst, uint8_t *tie) {
  if (!t || n < 0 || !list || !cnt || !tfirst || !tie) return set_err(RT_E_INVALID, "bad arguments");
  for (int64_t i = 0; i < n; ++i) {
    uint32_t tb[8];
    for (uint32_t c = 0; c < 8; ++c) {
      const float v = t[8 * i + c];
      uint32_t b;
      __builtin_memcpy(&b, &v, 4);
      tb[c] = v < 0.0f ? rtd::order_miss_bits(c) : b;
    }
    const rtd::KeyOrder r = rtd::key_order(tb);
    list[i] = r.list;
    cnt[i] = r.cnt;
    tfirst[i] = r.tfirst;
    tie[i] = r.tie ? 1 : 0;
  }
  return RT_OK;
}

// Exhaustive check of rtm::rcp_rn (rt_rcp.h, tri_t's reciprocal) on this
// device: every float x with 1e-8 <= |x| < 2^126 against the IEEE division
// 1 / x. *checked = floats in that range, *bad = mismatches, *first_bad = the
// bits of one mismatching x (0 if none). Not part of include/rtamd.h.
int rtx_rcp_check(uint64_t *checked, uint64_t *bad, uint32_t *first_bad) {
  if (!checked || !bad || !first_bad) return set_err(RT_E_INVALID, "NULL argument");
  unsigned long long *d = nullptr;
  HIP_TRY(hipMalloc(&d, 3 * sizeof(unsigned long long)));
  hipError_t e = hipMemset(d, 0, 3 * sizeof(unsigned long long));
  const uint32_t block = 256, chunk = 1u << 28;  // 2^28 bit patterns per launch
  for (uint64_t base = 0; e == hipSuccess && base < (1ull << 32); base += chunk) {
    rcp_check_kernel<<<chunk / block, block>>>((uint32_t)base, d);
    e = hipGetLastError();
  }
  unsigned long long h[3] = {0, 0, 0};
  if (e == hipSuccess) e = hipMemcpy(h, d, sizeof h, hipMemcpyDeviceToHost);
  HIP_NOTE(hipFree(d));
  if (e != hipSuccess) return set_err(RT_E_DEVICE, std::string("rcp check: ") + hipGetErrorString(e));
  *checked = h[0];
  *bad = h[1];
  *first_bad = (uint32_t)h[2];
  return RT_OK;
}

// Diagnostic (bench.py's PMC calibration, tools/prof_frames.py): one pass of
// calib_read_kernel over `bytes` of device memory, every byte loaded once
// (`width` = 4 or 16 bytes per lane, consecutive lanes on consecutive
// addresses), so the vector L1 misses every line exactly once and the
// dispatch's TCP_TCC_READ_REQ / TCP_TOTAL_CACHE_ACCESSES counts give the bytes
// per L1->L2 read request and per L1 access on gfx950. Not part of rtamd.h.
int rtx_calib_read(int64_t bytes, int32_t width, uint32_t *sink) {
  if (bytes <= 0 || (width != 4 && width != 16) || bytes % 1024) return set_err(RT_E_INVALID, "bad arguments");
  void *d = nullptr;
  uint32_t *o = nullptr;
  HIP_TRY(hipMalloc(&d, (size_t)bytes));
  hipError_t e = hipMalloc(&o, 4);
  if (e == hipSuccess) e = hipMemset(d, 0, (size_t)bytes);
  if (e == hipSuccess) e = hipMemset(o, 0, 4);
  if (e == hipSuccess) {
    const int64_t n = bytes / width;
    const unsigned blocks = (unsigned)std::min<int64_t>((n + 255) / 256, 4096);
    if (width == 16)
      calib_read_kernel<uint4><<<blocks, 256>>>((const uint4 *)d, n, o);
    else
      calib_read_kernel<uint32_t><<<blocks, 256>>>((const uint32_t *)d, n, o);
    e = hipGetLastError();
  }
  uint32_t h = 0;
  if (e == hipSuccess) e = hipMemcpy(&h, o, 4, hipMemcpyDeviceToHost);
  HIP_NOTE(hipFree(d));
  if (o) HIP_NOTE(hipFree(o));
  if (e != hipSuccess) return set_err(RT_E_DEVICE, std::string("calib read: ") + hipGetErrorString(e));
  if (sink) *sink = h;
  return RT_OK;
}

// Diagnostic (tools/l1_rate.py): l1_rate_kernel's `mode` with `blocks`
// workgroups of 16 waves, `iters` rounds per wave. out[0] = waves, out[1] =
// load instructions per wave, out[2] / out[3] = sum / max over waves of shader
// cycles, out[4] = sum over waves of 100 MHz ticks. Not part of rtamd.h.
int rtx_l1_rate(int32_t mode, int32_t iters, int32_t blocks, uint64_t out[5]) {
  if (!out || mode < 0 || mode > 2 || iters <= 0 || iters > (1 << 20) || blocks <= 0 || blocks > 4096)
    return set_err(RT_E_INVALID, "bad arguments");
  const size_t waves = (size_t)blocks * (kRateBlock / 64);
  char *buf = nullptr;
  unsigned long long *d = nullptr;
  HIP_TRY(hipMalloc(&buf, 8192));
  hipError_t e = hipMalloc(&d, waves * 2 * sizeof(unsigned long long));
  if (e == hipSuccess) e = hipMemset(buf, 0, 8192);
  if (e == hipSuccess) {
    l1_rate_kernel<<<(unsigned)blocks, kRateBlock>>>(mode, iters, buf, d);
    e = hipGetLastError();
  }
  std::vector<unsigned long long> h(waves * 2);
  if (e == hipSuccess) e = hipMemcpy(h.data(), d, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost);
  HIP_NOTE(hipFree(buf));
  if (d) HIP_NOTE(hipFree(d));
  if (e != hipSuccess) return set_err(RT_E_DEVICE, std::string("l1 rate: ") + hipGetErrorString(e));
  out[0] = waves;
  out[1] = (uint64_t)iters * (mode == 2 ? kRateLds : kRateLoads);
  out[2] = out[3] = out[4] = 0;
  for (size_t w = 0; w < waves; ++w) {
    out[2] += h[2 * w];
    out[3] = std::max<uint64_t>(out[3], h[2 * w]);
    out[4] += h[2 * w + 1] & ~(1ull << 63);
  }
  return RT_OK;
}

// The checks behind rtm::div_mk on this device (div_check_kernel's modes; n:
// pairs for mode 1). out[0] = checked, out[1] = mismatches, out[2] = one
// mismatching pair's bits. Not part of include/rtamd.h.
int rtx_div_check(int32_t mode, uint64_t n, uint64_t seed, uint64_t out[3]) {
  if (!out || mode < 0 || mode > 1) return set_err(RT_E_INVALID, "bad arguments");
  unsigned long long *d = nullptr;
  HIP_TRY(hipMalloc(&d, 3 * sizeof(unsigned long long)));
  hipError_t e = hipMemset(d, 0, 3 * sizeof(unsigned long long));
  const uint32_t block = 256;
  if (e == hipSuccess && mode == 0) {
    div_check_kernel<<<dim3(1, 32768), block>>>(0, 0, seed, d);
    e = hipGetLastError();
  } else if (e == hipSuccess) {
    const uint64_t chunk = 1ull << 28;
    for (uint64_t b0 = 0; e == hipSuccess && b0 < n; b0 += chunk) {
      const uint64_t m = std::min(chunk, n - b0);
      div_check_kernel<<<(unsigned)((m + block - 1) / block), block>>>(mode, b0, seed, d);
      e = hipGetLastError();
    }
  }
  unsigned long long h[3] = {0, 0, 0};
  if (e == hipSuccess) e = hipMemcpy(h, d, sizeof h, hipMemcpyDeviceToHost);
  HIP_NOTE(hipFree(d));
  if (e != hipSuccess) return set_err(RT_E_DEVICE, std::string("div check: ") + hipGetErrorString(e));
  for (int i = 0; i < 3; ++i) out[i] = h[i];
  return RT_OK;
}

}  // extern "C"
