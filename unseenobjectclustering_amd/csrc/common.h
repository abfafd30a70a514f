// Shared helpers for libuoc_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <atomic>

#include "../../include/uoc_hip.h"

namespace uoc {

void set_error(const char *fmt, ...);

#define UOC_HIP_CHECK(expr)                                                              \
  do {                                                                                   \
    hipError_t _e = (expr);                                                              \
    if (_e != hipSuccess) {                                                              \
      ::uoc::set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e)); \
      return UOC_EHIP;                                                                   \
    }                                                                                    \
  } while (0)

#define UOC_REQUIRE(cond, ...)        \
  do {                                \
    if (!(cond)) {                    \
      ::uoc::set_error(__VA_ARGS__);  \
      return UOC_EINVAL;              \
    }                                 \
  } while (0)

#define UOC_LAUNCH_CHECK() UOC_HIP_CHECK(hipGetLastError())

// Development knobs from the environment, read ONCE (not per launch): the value is cached until uoc_reload_env() bumps
// the epoch (tests / micro-benchmarks that switch a knob inside one process call that).
extern std::atomic<int> g_env_epoch;
struct EnvInt {
  const char *name;
  int def;
  std::atomic<int> seen{-1};
  std::atomic<int> val{0};
  EnvInt(const char *n, int d) : name(n), def(d) {}
  int get();
};

// The library has ONE implementation per step and no knob that selects a kernel or changes a rounding (the measured-and-
// rejected alternates of rounds 1-5 live in the git history, HISTORY.md names the commits).  What it still reads from
// the environment is speed-only and listed in INTEGRATION.md.

static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// Carves a caller-owned workspace into arrays that start on 256-byte boundaries, in the order they are taken.  With a null
// base it only measures: every take() is null and total() is the size the same sequence of takes needs.
struct Carver {
  char *base;
  size_t off = 0;
  explicit Carver(void *b) : base((char *)b) {}
  template <typename T>
  T *take(size_t count) {
    T *p = base ? (T *)(base + off) : nullptr;
    off += align_up(count * sizeof(T), 256);
    return p;
  }
  size_t total() const { return off; }
};

// True while `st` is being captured into a hipGraph (fcn/graph_replay.py): nothing that synchronises, times or launches
// cooperatively may run then.
static inline bool stream_is_capturing(hipStream_t st) {
  hipStreamCaptureStatus s = hipStreamCaptureStatusNone;
  return hipStreamIsCapturing(st, &s) == hipSuccess && s != hipStreamCaptureStatusNone;
}

typedef float f32x4 __attribute__((ext_vector_type(4)));

// Per-device one-time state.  hipFuncSetAttribute (dynamic LDS above 64 KB) applies to the CURRENT device's copy of a
// kernel, and a process may drive several GPUs (the reference wraps its nets in DataParallel), so "done once" flags
// are kept per device ordinal, not per process.
constexpr int kMaxDevices = 64;
static inline int current_device() {
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= kMaxDevices) d = 0;
  return d;
}
struct DeviceOnce {
  std::atomic<unsigned long long> bits{0};
  bool done() const { return (bits.load(std::memory_order_acquire) >> current_device()) & 1ull; }
  void mark() { bits.fetch_or(1ull << current_device(), std::memory_order_release); }
};
// Dynamic LDS above 48 KB has to be allowed per kernel and per device before the launch.  `bytes` is the most the kernel is
// ever launched with, the same at every call that shares `once`; at or below 48 KB there is nothing to allow.  A refusal
// goes through the error channel: the launch that would follow could only fail.
static inline int opt_in_dynamic_lds(const void *kernel, size_t bytes, DeviceOnce &once) {
  if (bytes <= 48 * 1024 || once.done()) return UOC_OK;
  UOC_HIP_CHECK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  once.mark();
  return UOC_OK;
}
// Compute-unit count of the current device (cached per device).
static inline int device_num_cu() {
  static std::atomic<int> cached[kMaxDevices];
  const int d = current_device();
  int v = cached[d].load(std::memory_order_relaxed);
  if (v == 0) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, d) != hipSuccess) return 0;
    v = prop.multiProcessorCount;
    cached[d].store(v, std::memory_order_relaxed);
  }
  return v;
}

// ---- wave64 cross-lane helpers (DPP; one VALU op each, no LDS) -------------------------
// Row = 16 lanes.  quad_perm [1,0,3,2] = 0xB1, [2,3,0,1] = 0x4E, row_half_mirror = 0x141,
// row_mirror = 0x140.
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
template <int CTRL>
__device__ __forceinline__ int dpp_i(int v) {
  return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true);
}
// Sum over each 16-lane row; every lane of the row ends with the bitwise-identical total.
__device__ __forceinline__ float row16_sum(float v) {
  v += dpp_f<0xB1>(v);
  v += dpp_f<0x4E>(v);
  v += dpp_f<0x141>(v);
  v += dpp_f<0x140>(v);
  return v;
}
// Integer reductions over the 64 lanes by shuffles; every lane must take part and ends with the result.
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int sft = 32; sft > 0; sft >>= 1) v += __shfl_xor(v, sft);
  return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int sft = 32; sft > 0; sft >>= 1) v = max(v, __shfl_xor(v, sft));
  return v;
}
__device__ __forceinline__ unsigned long long wave_max64(unsigned long long v) {
#pragma unroll
  for (int sft = 32; sft > 0; sft >>= 1) v = max(v, (unsigned long long)__shfl_xor((long long)v, sft));
  return v;
}
// The unsigned maximum: a DPP tree per 16-lane row, then the four rows.  All 64 lanes active.
__device__ __forceinline__ unsigned wave_max_u(unsigned v) {
  v = max(v, (unsigned)dpp_i<0xB1>((int)v));
  v = max(v, (unsigned)dpp_i<0x4E>((int)v));
  v = max(v, (unsigned)dpp_i<0x141>((int)v));
  v = max(v, (unsigned)dpp_i<0x140>((int)v));
  const unsigned a = __builtin_amdgcn_readlane((int)v, 0), b = __builtin_amdgcn_readlane((int)v, 16);
  const unsigned c = __builtin_amdgcn_readlane((int)v, 32), d = __builtin_amdgcn_readlane((int)v, 48);
  return max(max(a, b), max(c, d));
}
__device__ __forceinline__ int lane_rank(unsigned long long mask) {  // set bits of mask below this lane
  return __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

// The wave-group loop.  Every distinct key >= 0 among the wave's lanes gets one turn, in the order of the lowest lane
// that holds it: body(c, mask, first) with the key, the ballot of the lanes holding it and the lowest of them.  Every
// lane of the wave must call this, and every lane runs the body, so the body may ballot and reduce over the wave; what
// only one lane should do, it does under `lane == first`.
template <typename Body>
__device__ __forceinline__ void for_each_wave_key(int key, Body body) {
  unsigned long long rem = __ballot(key >= 0);
  while (rem) {
    const int first = __ffsll((long long)rem) - 1;
    const int c = __builtin_amdgcn_readlane(key, first);
    const unsigned long long m = __ballot(key == c);
    rem &= ~m;
    body(c, m, first);
  }
}
// Its commonest user: table[c] += weight * (lanes holding c), one atomic per distinct key c.
__device__ __forceinline__ void wave_add_keys(int *__restrict__ table, int key, int weight, int lane) {
  for_each_wave_key(key, [&](int c, unsigned long long m, int first) {
    if (lane == first) atomicAdd(&table[c], weight * (int)__popcll(m));
  });
}

}  // namespace uoc
