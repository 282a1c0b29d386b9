// Shared helpers for the libslu_hip kernels (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <utility>
#include "slu.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));      // D fragment of a 32x32 MFMA

#define SLU_CHECK_LAUNCH()                                   \
  do {                                                       \
    if (hipGetLastError() != hipSuccess) return SLU_ELAUNCH; \
    return SLU_OK;                                           \
  } while (0)

static inline hipStream_t slu_stream(slu_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

// Where a conv dispatch ends.  name == nullptr: the leaf launches on `st`.  Otherwise it writes the name of the instantiation it
// would launch (as rocprofv3 prints it) after its own refusal checks and makes no HIP call: slu_*_fwd and slu_*_kernel_name walk
// the same code.
struct SluEmit {
  hipStream_t st;
  char* name;
  size_t n;
};
__attribute__((format(printf, 2, 3))) static inline int slu_emit_name(const SluEmit& e, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  const int len = e.name ? vsnprintf(e.name, e.n, fmt, ap) : -1;
  va_end(ap);
  return len >= 0 && (size_t)len < e.n ? SLU_OK : SLU_EINVAL;
}
static inline const char* slu_tf(bool b) { return b ? "true" : "false"; }

// An integer switch of the environment, `dflt` when unset.  Call sites keep the value in a `static const`: read once per process.
static inline int slu_env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}

// Ablation switches (a kernel drops its DMAs or MFMAs and computes WRONG results, to see what the rest costs) exist only in the
// development build (-DSLU_H8_AB, tools/h8_ab.py): there the host reads SLU_GEMM_DBG / SLU_TAIL_DBG into the argument structs' `dbg`;
// in the shipped library the tests below are the constant false and the structs have no such field.
#ifdef SLU_H8_AB
#define SLU_ABLATE(args, bit) (((args).dbg & (bit)) != 0)
#else
#define SLU_ABLATE(args, bit) false
#endif

// hipFuncAttributeMaxDynamicSharedMemorySize is a per-DEVICE property of a kernel: one of these per kernel instantiation remembers
// what has been granted on each device of the process (one process may drive several GPUs).  Benign race: the call is idempotent.
struct SluLdsGrant {
  size_t granted[32] = {};
};
static inline int slu_grant_dynamic_lds(const void* kern, size_t lds, SluLdsGrant& g) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 32) return SLU_ELAUNCH;
  if (lds > g.granted[dev]) {
    if (hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return SLU_ELAUNCH;
    g.granted[dev] = lds;
  }
  return SLU_OK;
}

// "grant dynamic LDS, launch, check": the tail of every launcher whose kernel takes more than the default 64 KB of dynamic LDS.  The caller
// owns the grant record (`static SluLdsGrant grant;` in the launcher template: one per kernel instantiation).
template <class K, class... Args>
static inline int slu_launch_lds(K kern, dim3 grid, dim3 block, size_t lds, hipStream_t st, SluLdsGrant& grant, Args... args) {
  if (slu_grant_dynamic_lds(reinterpret_cast<const void*>(kern), lds, grant) != SLU_OK) return SLU_ELAUNCH;
  hipLaunchKernelGGL(kern, grid, block, lds, st, args...);
  SLU_CHECK_LAUNCH();
}

// blocks of a grid-stride kernel with 256 threads over `total` items, at most `cap`
static inline unsigned slu_grid_1d(size_t total, unsigned cap) { return (unsigned)((total + 255) / 256 > cap ? cap : (total + 255) / 256); }

// The conv geometries the kernels are instantiated for: f receives the one that matches (ksize, dil, pad) as a type.
template <int KS_, int DIL_, int PAD_>
struct SluConvGeo {
  static constexpr int KS = KS_, DIL = DIL_, PAD = PAD_;
};
template <class F>
static inline int slu_conv_family(int ksize, int dil, int pad, F&& f) {
  if (ksize == 1 && dil == 1 && pad == 0) return f(SluConvGeo<1, 1, 0>{});
  if (ksize == 3 && dil == 1 && pad == 1) return f(SluConvGeo<3, 1, 1>{});
  if (ksize == 3 && dil == 2 && pad == 2) return f(SluConvGeo<3, 2, 2>{});
  if (ksize == 2 && dil == 2 && pad == 1) return f(SluConvGeo<2, 2, 1>{});
  if (ksize == 2 && dil == 1 && pad == 1) return f(SluConvGeo<2, 1, 1>{});
  return SLU_EUNSUPPORTED;
}

// The class counts the per-pixel metric kernels (one thread holds a pixel's C values in registers) are instantiated for: f receives
// the smaller one that holds C as a std::integral_constant.  The caller has refused C > 32.
template <class F>
static inline void slu_class_cap(int C, F&& f) {
  if (C <= 20) f(std::integral_constant<int, 20>{});
  else f(std::integral_constant<int, 32>{});
}

// compile-time loop: f(std::integral_constant<int, 0>{}), ..., f(std::integral_constant<int, N - 1>{}) -- for bodies too large for `#pragma unroll`
// whose index must stay a constant (register arrays indexed by it would otherwise move to scratch memory)
template <class F, int... Is>
__device__ __forceinline__ void slu_static_for_impl(F&& f, std::integer_sequence<int, Is...>) {
  (f(std::integral_constant<int, Is>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void slu_static_for(F&& f) {
  slu_static_for_impl(f, std::make_integer_sequence<int, N>{});
}

// Row (the M index: an output channel) of register r of the f32x16 D fragment held by lane half hh = lane >> 5, counted from row0; the column
// is lane & 31.  row0 comes first in the sum, as the copies had it: without it (`row0 + slu_frag_row(r, hh)`) the sum re-associates and 9 of
// the 14 wgrad kernels change.
__device__ __forceinline__ constexpr int slu_frag_row(int row0, int r, int hh) { return row0 + (r & 3) + 8 * (r >> 2) + 4 * hh; }

// acc[0 .. n) = 0 for f32x16 accumulators; a 2-D array goes row by row.  Macros: as a function taking the array by reference the zeroing
// re-scheduled 30 of the 55 split-fp16 conv kernels.
#define SLU_ZERO_ACC(acc, n)                 \
  _Pragma("unroll") for (int z_ = 0; z_ < (n); ++z_) \
  _Pragma("unroll") for (int r_ = 0; r_ < 16; ++r_) (acc)[z_][r_] = 0.0f
#define SLU_ZERO_ACC2(acc, m, n) \
  _Pragma("unroll") for (int y_ = 0; y_ < (m); ++y_) SLU_ZERO_ACC((acc)[y_], n)

// 64-lane wavefront sum (all lanes receive the total).
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// 64-lane wavefront maximum (all lanes receive it).
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}