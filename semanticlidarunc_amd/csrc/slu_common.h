// Shared helpers for the libslu_hip kernels (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include "slu.h"

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
