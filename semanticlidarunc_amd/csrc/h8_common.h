// Vocabulary shared by the half-precision ("h8") kernels and their launchers: the conv families of conv_h8.h, conv_tail_h8.hip, ctx_block_h8.hip, head_mc_h8.hip,
// layout_h8.hip, fpn_h8.hip, fpn_opt_h8.hip.
// Every helper is forced inline, and its form (what comes by value, by reference, as a macro) is the one with which the kernels compile
// to the instruction streams of the hand-written copies they replace: check a change here with tools/h8_isa_diff.py (profiles/r07).
#pragma once
#include "slu_common.h"
#include <utility>

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half2v __attribute__((ext_vector_type(2)));
typedef float float2v __attribute__((ext_vector_type(2)));
typedef float f32x4v __attribute__((ext_vector_type(4)));
typedef unsigned u32x4v __attribute__((ext_vector_type(4)));

// one global_load_lds_dwordx4: lane l copies the 16 bytes at its own `gsrc` to LDS address `ldst_wave_base + 16 l`
#define SLU_GLDS16(gsrc, ldst_wave_base)                                                                  \
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(gsrc),                 \
                                   (__attribute__((address_space(3))) void*)(ldst_wave_base), 16, 0, 0)

// The address of a global, once, in an SGPR pair the compiler cannot rematerialise: left alone it re-loaded the address of the zero record
// from the GOT for every piece (s_getpc + s_load_dwordx2 + s_waitcnt lgkmcnt(0): a scalar-memory round trip in every tap's staging slot).
#define H8_OPAQUE_ADDR(name, object)                          \
  uintptr_t name = reinterpret_cast<uintptr_t>(&(object));    \
  asm volatile("" : "+s"(name))

// Epilogue constants into LDS as bias | bn_a | bn_b, `stride` floats apart from s_epi[off]: the calling thread (the caller admits one per
// channel of the table) writes slot tid from channel co.  Defaults 0 / 1 / 0 for a missing array and where `ok` is false (channels past
// the layer's last).  A macro, with `off` an index: as an inlined function, and with the offset folded into the pointer, the fill
// compiled to another order of branches, loads and stores in every kernel.
#define H8_FILL_EPI(s_epi, off, stride, tid, ok, co, bias, bn_a, bn_b)              \
  {                                                                                \
    s_epi[off + tid] = (ok && bias) ? bias[co] : 0.0f;                             \
    s_epi[off + stride + tid] = (ok && bn_a) ? bn_a[co] : 1.0f;                    \
    s_epi[off + 2 * stride + tid] = (ok && bn_a) ? bn_b[co] : 0.0f;                \
  }

namespace {

// One pair per translation unit.  Zero: the source of every out-of-image / padding record of an LDS-DMA copy and what lanes outside the
// image load (never written).  Trash: where the lanes of a border tile that lie outside the image store, so that every lane of every
// tile issues its stores (no branch, and a compile-time number of vector-memory operations per tile for the counted waits).
__device__ uint4 h8_zero_rec [[maybe_unused]];
__device__ uint4 h8_trash_rec [[maybe_unused]];

__device__ __forceinline__ unsigned pack2(float x, float y) {
  half2v h;
  h[0] = (_Float16)x;      // round to nearest even
  h[1] = (_Float16)y;
  return __builtin_bit_cast(unsigned, h);
}
__device__ __forceinline__ unsigned pack2(float2v t) { return __builtin_bit_cast(unsigned, __builtin_convertvector(t, half2v)); }
__device__ __forceinline__ float2v unpack2(unsigned u) { return __builtin_convertvector(__builtin_bit_cast(half2v, u), float2v); }
__device__ __forceinline__ float2v round_f16(float2v t) { return __builtin_convertvector(__builtin_convertvector(t, half2v), float2v); }
// 8 fp32 values -> one 16-byte record, each rounded to fp16 once
__device__ __forceinline__ uint4 h8_pack8(const float (&r)[8]) {
  return make_uint4(pack2(r[0], r[1]), pack2(r[2], r[3]), pack2(r[4], r[5]), pack2(r[6], r[7]));
}

// 4 channels (8 q + 4 hh + 0..3 of a 32-block) of one pixel: the share of accumulator group q that a lane holds
struct H8Quad {
  float2v t0, t1;
};
__device__ __forceinline__ uint2 pack4(H8Quad t) { return make_uint2(pack2(t.t0), pack2(t.t1)); }

// Packed fp32 epilogue arithmetic (v_pk_add / v_pk_mul / v_pk_fma: two channels per instruction) on group q of a 32x32 accumulator tile;
// the per-channel constants come as 16-byte LDS reads (V4: float4, or the native f32x4v where the read must carry a TBAA tag).
// LeakyReLU as max(t, slope t), exact for 0 <= slope <= 1 (sl = 1 means "no activation").
template <class V4>
__device__ __forceinline__ H8Quad h8_bias_leaky(const f32x16& acc, int q, V4 bi, float2v sl) {
  H8Quad t = {{acc[4 * q], acc[4 * q + 1]}, {acc[4 * q + 2], acc[4 * q + 3]}};
  t.t0 += float2v{bi.x, bi.y};
  t.t1 += float2v{bi.z, bi.w};
  t.t0 = __builtin_elementwise_max(t.t0, t.t0 * sl);
  t.t1 = __builtin_elementwise_max(t.t1, t.t1 * sl);
  return t;
}
// ... followed by the folded BatchNorm: bn_a * leaky(acc + bias) + bn_b
template <class V4>
__device__ __forceinline__ H8Quad h8_epilogue(const f32x16& acc, int q, V4 bi, V4 ba, V4 bb, float2v sl) {
  H8Quad t = h8_bias_leaky(acc, q, bi, sl);
  t.t0 = t.t0 * float2v{ba.x, ba.y} + float2v{bb.x, bb.y};
  t.t1 = t.t1 * float2v{ba.z, ba.w} + float2v{bb.z, bb.w};
  return t;
}
// += the lane's 4 channels of an fp16 residual (the two words of an 8-byte half record); in place: returning the sum by value
// re-allocated the registers of store_tile_swap16's callers
__device__ __forceinline__ void h8_add_resid(H8Quad& t, uint2 r) {
  t.t0 += unpack2(r.x);
  t.t1 += unpack2(r.y);
}

// The 32x32 accumulator gives lane (jj, hh) HALF of each 16-byte record (channels 8 q + 4 hh + 0..3 of pixel jj).  With the lane's words
// of records 2 pr (h0, h1) and 2 pr + 1 (h2, h3), v_permlane32_swap trades halves between lanes jj and jj + 32 so that lane (jj, hh) owns the
// WHOLE record 2 pr + hh: one dwordx4 per lane, each half-wave a contiguous 512 bytes.  Applied to a whole record loaded that way
// (x, y, z, w) it is its own inverse: the lane gets back its halves of both records.
__device__ __forceinline__ uint4 h8_swap16(unsigned h0, unsigned h1, unsigned h2, unsigned h3) {
  const auto s0 = __builtin_amdgcn_permlane32_swap(h0, h2, false, false);
  const auto s1 = __builtin_amdgcn_permlane32_swap(h1, h3, false, false);
  return make_uint4(s0[0], s1[0], s0[1], s1[1]);
}

// LeakyReLU in place, as max(t, slope t) like h8_bias_leaky (the late activation of conv_h8_late_kernel: after the residual add)
__device__ __forceinline__ void h8_leaky(H8Quad& t, float2v sl) {
  t.t0 = __builtin_elementwise_max(t.t0, t.t0 * sl);
  t.t1 = __builtin_elementwise_max(t.t1, t.t1 * sl);
}

// 8 fp32 multipliers (Dropout2d) of one channel block, rounded to fp16 first: B fragments take them as packed multiplies
__device__ __forceinline__ half8 h8_multipliers(const float* sp) {
  const float4 s0 = *reinterpret_cast<const float4*>(sp), s1 = *reinterpret_cast<const float4*>(sp + 4);
  half8 h;
  h[0] = (_Float16)s0.x; h[1] = (_Float16)s0.y; h[2] = (_Float16)s0.z; h[3] = (_Float16)s0.w;
  h[4] = (_Float16)s1.x; h[5] = (_Float16)s1.y; h[6] = (_Float16)s1.z; h[7] = (_Float16)s1.w;
  return h;
}

// The run of work items (tiles, strips; nx * ny * n of them) of a persistent workgroup: item = beg, beg + step, ... < end.  Workgroups that
// share an XCD (blockIdx.x % 8) are numbered side by side (w), and item = w + i * #workgroups: at any moment the resident workgroups cover
// one compact band of the image, so neighbouring halos meet in L2 and DRAM sees long contiguous rows.  The three factors come as scalars and
// the result as a struct by value: with the product as one argument, or with out-parameters, the callers' prologues compiled differently.
struct H8Run {
  int beg, end, step;
};
__device__ __forceinline__ H8Run h8_tile_run(int nx, int ny, int n) {
  const int nwg = gridDim.x, b = blockIdx.x, xcd = b & 7, qq = nwg >> 3, rr = nwg & 7;
  const int w = (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + (b >> 3);
  const long long nt = (long long)nx * ny * n;
  return H8Run{w, w < nt ? w + (int)((nt - w + nwg - 1) / nwg) * nwg : w, nwg};
}

// accumulator tiles := 0 (conv_h8_kernel, conv1x1_h8_res_kernel and the two tail kernels keep their loops: see there)
template <int M, int N>
__device__ __forceinline__ void h8_zero(f32x16 (&acc)[M][N]) {
#pragma unroll
  for (int i = 0; i < M; ++i)
#pragma unroll
    for (int b = 0; b < N; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][b][r] = 0.0f;
}
// f(integral_constant<int, 0>), f(<1>), ... : a loop whose index is a compile-time constant in its body (counted waits, register names)
template <class F, int... Cs>
__device__ __forceinline__ void h8_static_for(F&& f, std::integer_sequence<int, Cs...>) {
  (f(std::integral_constant<int, Cs>{}), ...);
}

// "The chunk has landed and nobody reads the buffer that is filled next."  vmcnt counts loads, LDS-DMA and stores in issue order, so
// h8_vmcnt<N> retires all but the N youngest vector-memory operations: N = what the kernel issued after the DMA it waits for (a kernel
// computes its own counts); h8_lds_barrier then makes every wave's LDS traffic visible and holds the compiler's memory operations in place.
template <int N>
__device__ __forceinline__ void h8_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
__device__ __forceinline__ void h8_lgkmcnt0() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
__device__ __forceinline__ void h8_barrier() {
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}
__device__ __forceinline__ void h8_lds_barrier() {
  h8_lgkmcnt0();
  h8_barrier();
}
template <int N>
__device__ __forceinline__ void h8_chunk_landed() {
  h8_vmcnt<N>();
  h8_lds_barrier();
}

// The row walk of the one-thread-per-record kernels (pooling, space <-> depth, bilinear): grid x = (channel block g, tile of 256 columns),
// y = row, z = image, so a thread's only division is the uniform blockIdx.x / tiles; y and z stride where a launch has more rows or images
// than a grid dimension holds.  The kernel returns where x is past its last column.  By value as a struct, like H8Run.
struct H8Col { int g, x; };
__device__ __forceinline__ H8Col h8_row_col(int tiles) {
  const int g = (int)(blockIdx.x / (unsigned)tiles);
  return H8Col{g, (int)(blockIdx.x - (unsigned)g * (unsigned)tiles) * 256 + (int)threadIdx.x};
}
// ... and its grid for `blocks` channel blocks of rows x cols records in n images; false where grid x would not fit
inline bool h8_row_grid(int blocks, int cols, int rows, int n, dim3& grid, int& tiles) {
  tiles = (cols + 255) / 256;
  if ((long long)tiles * blocks > 0x7fffffffLL) return false;
  grid = dim3((unsigned)(tiles * blocks), (unsigned)(rows < 65535 ? rows : 65535), (unsigned)(n < 65535 ? n : 65535));
  return true;
}
// every pointer on a 16-byte boundary (a null pointer counts as aligned: optional arguments)
template <class... P>
inline bool h8_aligned16(const P*... p) {
  return ((... | (uintptr_t)p) & 15) == 0;
}

}  // namespace
