// Half-precision storage path ("h8"): activations live in HBM as fp16 in channel blocks of 8,
//     x[N][G = C/8][H][W][8]         (16 bytes per (pixel, block); azimuth-adjacent pixels are adjacent records)
// and every conv multiplies fp16 x fp16 on v_mfma_f32_32x32x16_f16 with fp32 accumulation and an fp32 epilogue
// (bias, LeakyReLU, folded BatchNorm, residual) before rounding the result to fp16 once.  The layout makes ONE
// 16-byte record = ONE MFMA B operand of one lane (lane (pixel r, half h) holds the 8 channels of block 2k+h), so
// staging a tile is a plain 16-byte copy (no conversion, no transpose), a wave's global loads / stores are 1 KB
// contiguous along the azimuth, and HBM traffic is half of the fp32 path.  BASELINE.json configs[2],[4] name this
// storage precision ("bf16"); fp16 is used instead because the activations of the range-image stack are O(1..100)
// and fp16's 11-bit mantissa keeps the logits within the 1e-3 parity bar (bf16 does not).
//
//   conv_h8_kernel      3x3 / dilated / 2x2 convs: LDS tile [blocks][rows+halo][cols+halo] of 16-byte records,
//                       register prefetch of the next channel chunk during the MFMA phase
//   conv1x1_h8_kernel   1x1 convs: no halo => B operands straight from global memory, weights through LDS
//   The layout / pooling / pixel-shuffle kernels around the convs are in layout_h8.hip.
#include <stdio.h>
#include "h8_common.h"
#include <cstdlib>

// scheduling options of the 8-wave 128-channel configuration (conv_h8_kernel's OPT), as measured with tools/h8_ab.py (one process,
// interleaved rounds, N = 64, single-source form): 15 is +1 ... +3 % on the 3x3 layers and +3 ... +7 % on the 2x2-dilated ones; two K-steps
// per barrier paid (+6 ... +8 %) only while the per-chunk set-up was expensive and costs 2 ... 4 % since it is one scalar multiply-add
#ifndef H8_M128_OPT_3X3
#define H8_M128_OPT_3X3 15
#endif
#ifndef H8_M128_OPT_2X2
#define H8_M128_OPT_2X2 15
#endif
#ifndef H8_M128_KPC2_DEFAULT
#define H8_M128_KPC2_DEFAULT 0      // 2x2-dilated 128 / 256-channel layers: two K-steps per barrier (kept as an A/B switch, SLU_H8_KPC2=1)
#endif

namespace {

struct H8Src {
  const uint4* ptr;    // [nimg][G][H][W] records
  const float* scale;  // [N][8 G] fp32 multiplier per (output image, channel) or nullptr
  int G;               // channel blocks of the stored tensor
  int gbeg;            // first block of this source in the concatenated input
  int nb;              // 0: holds N images; k > 0: holds k images, output image n reads n % k
  int shuf;            // 1: read through PixelShuffle(2) in place: ptr is [nimg][4 G][H/2][W/2] with its channels stored in shuffle order (slu.h)
};

struct H8Args {
  H8Src src[SLU_MAX_SRC];
  int nsrc;
  int N, H, W, Gin, Cout, Gout, nmblk, nks;   // nks = 16-channel K-steps = ceil(Gin / 2)
  const uint4* wpack;
  const float *bias, *bn_a, *bn_b;
  int has_act;
  float slope;
  int out_f32;         // 1: `out` is fp32 NCHW [N][Cout][H][W] (the logits head); 0: h8
  int tiles_x, tiles_y;
  int order;                 // 0: each workgroup walks a contiguous run of tiles; 1: tiles interleaved across workgroups
#ifdef SLU_H8_AB
  int dbg;                   // ablation switches of gemm1x1_h8_kernel (SLU_GEMM_DBG, -DSLU_H8_AB builds only): 1 no input DMA, 2 no weight DMA, 4 no MFMA
#endif
};

struct SrcSel {
  const uint4* ptr;
  const float* scale;
  int G, gl, ns;
};

__device__ __forceinline__ SrcSel select_src(const H8Args& a, const int (&img)[SLU_MAX_SRC], int g) {
  SrcSel p{a.src[0].ptr, a.src[0].scale, a.src[0].G, g, img[0]};
#pragma unroll
  for (int s = 1; s < SLU_MAX_SRC; ++s)
    if (s < a.nsrc && g >= a.src[s].gbeg) p = SrcSel{a.src[s].ptr, a.src[s].scale, a.src[s].G, g - a.src[s].gbeg, img[s]};
  return p;
}

// Epilogue shared by both kernels: one 32-channel x 32-pixel accumulator tile of a lane -> 4 x (4 channels)
//   chan0: first channel of the 32-block; se: LDS constants bias | bn_a | bn_b indexed by `cl0 + ...`
template <int STRIDE>
__device__ __forceinline__ void store_tile(const H8Args& a, const f32x16& acc, const float* se, int cl0, int co0, int hh, bool pix_ok,
                                           size_t n, size_t pix, size_t HW, const void* __restrict__ resid, void* __restrict__ out,
                                           float slope_pre) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int cl = cl0 + 8 * q + 4 * hh + k;
      float t = acc[4 * q + k] + se[cl];
      t = t > 0.0f ? t : t * slope_pre;
      v[k] = t * se[STRIDE + cl] + se[2 * STRIDE + cl];
    }
    const int co = co0 + 8 * q + 4 * hh;           // first of this lane's 4 channels
    if (a.out_f32) {
      float* o = reinterpret_cast<float*>(out);
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (pix_ok && co + k < a.Cout) o[(n * a.Cout + co + k) * HW + pix] = v[k];
    } else {
      const int go = co >> 3;
      const bool ok = pix_ok && go < a.Gout;
      const size_t idx = ok ? ((n * a.Gout + go) * HW + pix) * 2 + hh : 0;   // 8-byte half records
      if (resid) {
        const uint2 rv = reinterpret_cast<const uint2*>(resid)[idx];
        const half2v r0 = __builtin_bit_cast(half2v, rv.x), r1 = __builtin_bit_cast(half2v, rv.y);
        v[0] += (float)r0[0]; v[1] += (float)r0[1]; v[2] += (float)r1[0]; v[3] += (float)r1[1];
      }
      if (ok) reinterpret_cast<uint2*>(out)[idx] = make_uint2(pack2(v[0], v[1]), pack2(v[2], v[3]));
    }
  }
}

// Epilogue of the persistent kernel (h8 output): EVERY lane issues its 4 stores (and its 4 residual loads when they were
// not prefetched) -- lanes outside the image / past the last channel block read the zero record and store to a scratch
// record -- so the number of vector-memory operations per tile is a compile-time constant the kernel's counted waits rely on.
// LATE (conv_h8_late_kernel): the activation comes AFTER the residual add, out = leaky(conv + bias + resid) with slope `slope_late`; the caller
// passes slope_pre = 1 and the layer carries no folded BatchNorm (its constants are the defaults 1 / 0).
template <int STRIDE, bool PRE, bool LATE = false>
__device__ __forceinline__ void store_tile_full(const H8Args& a, const f32x16& acc, const float* se, int cl0, int go0, int hh, bool pix_ok, size_t n,
                                                size_t pix, size_t HW, const uint2* __restrict__ resid, const uint2 (&rv)[4],
                                                uint2* __restrict__ out, float slope_pre, uintptr_t zero_addr, uintptr_t trash_addr,
                                                float slope_late = 1.0f) {
  const float4* se4 = reinterpret_cast<const float4*>(se);
  const float2v sl = {slope_pre, slope_pre};
  const size_t plane2 = HW * 2;
  const size_t idx0 = ((n * a.Gout + go0) * HW + pix) * 2 + hh;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int c4 = (cl0 + 8 * q) / 4 + hh;
    H8Quad t = h8_epilogue(acc, q, se4[c4], se4[STRIDE / 4 + c4], se4[2 * STRIDE / 4 + c4], sl);
    const bool ok = pix_ok && go0 + q < a.Gout;
    const size_t idx = idx0 + q * plane2;
    if (resid) h8_add_resid(t, PRE ? rv[q] : *(ok ? resid + idx : reinterpret_cast<const uint2*>(zero_addr)));
    if constexpr (LATE) h8_leaky(t, float2v{slope_late, slope_late});
    *(ok ? out + idx : reinterpret_cast<uint2*>(trash_addr)) = pack4(t);
  }
}

// The same epilogue with whole 16-byte records on the way out (h8_swap16): lane half 0 stores the record of block 2 pr and lane half 1
// that of block 2 pr + 1 -- 2 store instructions per accumulator tile instead of 4.  The residual is added before the exchange from 8-byte
// loads of the lane's own channels, each waited for in full where it is used: rare on the layers the TILED kernel serves; the GEMM, whose
// 768 -> 256 layers all carry one, has its own form (gemm_store_tile) and keeps this one as its A/B fallback.  The tensor-or-trash choice
// goes through an integer, so the loads and stores here are FLAT operations (they count in lgkmcnt as well as vmcnt).
template <int STRIDE, bool LATE = false>
__device__ __forceinline__ void store_tile_swap16(const H8Args& a, const f32x16& acc, const float* se, int cl0, int go0, int hh, bool pix_ok, size_t n,
                                                  size_t pix, size_t HW, const uint2* __restrict__ resid, uint4* __restrict__ out, float slope_pre,
                                                  uintptr_t zero_addr, uintptr_t trash_addr, float slope_late = 1.0f) {
  const float4* se4 = reinterpret_cast<const float4*>(se);
  const float2v sl = {slope_pre, slope_pre};
#pragma unroll
  for (int pr = 0; pr < 2; ++pr) {
    unsigned hw[4];
#pragma unroll
    for (int q2 = 0; q2 < 2; ++q2) {
      const int q = 2 * pr + q2;
      const int c4 = (cl0 + 8 * q) / 4 + hh;
      H8Quad t = h8_epilogue(acc, q, se4[c4], se4[STRIDE / 4 + c4], se4[2 * STRIDE / 4 + c4], sl);
      if (resid) {
        const bool okq = pix_ok && go0 + q < a.Gout;
        h8_add_resid(t, *(okq ? resid + (((n * a.Gout + go0 + q) * HW + pix) * 2 + hh) : reinterpret_cast<const uint2*>(zero_addr)));
      }
      if constexpr (LATE) h8_leaky(t, float2v{slope_late, slope_late});
      hw[2 * q2] = pack2(t.t0);
      hw[2 * q2 + 1] = pack2(t.t1);
    }
    const uint4 rec = h8_swap16(hw[0], hw[1], hw[2], hw[3]);
    const int go = go0 + 2 * pr + hh;
    *((pix_ok && go < a.Gout) ? out + ((n * a.Gout + go) * HW + pix) : reinterpret_cast<uint4*>(trash_addr)) = rec;
  }
}

// gemm1x1_h8_kernel's form of the same epilogue.  Every lane of every tile is live there (H W % 256 == 0, Cout = 64 MB), so there is no trash
// record and the address keeps its address space: global_store_dwordx4 at `obase` (wave-uniform: the tile's first record of the accumulator
// tile's first block) plus the lane's 32-bit byte offset `vo` (half hh, pixel), record 2 pr + hh; pr = 0 / 1 are `plane2` bytes (two planes of
// H W records) apart, added on the scalar side.  RES: res[pr] is the residual's record 2 pr + hh, loaded whole by the caller (the same offsets
// from the residual's base) and retired by a counted wait before the call; h8_swap16 gives the lane back its halves of records 2 pr and 2 pr + 1.  Same arithmetic, in the same order, as
// store_tile_swap16: h8_epilogue, h8_add_resid, pack2, swap.
template <int STRIDE, bool RES>
__device__ __forceinline__ void gemm_store_tile(const f32x16& acc, const float* se, int cl0, int hh, const u32x4v (&res)[2], char* obase, unsigned vo,
                                                unsigned plane2, float slope_pre) {
  const float4* se4 = reinterpret_cast<const float4*>(se);
  const float2v sl = {slope_pre, slope_pre};
#pragma unroll
  for (int pr = 0; pr < 2; ++pr) {
    uint4 rw = make_uint4(0u, 0u, 0u, 0u);       // residual words: x, y for q = 2 pr; z, w for q = 2 pr + 1
    if constexpr (RES) rw = h8_swap16(res[pr].x, res[pr].y, res[pr].z, res[pr].w);
    unsigned hw[4];
#pragma unroll
    for (int q2 = 0; q2 < 2; ++q2) {
      const int q = 2 * pr + q2;
      const int c4 = (cl0 + 8 * q) / 4 + hh;
      H8Quad t = h8_epilogue(acc, q, se4[c4], se4[STRIDE / 4 + c4], se4[2 * STRIDE / 4 + c4], sl);
      if constexpr (RES) h8_add_resid(t, q2 ? make_uint2(rw.z, rw.w) : make_uint2(rw.x, rw.y));
      hw[2 * q2] = pack2(t.t0);
      hw[2 * q2 + 1] = pack2(t.t1);
    }
    *reinterpret_cast<uint4*>(obase + (size_t)pr * plane2 + vo) = h8_swap16(hw[0], hw[1], hw[2], hw[3]);
  }
}

#ifdef SLU_H8_PROF      // development aid: per-phase shader-clock totals of wave 0 of every workgroup of the tiled kernel
__device__ unsigned long long g_h8_prof[8];
#define H8_PROF_MARK(i)                                         \
  {                                                             \
    const unsigned long long t_now = __builtin_amdgcn_s_memtime(); \
    asm volatile("" ::: "memory");                              \
    prof_acc[i] += t_now - prof_t;                              \
    prof_t = t_now;                                             \
  }
#else
#define H8_PROF_MARK(i)
#endif

// -----------------------------------------------------------------------------------------------------------
// Tiled kernel, persistent, LDS-DMA staged.  Workgroup = WM x WN waves; output tile = TH rows x 64 columns x
// (32 WM MB) channels.  Tiles are dealt to the resident workgroups round-robin (tile = w + i * #workgroups, the 32
// workgroups of an XCD side by side along the azimuth), so at any moment the chip works on one compact band of the
// image: neighbouring halos meet in L2 and DRAM sees long contiguous rows.  The unit of staging is a chunk = one
// K-step (16 channels): the input tile (2 channel blocks, halo included) and the weight fragments are copied
// global -> LDS by global_load_lds (no staging registers), into the buffer the previous chunk is not using, piece
// by piece BETWEEN the taps of the current chunk's MFMA phase; the chunk after a tile's last one is the first
// chunk of the NEXT tile, so loads stay in flight across the epilogue.
// One barrier per chunk.  WRES: the weight fragments of ALL K-steps stay in LDS for the whole kernel (small
// layers).  SCALED: per-(image, channel) multipliers (Dropout2d on a concatenated input) are applied to the B
// fragments after the LDS read.
// -----------------------------------------------------------------------------------------------------------
// KPC: K-steps (16 channels each) per chunk = per barrier (2 for the 2x2-dilated 128-channel layers, whose 4 taps per K-step are too
// little MFMA work per barrier).  OPT (bit mask, the 8-wave 128-channel configuration): 1 = waves 4..7 (the SIMD partners of waves
// 0..3) issue a tap's LDS-DMA pieces BEFORE its MFMAs, waves 0..3 after them, so the two waves of a SIMD stop stalling on the
// address pipe at the same moment; 2 = s_setprio 1 around the MFMA cluster; 4 = the next chunk's staging set-up runs before the
// wait + barrier instead of after; 8 = whole 16-byte records per lane on the way out (v_permlane32_swap).
// ONE: the layer has ONE plain source (no concatenation, no batch broadcast): the staging set-up of a chunk is one 64-bit multiply-add on
// the scalar unit instead of the source-selection chains of the general form.
// waves per SIMD the registers allow: the kernel's __launch_bounds__ and launch_h8_k's persistent grid
constexpr int h8_waves_per_simd(int mb, int nwave, int rpw) { return (mb * rpw >= 8) ? 1 : ((nwave >= 8 || mb >= 2 || rpw >= 2) ? 2 : 3); }

// The kernel's text is conv_h8_tiled_kernel.h, compiled into two symbols.  conv_h8_late_kernel: the 3x3 / dil 1 / pad 1 layer with the activation
// AFTER the residual add, out = leaky(conv + bias + resid) -- the second conv of a ResNet BasicBlock (BatchNorm folded into weight and bias,
// ReLU = slope 0); same template parameters, tile walk, staging and counted waits, no SCALED / fp32-output / multi-K-step forms.
#define H8_TILED_KERNEL conv_h8_kernel
#define H8_TILED_LATE false
#include "conv_h8_tiled_kernel.h"
#undef H8_TILED_KERNEL
#undef H8_TILED_LATE
#define H8_TILED_KERNEL conv_h8_late_kernel
#define H8_TILED_LATE true
#include "conv_h8_tiled_kernel.h"
#undef H8_TILED_KERNEL
#undef H8_TILED_LATE

// -----------------------------------------------------------------------------------------------------------
// 1x1 convs, streaming: a wave owns NBW blocks of 32 consecutive pixels and ALL output channels (MB blocks of 32).
// Its B operands are 16-byte global loads (lane (r, h): block 2k+h of pixel r; per wave two 512-byte runs), the
// input is read exactly once, the output written once; only the weight fragments go through LDS.
// Needs H*W % 32 == 0 and no multipliers.
// -----------------------------------------------------------------------------------------------------------
template <int MB, int NBW>
__global__ __launch_bounds__(256, (MB * NBW >= 8) ? 2 : ((MB * NBW >= 4) ? 3 : 4)) void conv1x1_h8_kernel(const H8Args a, const void* __restrict__ resid,
                                                                                                         void* __restrict__ out) {
  constexpr int KSPC = 4;                               // K-steps (16 channels each) per weight chunk
  constexpr int NWV = MB * KSPC * 64, NW = (NWV + 255) / 256;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint4* s_a = reinterpret_cast<uint4*>(smem);          // [MB][KSPC][64]
  float* s_epi = reinterpret_cast<float*>(s_a + MB * KSPC * 64);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int hh = lane >> 5, jj = lane & 31;
  const long long HW = (long long)a.H * a.W;
  const long long nblocks = (long long)a.N * HW / 32;
  const long long pb0 = ((long long)blockIdx.x * 4 + wave) * NBW;

  if (tid < MB * 32) {
    const bool ok = tid < a.Cout;
    H8_FILL_EPI(s_epi, 0, MB * 32, tid, ok, tid, a.bias, a.bn_a, a.bn_b);
  }

  f32x16 acc[MB][NBW];
  h8_zero(acc);

  int nimg[NBW];
  long long hw[NBW];
  bool live[NBW];
  int simg[NBW][SLU_MAX_SRC];
#pragma unroll
  for (int b = 0; b < NBW; ++b) {
    const long long pb = pb0 + b;
    live[b] = pb < nblocks;
    const long long pix = (live[b] ? pb : 0) * 32 + jj;
    nimg[b] = (int)(pix / HW);
    hw[b] = pix - nimg[b] * HW;
#pragma unroll
    for (int s = 0; s < SLU_MAX_SRC; ++s) simg[b][s] = (s < a.nsrc && a.src[s].nb) ? nimg[b] % a.src[s].nb : nimg[b];
  }

  const int nq = (a.nks + KSPC - 1) / KSPC;
#ifdef SLU_H8_PROF      // phases: input loads issued + first barrier | weight staging | second barrier | MFMAs (incl. waiting for the inputs) | epilogue
  unsigned long long prof_acc[6] = {0, 0, 0, 0, 0, 0}, prof_t = __builtin_amdgcn_s_memtime();
#endif
  for (int q = 0; q < nq; ++q) {
    uint4 x[KSPC][NBW];
#pragma unroll
    for (int ks = 0; ks < KSPC; ++ks) {
      const int g = 2 * (q * KSPC + ks) + hh;           // this lane half's channel block
#pragma unroll
      for (int b = 0; b < NBW; ++b) {
        const bool ok = live[b] && g < a.Gin;
        const SrcSel p = select_src(a, simg[b], ok ? g : 0);
        const size_t idx = ok ? ((size_t)p.ns * p.G + p.gl) * HW + hw[b] : 0;
        const uint4 v = p.ptr[idx];
        x[ks][b] = ok ? v : make_uint4(0u, 0u, 0u, 0u);
      }
    }
    __syncthreads();
    H8_PROF_MARK(0)
    uint4 sw[NW];
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      const int e = tid + i * 256;
      const int m = e / (KSPC * 64);
      const int r = e - m * (KSPC * 64);
      const int ks = r >> 6;
      const bool ok = (NWV % 256 == 0 || e < NWV) && m < a.nmblk && q * KSPC + ks < a.nks;
      const size_t off = ok ? ((size_t)m * a.nks + q * KSPC) * 64 + r : 0;
      sw[i] = a.wpack[off];
      if (!ok) sw[i] = make_uint4(0u, 0u, 0u, 0u);
    }
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      const int e = tid + i * 256;
      if (NWV % 256 == 0 || e < NWV) s_a[e] = sw[i];
    }
#ifdef SLU_H8_PROF
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#endif
    H8_PROF_MARK(1)
    __syncthreads();
    H8_PROF_MARK(2)
#pragma unroll
    for (int ks = 0; ks < KSPC; ++ks)
#pragma unroll
      for (int i = 0; i < MB; ++i) {
        const half8 af = __builtin_bit_cast(half8, s_a[(i * KSPC + ks) * 64 + lane]);
#pragma unroll
        for (int b = 0; b < NBW; ++b)
          acc[i][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af, __builtin_bit_cast(half8, x[ks][b]), acc[i][b], 0, 0, 0);
      }
#ifdef SLU_H8_PROF
    asm volatile("s_nop 0" ::"v"(acc[MB - 1][NBW - 1][0]));      // the last MFMA has retired
#endif
    H8_PROF_MARK(3)
  }

  const float slope_pre = (a.has_act & 3) == 1 ? a.slope : 1.0f;
#pragma unroll
  for (int i = 0; i < MB; ++i)
#pragma unroll
    for (int b = 0; b < NBW; ++b)
      store_tile<MB * 32>(a, acc[i][b], s_epi, i * 32, i * 32, hh, live[b], (size_t)nimg[b], (size_t)hw[b], (size_t)HW, resid, out, slope_pre);
#ifdef SLU_H8_PROF
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  H8_PROF_MARK(4)
  if (tid == 0) {
    for (int i = 0; i < 5; ++i) atomicAdd(&g_h8_prof[i], prof_acc[i]);
    atomicAdd(&g_h8_prof[5], 1ull);
  }
#endif
}

// -----------------------------------------------------------------------------------------------------------
// 1x1 convs with few output channels (MB <= 2 blocks of 32) and few input channels (NKS K-steps, all of them resident
// in LDS as weight fragments): pure streaming.  No barrier after the prologue: a wave takes one block of 32 pixels at
// a time (grid-stride, so the chip sweeps memory as one front), issues ALL its NKS input loads (16 B per lane each, two
// 512-byte runs per wave) and the residual loads at once, and multiplies as they arrive.  Memory-level parallelism
// comes from occupancy (4-5 waves per SIMD, up to NKS KB in flight per wave); LDS only serves the A fragments.
// -----------------------------------------------------------------------------------------------------------
// 4-wave workgroups per CU (= waves per SIMD) the registers allow: the kernel's __launch_bounds__ and launch_h8_1x1_res's grid
constexpr int h8_1x1_res_waves_per_simd(int mb, int nks) { return (mb * nks >= 12) ? 2 : ((mb * nks >= 2) ? 3 : 4); }

template <int MB, int NKS>
__global__ __launch_bounds__(256, h8_1x1_res_waves_per_simd(MB, NKS)) void conv1x1_h8_res_kernel(const H8Args a, const void* __restrict__ resid, void* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* s_epi = reinterpret_cast<float*>(smem);                 // bias | bn_a | bn_b
  uint4* s_a = reinterpret_cast<uint4*>(s_epi + 3 * MB * 32);    // [MB][NKS][64]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int hh = lane >> 5, jj = lane & 31;
  const long long HW = (long long)a.H * a.W;
  const long long nblocks = (long long)a.N * HW / 32;

  if (tid < MB * 32) {
    const bool ok = tid < a.Cout;
    H8_FILL_EPI(s_epi, 0, MB * 32, tid, ok, tid, a.bias, a.bn_a, a.bn_b);
  }
  for (int e = tid; e < MB * NKS * 64; e += 256) {
    const int m = e / (NKS * 64);
    const int r = e - m * (NKS * 64);
    const bool ok = m < a.nmblk && (r >> 6) < a.nks;
    s_a[e] = ok ? a.wpack[(size_t)m * a.nks * 64 + r] : make_uint4(0u, 0u, 0u, 0u);
  }
  __syncthreads();

  const float slope_pre = (a.has_act & 3) == 1 ? a.slope : 1.0f;
  const uint2* resid2 = reinterpret_cast<const uint2*>(resid);
  const long long stride = (long long)gridDim.x * 4;
  for (long long pb = (long long)blockIdx.x * 4 + wave; pb < nblocks; pb += stride) {
    const long long pix = pb * 32 + jj;
    const int n = (int)(pix / HW);
    const size_t hw = (size_t)(pix - n * HW);
    int img[SLU_MAX_SRC];
#pragma unroll
    for (int s = 0; s < SLU_MAX_SRC; ++s) img[s] = (s < a.nsrc && a.src[s].nb) ? n % a.src[s].nb : n;
    uint4 x[NKS];
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      const int g = 2 * ks + hh;                        // this lane half's channel block
      const bool ok = g < a.Gin;
      const SrcSel p = select_src(a, img, ok ? g : 0);
      const uint4 v = p.ptr[ok ? ((size_t)p.ns * p.G + p.gl) * HW + hw : 0];
      x[ks] = ok ? v : make_uint4(0u, 0u, 0u, 0u);
    }
    uint2 rv[MB][4];
    if (resid) {
#pragma unroll
      for (int i = 0; i < MB; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int go = i * 4 + q;
          rv[i][q] = go < a.Gout ? resid2[(((size_t)n * a.Gout + go) * HW + hw) * 2 + hh] : make_uint2(0u, 0u);
        }
    }
    f32x16 acc[MB];
#pragma unroll
    for (int i = 0; i < MB; ++i)      // written out: a helper inverts a branch of <1, 1>
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][r] = 0.0f;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks)
#pragma unroll
      for (int i = 0; i < MB; ++i)
        acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(half8, s_a[(i * NKS + ks) * 64 + lane]), __builtin_bit_cast(half8, x[ks]),
                                                        acc[i], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < MB; ++i) {
      if (a.out_f32) {
        store_tile<MB * 32>(a, acc[i], s_epi, i * 32, i * 32, hh, true, (size_t)n, hw, (size_t)HW, nullptr, out, slope_pre);
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          float v[4];
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const int cl = i * 32 + 8 * q + 4 * hh + k;
            float t = acc[i][4 * q + k] + s_epi[cl];
            t = t > 0.0f ? t : t * slope_pre;
            v[k] = t * s_epi[MB * 32 + cl] + s_epi[2 * MB * 32 + cl];
          }
          if (resid) {
            const half2v r0 = __builtin_bit_cast(half2v, rv[i][q].x), r1 = __builtin_bit_cast(half2v, rv[i][q].y);
            v[0] += (float)r0[0]; v[1] += (float)r0[1]; v[2] += (float)r1[0]; v[3] += (float)r1[1];
          }
          const int go = i * 4 + q;
          if (go < a.Gout)
            reinterpret_cast<uint2*>(out)[(((size_t)n * a.Gout + go) * HW + hw) * 2 + hh] = make_uint2(pack2(v[0], v[1]), pack2(v[2], v[3]));
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
  }
}

// -----------------------------------------------------------------------------------------------------------
// Wide 1x1 convs with 256 output channels (768 -> 256 concat convs and the 128 / 256 -> 256 shortcuts of the U-Net's lower levels) as a plain
// GEMM, out[Cout][pixels] = W[Cout][Cin] x[Cin][pixels]: BOTH operands go global -> LDS by global_load_lds into a ring of D chunks of KC K-steps,
// D - 1 in flight, issued as one burst behind the barrier that frees the slot; one barrier per chunk; every wave issues the same number of DMAs
// at every position (beyond the end: the zero record), so "chunk c has landed" is the constant vmcnt((D - 2) NPIECE).  A workgroup of 8 waves
// (2 along the channels x 4 along the pixels) owns 256 consecutive pixels of one image plane and all channels: the weights stream once per 256
// pixels (the streaming conv1x1_h8_kernel re-reads them per 128 and stages them through registers + two barriers per 64 channels).
// Measured (N = 64, tools/h8_1x1_bench.py, profiles/r10; streaming kernel -> this one): 768 -> 256 + residual at 16x512 502 -> 372 us, at 8x256
// 131 -> 90, 128 -> 256 at 16x512 118 -> 89, 256 -> 256 at 8x256 46 -> 37; the 128-output instantiation <2, 4, 3> 543 -> 478 us on 384 -> 128 +
// residual at 32x1024 (149 -> 137 at 16x512) and is dispatched for exactly those layers (gemm1x1_ok).  With the epilogue before r10 (below) the
// 768 -> 256 layer took 449 us and the 128-output form 618: its residual cost 159 of the 449 us, now 86 of 372.  What the r03 ablation
// switches (SLU_GEMM_DBG in -DSLU_H8_AB builds) showed on 768 -> 256: no input DMA 399 us, no weight DMA 413, no MFMA 354, none of the three STILL 306 of
// 481 -- the time is in the per-chunk skeleton (32 DMA instructions per CU and chunk, barrier, fragment reads) and the epilogue, not in HBM,
// L2 or the matrix cores; a deeper ring of smaller chunks (KC 2, D 4) was slower (484) than two 64-channel chunks (459).
// The residual (AHEAD, the default).  The 768 -> 256 layers all carry one.  It is loaded in whole 16-byte records (lane (jj, hh): record
// 2 pr + hh of each accumulator tile, un-swapped by h8_swap16 before the add) by inline-asm global_load_dwordx4 the compiler does not
// track, so it places no wait of its own: the records of the first two M-blocks (8 loads, 32 registers) are issued behind the barrier of the
// tile's LAST chunk, BEFORE that chunk's stage_next(), and retired at the top of the epilogue by vmcnt(NPIECE) -- vmcnt retires in issue order,
// and the only younger operations are the NPIECE DMAs of that stage_next(), the next tile's burst, which stays in flight.  With MB = 4 the
// records of M-blocks 2, 3 are issued at the top of the epilogue, into the registers the fragments have left, and retired by vmcnt(8) behind
// the 8 stores of M-blocks 0, 1 (which retires the burst too: it has had the last chunk's MFMA phase and half an epilogue to land).  Every
// wave issues the same vector-memory operations at every tile, and all of them are global_*: nothing counts in lgkmcnt but LDS reads.
// The chunk wait vmcnt((D - 2) NPIECE) assumes that only DMA pieces are younger than the chunk it waits for; residual loads and stores issued
// in between make it stricter (the chunk is then older than the (D - 2) NPIECE youngest operations by more), never wrong.  With D = 2 it is a
// full wait anyway.
// The form before that (AHEAD = false, SLU_GEMM1X1_RES_AHEAD=0, kept for A/B runs and the bit-equality test: gemm1x1_h8_kernel_v1) is
// store_tile_swap16: 4 FLAT 8-byte loads per accumulator tile, each followed by the compiler's vmcnt(0) lgkmcnt(0) -- 32 serial round trips per
// wave and tile in <4, 4, 2>, each draining the next tile's burst and the stores just issued, with all eight waves in the epilogue together.
// Needs: Cout = 64 MB, H W % 256 == 0 (so every lane of every tile is live), nks % KC == 0, every source a whole number of chunks, no
// multipliers / batch broadcast, 16 Gout H W < 2^32 (the lane's byte offset inside one image of the output is 32-bit).
// -----------------------------------------------------------------------------------------------------------
template <int MB, int KC, int D, bool AHEAD, bool RES>
__device__ __forceinline__ void gemm1x1_h8_body(const H8Args& a, const void* __restrict__ resid, void* __restrict__ out) {
  constexpr int NWAVE = 8, MBLK = 2 * MB, TP = 256, NB = 2;
  constexpr int NREC_A = MBLK * KC * 64, NREC_B = 2 * KC * TP;           // records per chunk: weight fragments, input tile [2 KC blocks][256 px]
  constexpr int NPA = MBLK * KC, NPB = 2 * KC * 4;                       // 64-record pieces
  constexpr int NIA = (NPA + NWAVE - 1) / NWAVE, NIB = NPB / NWAVE;
  constexpr int NPIECE = NIA + NIB;
  static_assert(NPB % NWAVE == 0 && NPA % NWAVE == 0 && D >= 2 && (D - 2) * NPIECE <= 63, "pieces divide over the waves; vmcnt is 6 bits");

  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* s_epi = reinterpret_cast<float*>(smem);                         // bias | bn_a | bn_b
  uint4* s_b = reinterpret_cast<uint4*>(s_epi + 3 * MBLK * 32);          // [D][NREC_B]
  uint4* s_a = s_b + D * NREC_B;                                         // [D][MBLK][KC][64]

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3, hh = lane >> 5, jj = lane & 31;
  const size_t HW = (size_t)a.H * a.W;
  const int tiles_per_img = (int)(HW / TP);
  const int ntiles = tiles_per_img * a.N, nch = a.nks / KC;
  const int t_step = gridDim.x, t_beg = (int)blockIdx.x;
  if (t_beg >= ntiles) return;

  if (tid < MBLK * 32) {
    const bool ok = tid < a.Cout;
    H8_FILL_EPI(s_epi, 0, MBLK * 32, tid, ok, tid, a.bias, a.bn_a, a.bn_b);
  }
  H8_OPAQUE_ADDR(zero_addr, h8_zero_rec);
  H8_OPAQUE_ADDR(trash_addr, h8_trash_rec);

  // the staging cursor runs D - 1 chunks ahead of the compute cursor: (s_tile, s_q) = the next chunk to copy, into ring slot s_slot
  int s_tile = t_beg, s_q = 0, s_slot = 0;
  auto stage_next = [&]() __attribute__((always_inline)) {
    const bool valid = s_tile < ntiles;
    int wv = wave;
    asm volatile("" : "+s"(wv));                                        // (keeps the per-piece address arithmetic out of the loop-invariant set)
    uintptr_t base = zero_addr;
    if (valid) {
      const int n = s_tile / tiles_per_img, p0 = (s_tile - n * tiles_per_img) * TP;
      const int g = 2 * KC * s_q;                                        // first channel block of the chunk: one source holds the whole chunk
      const uint4* ptr = a.src[0].ptr;
      int G = a.src[0].G, gl = g;
#pragma unroll
      for (int s = 1; s < SLU_MAX_SRC; ++s)
        if (s < a.nsrc && g >= a.src[s].gbeg) ptr = a.src[s].ptr, G = a.src[s].G, gl = g - a.src[s].gbeg;
      base = reinterpret_cast<uintptr_t>(ptr) + 16 * (((size_t)n * G + gl) * HW + p0);
    }
    uint4* db = s_b + s_slot * NREC_B;
    uint4* da = s_a + s_slot * NREC_A;
#pragma unroll
    for (int i = 0; i < NIB; ++i) {
      const int p = i * NWAVE + wv;                                      // block = p / 4, pixel quarter = p % 4
      const uintptr_t src = (valid && !SLU_ABLATE(a, 1)) ? base + 16 * ((size_t)(p >> 2) * HW + (size_t)((p & 3) * 64 + lane)) : zero_addr;
      SLU_GLDS16(reinterpret_cast<const uint4*>(src), db + p * 64);
    }
#pragma unroll
    for (int i = 0; i < NIA; ++i) {
      const int p = i * NWAVE + wv;                                      // = m * KC + ks
      const int m = p / KC, ks = p - m * KC;
      const uint4* src = (valid && !SLU_ABLATE(a, 2)) ? a.wpack + ((size_t)m * a.nks + KC * s_q + ks) * 64 + lane : reinterpret_cast<const uint4*>(zero_addr);
      SLU_GLDS16(src, da + p * 64);
    }
    asm volatile("" ::: "memory");
    s_slot = s_slot + 1 == D ? 0 : s_slot + 1;
    if (++s_q == nch) s_q = 0, s_tile += t_step;
  };
#pragma unroll
  for (int c = 0; c < D - 1; ++c) stage_next();

  int r_slot = 0;
  const float slope_pre = (a.has_act & 3) == 1 ? a.slope : 1.0f;
  [[maybe_unused]] const uint2* resid2 = reinterpret_cast<const uint2*>(resid);
  const int abase = (wm * MB) * KC * 64 + lane;
  const int bbase = hh * TP + wn * 64 + jj;

  // AHEAD: byte offset of the lane's record (block hh, pixel of accumulator column b) from the tile's first record of block 0, the same in the
  // residual and in the output; the wave's M-block i and pair pr add (4 (wm MB + i) + 2 pr) planes to the scalar base, which keeps the sixteen
  // offsets of a tile out of the vector registers.  Two sets of 8 residual records: M-blocks 0, 1 / 2, 3.
  static_assert(!AHEAD || MB == 2 || MB == 4, "the residual waits name 8 registers per set");
  const unsigned plane = (unsigned)(HW * 16);
  unsigned voff[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) voff[b] = (unsigned)(hh * HW * 16) + (unsigned)((wn * 64 + b * 32 + jj) * 16);
  unsigned long long rbase = 0;
  auto load_resid = [&](u32x4v (&r)[2][NB][2], int i0) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int pr = 0; pr < 2; ++pr) {
          const unsigned long long base = rbase + (unsigned long long)((wm * MB + i0 + i) * 4 + 2 * pr) * plane;
          asm volatile("global_load_dwordx4 %0, %1, %2" : "=&v"(r[i][b][pr]) : "v"(voff[b]), "s"(base) : "memory");
        }
  };

  for (int tile = t_beg; tile < ntiles; tile += t_step) {
    f32x16 acc[MB][NB];
    h8_zero(acc);
    u32x4v ra[2][NB][2], rb[2][NB][2];
    const int n = tile / tiles_per_img, p0 = (tile - n * tiles_per_img) * TP;
    const size_t tile16 = 16 * ((size_t)n * a.Gout * HW + p0);        // the tile's first record of block 0, in bytes
    if constexpr (AHEAD) rbase = reinterpret_cast<unsigned long long>(resid) + tile16;
    for (int q = 0; q < nch; ++q) {
      // the oldest chunk in flight has landed once at most the (D - 2) younger chunks' pieces are outstanding (residual loads and stores of an
      // epilogue in between only make the wait stricter); then every wave is past its reads of the slot that is re-filled next
      h8_chunk_landed<(D - 2) * NPIECE>();
      if constexpr (AHEAD && RES)
        if (q == nch - 1) load_resid(ra, 0);      // older than the burst below: vmcnt(NPIECE) retires them and not the burst
      stage_next();
      const uint4* sb = s_b + r_slot * NREC_B + bbase;
      const uint4* sa = s_a + r_slot * NREC_A + abase;
      r_slot = r_slot + 1 == D ? 0 : r_slot + 1;
      half8 af[2][MB], bf[2][NB];
      auto read_frags = [&](int set, int ks) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < MB; ++i) af[set][i] = __builtin_bit_cast(half8, sa[(i * KC + ks) * 64]);
#pragma unroll
        for (int b = 0; b < NB; ++b) bf[set][b] = __builtin_bit_cast(half8, sb[2 * ks * TP + b * 32]);
      };
      read_frags(0, 0);
#pragma unroll
      for (int ks = 0; ks < KC; ++ks) {
        if (ks + 1 < KC) read_frags((ks + 1) & 1, ks + 1);
        __builtin_amdgcn_sched_barrier(0);
        if (!SLU_ABLATE(a, 4)) {
#pragma unroll
          for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int i = 0; i < MB; ++i) acc[i][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[ks & 1][i], bf[ks & 1][b], acc[i][b], 0, 0, 0);
        } else {
#pragma unroll
          for (int i = 0; i < MB; ++i) asm volatile("" ::"v"(af[ks & 1][i]));
#pragma unroll
          for (int b = 0; b < NB; ++b) asm volatile("" ::"v"(bf[ks & 1][b]));
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    if constexpr (AHEAD) {
      char* obase = reinterpret_cast<char*>(out) + tile16;
      {
        auto blocks = [&](const u32x4v (&r)[2][NB][2], int i0) __attribute__((always_inline)) {
#pragma unroll
          for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int b = 0; b < NB; ++b) {
              gemm_store_tile<MBLK * 32, RES>(acc[i0 + i][b], s_epi, (wm * MB + i0 + i) * 32, hh, r[i][b], obase + (size_t)((wm * MB + i0 + i) * 4) * plane,
                                              voff[b], 2 * plane, slope_pre);
              __builtin_amdgcn_sched_barrier(0);
            }
        };
        // M-blocks 0, 1: their records were issued before the last chunk's stage_next(), whose NPIECE DMAs are all that is younger
        if constexpr (RES)
          asm volatile("s_waitcnt vmcnt(%8)"
                       : "+v"(ra[0][0][0]), "+v"(ra[0][0][1]), "+v"(ra[0][1][0]), "+v"(ra[0][1][1]), "+v"(ra[1][0][0]), "+v"(ra[1][0][1]),
                         "+v"(ra[1][1][0]), "+v"(ra[1][1][1])
                       : "n"(NPIECE));
        if constexpr (RES && MB == 4) load_resid(rb, 2);
        blocks(ra, 0);
        if constexpr (MB == 4) {
          // M-blocks 2, 3: younger than their records are the 2 NB 2 stores above
          if constexpr (RES)
            asm volatile("s_waitcnt vmcnt(%8)"
                         : "+v"(rb[0][0][0]), "+v"(rb[0][0][1]), "+v"(rb[0][1][0]), "+v"(rb[0][1][1]), "+v"(rb[1][0][0]), "+v"(rb[1][0][1]),
                           "+v"(rb[1][1][0]), "+v"(rb[1][1][1])
                         : "n"(2 * NB * 2));
          blocks(rb, 2);
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < MB; ++i) {
        const int ml = wm * MB + i;
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          const size_t pix = (size_t)p0 + wn * 64 + b * 32 + jj;
          store_tile_swap16<MBLK * 32>(a, acc[i][b], s_epi, ml * 32, ml * 4, hh, true, (size_t)n, pix, HW, resid2, reinterpret_cast<uint4*>(out), slope_pre,
                                       zero_addr, trash_addr);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // zero-record DMAs issued beyond the last chunk: LDS must not be released under them
}

template <int MB, int KC, int D>
__global__ __launch_bounds__(512, 2) void gemm1x1_h8_kernel(const H8Args a, const void* __restrict__ resid, void* __restrict__ out) {
  // with and without a residual: two whole tile loops (one uniform branch per launch, and the registers of the residual records stay out of
  // the loop that has none)
  if (resid) gemm1x1_h8_body<MB, KC, D, true, true>(a, resid, out);
  else gemm1x1_h8_body<MB, KC, D, true, false>(a, resid, out);
}
// the epilogue before the residual was loaded ahead (SLU_GEMM1X1_RES_AHEAD=0)
template <int MB, int KC, int D>
__global__ __launch_bounds__(512, 2) void gemm1x1_h8_kernel_v1(const H8Args a, const void* __restrict__ resid, void* __restrict__ out) {
  gemm1x1_h8_body<MB, KC, D, false, false>(a, resid, out);      // (RES is not read: store_tile_swap16 tests `resid` per tile)
}

// wpack[mblk][kstep][tap][lane][8]: lane (r, h) holds W[co = 32 mblk + r][ci = 16 kstep + 8 h + j][tap], j = 0..7, as fp16
__global__ void pack_h8_kernel(const float* __restrict__ w, int cout, int cin, int ks, int nks, size_t total, uint4* __restrict__ out) {
  const int T = ks * ks;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const int lane = (int)(e & 63);
    size_t r = e >> 6;
    const int tap = (int)(r % T);
    r /= T;
    const int k = (int)(r % nks);
    const int m = (int)(r / nks);
    const int co = m * 32 + (lane & 31);
    float x[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int ci = k * 16 + 8 * (lane >> 5) + j;
      x[j] = (co < cout && ci < cin) ? w[((size_t)co * cin + ci) * T + tap] : 0.0f;
    }
    out[e] = h8_pack8(x);
  }
}

int fill_h8(const slu_conv_h8_desc* d, H8Args& a) {
  if (!d || !d->out || !d->wpack || d->nsrc < 1 || d->nsrc > SLU_MAX_SRC) return SLU_EINVAL;
  if (d->N <= 0 || d->H <= 0 || d->W <= 0 || d->Cout <= 0) return SLU_EINVAL;
  if (d->bn_a && !d->bn_b) return SLU_EINVAL;
  if (d->has_act != 0 && d->has_act != 1) return SLU_EINVAL;
  if (d->has_act && !(d->slope >= 0.0f && d->slope <= 1.0f)) return SLU_EINVAL;      // LeakyReLU is evaluated as max(v, slope v)
  int g = 0;
  for (int s = 0; s < d->nsrc; ++s) {
    const slu_h8_src& S = d->src[s];
    if (!S.ptr || S.G <= 0 || S.nbatch < 0 || (S.shuffle != 0 && S.shuffle != 1)) return SLU_EINVAL;
    if (((uintptr_t)S.ptr & 15) || ((uintptr_t)S.scale & 15)) return SLU_EINVAL;
    // a shuffled source: the first one, whole groups of 64 stored channels (an even number of contributed blocks), even output size
    if (S.shuffle && (s != 0 || S.G % 8 || (d->H & 1) || (d->W & 1) || S.nbatch)) return SLU_EINVAL;
    const int gc = S.shuffle ? S.G / 4 : S.G;      // blocks this source contributes to the concatenated input
    a.src[s] = H8Src{reinterpret_cast<const uint4*>(S.ptr), S.scale, gc, g, S.nbatch, S.shuffle};
    g += gc;
  }
  for (int s = d->nsrc; s < SLU_MAX_SRC; ++s) a.src[s] = H8Src{nullptr, nullptr, 0, 0x7fffffff, 0, 0};
  if (((uintptr_t)d->out & 15) || ((uintptr_t)d->resid & 15) || ((uintptr_t)d->wpack & 15)) return SLU_EINVAL;
  if (d->resid && d->out_f32_nchw) return SLU_EINVAL;
  if (d->act_after_resid != 0 && d->act_after_resid != 1) return SLU_EINVAL;
  a.nsrc = d->nsrc;
  a.N = d->N; a.H = d->H; a.W = d->W;
  a.Gin = g;
  a.Cout = d->Cout;
  a.Gout = (d->Cout + 7) / 8;
  a.nmblk = (d->Cout + 31) / 32;
  a.nks = (g + 1) / 2;
  a.wpack = reinterpret_cast<const uint4*>(d->wpack);
  a.bias = d->bias; a.bn_a = d->bn_a; a.bn_b = d->bn_b;
  a.has_act = d->has_act; a.slope = d->slope;
  a.out_f32 = d->out_f32_nchw ? 1 : 0;
  a.tiles_x = a.tiles_y = 0;
#ifdef SLU_H8_AB
  static const int dbg = [] { const char* e = getenv("SLU_GEMM_DBG"); return e ? atoi(e) : 0; }();
  a.dbg = dbg;
#endif
  return SLU_OK;
}

template <int KS, int DIL, int PAD, int MB, int WM, int WN, int RPW, bool SCALED, bool WRES, bool F32OUT = false, int KPC = 1, int OPT = 0, bool ONE = false,
          bool LATE = false>
int launch_h8_k(H8Args& a, const slu_conv_h8_desc* d, const SluEmit& e) {
  constexpr int TH = WN * RPW, MBLK = WM * MB, T = KS * KS, NWAVE = WM * WN;
  constexpr size_t nb_alloc = (size_t)((KPC * 2 * (TH + 2 * PAD) * (64 + 2 * PAD) + 63) / 64) * 64;
  const size_t lds = (size_t)3 * MBLK * 32 * 4 + (SCALED ? 2048 : 0) + 2 * nb_alloc * 16 + (size_t)MBLK * (WRES ? a.nks : 2 * KPC) * T * 64 * 16;
  if (lds > 160 * 1024) return SLU_EUNSUPPORTED;
  if (SCALED && a.Gin > 64) return SLU_EUNSUPPORTED;
  if (a.src[0].shuf) {      // a source read through PixelShuffle in place: the SCALED 3x3 kernels only; one table record per stored block of it
    if (!(SCALED && KS == 3 && DIL == 1 && PAD == 1 && !ONE && KPC == 1 && !F32OUT)) return SLU_EUNSUPPORTED;
    if (3 * a.src[0].G + a.Gin > 64) return SLU_EUNSUPPORTED;
  }
  a.tiles_x = (a.W + 63) / 64;
  a.tiles_y = (a.H + TH - 1) / TH;
  static const int order = [] { const char* e = getenv("SLU_H8_ORDER"); return e ? atoi(e) : 1; }();      // 0 is kept for A/B runs
  a.order = order;
  const long long nt = (long long)a.tiles_x * a.tiles_y * a.N;
  const int gy = (a.nmblk + MBLK - 1) / MBLK;
  if (nt <= 0 || nt > 0x7fffffffLL || gy > 65535) return SLU_EUNSUPPORTED;
  if (e.name) {
    return slu_emit_name(e, LATE ? "conv_h8_late_kernel<%d, %d, %d, %d, %d, %d, %d, %s, %s, %s, %d, %d, %s>"
                                 : "conv_h8_kernel<%d, %d, %d, %d, %d, %d, %d, %s, %s, %s, %d, %d, %s>",
                         KS, DIL, PAD, MB, WM, WN, RPW, slu_tf(SCALED), slu_tf(WRES), slu_tf(F32OUT), KPC, OPT, slu_tf(ONE));
  }
  // persistent grid: as many workgroups as fit on the 256 CUs at once (registers / LDS), never more than tiles
  long long per_cu = h8_waves_per_simd(MB, NWAVE, RPW) * 4 / NWAVE;
  const long long by_lds = (long long)(160 * 1024 / lds);
  if (by_lds < per_cu) per_cu = by_lds;
  if (per_cu < 1) per_cu = 1;
  long long gx = (256 * per_cu + gy - 1) / gy;
  if (gx < 8) gx = 8;
  if (gx > nt) gx = nt;
  static SluLdsGrant grant;
  if constexpr (LATE)
    return slu_launch_lds(conv_h8_late_kernel<KS, DIL, PAD, MB, WM, WN, RPW, SCALED, WRES, F32OUT, KPC, OPT, ONE>, dim3((unsigned)gx, (unsigned)gy),
                          dim3(64 * NWAVE), lds, e.st, grant, a, d->resid, d->out);
  else
    return slu_launch_lds(conv_h8_kernel<KS, DIL, PAD, MB, WM, WN, RPW, SCALED, WRES, F32OUT, KPC, OPT, ONE>, dim3((unsigned)gx, (unsigned)gy),
                          dim3(64 * NWAVE), lds, e.st, grant, a, d->resid, d->out);
}

// -----------------------------------------------------------------------------------------------------------
// 3x3 convs of the full-resolution layers with 32 / 64 input and output channels, ONE plain source: the deep-ring form.
// conv_h8_kernel keeps one 16-channel chunk (~21-43 KB) of DMA in flight per CU while it multiplies the previous one; at
// 5.5 TB/s x ~2 us of loaded latency a CU needs ~43 KB in flight ALL the time, and these layers have too little MFMA work
// per chunk to cover one round trip.  Here (the structure of tail2_h8_kernel, conv_tail_h8.hip):
//   * all weights resident in LDS for the life of the persistent workgroup (<= 72 KB);
//   * the rest of the LDS is a ring of D input chunks (16 channels with halo), D - 1 of them in flight;
//   * one wave owns ALL output channels of its pixels (MB blocks) and RPW rows; fragments double-buffered in source order;
//   * counted vmcnt waits: every wave issues the same VM operations at every position of every tile (surplus DMA slots
//     copy the zero record to a trash block, beyond the last tile whole chunks do);
//   * whole 16-byte records per lane on the way out (v_permlane32_swap between lanes jj and jj + 32).
// One tile = NKS positions: wait(chunk s) | barrier | DMA(chunk s + P) | 9 taps of chunk s ; after the last: epilogue, NST stores.
// -----------------------------------------------------------------------------------------------------------
struct RingArgs {
  const uint4 *x, *x1;         // h8 [N][G0][H][W] (+ a second plain source [N][G1][H][W], G0 + G1 = 2 NKS, G0 even: the concatenation)
  int G0, G1;
  const uint4* wpack;          // [MB][NKS][9][64]
  const float *bias, *bn_a, *bn_b;
  float slope;                 // 1 = no activation
  uint4* out;                  // h8 [N][4 MB][H][W]
  int N, H, W, tiles_x, tiles_y;
  // x read through PixelShuffle(2) in place (NKS = 5 only): x is [N][4 G0][H/2][W/2] with channels stored in shuffle order, so the record of
  // contributed block g at pixel (gy, gx) is the stored record of plane 4 g + 2 (gy & 1) + (gx & 1) at (gy >> 1, gx >> 1)
  int shuf;
  const float* sc0;            // shuf: [N][32 G0] fp32 multipliers per stored channel (stored order) or nullptr
};

template <int NKS, int NIB, int P, int NST>
constexpr int ring3_younger(int c) {             // VM operations issued after the DMA of chunk c and before the top of position c
  const int s0 = ((c - P) % NKS + NKS) % NKS;
  int n = s0 == NKS - 1 ? NST : 0;
  for (int d = 1; d < P; ++d) n += NIB + ((s0 + d) % NKS == NKS - 1 ? NST : 0);
  return n;
}

template <int DIL, int MB, int NKS, int RPW, int D>
__global__ __launch_bounds__(512, 2) void ring3_h8_kernel(const RingArgs a) {
  constexpr int NWAVE = 8, KS = 3, T = 9, PAD = DIL, P = D - 1;
  constexpr int C = 32 * MB, GO = 4 * MB;
  constexpr int TW = 64, TH = NWAVE * RPW, NB = 2 * RPW;
  constexpr int LW = TW + 2 * PAD, LH = TH + 2 * PAD, REC = LH * LW;
  constexpr int NBLK_B = (2 * REC + 63) / 64, NIB = (NBLK_B + NWAVE - 1) / NWAVE;
  constexpr int BUFREC = NBLK_B * 64;
  constexpr int NST = MB * NB * 2;
  static_assert(P >= 1 && P <= NKS, "ring depth");

  // static array + native vector loads: see tail2_h8_kernel (reads without a TBAA tag are guarded with vmcnt(0) by the compiler)
  __shared__ __attribute__((aligned(16))) float s_epi[3 * C];
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint4* s_w = reinterpret_cast<uint4*>(smem);                      // [MB][NKS][9][64]
  uint4* s_ring = s_w + MB * NKS * T * 64;                          // [D][BUFREC]
  uint4* s_trash = s_ring + D * BUFREC;                             // [64]
  uint4* s_mul = s_trash + 64;                                      // shuf with multipliers: [N][4 G0] fp16 records, one per stored block

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), wn = wave;
  const int hh = lane >> 5, jj = lane & 31;
  const size_t HW = (size_t)a.H * a.W;

  const H8Run run = h8_tile_run(a.tiles_x, a.tiles_y, a.N);
  const int t_beg = run.beg, t_end = run.end, t_step = run.step;
  if (t_beg >= t_end) return;

  if (tid < C) H8_FILL_EPI(s_epi, 0, C, tid, true, tid, a.bias, a.bn_a, a.bn_b);
  for (int blk = wave; blk < MB * NKS * T; blk += NWAVE) SLU_GLDS16(a.wpack + (size_t)blk * 64 + lane, s_w + blk * 64);
  const bool mul0 = NKS == 5 && a.shuf && a.sc0;
  if constexpr (NKS == 5) {
    // the multiplier table goes to LDS once, here: the tile loop's VM operations (and ring3_younger) stay what they are
    if (mul0) {
      for (int e = tid; e < a.N * 4 * a.G0; e += 64 * NWAVE) {
        s_mul[e] = __builtin_bit_cast(uint4, h8_multipliers(a.sc0 + (size_t)e * 8));
      }
    }
  }
  const int hw4 = (a.H >> 1) * (a.W >> 1), w2 = a.W >> 1;

  struct TilePos { int x0, y0, n; };
  auto decode = [&](int t) {
    TilePos p;
    const int tx = t % a.tiles_x;
    t /= a.tiles_x;
    p.x0 = tx * TW;
    p.y0 = (t % a.tiles_y) * TH;
    p.n = t / a.tiles_y;
    return p;
  };
  int pc_rc[NIB], pc_off[NIB];
#pragma unroll
  for (int i = 0; i < NIB; ++i) {
    const int e = (i * NWAVE + wave) * 64 + lane;
    const int g2 = e / REC, rem = e - g2 * REC, r = rem / LW, c = rem - r * LW;
    pc_rc[i] = r | (c << 8) | ((g2 & 1) << 16) | ((e < 2 * REC ? 1 : 0) << 17);
    pc_off[i] = (r * a.W + c) * 16;
  }
  auto stage = [&](const TilePos& tp, int c, int slot, bool valid) {
    uint4* db = s_ring + slot * BUFREC;
    const uintptr_t zero = reinterpret_cast<uintptr_t>(&h8_zero_rec);
    const bool second = 2 * c >= a.G0;                  // a K-step never straddles the two sources (G0 is even)
    const uint4* src = second ? a.x1 : a.x;
    const int gs = second ? a.G1 : a.G0, g = second ? 2 * c - a.G0 : 2 * c;
    const bool sh = NKS == 5 && a.shuf && !second;      // the 4 stored planes of a contributed block span HW records, as a plain block does
    const uintptr_t base0 = reinterpret_cast<uintptr_t>(src) +
                            16 * ((long long)(((size_t)tp.n * gs + g) * HW) + (sh ? 0ll : (long long)(tp.y0 - PAD) * a.W + (tp.x0 - PAD)));
    const uintptr_t base1 = base0 + 16 * (long long)HW;
#pragma unroll
    for (int i = 0; i < NIB; ++i) {
      const int blk = i * NWAVE + wave;
      const int rc = pc_rc[i];
      const int gy = tp.y0 - PAD + (rc & 255), gx = tp.x0 - PAD + ((rc >> 8) & 255);
      const bool ok = valid && (rc >> 17) && (unsigned)gy < (unsigned)a.H && (unsigned)gx < (unsigned)a.W;
      int off = pc_off[i];
      if constexpr (NKS == 5) {
        if (sh) off = 16 * ((2 * (gy & 1) + (gx & 1)) * hw4 + (gy >> 1) * w2 + (gx >> 1));
      }
      const uintptr_t p = ok ? (((rc >> 16) & 1) ? base1 : base0) + (long long)off : zero;
      SLU_GLDS16(reinterpret_cast<const uint4*>(p), (NBLK_B % NWAVE == 0 || blk < NBLK_B) ? db + blk * 64 : s_trash);
    }
    asm volatile("" ::: "memory");
  };

  const int bbase = hh * REC + (wn * RPW) * LW + jj;
  TilePos cur = decode(t_beg), nxt = cur;
  bool has_next = t_beg + t_step < t_end;
  if (has_next) nxt = decode(t_beg + t_step);
#pragma unroll
  for (int c = 0; c < P; ++c) stage(cur, c, c, true);
  int rslot = 0, wslot = P % D;
  bool first = true;
  const float2v sl = {a.slope, a.slope};
  const f32x4v* se4p = reinterpret_cast<const f32x4v*>(s_epi) + hh;

  for (int tile = t_beg; tile < t_end; tile += t_step) {
    f32x16 acc[MB][NB];
    h8_zero(acc);

    auto position = [&](auto cc) {
      constexpr int c = decltype(cc)::value;
      constexpr int YOUNG = ring3_younger<NKS, NIB, P, NST>(c);
      static_assert(YOUNG <= 63, "vmcnt is a 6-bit counter");
      if (first && c < P) h8_vmcnt<0>();          // the first tile's prologue (and the resident weights)
      else h8_vmcnt<YOUNG>();
      h8_lds_barrier();
      {
        constexpr int cn = (c + P) % NKS;
        if (c + P < NKS) stage(cur, cn, wslot, true);
        else stage(nxt, cn, wslot, has_next);
        wslot = wslot + 1 == D ? 0 : wslot + 1;
      }
      const uint4* sb = s_ring + rslot * BUFREC + bbase;
      rslot = rslot + 1 == D ? 0 : rslot + 1;
      half8 fa[2][MB], fb[2][NB];
      // K-step 0 of a shuffled source with multipliers: the lane's B fragment at tap (ty, tx) is input pixel (y0 + wn + ty - 1, x0 + 32 b + jj + tx - 1)
      // of contributed block hh = stored block 4 hh + 2 (row parity) + (column parity); y0 and x0 are even, so the lane needs four records of
      // its image's table: msc[ty & 1][tx & 1]
      constexpr bool MUL = NKS == 5 && c == 0 && RPW == 1 && DIL == 1;
      half8 msc[MUL ? 2 : 1][MUL ? 2 : 1];
      if constexpr (MUL) {
        if (mul0) {
#pragma unroll
          for (int ty = 0; ty < 2; ++ty)
#pragma unroll
            for (int tx = 0; tx < 2; ++tx)
              msc[ty][tx] = __builtin_bit_cast(half8, s_mul[cur.n * 4 * a.G0 + 4 * hh + 2 * ((wn + ty + 1) & 1) + ((jj + tx + 1) & 1)]);
        }
      }
      auto rd = [&](int tap, int buf) {
        const int dy = (tap / KS) * DIL, dx = (tap % KS) * DIL;
#pragma unroll
        for (int i = 0; i < MB; ++i) fa[buf][i] = __builtin_bit_cast(half8, s_w[((i * NKS + c) * T + tap) * 64 + lane]);
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          fb[buf][b] = __builtin_bit_cast(half8, sb[((b >> 1) + dy) * LW + (b & 1) * 32 + dx]);
          if constexpr (MUL) {
            if (mul0) fb[buf][b] *= msc[(tap / KS) & 1][(tap % KS) & 1];
          }
        }
      };
      rd(0, 0);
#pragma unroll
      for (int tap = 0; tap < T; ++tap) {
        if (tap + 1 < T) rd(tap + 1, (tap + 1) & 1);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
          for (int i = 0; i < MB; ++i) acc[i][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[tap & 1][i], fb[tap & 1][b], acc[i][b], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
    };
    h8_static_for(position, std::make_integer_sequence<int, NKS>{});
    first = false;

#pragma unroll
    for (int i = 0; i < MB; ++i)
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const int gy = cur.y0 + wn * RPW + (b >> 1), gx = cur.x0 + (b & 1) * 32 + jj;
        const bool ok = gy < a.H && gx < a.W;
        const size_t idx0 = ok ? ((size_t)cur.n * GO + i * 4 + hh) * HW + (size_t)gy * a.W + gx : 0;
#pragma unroll
        for (int pr = 0; pr < 2; ++pr) {
          unsigned hw[4];
#pragma unroll
          for (int q2 = 0; q2 < 2; ++q2) {
            const int q = 2 * pr + q2;
            const int c4 = (i * 32 + 8 * q) / 4;
            const H8Quad t = h8_epilogue(acc[i][b], q, se4p[c4], se4p[C / 4 + c4], se4p[2 * C / 4 + c4], sl);
            hw[2 * q2] = pack2(t.t0);
            hw[2 * q2 + 1] = pack2(t.t1);
          }
          const uint4 rec = h8_swap16(hw[0], hw[1], hw[2], hw[3]);
          *(ok ? a.out + idx0 + (size_t)(2 * pr) * HW : &h8_trash_rec) = rec;
        }
      }
    asm volatile("" ::: "memory");
    cur = nxt;
    has_next = tile + 2 * t_step < t_end;
    if (has_next) nxt = decode(tile + 2 * t_step);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // zero-record DMAs issued for the tile after the last: LDS must not be released under them
}

template <int DIL, int MB, int NKS, int RPW, int D>
int launch_ring3(const H8Args& h, const slu_conv_h8_desc* d, const SluEmit& e) {
  constexpr int TH = 8 * RPW, PAD = DIL;
  constexpr size_t nblk_b = (size_t)(2 * (TH + 2 * PAD) * (64 + 2 * PAD) + 63) / 64;
  constexpr size_t lds0 = ((size_t)MB * NKS * 9 * 64 + (size_t)D * nblk_b * 64 + 64) * 16;      // + 3 * 32 MB floats static
  static_assert(lds0 + 3 * 32 * MB * 4 <= 160 * 1024, "ring does not fit in LDS");
  // a shuffled first source (NKS = 5: UpBlock.conv1 at full resolution): its multiplier table [N][4 G0] records joins the ring in LDS
  const bool shuf = h.src[0].shuf != 0;
  if (shuf && (NKS != 5 || RPW != 1 || DIL != 1 || h.src[0].G != 2)) return SLU_EUNSUPPORTED;      // K-step 0 is the only one multiplied
  const size_t lds = lds0 + ((shuf && h.src[0].scale) ? (size_t)h.N * 4 * h.src[0].G * 16 : 0);
  if (lds + 3 * 32 * MB * 4 > 160 * 1024) return -1;      // the table does not fit: the tiled SCALED kernel
  RingArgs a{};
  a.shuf = shuf ? 1 : 0;
  a.sc0 = shuf ? h.src[0].scale : nullptr;
  a.x = h.src[0].ptr; a.G0 = h.src[0].G;
  a.x1 = h.nsrc > 1 ? h.src[1].ptr : h.src[0].ptr; a.G1 = h.nsrc > 1 ? h.src[1].G : 0;
  a.wpack = h.wpack; a.bias = h.bias; a.bn_a = h.bn_a; a.bn_b = h.bn_b;
  a.slope = (h.has_act & 3) == 1 ? h.slope : 1.0f;
  a.out = reinterpret_cast<uint4*>(d->out);
  a.N = h.N; a.H = h.H; a.W = h.W;
  a.tiles_x = (a.W + 63) / 64;
  a.tiles_y = (a.H + TH - 1) / TH;
  const long long nt = (long long)a.tiles_x * a.tiles_y * a.N;
  if (nt < 256) return -1;      // too few tiles to fill the chip: the tiled kernel
  if (nt > 0x7fffffffLL) return SLU_EUNSUPPORTED;
  if (e.name) return slu_emit_name(e, "ring3_h8_kernel<%d, %d, %d, %d, %d>", DIL, MB, NKS, RPW, D);
  static SluLdsGrant grant;
  return slu_launch_lds(ring3_h8_kernel<DIL, MB, NKS, RPW, D>, dim3(256), dim3(512), lds, e.st, grant, a);
}

// the layers ring3_h8_kernel covers: 3x3 (dil 1 / 2), one or two plain sources of 32 / 64 (80 -> 32: dil 1) channels in all, 32 / 64 output
// channels, h8 output, no residual, activation before BN only
bool ring3_ok(const slu_conv_h8_desc* d, const H8Args& a) {
  static const bool off = [] { const char* e = getenv("SLU_H8_RING3"); return e && e[0] == '0'; }();      // A/B switch
  if (off || d->ksize != 3 || d->pad != d->dil || (d->dil != 1 && d->dil != 2) || a.nsrc < 1 || a.nsrc > 2) return false;
  int gsum = 0;
  for (int s = 0; s < a.nsrc; ++s) {
    if ((a.src[s].scale && !a.src[s].shuf) || a.src[s].nb) return false;
    gsum += a.src[s].G;
  }
  // in-place PixelShuffle: the 80 -> 32 instantiation with exactly ONE shuffled K-step (64 stored channels -> blocks 0, 1): the kernel
  // stages any K-step of source 0 through the shuffle but multiplies K-step 0 only
  if (a.src[0].shuf && !(a.nsrc == 2 && a.Gin == 10 && a.src[0].G == 2)) return false;
  if (gsum != a.Gin || (a.nsrc == 2 && (a.src[0].G & 1)) || a.out_f32 || d->resid || (a.has_act & ~1)) return false;
  if ((a.has_act & 1) && !(a.slope >= 0.0f && a.slope <= 1.0f)) return false;      // LeakyReLU as max(t, slope t)
  return (a.Cout == 32 || a.Cout == 64) && ((a.Gin == 4 || a.Gin == 8) || (a.Gin == 10 && a.Cout == 32 && d->dil == 1));
}

// <DIL, MB, NKS, RPW, D>: 16-row tiles (RPW 2) where the weights and the ring fit in LDS; -1 when the layer has fewer than 256 tiles of that height
int launch_ring3_any(const H8Args& a, const slu_conv_h8_desc* d, const SluEmit& e) {
  const int mb = a.Cout / 32, nks = a.Gin / 2;
  if (nks == 5) return launch_ring3<1, 1, 5, 1, 4>(a, d, e);                       // 80 -> 32: PixelShuffle output | skip (UpBlock.conv1, full resolution)
  if (mb == 2 && nks == 4) return d->dil == 1 ? launch_ring3<1, 2, 4, 1, 3>(a, d, e) : launch_ring3<2, 2, 4, 1, 3>(a, d, e);
  if (mb == 2 && nks == 2) return d->dil == 1 ? launch_ring3<1, 2, 2, 2, 3>(a, d, e) : launch_ring3<2, 2, 2, 1, 3>(a, d, e);
  if (mb == 1 && nks == 4) return d->dil == 1 ? launch_ring3<1, 1, 4, 2, 3>(a, d, e) : launch_ring3<2, 1, 4, 1, 3>(a, d, e);
  return d->dil == 1 ? launch_ring3<1, 1, 2, 2, 3>(a, d, e) : launch_ring3<2, 1, 2, 2, 3>(a, d, e);
}

constexpr size_t WRES_MAX_BYTES = 24 * 1024;

// weights of all K-steps stay resident in LDS when they are small (full-resolution 32-channel layers)
template <int KS, int DIL, int PAD, int MB, int WM, int WN, int RPW, bool SCALED>
int launch_h8(H8Args& a, const slu_conv_h8_desc* d, const SluEmit& e) {
  const size_t wbytes = (size_t)WM * MB * a.nks * KS * KS * 64 * 16;
  if (wbytes <= WRES_MAX_BYTES) return launch_h8_k<KS, DIL, PAD, MB, WM, WN, RPW, SCALED, true>(a, d, e);
  return launch_h8_k<KS, DIL, PAD, MB, WM, WN, RPW, SCALED, false>(a, d, e);
}

inline long long wg_count(const H8Args& a, int th, int mblk) {
  return (long long)a.N * ((a.H + th - 1) / th) * ((a.W + 63) / 64) * ((a.nmblk + mblk - 1) / mblk);
}

// tile configurations {MB, WM, WN, RPW}: 8-wave workgroups (16 or 8 rows) when the layer has enough tiles for
// every CU, 4-wave ones with 8 / 4 rows for the small feature maps at the bottom of the U-Net
enum { CFG_M32_TH16 = 0, CFG_M64_TH16, CFG_M128_TH8, CFG_M32_TH8, CFG_M64_TH8, CFG_M128_TH4, CFG_M32_TH4, CFG_M64_TH4, CFG_COUNT };

int choose_h8(const H8Args& a) {
  const long long want = 256;
  static const int forced = [] { const char* e = getenv("SLU_H8_CFG"); return e ? atoi(e) : -1; }();      // development aid
  if (forced >= 0 && forced < CFG_COUNT) return forced;
  if (a.nmblk >= 4) {
    if (a.H >= 8 && wg_count(a, 8, 4) >= want) return CFG_M128_TH8;
    if (wg_count(a, 4, 4) >= want) return CFG_M128_TH4;
    if (wg_count(a, 4, 2) >= want) return CFG_M64_TH4;
    return CFG_M32_TH4;
  }
  if (a.nmblk >= 2) {
    if (a.H >= 16 && wg_count(a, 16, 2) >= want) return CFG_M64_TH16;
    if (a.H >= 8 && wg_count(a, 8, 2) >= want) return CFG_M64_TH8;
    if (wg_count(a, 4, 2) >= want) return CFG_M64_TH4;
    return CFG_M32_TH4;
  }
  if (a.H >= 16 && wg_count(a, 16, 1) >= want) return CFG_M32_TH16;
  if (a.H >= 8 && wg_count(a, 8, 1) >= want) return CFG_M32_TH8;
  return CFG_M32_TH4;
}

// The 8-wave 128-channel configuration (the MFMA-bound 128 / 256-channel layers of the U-Net's lower levels) with its scheduling
// options (conv_h8_kernel's OPT / KPC).  SLU_H8_OPT / SLU_H8_KPC2 (environment) and, in -DSLU_H8_AB builds, slu_h8_dev_set_opt()
// are A/B switches of the development tools.
int g_h8_opt = [] { const char* e = getenv("SLU_H8_OPT"); return e ? atoi(e) : -1; }();
int g_h8_kpc2 = [] { const char* e = getenv("SLU_H8_KPC2"); return e ? atoi(e) : H8_M128_KPC2_DEFAULT; }();

constexpr size_t h8_m128_weight_bytes(int nks, int T) { return (size_t)4 * nks * T * 64 * 16; }

inline bool h8_one_plain_source(const H8Args& a) { return a.nsrc == 1 && a.src[0].nb == 0 && !a.src[0].scale; }

template <int KS, int DIL, int PAD, bool SCALED>
int launch_h8_m128(H8Args& a, const slu_conv_h8_desc* d, const SluEmit& e) {
  if (h8_m128_weight_bytes(a.nks, KS * KS) <= WRES_MAX_BYTES) return launch_h8_k<KS, DIL, PAD, 2, 2, 4, 2, SCALED, true>(a, d, e);
  if constexpr (!SCALED) {
    if (h8_one_plain_source(a)) {
      if constexpr (KS == 2) {
        if (g_h8_kpc2 && a.nks >= 2) {
#ifdef SLU_H8_AB
          if (g_h8_opt == 0) return launch_h8_k<KS, DIL, PAD, 2, 2, 4, 2, false, false, false, 2, 0, true>(a, d, e);
#endif
          return launch_h8_k<KS, DIL, PAD, 2, 2, 4, 2, false, false, false, 2, H8_M128_OPT_2X2, true>(a, d, e);
        }
      }
#ifdef SLU_H8_AB
      switch (g_h8_opt) {
        case 0: return launch_h8_k<KS, DIL, PAD, 2, 2, 4, 2, false, false, false, 1, 0, true>(a, d, e);
        case 8: return launch_h8_k<KS, DIL, PAD, 2, 2, 4, 2, false, false, false, 1, 8, true>(a, d, e);
        case 15: return launch_h8_k<KS, DIL, PAD, 2, 2, 4, 2, false, false, false, 1, 15, true>(a, d, e);
        case 100: return launch_h8_k<KS, DIL, PAD, 2, 2, 4, 2, false, false, false, 1, 0, false>(a, d, e);      // the general form, for comparison
      }
#endif
      return launch_h8_k<KS, DIL, PAD, 2, 2, 4, 2, false, false, false, 1, KS == 2 ? H8_M128_OPT_2X2 : H8_M128_OPT_3X3, true>(a, d, e);
    }
  }
  return launch_h8_k<KS, DIL, PAD, 2, 2, 4, 2, SCALED, false>(a, d, e);
}

template <int KS, int DIL, int PAD, bool SCALED>
int launch_h8_tiles(H8Args& a, const slu_conv_h8_desc* d, int cfg, const SluEmit& e) {
  switch (cfg) {
    case CFG_M32_TH16: return launch_h8<KS, DIL, PAD, 1, 1, 8, 2, SCALED>(a, d, e);
    case CFG_M64_TH16: return launch_h8<KS, DIL, PAD, 2, 1, 8, 2, SCALED>(a, d, e);
    case CFG_M128_TH8: return launch_h8_m128<KS, DIL, PAD, SCALED>(a, d, e);
    case CFG_M32_TH8:  return launch_h8<KS, DIL, PAD, 1, 1, 4, 2, SCALED>(a, d, e);
    case CFG_M64_TH8:  return launch_h8<KS, DIL, PAD, 2, 1, 4, 2, SCALED>(a, d, e);
    case CFG_M128_TH4: return launch_h8<KS, DIL, PAD, 2, 2, 2, 2, SCALED>(a, d, e);
    case CFG_M32_TH4:  return launch_h8<KS, DIL, PAD, 1, 1, 4, 1, SCALED>(a, d, e);
    case CFG_M64_TH4:  return launch_h8<KS, DIL, PAD, 2, 1, 4, 1, SCALED>(a, d, e);
  }
  return SLU_EUNSUPPORTED;
}

// out = leaky(conv3x3 + bias + resid) (slu_conv_h8_desc.act_after_resid): conv_h8_late_kernel in the tile configuration choose_h8 picks, weights
// streamed per chunk (a BasicBlock's 64 .. 512-channel weights never fit the resident form); the 128-channel configuration with the
// scheduling options of its plain 3x3 form where the layer has one plain source
template <int MB, int WM, int WN, int RPW, int OPT = 0, bool ONE = false>
int launch_h8_late_k(H8Args& a, const slu_conv_h8_desc* d, const SluEmit& e) {
  return launch_h8_k<3, 1, 1, MB, WM, WN, RPW, false, false, false, 1, OPT, ONE, true>(a, d, e);
}
int launch_h8_late(H8Args& a, const slu_conv_h8_desc* d, int cfg, const SluEmit& e) {
  switch (cfg) {
    case CFG_M32_TH16: return launch_h8_late_k<1, 1, 8, 2>(a, d, e);
    case CFG_M64_TH16: return launch_h8_late_k<2, 1, 8, 2>(a, d, e);
    case CFG_M128_TH8:
      return h8_one_plain_source(a) ? launch_h8_late_k<2, 2, 4, 2, H8_M128_OPT_3X3, true>(a, d, e) : launch_h8_late_k<2, 2, 4, 2>(a, d, e);
    case CFG_M32_TH8:  return launch_h8_late_k<1, 1, 4, 2>(a, d, e);
    case CFG_M64_TH8:  return launch_h8_late_k<2, 1, 4, 2>(a, d, e);
    case CFG_M128_TH4: return launch_h8_late_k<2, 2, 2, 2>(a, d, e);
    case CFG_M32_TH4:  return launch_h8_late_k<1, 1, 4, 1>(a, d, e);
    case CFG_M64_TH4:  return launch_h8_late_k<2, 1, 4, 1>(a, d, e);
  }
  return SLU_EUNSUPPORTED;
}

template <int KS, int DIL, int PAD>
int launch_h8_family(H8Args& a, const slu_conv_h8_desc* d, int cfg, bool scaled, const SluEmit& e) {
  return scaled ? launch_h8_tiles<KS, DIL, PAD, true>(a, d, cfg, e) : launch_h8_tiles<KS, DIL, PAD, false>(a, d, cfg, e);
}

template <int MB, int NBW>
int launch_h8_1x1(H8Args& a, const slu_conv_h8_desc* d, const SluEmit& e) {
  constexpr size_t lds = (size_t)MB * 4 * 64 * 16 + (size_t)3 * MB * 32 * 4;
  const long long nblocks = (long long)a.N * a.H * a.W / 32;
  const long long gx = (nblocks + 4 * NBW - 1) / (4 * NBW);
  if (gx <= 0 || gx > 0x7fffffffLL) return SLU_EUNSUPPORTED;
  if (e.name) return slu_emit_name(e, "conv1x1_h8_kernel<%d, %d>", MB, NBW);
  hipLaunchKernelGGL((conv1x1_h8_kernel<MB, NBW>), dim3((unsigned)gx), dim3(256), lds, e.st, a, d->resid, d->out);
  SLU_CHECK_LAUNCH();
}

template <int MB, int NKS>
int launch_h8_1x1_res(H8Args& a, const slu_conv_h8_desc* d, const SluEmit& e) {
  constexpr size_t lds = (size_t)MB * NKS * 64 * 16 + (size_t)3 * MB * 32 * 4;
  const long long nblocks = (long long)a.N * a.H * a.W / 32;
  long long gx = 256 * h8_1x1_res_waves_per_simd(MB, NKS);      // as many 4-wave workgroups per CU as the registers allow
  if (gx * 4 > nblocks) gx = (nblocks + 3) / 4;
  if (gx <= 0) return SLU_EUNSUPPORTED;
  if (e.name) return slu_emit_name(e, "conv1x1_h8_res_kernel<%d, %d>", MB, NKS);
  hipLaunchKernelGGL((conv1x1_h8_res_kernel<MB, NKS>), dim3((unsigned)gx), dim3(256), lds, e.st, a, d->resid, d->out);
  SLU_CHECK_LAUNCH();
}

// resident-weight streaming form: <= 64 output channels and 1 / 2 / 6 / 12 K-steps (the 1x1 convs of the full- and
// half-resolution blocks); returns -1 when the shape is not covered
template <int MB>
int launch_h8_1x1_res_nks(H8Args& a, const slu_conv_h8_desc* d, const SluEmit& e) {
  switch (a.nks) {
    case 1:  return launch_h8_1x1_res<MB, 1>(a, d, e);
    case 2:  return launch_h8_1x1_res<MB, 2>(a, d, e);
    case 5: case 6:   return launch_h8_1x1_res<MB, 6>(a, d, e);
    case 10: case 12: return launch_h8_1x1_res<MB, 12>(a, d, e);
  }
  return -1;
}

// the layers gemm1x1_h8_kernel covers; SLU_H8_GEMM1X1=0 is the A/B switch back to the streaming kernels
constexpr int GEMM1X1_KC = 4, GEMM1X1_D256 = 2, GEMM1X1_D128 = 3;      // chunk = 64 channels; ring: 2 x 64 KB (256 outputs), 3 x 48 KB (128)
bool gemm1x1_ok(const slu_conv_h8_desc* d, const H8Args& a) {
  static const bool off = [] { const char* e = getenv("SLU_H8_GEMM1X1"); return e && e[0] == '0'; }();
  // 256 output channels: measured (tools/h8_1x1_bench.py, N = 64, profiles/r10) 502 -> 372 us against the streaming kernel on 768->256 at 16x512.
  // 128 outputs: only the 384 -> 128 concat convs that carry a residual (three sources, 24 K-steps): 543 -> 478 us at 32x1024 and 149 -> 137 at
  // 16x512 since the residual is loaded ahead (with the epilogue before that the GEMM was the slower one, 618 us); the other 128-output
  // layers stay on the streaming kernel, and SLU_H8_GEMM1X1=2 sends every 128-output layer within reach here (tests, A/B runs)
  static const bool all = [] { const char* e = getenv("SLU_H8_GEMM1X1"); return e && e[0] == '2'; }();
  const bool concat128 = a.Cout == 128 && d->resid && a.nsrc == 3 && a.nks == 24;
  if (off || d->ksize != 1 || d->pad != 0 || a.out_f32 || (a.Cout != 256 && !(a.Cout == 128 && (all || concat128)))) return false;
  if (((long long)a.H * a.W) % 256 || a.nks % GEMM1X1_KC || a.Gin != 2 * a.nks) return false;
  if ((a.has_act & ~1) || ((a.has_act & 1) && !(a.slope >= 0.0f && a.slope <= 1.0f))) return false;
  for (int s = 0; s < a.nsrc; ++s)
    if (a.src[s].scale || a.src[s].nb || a.src[s].G % (2 * GEMM1X1_KC)) return false;
  if (16LL * a.Gout * a.H * a.W > 0xffffffffLL) return false;      // a lane's byte offset inside one image of the output / residual is 32-bit
  return (long long)a.N * a.H * a.W / 256 <= 0x7fffffffLL;
}

template <int MB, int D>
int launch_gemm1x1(H8Args& a, const slu_conv_h8_desc* d, const SluEmit& e) {
  constexpr int KC = GEMM1X1_KC, MBLK = 2 * MB;
  constexpr size_t lds = (size_t)3 * MBLK * 32 * 4 + (size_t)D * (2 * KC * 256) * 16 + (size_t)D * (MBLK * KC * 64) * 16;
  static_assert(lds <= 160 * 1024, "gemm1x1 LDS");
  const long long nt = (long long)a.N * a.H * a.W / 256;
  const long long gx = nt < 256 ? nt : 256;
  // A/B switch: SLU_GEMM1X1_RES_AHEAD=0 is the epilogue that loads the residual where it is used (gemm1x1_h8_kernel_v1)
  static const bool v1 = [] { const char* v = getenv("SLU_GEMM1X1_RES_AHEAD"); return v && v[0] == '0'; }();
  if (e.name) return slu_emit_name(e, v1 ? "gemm1x1_h8_kernel_v1<%d, %d, %d>" : "gemm1x1_h8_kernel<%d, %d, %d>", MB, KC, D);
  static SluLdsGrant grant, grant_v1;
  if (v1) return slu_launch_lds(gemm1x1_h8_kernel_v1<MB, KC, D>, dim3((unsigned)gx), dim3(512), lds, e.st, grant_v1, a, d->resid, d->out);
  return slu_launch_lds(gemm1x1_h8_kernel<MB, KC, D>, dim3((unsigned)gx), dim3(512), lds, e.st, grant, a, d->resid, d->out);
}

bool any_scale(const slu_conv_h8_desc* d) {
  for (int s = 0; s < d->nsrc; ++s)
    if (d->src[s].scale) return true;
  return false;
}

bool stream_ok(const slu_conv_h8_desc* d, const H8Args& a) {
  return d->ksize == 1 && d->pad == 0 && a.nmblk <= 8 && ((long long)a.H * a.W) % 32 == 0 && !any_scale(d);
}

// the one traversal of the h8 forward dispatch: slu_conv2d_h8_fwd launches at its leaf, slu_conv2d_h8_kernel_name has the leaf name itself
int conv_h8_dispatch(const slu_conv_h8_desc* d, const SluEmit& e) {
  H8Args a{};
  const int rc = fill_h8(d, a);
  if (rc != SLU_OK) return rc;
  if (d->act_after_resid) {      // one family implements the late activation; every other path refuses the flag, none ignores it
    if (d->ksize != 3 || d->dil != 1 || d->pad != 1 || !d->resid || !d->has_act || d->bn_a || a.out_f32 || a.src[0].shuf || any_scale(d))
      return SLU_EUNSUPPORTED;
    return launch_h8_late(a, d, choose_h8(a), e);
  }
  if (a.src[0].shuf) {      // read in place by ring3_h8_kernel<1, 1, 5, 1, 4> or by the SCALED 3x3 tiled kernels; anything else: slu_pixel_shuffle_h8
    if (ring3_ok(d, a)) {
      const int rc2 = launch_ring3_any(a, d, e);
      if (rc2 != -1) return rc2;
    }
    if (!any_scale(d) || d->ksize != 3 || d->dil != 1 || d->pad != 1 || a.out_f32) return SLU_EUNSUPPORTED;
    return launch_h8_family<3, 1, 1>(a, d, choose_h8(a), true, e);
  }
  if (gemm1x1_ok(d, a)) return a.Cout == 128 ? launch_gemm1x1<2, GEMM1X1_D128>(a, d, e) : launch_gemm1x1<4, GEMM1X1_D256>(a, d, e);
  if (stream_ok(d, a)) {
    if (a.nmblk <= 2) {
      const int rc2 = a.nmblk == 1 ? launch_h8_1x1_res_nks<1>(a, d, e) : launch_h8_1x1_res_nks<2>(a, d, e);
      if (rc2 != -1) return rc2;
    }
    if (a.nmblk == 1) return launch_h8_1x1<1, 2>(a, d, e);
    if (a.nmblk == 2) return launch_h8_1x1<2, 2>(a, d, e);
    if (a.nmblk <= 4) return launch_h8_1x1<4, 1>(a, d, e);
    return launch_h8_1x1<8, 1>(a, d, e);
  }
  if (ring3_ok(d, a)) {
    const int rc2 = launch_ring3_any(a, d, e);
    if (rc2 != -1) return rc2;
  }
  const bool sc = any_scale(d);
  if (a.out_f32) {      // fp32 NCHW output outside the streaming kernel's reach (odd H*W): 1x1 head only
    if (d->ksize != 1 || d->dil != 1 || d->pad != 0 || sc) return SLU_EUNSUPPORTED;
    return launch_h8_k<1, 1, 0, 1, 1, 4, 1, false, false, true>(a, d, e);
  }
  const int cfg = choose_h8(a);
  if (d->ksize == 1 && d->dil == 1 && d->pad == 0) return launch_h8_family<1, 1, 0>(a, d, cfg, sc, e);
  if (d->ksize == 3 && d->dil == 1 && d->pad == 1) return launch_h8_family<3, 1, 1>(a, d, cfg, sc, e);
  if (d->ksize == 3 && d->dil == 2 && d->pad == 2) return launch_h8_family<3, 2, 2>(a, d, cfg, sc, e);
  if (d->ksize == 2 && d->dil == 2 && d->pad == 1) return launch_h8_family<2, 2, 1>(a, d, cfg, sc, e);
  // taps at offsets -1 and 0: a 3x3 / stride 2 / pad 1 conv over the space-to-depth image of its input (slu_space_to_depth2_h8); no multipliers
  if (d->ksize == 2 && d->dil == 1 && d->pad == 1) return sc ? SLU_EUNSUPPORTED : launch_h8_tiles<2, 1, 1, false>(a, d, cfg, e);
  return SLU_EUNSUPPORTED;
}

}  // namespace

extern "C" size_t slu_packed_weight_bytes_h8(int cout, int cin, int ksize) {
  if (cout <= 0 || cin <= 0 || ksize <= 0) return 0;
  const size_t nmblk = (cout + 31) / 32, nks = (cin + 15) / 16;
  return nmblk * nks * (size_t)(ksize * ksize) * 64 * 16;
}

extern "C" int slu_pack_conv_weight_h8(const float* w, int cout, int cin, int ksize, void* out, slu_stream_t stream) {
  if (!w || !out) return SLU_EINVAL;
  const size_t bytes = slu_packed_weight_bytes_h8(cout, cin, ksize);
  if (bytes == 0) return SLU_EINVAL;
  const size_t total = bytes / 16;      // > 0: whole 1 KB fragments
  hipLaunchKernelGGL(pack_h8_kernel, dim3(slu_grid_1d(total, 32768)), dim3(256), 0, slu_stream(stream), w, cout, cin, ksize, (cin + 15) / 16, total,
                     reinterpret_cast<uint4*>(out));
  SLU_CHECK_LAUNCH();
}

extern "C" int slu_conv2d_h8_fwd(const slu_conv_h8_desc* d, slu_stream_t stream) { return conv_h8_dispatch(d, SluEmit{slu_stream(stream), nullptr, 0}); }

// name of the kernel instantiation slu_conv2d_h8_fwd launches for `d` (as rocprofv3 prints it), or the status with which it refuses `d`
extern "C" int slu_conv2d_h8_kernel_name(const slu_conv_h8_desc* d, char* buf, size_t n) {
  return buf ? conv_h8_dispatch(d, SluEmit{nullptr, buf, n}) : SLU_EINVAL;
}

#ifdef SLU_H8_AB
extern "C" void slu_h8_dev_set_opt(int opt, int kpc2) { g_h8_opt = opt; g_h8_kpc2 = kpc2; }
#endif

#ifdef SLU_H8_PROF
extern "C" int slu_h8_prof_read(unsigned long long* out8) {
  if (hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_h8_prof), sizeof(unsigned long long) * 8) != hipSuccess) return SLU_ELAUNCH;
  unsigned long long z[8] = {};
  return hipMemcpyToSymbol(HIP_SYMBOL(g_h8_prof), z, sizeof(z)) == hipSuccess ? SLU_OK : SLU_ELAUNCH;
}
#endif
