// h8 convs, the streaming 1x1 family (conv1x1_h8_kernel, conv1x1_h8_res_kernel): the 1x1 convs up to 256 output channels that the GEMM
// (gemm1x1_h8.hip) does not take, and the fp32 logits head.  The map of the families is in conv2d_h8.hip.
// Not a translation unit of its own: conv_h8_tiled.hip includes this file at its end.  Both families inline store_tile<32> (the fp32 output
// form), and compiled apart conv1x1_h8_kernel<1, 2> and conv_h8_kernel<1, 1, 0, 1, 1, 4, 1, false, false, true> come out in another schedule
// (tools/h8_isa_diff.py, profiles/r17); compiled together, in either order, every kernel keeps its instructions.
#pragma once
#include "conv_h8.h"

namespace {

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

bool stream_ok(const slu_conv_h8_desc* d, const H8Args& a) {
  return d->ksize == 1 && d->pad == 0 && a.nmblk <= 8 && ((long long)a.H * a.W) % 32 == 0 && !any_scale(d);
}

}  // namespace

int slu_h8::h8_conv1x1(H8Args& a, const slu_conv_h8_desc* d, const SluEmit& e) {
  if (!stream_ok(d, a)) return -1;
  if (a.nmblk <= 2) {
    const int rc2 = a.nmblk == 1 ? launch_h8_1x1_res_nks<1>(a, d, e) : launch_h8_1x1_res_nks<2>(a, d, e);
    if (rc2 != -1) return rc2;
  }
  if (a.nmblk == 1) return launch_h8_1x1<1, 2>(a, d, e);
  if (a.nmblk == 2) return launch_h8_1x1<2, 2>(a, d, e);
  if (a.nmblk <= 4) return launch_h8_1x1<4, 1>(a, d, e);
  return launch_h8_1x1<8, 1>(a, d, e);
}
