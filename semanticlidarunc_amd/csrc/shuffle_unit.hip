// The tail of a ShuffleNetV2 unit (torchvision's InvertedResidual) in ONE launch:
//
//   y = relu(W_pw . (dw3x3_stride_s(src) + b_dw) + b_pw)          out[:, 2 j + parity] = y[j]          [out[:, 2 j] = pass[:, j]]
//
// i.e. branch2[3:] (or branch1) with both eval BatchNorms folded in, plus the unit's concat and channel_shuffle(., 2) as the store address, plus
// (stride-1 units) the copy of the pass-through half.  The depthwise result never leaves the chip: a workgroup computes it for 64 output pixels
// and one 32-channel K-chunk at a time into LDS, and the pointwise product consumes it from there.
//
//   shuffle_tail_kernel<STRIDE, UPW>   256 threads = 4 waves, 64 consecutive output pixels of one image (counted over Ho Wo, so small maps do not
//                                      waste lanes), every output channel.  Per K-chunk: each wave computes 8 channels x 64 pixels of the depthwise
//                                      conv (lane = pixel, the channel is wave-uniform so its nine taps and bias are scalar loads), then
//                                      wave w owns pixel half w & 1 and the 32-channel output blocks (w >> 1) + 2 i, i < UPW, and runs
//                                      v_mfma_f32_32x32x2_f32 (exact fp32: a k-ordered fmaf chain) with A from the packed weight image (L2) and B
//                                      from LDS.  A chunk's A operands are loaded in one batch ahead of its barriers and the next chunk's depthwise
//                                      loads are issued before the current chunk's MFMAs, so a chunk pays about one memory round trip.  On small
//                                      maps the output blocks are split over workgroups (blockIdx.z, slu_cu_fill_split) to fill the CUs.
//   shuffle_tail_pack_kernel           [Co][C] fp32 -> the A-fragment image (encoder_unit.h) with K-chunk TAIL_KC.
// The weight is streamed from L2 in K-chunks (the 488 x 488 one is 952 KB).  No atomics: results are bit-identical run to run.
#include "encoder_unit.h"

namespace {

constexpr int TAIL_KC = 32;       // input channels per K-chunk
constexpr int TAIL_PIX = 64;      // output pixels per workgroup
constexpr int TAIL_LDW = 96;      // LDS row stride in floats: rows k and k + 1 (the two lane halves of one B operand) land in different bank halves
constexpr int TAIL_MAX_CO = 512;  // 16 output blocks: UPW <= 8

struct TailArgs {
  const float* src0;      // the fields of Cat2Args (slu_cat2_fill), flat: as a member struct the kernels' argument loads change
  const float* src1;
  long long bs0, bs1;
  int c0, C;
  int H, W, Ho, Wo;
  int Co, parity, nmblk, nchunks;
  int mps;                // 32-channel output blocks per workgroup: blockIdx.z owns blocks [z mps, (z + 1) mps)
  const float *wdw, *bdw, *wpack, *bpw;
  const float* pass;
  long long bsp;
  float* out;
};

// the depthwise conv of this lane's pixel for the 8 channels wave w owns in chunk q
__device__ __forceinline__ void tail_depthwise(const TailArgs& a, int n, int q, int w, const int (&off)[9], const bool (&tv)[9], float (&dv)[8]) {
  const size_t HW = (size_t)a.H * a.W;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int c = q * TAIL_KC + w + 4 * i;      // wave-uniform
    float v = 0.0f;
    if (c < a.C) {
      const float* sp = CAT2_PLANE(c, a.c0, a.src0 + (size_t)n * a.bs0, a.src1 + (size_t)n * a.bs1, HW);
      const float* wc = a.wdw + (size_t)c * 9;
      v = a.bdw[c];
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const float x = sp[off[t]];             // off = 0 (always mapped) where the tap is outside the image
        v = fmaf(wc[t], tv[t] ? x : 0.0f, v);
      }
    }
    dv[i] = v;
  }
}

template <int STRIDE, int UPW>
__global__ __launch_bounds__(256) void shuffle_tail_kernel(const TailArgs a) {
  __shared__ float s_d[TAIL_KC * TAIL_LDW];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = blockIdx.y;
  const int HWo = a.Ho * a.Wo;
  const int pl = blockIdx.x * TAIL_PIX + lane;
  const bool pok = pl < HWo;
  const int oy = pok ? pl / a.Wo : 0, ox = pok ? pl - oy * a.Wo : 0;
  int off[9];
  bool tv[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int iy = oy * STRIDE + i - 1, ix = ox * STRIDE + j - 1;
      const bool ok = pok && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
      tv[i * 3 + j] = ok;
      off[i * 3 + j] = ok ? iy * a.W + ix : 0;
    }
  float* __restrict__ po = a.out + (size_t)n * 2 * a.Co * HWo;

  float dv[8];
  tail_depthwise(a, n, 0, w, off, tv, dv);

  // the pass-through half: out[:, 2 j] = pass[:, j] -- eight planes in flight per lane (a load -> store chain per plane would pay one memory
  // round trip per channel)
  if (a.pass && pok && blockIdx.z == 0) {
    const float* __restrict__ ps = a.pass + (size_t)n * a.bsp;
    for (int j0 = w; j0 < a.Co; j0 += 32) {
      float t[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int j = j0 + 4 * u;
        t[u] = ps[(size_t)(j < a.Co ? j : j0) * HWo + pl];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int j = j0 + 4 * u;
        if (j < a.Co) po[(size_t)(2 * j) * HWo + pl] = t[u];
      }
    }
  }

  f32x16 acc[UPW];
  SLU_ZERO_ACC(acc, UPW);
  const int nb = w & 1;
  const int mlo = blockIdx.z * a.mps, mhi = min(a.nmblk, mlo + a.mps), mb0 = mlo + (w >> 1);
  const int hh = lane >> 5, jj = lane & 31;
  const size_t kp2 = (size_t)a.nchunks * (TAIL_KC / 2);      // K-steps of one output block in the packed image
  // this wave's output blocks; one past the last block is clamped (its products are computed and never stored), so nothing below branches
  const float* wrow[UPW];
#pragma unroll
  for (int i = 0; i < UPW; ++i) {
    const int mblk = mb0 + 2 * i;
    wrow[i] = a.wpack + (size_t)(mblk < mhi ? mblk : mhi - 1) * kp2 * 64 + lane;
  }

  for (int q = 0; q < a.nchunks; ++q) {
    // the A operands of the whole chunk in one batch of loads, ahead of the barriers: one L2 round trip per chunk instead of one per K-step
    float av[UPW][TAIL_KC / 2];
#pragma unroll
    for (int i = 0; i < UPW; ++i)
#pragma unroll
      for (int kk = 0; kk < TAIL_KC / 2; ++kk) av[i][kk] = wrow[i][((size_t)q * (TAIL_KC / 2) + kk) * 64];
    __syncthreads();                                          // the previous chunk's B reads are done
#pragma unroll
    for (int i = 0; i < 8; ++i) s_d[(w + 4 * i) * TAIL_LDW + lane] = dv[i];
    __syncthreads();
    if (q + 1 < a.nchunks) tail_depthwise(a, n, q + 1, w, off, tv, dv);
#pragma unroll
    for (int kk = 0; kk < TAIL_KC / 2; ++kk) {
      const float b = s_d[(2 * kk + hh) * TAIL_LDW + nb * 32 + jj];
#pragma unroll
      for (int i = 0; i < UPW; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i][kk], b, acc[i], 0, 0, 0);
    }
  }

  // bias, ReLU, store at the shuffled channel
  const int px = blockIdx.x * TAIL_PIX + nb * 32 + jj;
  const bool sok = px < HWo;
  slu_static_for<UPW>([&](auto ic) __attribute__((always_inline)) {
    constexpr int i = decltype(ic)::value;
    const int mblk = mb0 + 2 * i;
    if (mblk < mhi) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = slu_frag_row(mblk * 32, r, hh);
        if (sok && co < a.Co) {
          const float v = acc[i][r] + a.bpw[co];
          po[(size_t)(2 * co + a.parity) * HWo + px] = v > 0.0f ? v : 0.0f;
        }
      }
    }
  });
}

__global__ __launch_bounds__(256) void shuffle_tail_pack_kernel(const float* __restrict__ w, int co, int c, size_t total, float* __restrict__ out) {
  PIX_GRID_STRIDE(e, total) out[e] = afrag_element(w, e, co, c, TAIL_KC, 1);
}

template <int STRIDE>
int launch_tail(TailArgs& a, int N, hipStream_t st) {
  const int split = slu_cu_fill_split((long long)((a.Ho * a.Wo + TAIL_PIX - 1) / TAIL_PIX) * N, a.nmblk);      // each z recomputes the depthwise chunk
  a.mps = (a.nmblk + split - 1) / split;
  const dim3 grid((unsigned)((a.Ho * a.Wo + TAIL_PIX - 1) / TAIL_PIX), (unsigned)N, (unsigned)((a.nmblk + a.mps - 1) / a.mps)), block(256);
  const int units = (a.mps + 1) / 2;
  if (units <= 1) hipLaunchKernelGGL((shuffle_tail_kernel<STRIDE, 1>), grid, block, 0, st, a);
  else if (units <= 2) hipLaunchKernelGGL((shuffle_tail_kernel<STRIDE, 2>), grid, block, 0, st, a);
  else if (units <= 4) hipLaunchKernelGGL((shuffle_tail_kernel<STRIDE, 4>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((shuffle_tail_kernel<STRIDE, 8>), grid, block, 0, st, a);
  SLU_CHECK_LAUNCH();
}

}  // namespace

extern "C" size_t slu_shuffle_tail_packed_floats(int co, int c) {
  if (co <= 0 || c <= 0 || co > TAIL_MAX_CO) return 0;
  return afrag_floats(co, c, TAIL_KC, 1);
}

extern "C" int slu_shuffle_tail_pack(const float* w, int co, int c, float* out, slu_stream_t stream) {
  if (!w || !out || co <= 0 || c <= 0) return SLU_EINVAL;
  const size_t total = slu_shuffle_tail_packed_floats(co, c);
  if (total == 0) return SLU_EUNSUPPORTED;
  hipLaunchKernelGGL(shuffle_tail_pack_kernel, dim3(slu_grid_1d(total, 4096)), dim3(256), 0, slu_stream(stream), w, co, c, total, out);
  SLU_CHECK_LAUNCH();
}

extern "C" int slu_shuffle_tail_fwd(const slu_shuffle_tail_desc* d, slu_stream_t stream) {
  if (!d || !d->wdw || !d->bdw || !d->wpack || !d->bpw || !d->out || d->Co <= 0 || slu_cat2_check(d->in, d->N, d->H, d->W)) return SLU_EINVAL;
  if ((d->parity != 0 && d->parity != 1) || (d->pass && (d->pass_ct < d->Co || d->parity != 1))) return SLU_EINVAL;
  if (d->stride != 1 && d->stride != 2) return SLU_EUNSUPPORTED;
  if (d->Co > TAIL_MAX_CO || slu_unit_grid_check(d->N, d->H, d->W)) return SLU_EUNSUPPORTED;
  TailArgs a;
  const size_t HW = (size_t)d->H * d->W;
  a.Ho = slu_strided_out(d->H, d->stride);
  a.Wo = slu_strided_out(d->W, d->stride);
  const size_t HWo = (size_t)a.Ho * a.Wo, nout = (size_t)d->N * 2 * d->Co * HWo;
  if (slu_cat2_overlaps(d->in, d->N, HW, d->out, nout) || (d->pass && slu_overlaps(d->out, nout, d->pass, (size_t)d->N * d->pass_ct * HWo)))
    return SLU_EINVAL;
  slu_cat2_fill(a, d->in, HW);
  a.H = d->H; a.W = d->W;
  a.Co = d->Co; a.parity = d->parity;
  a.nmblk = (d->Co + 31) / 32;
  a.nchunks = (a.C + TAIL_KC - 1) / TAIL_KC;
  a.wdw = d->wdw; a.bdw = d->bdw; a.wpack = d->wpack; a.bpw = d->bpw;
  a.pass = d->pass;
  a.bsp = (long long)d->pass_ct * a.Ho * a.Wo;
  a.out = d->out;
  return d->stride == 1 ? launch_tail<1>(a, d->N, slu_stream(stream)) : launch_tail<2>(a, d->N, slu_stream(stream));
}
