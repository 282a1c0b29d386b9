// The pieces of a RegNetY block (torchvision's ResBottleneckBlock with SqueezeExcitation) that the fused conv kernel does not cover:
//
//   regnet_gconv_kernel<GW, S, TH, TW>   f.b: grouped 3x3 conv (pad 1, stride S = 1 / 2, GW = 8 / 16 / 24 channels per group) + folded BatchNorm +
//                                        ReLU, and the per-workgroup partial sums of the SqueezeExcitation's spatial mean of what it stores:
//       y[n, g GW + o, oy, ox] = relu(b[g GW + o] + sum_{c < GW, a, b} w[g GW + o, c, a, b] x[n, g GW + c, S oy - 1 + a, S ox - 1 + b])
//       psum[n, g GW + o, tile] = sum over the tile's pixels inside the image of y
//     A workgroup of 256 owns one (image, group, TH x TW output tile), one lane per output pixel with GW accumulators.  The group's input comes
//     through LDS in chunks of 8 channels -- the tile's receptive field ((TH - 1) S + 3) x ((TW - 1) S + 3), zero outside the image, so stride 2
//     reads exactly the rows and columns it needs -- and every lane reads its nine taps of a channel from there (consecutive lanes, consecutive
//     (S = 1) or every second (S = 2) float).  The weights are the same for every lane of the workgroup: the host stores them as
//     [group][c][tap][o], 9 GW consecutive floats per input channel, and the compiler fetches them through the scalar cache and feeds them to
//     v_pk_fma_f32 (two output channels each) as scalar operands.  So a lane does 9 LDS reads per 9 GW FMAs.  Exact fp32 (an fmaf chain per
//     output, in (c, tap) order).
//     The mean: wave_sum per output channel, one LDS slot per wave, the four slots added in wave order, one float per (image, channel, tile) --
//     no atomics, so two runs give the same bits; the gate (slu_regnet_se_gate, se_gate.hip) adds the tiles in tile order.
//   regnet_sample2_kernel                y = in[:, :, ::2, ::2] of a slu_cat2: the input of a stride-2 block's 1x1 / stride-2 projection, with the
//                                        meta injection, in one pass that reads a quarter of the input.
#include "encoder_unit.h"

namespace {

constexpr int RG_CK = 8;      // input channels per LDS chunk: divides every group width

template <int GW, int S, int TH, int TW>
__global__ __launch_bounds__(256) void regnet_gconv_kernel(const float* __restrict__ x, const float* __restrict__ wg, const float* __restrict__ bias,
                                                           float* __restrict__ y, float* __restrict__ psum, long long bsx, int C, int H, int W, int OH,
                                                           int OW, int tx, int T) {
  static_assert(TH * TW == 256 && GW % RG_CK == 0, "one lane per output pixel; whole chunks");
  constexpr int IH = (TH - 1) * S + 3, IW = (TW - 1) * S + 3;
  __shared__ float s_in[RG_CK * IH * IW];
  __shared__ float s_red[4][GW];
  const int tid = threadIdx.x;
  const int g = blockIdx.y, n = blockIdx.z;
  const int tyi = blockIdx.x / tx;
  const int oy0 = tyi * TH, ox0 = (blockIdx.x - tyi * tx) * TW;
  const int ly = tid / TW, lx = tid - ly * TW;
  const int oy = oy0 + ly, ox = ox0 + lx;
  const size_t HW = (size_t)H * W;
  const float* __restrict__ xg = x + (size_t)n * bsx + (size_t)g * GW * HW;
  const float* __restrict__ wgrp = wg + (size_t)g * GW * 9 * GW;
  const int iy0 = oy0 * S - 1, ix0 = ox0 * S - 1;

  float acc[GW];
#pragma unroll
  for (int o = 0; o < GW; ++o) acc[o] = bias[g * GW + o];

  for (int ch = 0; ch < GW / RG_CK; ++ch) {
    if (ch) __syncthreads();      // the previous chunk has been read
    for (int e = tid; e < RG_CK * IH * IW; e += 256) {
      const int c = e / (IH * IW), r = e - c * (IH * IW);
      const int ry = r / IW, rx = r - ry * IW;
      const int iy = iy0 + ry, ix = ix0 + rx;
      float v = 0.0f;
      if (iy >= 0 && iy < H && ix >= 0 && ix < W) v = xg[(size_t)(ch * RG_CK + c) * HW + (size_t)iy * W + ix];
      s_in[e] = v;
    }
    __syncthreads();
#pragma unroll 2
    for (int c = 0; c < RG_CK; ++c) {
      const float* __restrict__ sp = s_in + c * (IH * IW) + (ly * S) * IW + lx * S;
      const float* __restrict__ wc = wgrp + (size_t)(ch * RG_CK + c) * 9 * GW;
      float v[9];
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) v[a * 3 + b] = sp[a * IW + b];
#pragma unroll
      for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int o = 0; o < GW; ++o) acc[o] = fmaf(wc[t * GW + o], v[t], acc[o]);
    }
  }

  const bool inside = oy < OH && ox < OW;
  const size_t OHW = (size_t)OH * OW;
  float* __restrict__ yo = y + ((size_t)n * C + (size_t)g * GW) * OHW + (size_t)oy * OW + ox;
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int o = 0; o < GW; ++o) {
    const float r = acc[o] > 0.0f ? acc[o] : 0.0f;
    if (inside) yo[(size_t)o * OHW] = r;
    const float s = wave_sum(inside ? r : 0.0f);
    if (lane == 0) s_red[wave][o] = s;
  }
  __syncthreads();
  if (tid < GW) psum[((size_t)n * C + (size_t)g * GW + tid) * T + blockIdx.x] = (s_red[0][tid] + s_red[1][tid]) + (s_red[2][tid] + s_red[3][tid]);
}

__global__ __launch_bounds__(256) void regnet_sample2_kernel(const float* __restrict__ s0, const float* __restrict__ s1, long long bs0, long long bs1,
                                                             int c0, int C, int N, int H, int W, int OH, int OW, float* __restrict__ y) {
  const size_t total = (size_t)N * C * OH * OW;
  PIX_GRID_STRIDE(e, total) {
    const PixXYCN o = pix_xycn(e, OW, OH, C);
    const float* p = CAT2_PLANE(o.c, c0, s0 + o.n * (size_t)bs0, s1 + o.n * (size_t)bs1, H * W);
    y[e] = p[(size_t)(2 * o.y) * W + 2 * o.x];
  }
}

// the output tile: 4 x 64 for maps of at most four output rows (the deep stages of a 64-row scan), 8 x 32 otherwise
bool rg_wide(int OH) { return OH <= 4; }
int rg_tiles(int OH, int OW, int& tx) {
  const int th = rg_wide(OH) ? 4 : 8, tw = rg_wide(OH) ? 64 : 32;
  tx = (OW + tw - 1) / tw;
  const long long t = (long long)tx * ((OH + th - 1) / th);
  return t > 0x7fffffffLL / 4 ? 0 : (int)t;
}

template <int GW, int S>
int launch_gconv(const float* x, const float* wg, const float* bias, float* y, float* psum, long long bsx, int N, int C, int H, int W, int OH, int OW,
                 hipStream_t st) {
  int tx;
  const int T = rg_tiles(OH, OW, tx);
  const dim3 grid((unsigned)T, (unsigned)(C / GW), (unsigned)N);
  if (rg_wide(OH))
    hipLaunchKernelGGL((regnet_gconv_kernel<GW, S, 4, 64>), grid, dim3(256), 0, st, x, wg, bias, y, psum, bsx, C, H, W, OH, OW, tx, T);
  else
    hipLaunchKernelGGL((regnet_gconv_kernel<GW, S, 8, 32>), grid, dim3(256), 0, st, x, wg, bias, y, psum, bsx, C, H, W, OH, OW, tx, T);
  SLU_CHECK_LAUNCH();
}

template <int GW>
int launch_gconv_s(int stride, const float* x, const float* wg, const float* bias, float* y, float* psum, long long bsx, int N, int C, int H, int W, int OH,
                   int OW, hipStream_t st) {
  return stride == 1 ? launch_gconv<GW, 1>(x, wg, bias, y, psum, bsx, N, C, H, W, OH, OW, st)
                     : launch_gconv<GW, 2>(x, wg, bias, y, psum, bsx, N, C, H, W, OH, OW, st);
}

}  // namespace

extern "C" int slu_regnet_gconv_tiles(int H, int W, int stride) {
  if (H <= 0 || W <= 0 || (stride != 1 && stride != 2)) return 0;
  int tx;
  return rg_tiles(slu_strided_out(H, stride), slu_strided_out(W, stride), tx);
}

extern "C" int slu_regnet_gconv_fwd(const float* x, int ct, int coff, const float* wg, const float* bias, float* y, float* psum, int N, int C, int gw,
                                    int H, int W, int stride, slu_stream_t stream) {
  const slu_cat2 in = {x, nullptr, ct, coff, C, 0, 0};      // one source: the kernel reads x alone
  if (!wg || !bias || !y || !psum || (stride != 1 && stride != 2) || slu_cat2_check(in, N, H, W)) return SLU_EINVAL;
  if ((gw != 8 && gw != 16 && gw != 24) || C % gw) return SLU_EUNSUPPORTED;
  if (C / gw > 65535 || slu_unit_grid_check(N, H, W)) return SLU_EUNSUPPORTED;
  const int OH = slu_strided_out(H, stride), OW = slu_strided_out(W, stride);
  int tx;
  if (rg_tiles(OH, OW, tx) <= 0) return SLU_EUNSUPPORTED;
  const size_t HW = (size_t)H * W;
  const float* xs = x + (size_t)coff * HW;
  const long long bsx = (long long)ct * HW;
  hipStream_t st = slu_stream(stream);
  if (gw == 8) return launch_gconv_s<8>(stride, xs, wg, bias, y, psum, bsx, N, C, H, W, OH, OW, st);
  if (gw == 16) return launch_gconv_s<16>(stride, xs, wg, bias, y, psum, bsx, N, C, H, W, OH, OW, st);
  return launch_gconv_s<24>(stride, xs, wg, bias, y, psum, bsx, N, C, H, W, OH, OW, st);
}

extern "C" int slu_regnet_sample2(const slu_cat2* in, float* y, int N, int H, int W, slu_stream_t stream) {
  if (!in || !y || slu_cat2_check(*in, N, H, W)) return SLU_EINVAL;
  return slu_cat2_resample(regnet_sample2_kernel, in, y, N, H, W, slu_strided_out(H, 2), slu_strided_out(W, 2), slu_stream(stream));
}
