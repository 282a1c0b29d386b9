// EfficientNetV2 pieces of the semanticFCN_opt encoder (reference baselines/Reichert/semanticFCN_opt.py:170-180,238-247,396-404 builds
// torchvision's efficientnet_v2_{s,m,l} and uses features[0], [2], [3], [4]: FusedMBConv and MBConv blocks).  The dense convs (3x3 expansions,
// 1x1 expansions / projections, with folded BatchNorm, SiLU, per-(sample, channel) SE multipliers and the residual) are launches of the fused
// conv kernel; what is new here is HBM-bound:
//   dwconv3x3_kernel      depthwise 3x3 (stride 1 / 2) + folded BatchNorm + SiLU: one lane per output pixel, lanes azimuth-adjacent
//   global_avgpool_kernel SqueezeExcitation's AdaptiveAvgPool2d(1): one wave per (sample, channel) plane
//   (the gate on the pooled vector, fc1 -> SiLU -> fc2 -> sigmoid, is slu_se_gate in se_gate.hip)
//   dwconv3x3_wgrad_kernel  training: dL/dw[c][tap] = sum over (sample, pixel) of dy * shifted x -- one workgroup per channel, nine fp64 block sums
//                           (the data gradient of the stride-1 depthwise conv is the forward kernel with the taps reversed)
#include "encoder_unit.h"

namespace {

template <int STRIDE>
__global__ __launch_bounds__(256) void dwconv3x3_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                        float* __restrict__ y, int NC, int C, int H, int W, int OH, int OW, int act) {
  const size_t total = (size_t)NC * OH * OW;
  PIX_GRID_STRIDE(e, total) {
    const PixXY o = pix_xy(e, OW, OH);
    const int c = (int)(o.plane % C);
    const float* p = x + o.plane * (size_t)H * W;
    const float* wc = w + (size_t)c * 9;
    float acc = bias ? bias[c] : 0.0f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {      // own copy of the window walk: in the pooling kernels' form (FOR_WINDOW3X3) both instantiations changed
      const int iy = o.y * STRIDE + i - 1;
      if (iy < 0 || iy >= H) continue;
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const int ix = o.x * STRIDE + j - 1;
        if (ix >= 0 && ix < W) acc = fmaf(wc[i * 3 + j], p[(size_t)iy * W + ix], acc);
      }
    }
    y[e] = act == 3 ? silu(acc) : acc;
  }
}

__global__ __launch_bounds__(256) void global_avgpool_kernel(const float* __restrict__ x, float* __restrict__ out, int NC, int HW) {
  const int plane = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (plane >= NC) return;
  const float* p = x + (size_t)plane * HW;
  double s = 0.0;
  for (int i = threadIdx.x & 63; i < HW; i += 64) s += (double)p[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) out[plane] = (float)(s / (double)HW);
}

__global__ __launch_bounds__(256) void dwconv3x3_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ dw, int N,
                                                              int C, int H, int W) {
  const int c = blockIdx.x;
  const size_t HW = (size_t)H * W;
  double acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) acc[t] = 0.0;
  for (int n = 0; n < N; ++n) {
    const float* px = x + ((size_t)n * C + c) * HW;
    const float* pg = dy + ((size_t)n * C + c) * HW;
    float part[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) part[t] = 0.0f;
    for (size_t e = threadIdx.x; e < HW; e += blockDim.x) {
      const int xx = (int)(e % W), yy = (int)(e / W);
      const float g = pg[e];
#pragma unroll
      for (int i = 0; i < 3; ++i) {      // own copy, as dwconv3x3_kernel
        const int iy = yy + i - 1;
        if (iy < 0 || iy >= H) continue;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const int ix = xx + j - 1;
          if (ix >= 0 && ix < W) part[i * 3 + j] = fmaf(g, px[(size_t)iy * W + ix], part[i * 3 + j]);
        }
      }
    }
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[t] += (double)part[t];      // fp32 within one plane and lane (<= HW / 256 terms), fp64 across planes and lanes
  }
  __shared__ double s_red[4][9];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;      // own copy of the workgroup sum: nine values per wave, slots wave-major
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    const double v = wave_sum(acc[t]);
    if (lane == 0) s_red[wave][t] = v;
  }
  __syncthreads();
  if (threadIdx.x < 9) dw[(size_t)c * 9 + threadIdx.x] = (float)(s_red[0][threadIdx.x] + s_red[1][threadIdx.x] + s_red[2][threadIdx.x] + s_red[3][threadIdx.x]);
}

}  // namespace

extern "C" int slu_dwconv3x3_fwd(const float* x, const float* w, const float* bias, float* y, int N, int C, int H, int W, int stride, int act,
                                 slu_stream_t stream) {
  if (!x || !w || !y || N <= 0 || C <= 0 || H <= 0 || W <= 0 || (stride != 1 && stride != 2) || (act != 0 && act != 3)) return SLU_EINVAL;
  const int OH = slu_strided_out(H, stride), OW = slu_strided_out(W, stride);
  const size_t total = (size_t)N * C * OH * OW;
  if (stride == 1)
    hipLaunchKernelGGL(dwconv3x3_kernel<1>, dim3(slu_grid_1d(total, 65535)), dim3(256), 0, slu_stream(stream), x, w, bias, y, N * C, C, H, W, OH, OW, act);
  else
    hipLaunchKernelGGL(dwconv3x3_kernel<2>, dim3(slu_grid_1d(total, 65535)), dim3(256), 0, slu_stream(stream), x, w, bias, y, N * C, C, H, W, OH, OW, act);
  SLU_CHECK_LAUNCH();
}

extern "C" int slu_dwconv3x3_wgrad(const float* x, const float* dy, float* dw, int N, int C, int H, int W, slu_stream_t stream) {
  if (!x || !dy || !dw || N <= 0 || C <= 0 || H <= 0 || W <= 0) return SLU_EINVAL;
  hipLaunchKernelGGL(dwconv3x3_wgrad_kernel, dim3((unsigned)C), dim3(256), 0, slu_stream(stream), x, dy, dw, N, C, H, W);
  SLU_CHECK_LAUNCH();
}

extern "C" int slu_global_avgpool(const float* x, float* out, int N, int C, int HW, slu_stream_t stream) {
  if (!x || !out || N <= 0 || C <= 0 || HW <= 0) return SLU_EINVAL;
  const long long planes = (long long)N * C;
  hipLaunchKernelGGL(global_avgpool_kernel, dim3((unsigned)((planes + 3) / 4)), dim3(256), 0, slu_stream(stream), x, out, (int)planes, HW);
  SLU_CHECK_LAUNCH();
}
