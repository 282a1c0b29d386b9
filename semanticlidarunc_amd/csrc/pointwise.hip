// BatchNorm fold (one thread per channel) and the 3x3 / stride-2 average pool (grid-stride over output elements, optionally
// broadcasting one source image to several outputs): HBM-bound.
#include "pixel_common.h"

namespace {

__global__ void bn_fold_kernel(const float* __restrict__ gamma, const float* __restrict__ beta,
                               const float* __restrict__ mean, const float* __restrict__ var, float eps, int C,
                               float* __restrict__ a, float* __restrict__ b) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < C) {
    const float s = gamma[c] / sqrtf(var[c] + eps);
    a[c] = s;
    b[c] = beta[c] - mean[c] * s;
  }
}

// y[n,c,oy,ox] = (1/9) sum_{i,j in -1..1} s * x[n,c,2oy+i,2ox+j]  (zeros outside; divisor always 9)
__global__ void avgpool3s2_kernel(const float* __restrict__ x, const float* __restrict__ scale, float* __restrict__ y,
                                  int NC, int H, int W, int OH, int OW, int C, int in_batch) {
  const size_t total = (size_t)NC * OH * OW;
  PIX_GRID_STRIDE(e, total) {
    const PixXY o = pix_xy(e, OW, OH);
    const size_t nc = o.plane;
    const float s = scale ? scale[nc] : 1.0f;
    const size_t nc_in = in_batch ? ((nc / C) % in_batch) * C + nc % C : nc;   // broadcast source image
    const float* p = x + nc_in * (size_t)H * W;
    float acc = 0.0f;
    FOR_WINDOW3X3(tap, iy, ix, 2, o.y, o.x, H, W) acc += p[(size_t)iy * W + ix] * s;
    y[e] = acc / 9.0f;
  }
}

}  // namespace

extern "C" int slu_bn_fold(const float* gamma, const float* beta, const float* mean, const float* var, float eps, int C,
                           float* a, float* b, slu_stream_t stream) {
  if (!gamma || !beta || !mean || !var || !a || !b || C <= 0) return SLU_EINVAL;
  hipLaunchKernelGGL(bn_fold_kernel, dim3((C + 255) / 256), dim3(256), 0, slu_stream(stream), gamma, beta, mean, var, eps, C, a, b);
  SLU_CHECK_LAUNCH();
}

extern "C" int slu_avgpool3s2_fwd(const float* x, const float* scale, float* y, int N, int C, int H, int W,
                                  slu_stream_t stream) {
  if (!x || !y || N <= 0 || C <= 0 || H <= 0 || W <= 0) return SLU_EINVAL;
  const int OH = (H + 1) / 2, OW = (W + 1) / 2;
  const size_t total = (size_t)N * C * OH * OW;
  hipLaunchKernelGGL(avgpool3s2_kernel, dim3(slu_grid_1d(total, 16384)), dim3(256), 0, slu_stream(stream), x, scale, y,
                     N * C, H, W, OH, OW, C, 0);
  SLU_CHECK_LAUNCH();
}

extern "C" int slu_avgpool3s2_bcast_fwd(const float* x, const float* scale, float* y, int N, int in_batch, int C, int H, int W,
                                        slu_stream_t stream) {
  if (!x || !y || N <= 0 || in_batch <= 0 || C <= 0 || H <= 0 || W <= 0) return SLU_EINVAL;
  const int OH = (H + 1) / 2, OW = (W + 1) / 2;
  const size_t total = (size_t)N * C * OH * OW;
  hipLaunchKernelGGL(avgpool3s2_kernel, dim3(slu_grid_1d(total, 16384)), dim3(256), 0, slu_stream(stream), x, scale, y,
                     N * C, H, W, OH, OW, C, in_batch);
  SLU_CHECK_LAUNCH();
}
