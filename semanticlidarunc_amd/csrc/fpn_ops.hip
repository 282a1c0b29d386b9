// Data-movement / per-pixel kernels of the ResNet-FPN model (reference src/models/semanticFCN.py), all HBM-bound:
//   max-pool 3x3/s2/p1 (:149 stem), nearest down-sampling of the meta channels (:283-285), space-to-depth (turns
//   the stride-2 3x3 convs of the ResNet stages into stride-1 2x2 convs), depth-to-space with optional ELU+1
//   (ConvTranspose2d as conv + rearrangement, :230-232,:244-245,:352), attention weights softmax over azimuth
//   multiplied into the value map (:32-38).
#include "pixel_common.h"

namespace {

// nn.MaxPool2d(3, stride 2, padding 1): padding never wins (-inf)
__global__ __launch_bounds__(256) void maxpool3s2_kernel(const float* __restrict__ x, float* __restrict__ y, int NC, int H, int W, int OH, int OW) {
  const size_t total = (size_t)NC * OH * OW;
  PIX_GRID_STRIDE(e, total) {
    const PixXY o = pix_xy(e, OW, OH);
    const float* p = x + o.plane * (size_t)H * W;
    float m = -INFINITY;
    FOR_WINDOW3X3(tap, iy, ix, 2, o.y, o.x, H, W) m = fmaxf(m, p[(size_t)iy * W + ix]);
    y[e] = m;
  }
}

// F.interpolate(mode='nearest', scale_factor=1/f): y[oy][ox] = x[oy*f][ox*f]
__global__ __launch_bounds__(256) void nearest_down_kernel(const float* __restrict__ x, float* __restrict__ y, int NC, int H, int W, int f) {
  const int OH = H / f, OW = W / f;
  const size_t total = (size_t)NC * OH * OW;
  PIX_GRID_STRIDE(e, total) {
    const PixXY o = pix_xy(e, OW, OH);
    y[e] = x[(o.plane * H + (size_t)o.y * f) * W + (size_t)o.x * f];
  }
}

// y[n, (p*2+q)*C + c, oy, ox] = x[n, c, 2*oy+p, 2*ox+q]   (phase-major so each phase is a contiguous channel group)
__global__ __launch_bounds__(256) void space_to_depth2_kernel(const float* __restrict__ x, float* __restrict__ y, int N, int C, int H, int W) {
  const int OH = H / 2, OW = W / 2;
  const size_t total = (size_t)N * 4 * C * OH * OW;
  PIX_GRID_STRIDE(e, total) {
    const PixXYCN o = pix_xycn(e, OW, OH, 4 * C);
    const int ph = o.c / C, c = o.c - ph * C;
    y[e] = x[((o.n * C + c) * H + 2 * o.y + (ph >> 1)) * W + 2 * o.x + (ph & 1)];
  }
}

// space-to-depth of the channel concatenation cat(a[:, :ca], b)  (a has Ca >= ca channels, b has Cb; Cc = ca + Cb):
// y[n, (2p+q)*Cc + c, oy, ox] = (c < ca ? a[n,c,..] : b[n,c-ca,..])[2*oy+p, 2*ox+q]     (semanticFCN.py:309-313 feeding a stride-2 stage)
__global__ __launch_bounds__(256) void space_to_depth2_cat_kernel(const float* __restrict__ a, int Ca, int ca, const float* __restrict__ b, int Cb,
                                                                  float* __restrict__ y, int N, int H, int W) {
  const int OH = H / 2, OW = W / 2, Cc = ca + Cb;
  const size_t total = (size_t)N * 4 * Cc * OH * OW;
  PIX_GRID_STRIDE(e, total) {
    const PixXYCN o = pix_xycn(e, OW, OH, 4 * Cc);
    const int ph = o.c / Cc, c = o.c - ph * Cc;
    const size_t pos = (size_t)(2 * o.y + (ph >> 1)) * W + 2 * o.x + (ph & 1);
    y[e] = c < ca ? a[(o.n * Ca + c) * (size_t)H * W + pos] : b[(o.n * Cb + (c - ca)) * (size_t)H * W + pos];
  }
}

// nn.PixelShuffle(r) (+ optional ELU(alpha=1) + 1): y[n,c,h*r+i,w*r+j] = f(x[n, c*r*r + i*r + j, h, w])
__global__ __launch_bounds__(256) void depth_to_space_kernel(const float* __restrict__ x, float* __restrict__ y, int N, int Cout, int H, int W, int r,
                                                             int elu_plus_one, int c_off, int Ctot) {
  const int OH = H * r, OW = W * r;
  const size_t total = (size_t)N * Cout * OH * OW;
  PIX_GRID_STRIDE(e, total) {
    const PixXYCN o = pix_xycn(e, OW, OH, Cout);
    const int cs = o.c * r * r + (o.y % r) * r + (o.x % r);
    float v = x[((o.n * (size_t)Cout * r * r + cs) * H + o.y / r) * W + o.x / r];
    if (elu_plus_one) v = ::elu_plus_one(v);
    y[((o.n * Ctot + c_off + o.c) * OH + o.y) * (size_t)OW + o.x] = v;
  }
}

// out[n,c,y,:] = value[n,c,y,:] * softmax_x(score[n,0,y,:])      one workgroup per (n, y) row
__global__ __launch_bounds__(256) void row_softmax_mul_kernel(const float* __restrict__ score, const float* __restrict__ value,
                                                              float* __restrict__ out, int C, int H, int W) {
  __shared__ float s_red[4];
  __shared__ float s_w[4096];
  const int n = blockIdx.x / H, y = blockIdx.x % H;
  const float inv = row_softmax_prologue(score + ((size_t)n * H + y) * W, W, s_red, s_w, nullptr);
  for (int c = 0; c < C; ++c) {
    const size_t base = (((size_t)n * C + c) * H + y) * W;
    for (int x = threadIdx.x; x < W; x += blockDim.x) out[base + x] = value[base + x] * (s_w[x] * inv);
  }
}

}  // namespace

extern "C" int slu_maxpool3s2_fwd(const float* x, float* y, int N, int C, int H, int W, slu_stream_t stream) {
  if (!x || !y || N <= 0 || C <= 0 || H <= 0 || W <= 0) return SLU_EINVAL;
  const int OH = (H + 1) / 2, OW = (W + 1) / 2;
  const size_t total = (size_t)N * C * OH * OW;
  hipLaunchKernelGGL(maxpool3s2_kernel, dim3(slu_grid_1d(total, 16384)), dim3(256), 0, slu_stream(stream), x, y, N * C, H, W, OH, OW);
  SLU_CHECK_LAUNCH();
}

extern "C" int slu_nearest_down(const float* x, float* y, int N, int C, int H, int W, int factor, slu_stream_t stream) {
  if (!x || !y || N <= 0 || C <= 0 || H <= 0 || W <= 0 || factor <= 0) return SLU_EINVAL;
  if (H % factor || W % factor) return SLU_EUNSUPPORTED;
  const size_t total = (size_t)N * C * (H / factor) * (W / factor);
  hipLaunchKernelGGL(nearest_down_kernel, dim3(slu_grid_1d(total, 16384)), dim3(256), 0, slu_stream(stream), x, y, N * C, H, W, factor);
  SLU_CHECK_LAUNCH();
}

extern "C" int slu_space_to_depth2(const float* x, float* y, int N, int C, int H, int W, slu_stream_t stream) {
  if (!x || !y || N <= 0 || C <= 0 || H <= 0 || W <= 0) return SLU_EINVAL;
  if ((H & 1) || (W & 1)) return SLU_EUNSUPPORTED;
  const size_t total = (size_t)N * C * H * W;
  hipLaunchKernelGGL(space_to_depth2_kernel, dim3(slu_grid_1d(total, 16384)), dim3(256), 0, slu_stream(stream), x, y, N, C, H, W);
  SLU_CHECK_LAUNCH();
}

extern "C" int slu_space_to_depth2_cat(const float* a, int Ca, int ca, const float* b, int Cb, float* y, int N, int H, int W, slu_stream_t stream) {
  if (!a || !b || !y || N <= 0 || Ca <= 0 || Cb <= 0 || ca <= 0 || ca > Ca || H <= 0 || W <= 0) return SLU_EINVAL;
  if ((H & 1) || (W & 1)) return SLU_EUNSUPPORTED;
  const size_t total = (size_t)N * (ca + Cb) * H * W;
  hipLaunchKernelGGL(space_to_depth2_cat_kernel, dim3(slu_grid_1d(total, 16384)), dim3(256), 0, slu_stream(stream), a, Ca, ca, b, Cb, y, N, H, W);
  SLU_CHECK_LAUNCH();
}

extern "C" int slu_depth_to_space(const float* x, float* y, int N, int Cout, int H, int W, int r, int elu_plus_one, int c_off, int Ctot,
                                  slu_stream_t stream) {
  if (!x || !y || N <= 0 || Cout <= 0 || H <= 0 || W <= 0 || r <= 0 || c_off < 0 || c_off + Cout > Ctot) return SLU_EINVAL;
  const size_t total = (size_t)N * Cout * H * W * r * r;
  hipLaunchKernelGGL(depth_to_space_kernel, dim3(slu_grid_1d(total, 16384)), dim3(256), 0, slu_stream(stream), x, y, N, Cout, H, W, r, elu_plus_one, c_off, Ctot);
  SLU_CHECK_LAUNCH();
}

extern "C" int slu_row_softmax_mul(const float* score, const float* value, float* out, int N, int C, int H, int W, slu_stream_t stream) {
  if (!score || !value || !out || N <= 0 || C <= 0 || H <= 0 || W <= 0) return SLU_EINVAL;
  if (W > 4096 || (long long)N * H > 0x7fffffffLL) return SLU_EUNSUPPORTED;
  hipLaunchKernelGGL(row_softmax_mul_kernel, dim3((unsigned)(N * H)), dim3(256), 0, slu_stream(stream), score, value, out, C, H, W);
  SLU_CHECK_LAUNCH();
}

// ---------------------------------------------------------------------------------------------------------------------
// Pieces of the `semanticFCN_opt` variant (baselines/Reichert/semanticFCN_opt.py):
//   bilinear_up_kernel        F.interpolate(scale_factor = s, mode = 'bilinear', align_corners = False)       UpsampleBlock :24-27
//   groupnorm_stats_kernel    per (sample, group) mean and 1 / sqrt(var + eps) over (C / G) * H * W           nn.GroupNorm :20,66-70
//   groupnorm_apply_kernel    y = (x - mean) * rstd * gamma[c] + beta[c]  [-> ReLU]
//   spatial_softmax_stats / spatial_gate    w = softmax(score over H * W);  out = x * w + x                    SpatialAttention :80-85
// ---------------------------------------------------------------------------------------------------------------------
namespace {

__global__ __launch_bounds__(256) void bilinear_up_kernel(const float* __restrict__ x, float* __restrict__ y, size_t total, int H, int W, int s) {
#pragma clang fp contract(off)
  const int OW = W * s, OH = H * s;
  PIX_GRID_STRIDE(e, total) {
    const PixXY o = pix_xy(e, OW, OH);
    int y0, y1, x0, x1;
    float hl0, hl1, wl0, wl1;
    bilinear_taps(o.y, 1.0f / (float)s, H, y0, y1, hl0, hl1);
    bilinear_taps(o.x, 1.0f / (float)s, W, x0, x1, wl0, wl1);
    const float* p = x + o.plane * (size_t)H * W;
    y[e] = hl0 * (wl0 * p[(size_t)y0 * W + x0] + wl1 * p[(size_t)y0 * W + x1]) + hl1 * (wl0 * p[(size_t)y1 * W + x0] + wl1 * p[(size_t)y1 * W + x1]);
  }
}

// one workgroup per (sample, group): the group's (C / G) * HW values are contiguous in NCHW
__global__ __launch_bounds__(1024) void groupnorm_stats_kernel(const float* __restrict__ x, size_t per_group, float eps, float* __restrict__ mean,
                                                               float* __restrict__ rstd) {
  __shared__ double s_a[16], s_b[16];
  const float* p = x + (size_t)blockIdx.x * per_group;
  double a = 0.0, b = 0.0;
  for (size_t i = threadIdx.x; i < per_group; i += blockDim.x) {
    const double v = (double)p[i];
    a += v;
    b += v * v;
  }
  BLOCK_PUT2(wave_sum, a, s_a, b, s_b);
  __syncthreads();
  if (threadIdx.x == 0) {
    double ta = 0.0, tb = 0.0;
    BLOCK_FOR_WAVES(w, 0) { ta += s_a[w]; tb += s_b[w]; }
    const double m = ta / (double)per_group;
    double var = tb / (double)per_group - m * m;            // biased variance, as nn.GroupNorm
    var = var < 0.0 ? 0.0 : var;
    mean[blockIdx.x] = (float)m;
    rstd[blockIdx.x] = (float)(1.0 / sqrt(var + (double)eps));
  }
}

__global__ __launch_bounds__(256) void groupnorm_apply_kernel(const float* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                              const float* __restrict__ gamma, const float* __restrict__ beta, float* __restrict__ y,
                                                              size_t total, int C, int cpg, size_t HW, int relu) {
  PIX_GRID_STRIDE(e, total) {
    const size_t nc = e / HW;
    const int c = (int)(nc % C);
    const size_t ng = (nc / C) * (size_t)(C / cpg) + c / cpg;
    float v = (x[e] - mean[ng]) * rstd[ng] * (gamma ? gamma[c] : 1.0f) + (beta ? beta[c] : 0.0f);
    y[e] = relu ? fmaxf(v, 0.0f) : v;
  }
}

// per sample: max and 1 / sum(exp(s - max)) of the score map [HW]
__global__ __launch_bounds__(1024) void spatial_softmax_stats_kernel(const float* __restrict__ score, size_t HW, float* __restrict__ stats) {
  __shared__ float s_r[16];
  const float* p = score + (size_t)blockIdx.x * HW;
  float m = -INFINITY;
  for (size_t i = threadIdx.x; i < HW; i += blockDim.x) m = fmaxf(m, p[i]);
  BLOCK_PUT(wave_max, m, s_r);
  __syncthreads();
  m = s_r[0];
  BLOCK_FOR_WAVES(w, 1) m = fmaxf(m, s_r[w]);
  __syncthreads();
  float sum = 0.0f;
  for (size_t i = threadIdx.x; i < HW; i += blockDim.x) sum += expf(p[i] - m);
  BLOCK_PUT(wave_sum, sum, s_r);
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.0f;
    BLOCK_FOR_WAVES(w, 0) t += s_r[w];
    stats[2 * blockIdx.x] = m;
    stats[2 * blockIdx.x + 1] = 1.0f / t;
  }
}

__global__ __launch_bounds__(256) void spatial_gate_kernel(const float* __restrict__ x, const float* __restrict__ score, const float* __restrict__ stats,
                                                           float* __restrict__ out, size_t total, int C, size_t HW) {
  PIX_GRID_STRIDE(e, total) {
    const size_t hw = e % HW, n = e / HW / C;
    const float w = spatial_softmax_weight(score[n * HW + hw], stats, n);
    const float v = x[e];
    out[e] = v * w + v;
  }
}

}  // namespace

extern "C" int slu_bilinear_upsample(const float* x, float* y, int N, int C, int H, int W, int scale, slu_stream_t stream) {
  if (!x || !y || N <= 0 || C <= 0 || H <= 0 || W <= 0 || scale < 1) return SLU_EINVAL;
  const size_t total = (size_t)N * C * H * W * scale * scale;
  hipLaunchKernelGGL(bilinear_up_kernel, dim3(slu_grid_1d(total, 65535)), dim3(256), 0, slu_stream(stream), x, y, total, H, W, scale);
  SLU_CHECK_LAUNCH();
}

extern "C" int slu_groupnorm_fwd(const float* x, const float* gamma, const float* beta, int N, int C, int HW, int groups, float eps, int relu,
                                 float* mean, float* rstd, float* y, slu_stream_t stream) {
  if (!x || !y || !mean || !rstd || N <= 0 || C <= 0 || HW <= 0 || groups <= 0 || C % groups || !(eps >= 0.0f)) return SLU_EINVAL;
  if ((long long)N * groups > 0x7fffffffLL) return SLU_EUNSUPPORTED;
  const int cpg = C / groups;
  hipStream_t st = slu_stream(stream);
  hipLaunchKernelGGL(groupnorm_stats_kernel, dim3((unsigned)(N * groups)), dim3(1024), 0, st, x, (size_t)cpg * HW, eps, mean, rstd);
  const size_t total = (size_t)N * C * HW;
  hipLaunchKernelGGL(groupnorm_apply_kernel, dim3(slu_grid_1d(total, 65535)), dim3(256), 0, st, x, mean, rstd, gamma, beta, y, total, C, cpg, (size_t)HW, relu);
  SLU_CHECK_LAUNCH();
}

extern "C" int slu_groupnorm_stats(const float* x, int N, int C, int HW, int groups, float eps, float* mean, float* rstd, slu_stream_t stream) {
  if (!x || !mean || !rstd || N <= 0 || C <= 0 || HW <= 0 || groups <= 0 || C % groups || !(eps >= 0.0f)) return SLU_EINVAL;
  if ((long long)N * groups > 0x7fffffffLL) return SLU_EUNSUPPORTED;
  hipLaunchKernelGGL(groupnorm_stats_kernel, dim3((unsigned)(N * groups)), dim3(1024), 0, slu_stream(stream), x, (size_t)(C / groups) * HW, eps, mean,
                     rstd);
  SLU_CHECK_LAUNCH();
}

extern "C" int slu_spatial_softmax_gate(const float* x, const float* score, float* stats, float* out, int N, int C, int HW, slu_stream_t stream) {
  if (!x || !score || !stats || !out || N <= 0 || C <= 0 || HW <= 0) return SLU_EINVAL;
  hipStream_t st = slu_stream(stream);
  hipLaunchKernelGGL(spatial_softmax_stats_kernel, dim3((unsigned)N), dim3(1024), 0, st, score, (size_t)HW, stats);
  const size_t total = (size_t)N * C * HW;
  hipLaunchKernelGGL(spatial_gate_kernel, dim3(slu_grid_1d(total, 65535)), dim3(256), 0, st, x, score, stats, out, total, C, (size_t)HW);
  SLU_CHECK_LAUNCH();
}
