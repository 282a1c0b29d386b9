// Layout and pooling of the half-precision storage path around the convs of conv2d_h8.hip: fp32 NCHW <-> h8 x[N][G][H][W][8] fp16, the
// AvgPool2d(3, 2, 1) between SalsaNext's encoder blocks and nn.PixelShuffle(2) materialised.  Bandwidth-bound, whole 16-byte records.
#include "h8_common.h"

namespace {

// fp32 NCHW [N][C][H][W] -> h8 [N][ceil(C/8)][H][W][8] (pad channels = 0), optional per-(n, c) multiplier
__global__ __launch_bounds__(256) void nchw_to_h8_kernel(const float* __restrict__ x, const float* __restrict__ scale, uint4* __restrict__ y, int N,
                                                         int C, int G, size_t HW) {
  const size_t total = (size_t)N * G * HW;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const size_t pix = e % HW;
    const size_t ng = e / HW;
    const int g = (int)(ng % G);
    const size_t n = ng / G;
    // Without a multiplier the value is converted as it is: x * 1.0f and the conversion fuse into fma(x, 1, +0) -> fp16, which turns -0 into +0.
    // (With a multiplier that fused form stays, one rounding of the exact product; it still stores +0 where x * scale is -0.)
    const auto fill = [&](auto scaled) {
      float v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int c = g * 8 + k;
        v[k] = c >= C ? 0.0f : scaled ? x[(n * C + c) * HW + pix] * scale[n * C + c] : x[(n * C + c) * HW + pix];
      }
      y[e] = h8_pack8(v);
    };
    if (scale) fill(std::true_type{});
    else fill(std::false_type{});
  }
}

__global__ __launch_bounds__(256) void h8_to_nchw_kernel(const uint4* __restrict__ x, float* __restrict__ y, int N, int C, int G, size_t HW) {
  const size_t total = (size_t)N * G * HW;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const size_t pix = e % HW;
    const size_t ng = e / HW;
    const int g = (int)(ng % G);
    const size_t n = ng / G;
    const half8 h = __builtin_bit_cast(half8, x[e]);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int c = g * 8 + k;
      if (c < C) y[(n * C + c) * HW + pix] = (float)h[k];
    }
  }
}

// AvgPool2d(3, stride 2, pad 1, count_include_pad) of x * scale[n, c]; x may hold `in_batch` images shared by all n.
// One thread per output record, the row walk of h8_common.h over the output image.  Each output is the parent form's arithmetic: acc = +0,
// the nine taps added rows -1 .. 1 outside and columns -1 .. 1 inside, a tap outside the image adding +0 (which leaves acc as it is), then
// acc * s / 9.  An output whose nine taps all lie inside the image takes the path without selects; a wave of such outputs -- all but the
// first of a row, and the rows 0 and (H odd) OH - 1 -- never runs the other one.
__global__ __launch_bounds__(256) void avgpool3s2_h8_kernel(const uint4* __restrict__ x, const float* __restrict__ scale, uint4* __restrict__ y,
                                                            int N, int G, int H, int W, int OH, int OW, int in_batch, int tiles) {
  const H8Col col = h8_row_col(tiles);
  const int g = col.g, ox = col.x;
  if (ox >= OW) return;
  const int ix = 2 * ox - 1;
  const bool xin = ox >= 1 && ix + 2 < W;
  for (int n = (int)blockIdx.z; n < N; n += (int)gridDim.z) {
    const size_t ni = in_batch ? (size_t)(n % in_batch) : (size_t)n;
    const uint4* img = x + (ni * G + g) * (size_t)H * W;
    float s[8];
    if (scale) {                                         // uniform: the eight multipliers of (n, g) as two 16-byte loads
      const float4 s0 = *reinterpret_cast<const float4*>(scale + ((size_t)n * G + g) * 8);
      const float4 s1 = *reinterpret_cast<const float4*>(scale + ((size_t)n * G + g) * 8 + 4);
      s[0] = s0.x; s[1] = s0.y; s[2] = s0.z; s[3] = s0.w;
      s[4] = s1.x; s[5] = s1.y; s[6] = s1.z; s[7] = s1.w;
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k) s[k] = 1.0f;
    }
    for (int oy = (int)blockIdx.y; oy < OH; oy += (int)gridDim.y) {
      const int iy = 2 * oy - 1;
      float acc[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[k] = 0.0f;
      if (xin && oy >= 1 && iy + 2 < H) {
        const uint4* p = img + (size_t)iy * W + ix;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
          for (int j = 0; j < 3; ++j) {
            const half8 h = __builtin_bit_cast(half8, p[(size_t)i * W + j]);
#pragma unroll
            for (int k = 0; k < 8; ++k) acc[k] += (float)h[k];
          }
      } else {
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
          for (int j = 0; j < 3; ++j) {
            const bool ok = iy + i >= 0 && iy + i < H && ix + j >= 0 && ix + j < W;
            const half8 h = __builtin_bit_cast(half8, img[ok ? (size_t)(iy + i) * W + (ix + j) : 0]);
#pragma unroll
            for (int k = 0; k < 8; ++k) acc[k] += ok ? (float)h[k] : 0.0f;
          }
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[k] = acc[k] * s[k] / 9.0f;
      y[(((size_t)n * G + g) * OH + oy) * OW + ox] = h8_pack8(acc);
    }
  }
}

// y[n, c, 2h+i, 2w+j] = x[n, 4c+2i+j, h, w] * s_in[n, 4c+2i+j] * s_out[n, c]   (nn.PixelShuffle(2) + both Dropout2d multipliers)
// x: h8 with Gi blocks at HxW; y: h8 with Go = ceil(2 Gi / 8) blocks at 2Hx2W.  One thread takes the four input records (blocks
// 4 go .. 4 go + 3) of one input pixel -- 32 stored channels = 8 output channels x 4 sub-pixels -- and writes the four complete
// output records of the 2x2 output patch: 16-byte loads and stores only, consecutive threads = consecutive azimuth.
__global__ __launch_bounds__(256) void pixel_shuffle_h8_kernel(const uint4* __restrict__ x, const float* __restrict__ s_in,
                                                               const float* __restrict__ s_out, uint4* __restrict__ y, int N, int Gi, int Go, int H,
                                                               int W) {
  const size_t total = (size_t)N * Go * H * W;
  const size_t HWi = (size_t)H * W;
  const int OW = 2 * W;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const int w = (int)(e % W);
    size_t r = e / W;
    const int h = (int)(r % H);
    r /= H;
    const int go = (int)(r % Go);
    const size_t n = r / Go;
    // v[sub][k]: output channel 8 go + k at sub-pixel sub = 2 i + j  <-  stored channel 32 go + 4 k + sub = block 4 go + (k >> 1), slot 4 (k & 1) + sub
    float v[4][8];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int gi = 4 * go + q;
      const bool ok = gi < Gi;
      const half8 rec = __builtin_bit_cast(half8, ok ? x[(n * Gi + gi) * HWi + (size_t)h * W + w] : make_uint4(0u, 0u, 0u, 0u));
#pragma unroll
      for (int slot = 0; slot < 8; ++slot) {
        float t = (float)rec[slot];
        if (ok && s_in) t *= s_in[n * Gi * 8 + gi * 8 + slot];
        v[slot & 3][2 * q + (slot >> 2)] = t;
      }
    }
    if (s_out) {
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int co = 8 * go + k;
        const float so = co < 2 * Gi ? s_out[n * (Gi * 2) + co] : 0.0f;
#pragma unroll
        for (int sub = 0; sub < 4; ++sub) v[sub][k] *= so;
      }
    }
#pragma unroll
    for (int sub = 0; sub < 4; ++sub) {
      const size_t o = ((n * Go + go) * (size_t)(2 * H) + (2 * h + (sub >> 1))) * OW + 2 * w + (sub & 1);
      y[o] = h8_pack8(v[sub]);
    }
  }
}

}  // namespace

extern "C" int slu_nchw_to_h8(const float* x, const float* scale, void* y, int N, int C, int H, int W, slu_stream_t stream) {
  if (!x || !y || N <= 0 || C <= 0 || H <= 0 || W <= 0 || !h8_aligned16(y)) return SLU_EINVAL;
  const int G = (C + 7) / 8;
  const size_t total = (size_t)N * G * H * W;
  hipLaunchKernelGGL(nchw_to_h8_kernel, dim3(slu_grid_1d(total, 32768)), dim3(256), 0, slu_stream(stream), x, scale, reinterpret_cast<uint4*>(y), N, C, G,
                     (size_t)H * W);
  SLU_CHECK_LAUNCH();
}

extern "C" int slu_h8_to_nchw(const void* x, float* y, int N, int C, int H, int W, slu_stream_t stream) {
  if (!x || !y || N <= 0 || C <= 0 || H <= 0 || W <= 0 || !h8_aligned16(x)) return SLU_EINVAL;
  const int G = (C + 7) / 8;
  const size_t total = (size_t)N * G * H * W;
  hipLaunchKernelGGL(h8_to_nchw_kernel, dim3(slu_grid_1d(total, 32768)), dim3(256), 0, slu_stream(stream), reinterpret_cast<const uint4*>(x), y, N, C, G,
                     (size_t)H * W);
  SLU_CHECK_LAUNCH();
}

extern "C" int slu_avgpool3s2_h8(const void* x, const float* scale, void* y, int N, int in_batch, int G, int H, int W, slu_stream_t stream) {
  if (!x || !y || N <= 0 || in_batch < 0 || G <= 0 || H <= 0 || W <= 0 || !h8_aligned16(x, y, scale)) return SLU_EINVAL;
  const int OH = (H + 1) / 2, OW = (W + 1) / 2;
  dim3 grid;
  int tiles;
  if (!h8_row_grid(G, OW, OH, N, grid, tiles)) return SLU_EUNSUPPORTED;
  hipLaunchKernelGGL(avgpool3s2_h8_kernel, grid, dim3(256), 0, slu_stream(stream), reinterpret_cast<const uint4*>(x), scale,
                     reinterpret_cast<uint4*>(y), N, G, H, W, OH, OW, in_batch, tiles);
  SLU_CHECK_LAUNCH();
}

extern "C" int slu_pixel_shuffle_h8(const void* x, const float* scale_in, const float* scale_out, void* y, int N, int Gin, int H, int W,
                                    slu_stream_t stream) {
  if (!x || !y || N <= 0 || Gin <= 0 || H <= 0 || W <= 0 || !h8_aligned16(x, y)) return SLU_EINVAL;
  const int Go = (Gin * 2 + 7) / 8;                 // Cin/4 = 2 Gin output channels
  const size_t total = (size_t)N * Go * H * W;      // one thread per (input pixel, output block)
  hipLaunchKernelGGL(pixel_shuffle_h8_kernel, dim3(slu_grid_1d(total, 32768)), dim3(256), 0, slu_stream(stream), reinterpret_cast<const uint4*>(x), scale_in,
                     scale_out, reinterpret_cast<uint4*>(y), N, Gin, Go, H, W);
  SLU_CHECK_LAUNCH();
}
