// Data movement of the ResNet-FPN model (models/semanticFCN.py) on the half-precision storage path: everything the model adds around the
// convs of conv2d_h8.hip.  Activations are h8, x[N][G][H][W][8] fp16 (conv2d_h8.hip); every kernel here is bandwidth-bound and moves whole
// 16-byte records, consecutive lanes on consecutive azimuth (W), so a wave's loads and stores are contiguous runs of up to 1 KB.
//   maxpool3s2_h8_kernel        MaxPool2d(3, 2, 1) of the stem
//   space_to_depth2_h8_kernel   the four phases of a stage's input (+ the multi-scale meta injection, + phase (0, 0) on its own)
//   attention_row_h8_kernel     score, softmax over the azimuth and the multiply into the value map of an AttentionModule
//   depth_to_space_h8_kernel    ConvTranspose2d(k = s) after its 1x1 conv, into a block slice of the concatenated up-sampled maps
//   depth_to_space2_elu_h8_kernel   the last ConvTranspose2d(4, 2, 1) after its 3x3 conv, with ELU + 1, as fp32 NCHW
#include "h8_common.h"
#include <math.h>

namespace {

// One thread per output record, as avgpool3s2_h8_kernel (layout_h8.hip): the row walk of h8_common.h over the output image.
// fp16 max is exact, so the nine taps are compared as packed halves; a tap outside the image is -inf.
__global__ __launch_bounds__(256) void maxpool3s2_h8_kernel(const uint4* __restrict__ x, uint4* __restrict__ y, int N, int G, int H, int W, int OH,
                                                            int OW, int tiles) {
  const H8Col col = h8_row_col(tiles);
  const int g = col.g, ox = col.x;
  if (ox >= OW) return;
  const int ix = 2 * ox - 1;
  half8 ninf;
#pragma unroll
  for (int k = 0; k < 8; ++k) ninf[k] = (_Float16)(-INFINITY);
  for (int n = (int)blockIdx.z; n < N; n += (int)gridDim.z) {
    const uint4* img = x + ((size_t)n * G + g) * (size_t)H * W;
    for (int oy = (int)blockIdx.y; oy < OH; oy += (int)gridDim.y) {
      const int iy = 2 * oy - 1;
      half8 m = ninf;
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const bool ok = iy + i >= 0 && iy + i < H && ix + j >= 0 && ix + j < W;
          const half8 h = __builtin_bit_cast(half8, img[ok ? (size_t)(iy + i) * W + (ix + j) : 0]);
          m = __builtin_elementwise_max(m, ok ? h : ninf);
        }
      y[(((size_t)n * G + g) * OH + oy) * OW + ox] = __builtin_bit_cast(uint4, m);
    }
  }
}

// One thread per output pixel (oy, ox) of one input block g: the 2 x 2 input records of the pixel (two 32-byte runs per lane, a wave reads
// 2 KB contiguous per input row) go to the four phase planes (2 p + q) G + g of y and, phase (0, 0), to plane g of y00.  With meta, the slots of
// channels C - m .. C - 1 take meta[n][c - (C - m)][f (2 oy + p)][f (2 ox + q)] instead: only the blocks that hold such a channel (uniform per
// workgroup) read meta.  Grid as the pooling kernels.
__global__ __launch_bounds__(256) void space_to_depth2_h8_kernel(const uint4* __restrict__ x, const float* __restrict__ meta, int m, int C, int f,
                                                                 uint4* __restrict__ y, uint4* __restrict__ y00, int N, int G, int H, int W,
                                                                 int tiles) {
  const int OH = H >> 1, OW = W >> 1;
  const H8Col col = h8_row_col(tiles);
  const int g = col.g, ox = col.x;
  if (ox >= OW) return;
  const int c_first = C - m;                                    // first replaced channel
  const bool inject = meta != nullptr && 8 * g + 7 >= c_first && 8 * g < C;
  const size_t MH = (size_t)f * H, MW = (size_t)f * W;
  for (int n = (int)blockIdx.z; n < N; n += (int)gridDim.z) {
    const uint4* img = x + ((size_t)n * G + g) * (size_t)H * W;
    for (int oy = (int)blockIdx.y; oy < OH; oy += (int)gridDim.y) {
#pragma unroll
      for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const int iy = 2 * oy + p, ix = 2 * ox + q;
          uint4 r = img[(size_t)iy * W + ix];
          if (inject) {
            half8 h = __builtin_bit_cast(half8, r);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
              const int c = 8 * g + k;
              if (c >= c_first && c < C) h[k] = (_Float16)meta[(((size_t)n * m + (c - c_first)) * MH + (size_t)f * iy) * MW + (size_t)f * ix];
            }
            r = __builtin_bit_cast(uint4, h);
          }
          y[((((size_t)n * 4 + (2 * p + q)) * G + g) * OH + oy) * OW + ox] = r;
          if (p == 0 && q == 0 && y00) y00[(((size_t)n * G + g) * OH + oy) * OW + ox] = r;
        }
    }
  }
}

// tanh(v) = 1 - 2 / (exp(2 v) + 1): saturates to +-1 through exp's inf / 0, absolute error ~1e-7 (the score sums C of them; the output's bar is
// 2^-10 relative)
__device__ __forceinline__ float att_tanh(float v) { return 1.0f - 2.0f * __builtin_amdgcn_rcpf(__expf(2.0f * v) + 1.0f); }

constexpr int ATT_MAX_W = 4096;

// One workgroup (4 waves) per image row (n, h).  Pass 1: thread t owns pixels w = t, t + 256, ...: the row's t records block by block (lanes on
// consecutive w), score into LDS.  Max and sum of the row through wave shuffles + one LDS exchange; p[w] stays in LDS.  Pass 2: the row's v
// records (g, w) flattened with w fastest, times p[w], stored as whole records.
__global__ __launch_bounds__(256) void attention_row_h8_kernel(const uint4* __restrict__ tv, const float* __restrict__ w_a, const float* __restrict__ b_a,
                                                               uint4* __restrict__ out, int G, int H, int W) {
  __shared__ float s_p[ATT_MAX_W];
  __shared__ float s_wa[512];                                   // C <= 512 here (the launcher checks)
  __shared__ float s_red[8];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t n = blockIdx.x / (unsigned)H, h = blockIdx.x - n * (unsigned)H;
  const size_t HW = (size_t)H * W;
  const uint4* trow = tv + (n * 2 * G) * HW + h * W;            // block g of t: + g HW;  block g of v: + (G + g) HW
  for (int c = tid; c < 8 * G; c += 256) s_wa[c] = w_a[c];
  __syncthreads();
  const float bias = b_a[0];
  float mx = -INFINITY;
  for (int w = tid; w < W; w += 256) {
    float s = bias;
    for (int g = 0; g < G; ++g) {
      const half8 t = __builtin_bit_cast(half8, trow[(size_t)g * HW + w]);
#pragma unroll
      for (int k = 0; k < 8; ++k) s += s_wa[8 * g + k] * att_tanh((float)t[k]);
    }
    s_p[w] = s;
    mx = fmaxf(mx, s);
  }
  mx = wave_max(mx);
  if (lane == 0) s_red[wave] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
  float sum = 0.0f;
  for (int w = tid; w < W; w += 256) {                          // each thread revisits the scores it wrote
    const float e = __expf(s_p[w] - mx);
    s_p[w] = e;
    sum += e;
  }
  sum = wave_sum(sum);
  if (lane == 0) s_red[4 + wave] = sum;
  __syncthreads();
  const float inv = 1.0f / (s_red[4] + s_red[5] + s_red[6] + s_red[7]);
  const uint4* vrow = trow + (size_t)G * HW;
  uint4* orow = out + (n * G) * HW + h * W;
  const int total = G * W;
  for (int i = tid; i < total; i += 256) {
    const int g = i / W, w = i - g * W;
    const half8 v = __builtin_bit_cast(half8, vrow[(size_t)g * HW + w]);
    const float p = s_p[w] * inv;
    float r[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) r[k] = (float)v[k] * p;
    orow[(size_t)g * HW + w] = h8_pack8(r);
  }
}

// One thread per output record: grid x = (block g of the slice, 256 output columns), y = output row, z = image.  Lanes on consecutive output
// columns read the s planes (i s + j) Go + g in turn, 64 / s consecutive records of each.
__global__ __launch_bounds__(256) void depth_to_space_h8_kernel(const uint4* __restrict__ y, uint4* __restrict__ out, int N, int Go, int s, int H, int W,
                                                                int Gtot, int g_off, int tiles) {
  const int OH = s * H, OW = s * W;
  const H8Col col = h8_row_col(tiles);
  const int g = col.g, ox = col.x;
  if (ox >= OW) return;
  const int w = ox / s, j = ox - w * s;
  for (int n = (int)blockIdx.z; n < N; n += (int)gridDim.z)
    for (int oy = (int)blockIdx.y; oy < OH; oy += (int)gridDim.y) {
      const int h = oy / s, i = oy - h * s;
      out[(((size_t)n * Gtot + g_off + g) * OH + oy) * OW + ox] = y[((((size_t)n * s * s + (i * s + j)) * Go + g) * H + h) * W + w];
    }
}

__device__ __forceinline__ float elu_plus_one(float v) { return (v > 0.0f ? v : expm1f(v)) + 1.0f; }

// One thread per input record (block g = classes 2 g, 2 g + 1 with their four sub-pixels each, pixel (h, w)): two 8-byte stores per class, lanes
// on consecutive columns, so a wave writes 512 contiguous bytes of each of its four output rows.  Grid as above over the INPUT image.
__global__ __launch_bounds__(256) void depth_to_space2_elu_h8_kernel(const uint4* __restrict__ y, float* __restrict__ out, int N, int classes, int G, int H,
                                                                     int W, int tiles) {
  const H8Col col = h8_row_col(tiles);
  const int g = col.g, w = col.x;
  if (w >= W) return;
  const size_t OW = 2 * (size_t)W, OH = 2 * (size_t)H;
  for (int n = (int)blockIdx.z; n < N; n += (int)gridDim.z)
    for (int h = (int)blockIdx.y; h < H; h += (int)gridDim.y) {
      const half8 v = __builtin_bit_cast(half8, y[(((size_t)n * G + g) * H + h) * W + w]);
#pragma unroll
      for (int cc = 0; cc < 2; ++cc) {
        const int c = 2 * g + cc;
        if (c < classes) {
          float* o = out + (((size_t)n * classes + c) * OH + 2 * (size_t)h) * OW + 2 * (size_t)w;
          *reinterpret_cast<float2*>(o) = make_float2(elu_plus_one((float)v[4 * cc]), elu_plus_one((float)v[4 * cc + 1]));
          *reinterpret_cast<float2*>(o + OW) = make_float2(elu_plus_one((float)v[4 * cc + 2]), elu_plus_one((float)v[4 * cc + 3]));
        }
      }
    }
}

}  // namespace

extern "C" int slu_maxpool3s2_h8(const void* x, void* y, int N, int G, int H, int W, slu_stream_t stream) {
  if (!x || !y || N <= 0 || G <= 0 || H <= 0 || W <= 0 || !h8_aligned16(x, y)) return SLU_EINVAL;
  const int OH = (H + 1) / 2, OW = (W + 1) / 2;
  dim3 grid;
  int tiles;
  if (!h8_row_grid(G, OW, OH, N, grid, tiles)) return SLU_EUNSUPPORTED;
  hipLaunchKernelGGL(maxpool3s2_h8_kernel, grid, dim3(256), 0, slu_stream(stream), reinterpret_cast<const uint4*>(x), reinterpret_cast<uint4*>(y), N, G,
                     H, W, OH, OW, tiles);
  SLU_CHECK_LAUNCH();
}

extern "C" int slu_space_to_depth2_h8(const void* x, const float* meta, int m, int C, int f, void* y, void* y00, int N, int G, int H, int W,
                                      slu_stream_t stream) {
  if (!x || !y || N <= 0 || G <= 0 || H <= 0 || W <= 0 || (H & 1) || (W & 1) || !h8_aligned16(x, y, y00)) return SLU_EINVAL;
  if (meta && (m <= 0 || m > C || C <= 8 * (G - 1) || C > 8 * G || (f != 1 && f != 2 && f != 4 && f != 8))) return SLU_EINVAL;
  dim3 grid;
  int tiles;
  if (!h8_row_grid(G, W / 2, H / 2, N, grid, tiles)) return SLU_EUNSUPPORTED;
  hipLaunchKernelGGL(space_to_depth2_h8_kernel, grid, dim3(256), 0, slu_stream(stream), reinterpret_cast<const uint4*>(x), meta, meta ? m : 0,
                     meta ? C : 0, meta ? f : 1, reinterpret_cast<uint4*>(y), reinterpret_cast<uint4*>(y00), N, G, H, W, tiles);
  SLU_CHECK_LAUNCH();
}

extern "C" int slu_attention_row_h8(const void* tv, const float* w_a, const float* b_a, void* out, int N, int C, int H, int W, slu_stream_t stream) {
  if (!tv || !w_a || !b_a || !out || N <= 0 || C <= 0 || (C & 7) || H <= 0 || W <= 0 || !h8_aligned16(tv, out)) return SLU_EINVAL;
  if (C > 512 || W > ATT_MAX_W || (long long)N * H > 0x7fffffffLL) return SLU_EUNSUPPORTED;
  hipLaunchKernelGGL(attention_row_h8_kernel, dim3((unsigned)(N * H)), dim3(256), 0, slu_stream(stream), reinterpret_cast<const uint4*>(tv), w_a, b_a,
                     reinterpret_cast<uint4*>(out), C / 8, H, W);
  SLU_CHECK_LAUNCH();
}

extern "C" int slu_depth_to_space_h8(const void* y, void* out, int N, int Cout, int s, int H, int W, int Gtot, int g_off, slu_stream_t stream) {
  if (!y || !out || N <= 0 || Cout <= 0 || (Cout & 7) || H <= 0 || W <= 0 || !h8_aligned16(y, out)) return SLU_EINVAL;
  if ((s != 2 && s != 4 && s != 8) || g_off < 0 || g_off + Cout / 8 > Gtot) return SLU_EINVAL;
  if ((long long)s * H > 0x7fffffffLL || (long long)s * W > 0x7fffffffLL) return SLU_EUNSUPPORTED;
  dim3 grid;
  int tiles;
  if (!h8_row_grid(Cout / 8, s * W, s * H, N, grid, tiles)) return SLU_EUNSUPPORTED;
  hipLaunchKernelGGL(depth_to_space_h8_kernel, grid, dim3(256), 0, slu_stream(stream), reinterpret_cast<const uint4*>(y), reinterpret_cast<uint4*>(out), N,
                     Cout / 8, s, H, W, Gtot, g_off, tiles);
  SLU_CHECK_LAUNCH();
}

extern "C" int slu_depth_to_space2_elu_h8(const void* y, float* out, int N, int classes, int H, int W, slu_stream_t stream) {
  if (!y || !out || N <= 0 || classes <= 0 || H <= 0 || W <= 0 || !h8_aligned16(y) || ((uintptr_t)out & 7)) return SLU_EINVAL;
  const int G = (4 * classes + 7) / 8;
  dim3 grid;
  int tiles;
  if (!h8_row_grid(G, W, H, N, grid, tiles)) return SLU_EUNSUPPORTED;
  hipLaunchKernelGGL(depth_to_space2_elu_h8_kernel, grid, dim3(256), 0, slu_stream(stream), reinterpret_cast<const uint4*>(y), out, N, classes, G, H, W,
                     tiles);
  SLU_CHECK_LAUNCH();
}
