// What `semanticFCN_opt` (baselines/Reichert/semanticFCN_opt.py) puts between its convs, on the half-precision storage path: the h8 forms of
// the four fp32 kernels at the end of fpn_ops.hip.  Activations are h8, x[N][G][H][W][8] fp16 (conv2d_h8.hip); every kernel is
// bandwidth-bound, every lane loads and stores whole 16-byte records on consecutive pixels, the arithmetic is fp32 (fp64 for the sums of
// GroupNorm) and a stored value is rounded to fp16 once.  No float atomics: every reduction has a fixed order, so two runs give the same bits.
//   bilinear_up_h8_kernel          F.interpolate(scale_factor = s, mode = 'bilinear', align_corners = False)        UpsampleBlock :24-27
//   groupnorm_partial_h8_kernel    per (plane, part): 8 channel sums and 8 sums of squares, fp64                     nn.GroupNorm :20,66-70
//   groupnorm_finalize_h8_kernel   per (image, group): mean and 1 / sqrt(var + eps) from the partials, in a fixed order
//   groupnorm_apply_h8_kernel      out = (x - mean) * rstd * gamma[c] + beta[c] [-> ReLU], into a block slice
//   spatial_softmax_stats_h8_kernel / spatial_gate_h8_kernel    w = softmax(score over H * W); out = x * w + x     SpatialAttention :80-85
#include "h8_common.h"
#include "pixel_common.h"      // bilinear_taps
#include <math.h>

namespace {

// One thread per output record, as depth_to_space_h8_kernel: grid x = (block g, 256 output columns), y = output row, z = image; y and z
// stride.  The four source records of a pixel are whole records too; s consecutive lanes share them.  The sum is written as
// bilinear_up_kernel (fpn_ops.hip) writes it, without contraction, so the fp32 value is the one the fp32 path stores.
__global__ __launch_bounds__(256) void bilinear_up_h8_kernel(const uint4* __restrict__ x, uint4* __restrict__ y, int N, int G, int H, int W, int s,
                                                             int tiles) {
#pragma clang fp contract(off)
  const int OH = s * H, OW = s * W;
  const H8Col col = h8_row_col(tiles);
  const int g = col.g, ox = col.x;
  if (ox >= OW) return;
  const float inv_s = 1.0f / (float)s;
  int x0, x1;
  float wl0, wl1;
  bilinear_taps(ox, inv_s, W, x0, x1, wl0, wl1);
  for (int n = (int)blockIdx.z; n < N; n += (int)gridDim.z) {
    const uint4* img = x + ((size_t)n * G + g) * (size_t)H * W;
    for (int oy = (int)blockIdx.y; oy < OH; oy += (int)gridDim.y) {
      int y0, y1;
      float hl0, hl1;
      bilinear_taps(oy, inv_s, H, y0, y1, hl0, hl1);
      const half8 a = __builtin_bit_cast(half8, img[(size_t)y0 * W + x0]), b = __builtin_bit_cast(half8, img[(size_t)y0 * W + x1]);
      const half8 c = __builtin_bit_cast(half8, img[(size_t)y1 * W + x0]), d = __builtin_bit_cast(half8, img[(size_t)y1 * W + x1]);
      float r[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) r[k] = hl0 * (wl0 * (float)a[k] + wl1 * (float)b[k]) + hl1 * (wl0 * (float)c[k] + wl1 * (float)d[k]);
      y[(((size_t)n * G + g) * OH + oy) * OW + ox] = h8_pack8(r);
    }
  }
}

constexpr int GN_SLOTS = 16;          // doubles per partial: 8 channel sums, then 8 sums of squares
constexpr int GN_MAX_PARTS = 256;

// grid x = part, y = plane (n G + g): the workgroup sums records [part chunk, (part + 1) chunk) of its plane.  fp16 values and their fp32
// squares (22 significant bits) are exact, and they are summed in fp64: the variance E[x^2] - mean^2 keeps ~1e-16 * (mean / std)^2 of
// relative error, whatever the mean.  Wave shuffles, then the four waves in a fixed order.
__global__ __launch_bounds__(256) void groupnorm_partial_h8_kernel(const uint4* __restrict__ x, size_t HW, size_t chunk, double* __restrict__ ws) {
  __shared__ double s_red[4][GN_SLOTS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t plane = blockIdx.y;
  const size_t beg = (size_t)blockIdx.x * chunk;
  const size_t end = beg + chunk < HW ? beg + chunk : HW;
  const uint4* p = x + plane * HW;
  double a[8], b[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) a[k] = b[k] = 0.0;
#pragma unroll 4
  for (size_t i = beg + tid; i < end; i += 256) {
    const half8 v = __builtin_bit_cast(half8, p[i]);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float f = (float)v[k];
      a[k] += (double)f;
      b[k] += (double)(f * f);
    }
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    a[k] = wave_sum(a[k]);
    b[k] = wave_sum(b[k]);
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      s_red[wave][k] = a[k];
      s_red[wave][8 + k] = b[k];
    }
  }
  __syncthreads();
  if (tid < GN_SLOTS) ws[(plane * gridDim.x + blockIdx.x) * GN_SLOTS + tid] = (s_red[0][tid] + s_red[1][tid]) + (s_red[2][tid] + s_red[3][tid]);
}

// One wave per (image, group): the group's cpg channels are slots k0 .. k0 + cpg - 1 of block g = c0 / 8.  Lane l adds parts l, l + 64, ...
// in that order, the wave adds its lanes by the butterfly of wave_sum: a fixed order.
__global__ __launch_bounds__(64) void groupnorm_finalize_h8_kernel(const double* __restrict__ ws, int parts, int G, int groups, int cpg, double count,
                                                                   float eps, float* __restrict__ mean, float* __restrict__ rstd) {
  const int n = (int)(blockIdx.x / (unsigned)groups), gr = (int)(blockIdx.x - (unsigned)n * (unsigned)groups);
  const int c0 = gr * cpg, g = c0 >> 3, k0 = c0 & 7;
  const double* p = ws + ((size_t)n * G + g) * (size_t)parts * GN_SLOTS;
  double a = 0.0, b = 0.0;
  for (int part = (int)threadIdx.x; part < parts; part += 64)
    for (int k = k0; k < k0 + cpg; ++k) {
      a += p[(size_t)part * GN_SLOTS + k];
      b += p[(size_t)part * GN_SLOTS + 8 + k];
    }
  a = wave_sum(a);
  b = wave_sum(b);
  if (threadIdx.x == 0) {
    const double m = a / count;
    double var = b / count - m * m;                               // biased variance, as nn.GroupNorm
    var = var < 0.0 ? 0.0 : var;
    mean[blockIdx.x] = (float)m;
    rstd[blockIdx.x] = (float)(1.0 / sqrt(var + (double)eps));
  }
}

// grid x = runs of 256 records of a plane (strided), y = block g, z = image (strided): the 8 means, rstd * gamma and beta of a workgroup are
// uniform.  Channels past C (the pad of the last block) get 0 * x + 0.  A thread reads its record before it writes it: out may be x.
__global__ __launch_bounds__(256) void groupnorm_apply_h8_kernel(const uint4* x, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                 const float* __restrict__ gamma, const float* __restrict__ beta, int relu,
                                                                 uint4* out, int N, int C, int G, size_t HW, int groups, int cpg, int Gtot, int g_off) {
  const int g = (int)blockIdx.y;
  for (int n = (int)blockIdx.z; n < N; n += (int)gridDim.z) {
    float mu[8], sa[8], sb[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int c = 8 * g + k;
      const bool ok = c < C;
      const int gi = n * groups + (ok ? c / cpg : 0);
      mu[k] = ok ? mean[gi] : 0.0f;
      sa[k] = ok ? rstd[gi] * (gamma ? gamma[c] : 1.0f) : 0.0f;
      sb[k] = ok && beta ? beta[c] : 0.0f;
    }
    const uint4* src = x + ((size_t)n * G + g) * HW;
    uint4* dst = out + ((size_t)n * Gtot + g_off + g) * HW;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < HW; i += (size_t)gridDim.x * 256) {
      const half8 v = __builtin_bit_cast(half8, src[i]);
      float r[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        r[k] = ((float)v[k] - mu[k]) * sa[k] + sb[k];
        r[k] = relu ? fmaxf(r[k], 0.0f) : r[k];
      }
      dst[i] = h8_pack8(r);
    }
  }
}

// (max, sum of exp(s - max)) of a run of scores joined with another: the running form of the softmax denominator
__device__ __forceinline__ void softmax_join(float& m, float& s, float m2, float s2) {
  const float mn = fmaxf(m, m2);
  s = (m == -INFINITY ? 0.0f : s * __expf(m - mn)) + (m2 == -INFINITY ? 0.0f : s2 * __expf(m2 - mn));
  m = mn;
}

// One workgroup (16 waves) per image: max and 1 / sum(exp(s - max)) of its HW scores, read once.  Thread t owns scores t, t + 1024, ... (VEC:
// groups of four, 16 bytes a load); lanes, then waves, are joined in a fixed order.  The largest map of the model (level 1 of a 128 x 2048
// scan: 64 x 1024 scores, 256 KB) is 16 loads per thread.
template <bool VEC>
__global__ __launch_bounds__(1024) void spatial_softmax_stats_h8_kernel(const float* __restrict__ score, size_t HW, float* __restrict__ stats) {
  __shared__ float s_m[16], s_s[16];
  const float* p = score + (size_t)blockIdx.x * HW;
  float m = -INFINITY, s = 0.0f;
  if (VEC) {
    const size_t nv = HW >> 2;
    for (size_t i = threadIdx.x; i < nv; i += 1024) {
      const float4 v = reinterpret_cast<const float4*>(p)[i];
      const float m4 = fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w));
      softmax_join(m, s, m4, (__expf(v.x - m4) + __expf(v.y - m4)) + (__expf(v.z - m4) + __expf(v.w - m4)));
    }
  } else {
    for (size_t i = threadIdx.x; i < HW; i += 1024) softmax_join(m, s, p[i], 1.0f);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
    // both lanes of a pair must compute the same bits: join (lower lane, upper lane) in that order on both
    float ma = (threadIdx.x & o) ? m2 : m, sa = (threadIdx.x & o) ? s2 : s;
    softmax_join(ma, sa, (threadIdx.x & o) ? m : m2, (threadIdx.x & o) ? s : s2);
    m = ma;
    s = sa;
  }
  if ((threadIdx.x & 63) == 0) {
    s_m[threadIdx.x >> 6] = m;
    s_s[threadIdx.x >> 6] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float tm = s_m[0], ts = s_s[0];
    for (int w = 1; w < 16; ++w) softmax_join(tm, ts, s_m[w], s_s[w]);
    stats[2 * blockIdx.x] = tm;
    stats[2 * blockIdx.x + 1] = 1.0f / ts;
  }
}

// grid x = runs of 256 pixels (strided), y = a share of the blocks, z = image (strided): a thread computes the weight of its pixel once and
// walks the blocks g = blockIdx.y, + gridDim.y, ...; lanes on consecutive pixels.  out = x * w + x as one fma, rounded to fp16 once.
__global__ __launch_bounds__(256) void spatial_gate_h8_kernel(const uint4* __restrict__ x, const float* __restrict__ score, const float* __restrict__ stats,
                                                              uint4* __restrict__ out, int N, int G, size_t HW) {
  for (int n = (int)blockIdx.z; n < N; n += (int)gridDim.z) {
    const float mx = stats[2 * n], inv = stats[2 * n + 1];
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < HW; i += (size_t)gridDim.x * 256) {
      const float w = __expf(score[(size_t)n * HW + i] - mx) * inv;
      for (int g = (int)blockIdx.y; g < G; g += (int)gridDim.y) {
        const size_t at = ((size_t)n * G + g) * HW + i;
        const half8 v = __builtin_bit_cast(half8, x[at]);
        float r[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) r[k] = fmaf((float)v[k], w, (float)v[k]);
        out[at] = h8_pack8(r);
      }
    }
  }
}

// parts of a plane for the GroupNorm sums: at least 1024 records each, and about 2048 workgroups over all planes (N = 1, C = 16 at
// 128 x 2048 is 2 planes of 4 MB: 256 parts each)
inline int gn_parts(long long planes, int HW) {
  long long by_size = ((long long)HW + 1023) / 1024, by_fill = (2048 + planes - 1) / planes;
  long long p = by_size < by_fill ? by_size : by_fill;
  return (int)(p < 1 ? 1 : (p > GN_MAX_PARTS ? GN_MAX_PARTS : p));
}

inline unsigned capped(size_t v, unsigned cap) { return (unsigned)(v > cap ? cap : (v ? v : 1)); }

}  // namespace

extern "C" int slu_bilinear_upsample_h8(const void* x, void* y, int N, int G, int H, int W, int s, slu_stream_t stream) {
  if (!x || !y || N <= 0 || G <= 0 || H <= 0 || W <= 0 || !h8_aligned16(x, y)) return SLU_EINVAL;
  if (s != 2 && s != 4 && s != 8) return SLU_EINVAL;
  if ((long long)s * H > 0x7fffffffLL || (long long)s * W > 0x7fffffffLL) return SLU_EUNSUPPORTED;
  dim3 grid;
  int tiles;
  if (!h8_row_grid(G, s * W, s * H, N, grid, tiles)) return SLU_EUNSUPPORTED;
  hipLaunchKernelGGL(bilinear_up_h8_kernel, grid, dim3(256), 0, slu_stream(stream), reinterpret_cast<const uint4*>(x), reinterpret_cast<uint4*>(y), N, G, H,
                     W, s, tiles);
  SLU_CHECK_LAUNCH();
}

extern "C" size_t slu_groupnorm_stats_h8_workspace_bytes(int N, int C, int HW) {
  if (N <= 0 || C <= 0 || HW <= 0) return 0;
  const long long planes = (long long)N * ((C + 7) / 8);
  return (size_t)planes * (size_t)gn_parts(planes, HW) * GN_SLOTS * sizeof(double);
}

extern "C" int slu_groupnorm_stats_h8(const void* x, int N, int C, int HW, int groups, float eps, float* mean, float* rstd, void* workspace,
                                      slu_stream_t stream) {
  if (!x || !mean || !rstd || !workspace || N <= 0 || C <= 0 || HW <= 0 || groups <= 0 || C % groups || !(eps >= 0.0f)) return SLU_EINVAL;
  if (!h8_aligned16(x) || ((uintptr_t)workspace & 7)) return SLU_EINVAL;
  const int cpg = C / groups, G = (C + 7) / 8;
  if (cpg != 1 && cpg != 2 && cpg != 4 && cpg != 8) return SLU_EUNSUPPORTED;      // a group must lie inside one record
  const long long planes = (long long)N * G;
  if (planes > 65535 || (long long)N * groups > 0x7fffffffLL) return SLU_EUNSUPPORTED;
  const int parts = gn_parts(planes, HW);
  const size_t chunk = ((size_t)HW + parts - 1) / parts;
  hipStream_t st = slu_stream(stream);
  hipLaunchKernelGGL(groupnorm_partial_h8_kernel, dim3((unsigned)parts, (unsigned)planes), dim3(256), 0, st, reinterpret_cast<const uint4*>(x), (size_t)HW,
                     chunk, reinterpret_cast<double*>(workspace));
  hipLaunchKernelGGL(groupnorm_finalize_h8_kernel, dim3((unsigned)(N * groups)), dim3(64), 0, st, reinterpret_cast<const double*>(workspace), parts, G, groups,
                     cpg, (double)cpg * (double)HW, eps, mean, rstd);
  SLU_CHECK_LAUNCH();
}

extern "C" int slu_groupnorm_apply_h8(const void* x, const float* mean, const float* rstd, const float* gamma, const float* beta, int relu, void* out, int N,
                                      int C, int HW, int groups, int Gtot, int g_off, slu_stream_t stream) {
  if (!x || !mean || !rstd || !out || N <= 0 || C <= 0 || HW <= 0 || groups <= 0 || C % groups || !h8_aligned16(x, out)) return SLU_EINVAL;
  const int G = (C + 7) / 8;
  if (g_off < 0 || g_off + G > Gtot) return SLU_EINVAL;
  if (x == out && (Gtot != G || g_off != 0)) return SLU_EINVAL;                   // in place only as the whole tensor
  if (G > 65535) return SLU_EUNSUPPORTED;
  const dim3 grid(capped(((size_t)HW + 255) / 256, 4096), (unsigned)G, capped((size_t)N, 65535));
  hipLaunchKernelGGL(groupnorm_apply_h8_kernel, grid, dim3(256), 0, slu_stream(stream), reinterpret_cast<const uint4*>(x), mean, rstd, gamma, beta, relu,
                     reinterpret_cast<uint4*>(out), N, C, G, (size_t)HW, groups, C / groups, Gtot, g_off);
  SLU_CHECK_LAUNCH();
}

extern "C" int slu_spatial_softmax_gate_h8(const void* x, const float* score, float* stats, void* out, int N, int C, int HW, slu_stream_t stream) {
  if (!x || !score || !stats || !out || N <= 0 || C <= 0 || HW <= 0 || !h8_aligned16(x, out) || ((uintptr_t)score & 3)) return SLU_EINVAL;
  const int G = (C + 7) / 8;
  hipStream_t st = slu_stream(stream);
  if ((HW & 3) == 0 && h8_aligned16(score))
    hipLaunchKernelGGL(spatial_softmax_stats_h8_kernel<true>, dim3((unsigned)N), dim3(1024), 0, st, score, (size_t)HW, stats);
  else
    hipLaunchKernelGGL(spatial_softmax_stats_h8_kernel<false>, dim3((unsigned)N), dim3(1024), 0, st, score, (size_t)HW, stats);
  // about 1024 workgroups: the blocks are shared out over grid y only where the pixels alone do not give that many
  const size_t tiles = ((size_t)HW + 255) / 256;
  const size_t want_y = (1024 + tiles * (size_t)N - 1) / (tiles * (size_t)N);
  const dim3 grid(capped(tiles, 4096), capped(want_y < (size_t)G ? want_y : (size_t)G, 65535), capped((size_t)N, 65535));
  hipLaunchKernelGGL(spatial_gate_h8_kernel, grid, dim3(256), 0, st, reinterpret_cast<const uint4*>(x), score, stats, reinterpret_cast<uint4*>(out), N, G,
                     (size_t)HW);
  SLU_CHECK_LAUNCH();
}
