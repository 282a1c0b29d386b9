// The SqueezeExcitation gate of the RegNetY and EfficientNetV2 blocks: one kernel behind three entry points.
//
//   se_gate_kernel<SILU, MAXT>   mean[n, c] = inv_count * sum_t psum[n, c, t]   (added in tile order)
//                                gate[n, c] = sigmoid(b2[c] + sum_s w2[c, s] act(b1[s] + sum_c' w1[s, c'] mean[n, c'])),  act = SiLU or ReLU
//     One workgroup per (image, slice of `cper` output channels); every workgroup of an image stages the whole mean in LDS ([C] means | [S]
//     hidden activations, dynamic) and computes the whole hidden vector -- one wave per hidden unit, a dot product over C with lane stride 64,
//     wave_sum, then the bias; the fc1 weights come from L2 -- and then walks its slice of fc2 with stride blockDim.x, an fmaf chain over s
//     from b2[c].  b1 / b2 may be null (no bias); `mean`, where given, is written by the first slice.  No atomics: the same bits every run.
//     A plain mean is the case T = 1, inv_count = 1: 0.0f + x and x * 1.0f are exact, so the staged value is the input for every x but -0.0f,
//     which is staged as +0.0f -- and no output can tell the two apart: fc1's accumulator starts from +0.0f, and +0.0f + w * (+-0.0f) is +0.0f.
//     MAXT is the launch bound of the instantiation (256 or 1024 threads).
//
//   slu_se_gate          [N, C] means, SiLU, nullable biases: 256 threads, grid (N, 1), cper = C
//   slu_regnet_se_gate   tile sums from regnet_gconv_kernel (regnet_unit.hip), ReLU, optional mean output: 256 threads, grid (N, ceil(C / 256))
//   slu_se_gate_psum     tile sums from dwconv3x3_se_kernel (mbconv_unit.hip), SiLU: 64 * clamp(S, 4, 16) threads, grid (N, ceil(C / threads)) --
//                        with 4 waves fc1 is the serial part of the wide blocks (24 dot products of 1536 in a row per wave at S = 96; here 6)
#include "pixel_common.h"

namespace {

template <bool SILU, int MAXT>
__global__ __launch_bounds__(MAXT) void se_gate_kernel(const float* __restrict__ psum, int T, float inv_count, const float* __restrict__ w1,
                                                       const float* __restrict__ b1, const float* __restrict__ w2, const float* __restrict__ b2,
                                                       float* __restrict__ gate, float* __restrict__ mean, int C, int S, int cper) {
  extern __shared__ float s_mem[];      // [C] means | [S] hidden activations
  float* s_avg = s_mem;
  float* s_hid = s_mem + C;
  const int n = blockIdx.x;
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    const float* p = psum + ((size_t)n * C + c) * T;
    float s = 0.0f;
    for (int t = 0; t < T; ++t) s += p[t];      // tile order
    s *= inv_count;
    s_avg[c] = s;
    if (mean && blockIdx.y == 0) mean[(size_t)n * C + c] = s;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  for (int s = wave; s < S; s += nw) {      // one wave per hidden unit: a dot product over C
    float acc = 0.0f;
    for (int c = lane; c < C; c += 64) acc = fmaf(w1[(size_t)s * C + c], s_avg[c], acc);
    acc = wave_sum(acc) + (b1 ? b1[s] : 0.0f);
    if (lane == 0) s_hid[s] = SILU ? silu(acc) : (acc > 0.0f ? acc : 0.0f);
  }
  __syncthreads();
  const int c0 = blockIdx.y * cper;
  const int c1 = min(C, c0 + cper);
  for (int c = c0 + threadIdx.x; c < c1; c += blockDim.x) {
    float acc = b2 ? b2[c] : 0.0f;
    for (int s = 0; s < S; ++s) acc = fmaf(w2[(size_t)c * S + s], s_hid[s], acc);
    gate[(size_t)n * C + c] = sigmoid(acc);
  }
}

constexpr int SEG_MAX_C = 1536, SEG_MAX_S = 96;      // slu_se_gate_psum's range: EfficientNetV2-L's widest MBConv

}  // namespace

extern "C" int slu_se_gate(const float* avg, const float* w1, const float* b1, const float* w2, const float* b2, float* scale, int N, int C, int S,
                           slu_stream_t stream) {
  if (!avg || !w1 || !w2 || !scale || N <= 0 || C <= 0 || S <= 0 || (size_t)(C + S) * 4 > 64 * 1024) return SLU_EINVAL;
  hipLaunchKernelGGL((se_gate_kernel<true, 256>), dim3((unsigned)N), dim3(256), (size_t)(C + S) * 4, slu_stream(stream), avg, 1, 1.0f, w1, b1, w2, b2,
                     scale, (float*)nullptr, C, S, C);
  SLU_CHECK_LAUNCH();
}

extern "C" int slu_regnet_se_gate(const float* psum, int T, float inv_count, const float* w1, const float* b1, const float* w2, const float* b2,
                                  float* gate, float* mean, int N, int C, int S, slu_stream_t stream) {
  if (!psum || !w1 || !b1 || !w2 || !b2 || !gate || T <= 0 || N <= 0 || C <= 0 || S <= 0) return SLU_EINVAL;
  if ((size_t)(C + S) * 4 > 64 * 1024 || N > 65535) return SLU_EUNSUPPORTED;
  const int slices = (C + 255) / 256;
  hipLaunchKernelGGL((se_gate_kernel<false, 256>), dim3((unsigned)N, (unsigned)slices), dim3(256), (size_t)(C + S) * 4, slu_stream(stream), psum, T,
                     inv_count, w1, b1, w2, b2, gate, mean, C, S, 256);
  SLU_CHECK_LAUNCH();
}

extern "C" int slu_se_gate_psum(const float* psum, int T, float inv_count, const float* w1, const float* b1, const float* w2, const float* b2,
                                float* scale, int N, int C, int S, slu_stream_t stream) {
  if (!psum || !w1 || !b1 || !w2 || !b2 || !scale || T <= 0 || N <= 0 || C <= 0 || S <= 0) return SLU_EINVAL;
  if (C > SEG_MAX_C || S > SEG_MAX_S || N > 65535) return SLU_EINVAL;
  const int waves = S < 4 ? 4 : (S > 16 ? 16 : S);
  const int threads = 64 * waves;
  hipLaunchKernelGGL((se_gate_kernel<true, 1024>), dim3((unsigned)N, (unsigned)((C + threads - 1) / threads)), dim3(threads), (size_t)(C + S) * 4,
                     slu_stream(stream), psum, T, inv_count, w1, b1, w2, b2, scale, (float*)nullptr, C, S, threads);
  SLU_CHECK_LAUNCH();
}
