// Vocabulary shared by the fp32 per-pixel, normalisation and data-movement kernels: backward.hip, fpn_ops.hip, fpn_train.hip, effnet_ops.hip,
// pointwise.hip (fpn_opt_h8.hip takes the bilinear taps only).  As in h8_common.h a helper has the form with which each kernel compiles to the
// instructions of the copy it replaced -- a forced-inline function where that holds, a macro (loop header or statement) where it does not: check
// a change here with tools/h8_isa_diff.py --match kernel (profiles/r21).
#pragma once
#include "slu_common.h"

// ---- element walk: one thread per element of a contiguous NCHW tensor, grid-stride ------------------------------------------------------
#define PIX_GRID_STRIDE(e, total) \
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < (total); e += (size_t)gridDim.x * blockDim.x)

struct PixXY   { int x, y; size_t plane; };      // plane = n C + c
struct PixXYCN { int x, y, c; size_t n; };
__device__ __forceinline__ PixXY pix_xy(size_t e, int W, int H) {
  const int x = (int)(e % W);
  const size_t r = e / W;
  return {x, (int)(r % H), r / H};
}
template <class TC>      // int, or size_t where C is a product
__device__ __forceinline__ PixXYCN pix_xycn(size_t e, int W, int H, TC C) {
  const int x = (int)(e % W);
  size_t r = e / W;
  const int y = (int)(r % H);
  r /= H;
  return {x, y, (int)(r % C), r / C};
}

// ---- 3x3 windows ---------------------------------------------------------------------------------------------------------------------------
// in-bounds taps (iy, ix) of the 3x3 / pad 1 window of output (oy, ox) at stride STRIDE, row-major; tap = 3 i + j.  Loop headers (macros), fully
// unrolled: as functions taking the body as a lambda the pooling kernels changed.
#define FOR_WINDOW3X3(tap, iy, ix, STRIDE, oy, ox, H, W)                                      \
  _Pragma("unroll") for (int i_ = -1, iy; i_ <= 1; ++i_)                                      \
    if ((iy = (STRIDE) * (oy) + i_) >= 0 && iy < (H))                                         \
      _Pragma("unroll") for (int j_ = -1, ix, tap; j_ <= 1; ++j_)                             \
        if ((tap = (i_ + 1) * 3 + j_ + 1, ix = (STRIDE) * (ox) + j_) >= 0 && ix < (W))

// ---- workgroup reduction: wave_sum / wave_max -> one LDS slot per wave -> barrier -> the slots combined in a fixed order ----------------------
//   BLOCK_PUT(wave_sum, v, s);  __syncthreads();  total = BLOCK_TOTAL4(s);          (workgroup of 256; sums left to right, as every copy had them)
//   BLOCK_PUT2 for two values that share the barrier; BLOCK_FOR_WAVES(w, first) { t += s[w]; } where the workgroup's size is the launcher's (1024).
// The caller puts a barrier before it reuses the slots.  Macros on the __shared__ arrays themselves: as functions taking the slots as pointers
// (LDS through generic pointers until late in the compilation) eight kernels re-scheduled.
#define BLOCK_PUT(wave_op, v, slots)                               \
  do {                                                             \
    v = wave_op(v);                                                \
    if ((threadIdx.x & 63) == 0) (slots)[threadIdx.x >> 6] = v;    \
  } while (0)
#define BLOCK_PUT2(wave_op, v1, slots1, v2, slots2)                                                    \
  do {                                                                                                 \
    v1 = wave_op(v1);                                                                                  \
    v2 = wave_op(v2);                                                                                  \
    if ((threadIdx.x & 63) == 0) { (slots1)[threadIdx.x >> 6] = v1; (slots2)[threadIdx.x >> 6] = v2; } \
  } while (0)
#define BLOCK_TOTAL4(s) ((s)[0] + (s)[1] + (s)[2] + (s)[3])
#define BLOCK_MAX4(s) fmaxf(fmaxf((s)[0], (s)[1]), fmaxf((s)[2], (s)[3]))
#define BLOCK_FOR_WAVES(w, first) for (int w = (first); w < (int)(blockDim.x >> 6); ++w)

// ---- softmax pieces ----------------------------------------------------------------------------------------------------------------------
// Row softmax, workgroup of 256 on one row of W <= 4096 scores: s_e[x] = expf(srow[x] - max); returns 1 / sum.  A thread writes the columns
// x = tid + 256 k only, so it may read them back without a barrier.  s_zero (optional): cleared over the same columns.
__device__ __forceinline__ float row_softmax_prologue(const float* srow, int W, float* s_red, float* s_e, float* s_zero) {
  float m = -INFINITY;
  for (int x = threadIdx.x; x < W; x += blockDim.x) m = fmaxf(m, srow[x]);
  BLOCK_PUT(wave_max, m, s_red);
  __syncthreads();
  m = BLOCK_MAX4(s_red);
  __syncthreads();
  float sum = 0.0f;
  for (int x = threadIdx.x; x < W; x += blockDim.x) {
    const float e = expf(srow[x] - m);
    s_e[x] = e;
    if (s_zero) s_zero[x] = 0.0f;
    sum += e;
  }
  BLOCK_PUT(wave_sum, sum, s_red);
  __syncthreads();
  return 1.0f / BLOCK_TOTAL4(s_red);
}
// Spatial softmax over H W of sample n: its weight at a pixel from the score there and stats[2 n] = max, stats[2 n + 1] = 1 / sum exp
// (spatial_softmax_stats_kernel)
__device__ __forceinline__ float spatial_softmax_weight(float score, float mx, float inv) { return expf(score - mx) * inv; }
__device__ __forceinline__ float spatial_softmax_weight(float score, const float* __restrict__ stats, size_t n) {
  return spatial_softmax_weight(score, stats[2 * n], stats[2 * n + 1]);
}

// ---- bilinear taps: source index of ATen's area_pixel_compute_source_index (align_corners = False, not cubic): max(0, (dst + 0.5) / s - 0.5)
// with inv_s = 1.0f / (float)s, exact for a power-of-two s.  i1 = min(i0 + 1, n_in - 1), weights l0 = 1 - l1, l1 = src - i0.  The forward kernels and
// the backward (which re-derives the forward's taps) call this one copy.  The tests' 1e-6 bar on the forward holds for power-of-two scales only:
// at s = 3, 5, 6 inv_s is rounded, and torch's own fp32 path is 1.2e-5 to 2.4e-5 from fp64 there (tests/test_gpu_pixel_kernel_edges.py).  s = 1
// gives l1 = 0 and the input back bit for bit.
__device__ __forceinline__ void bilinear_taps(int dst, float inv_s, int n_in, int& i0, int& i1, float& l0, float& l1) {
  float src = ((float)dst + 0.5f) * inv_s - 0.5f;
  src = src < 0.0f ? 0.0f : src;
  i0 = (int)src;
  i1 = i0 + (i0 < n_in - 1 ? 1 : 0);
  l1 = src - (float)i0;
  l0 = 1.0f - l1;
}

// ---- activations -------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }
__device__ __forceinline__ float silu(float v) { return v / (1.0f + expf(-v)); }
__device__ __forceinline__ float elu_plus_one(float v) { return (v > 0.0f ? v : expm1f(v)) + 1.0f; }      // nn.ELU(alpha = 1), then the reference's "+ 1"
