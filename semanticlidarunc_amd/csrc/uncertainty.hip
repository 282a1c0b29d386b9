// Uncertainty maps from logits (oracle/uncertainty.py): the MC-dropout reduction (softmax over C, running mean over T, predictive
// entropy, mutual information, argmax) and the single-pass softmax / entropy map.  One lane owns one pixel, the class axis
// (C <= 32, 20 for SemanticKITTI) lives in registers, never in LDS (class_column.h): HBM-bound.
// Both normalise as the reference does, p = exp(log_softmax(x)) = exp(x - m - log se), not e / se.
#include "class_column.h"

namespace {

// probs_t = exp(log_softmax(x_t)); accumulates over t in registers; never materialises [T,B,C,HW].
template <int CMAX>
__global__ __launch_bounds__(256) void mc_reduce_kernel(const float* __restrict__ logits, int T, int B, int C, int HW,
                                                        float eps, float lnC, float* __restrict__ p_bar,
                                                        float* __restrict__ h_norm, float* __restrict__ mi_norm,
                                                        int64_t* __restrict__ preds) {
  const size_t npix = (size_t)B * HW;
  const size_t pix = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (pix >= npix) return;
  const SluPixel px = slu_pixel(pix, C, HW);
  const size_t col = px.col;                                   // of the outputs
  float psum[CMAX];
#pragma unroll
  for (int c = 0; c < CMAX; ++c) psum[c] = 0.0f;
  float hsum = 0.0f;
  for (int t = 0; t < T; ++t) {
    // sample t's column from b and hw, not as t * B * C * HW + col: with that form mc_reduce_kernel<32> spills 20 bytes per lane
    float x[CMAX];
    const float m = slu_load_column(logits + ((size_t)t * B + px.b) * C * (size_t)HW + px.hw, C, HW, -INFINITY, x);
    const float lse = logf(slu_exp_sum(x, C, m));
    float ht = 0.0f;
#pragma unroll
    for (int c = 0; c < CMAX; ++c)
      if (c < C) {
        const float p = expf(x[c] - m - lse);
        psum[c] += p;
        const float pc = fmaxf(p, eps);
        ht -= pc * logf(pc);
      }
    hsum += ht;
  }
  float hb = 0.0f;
#pragma unroll
  for (int c = 0; c < CMAX; ++c)
    if (c < C) {
      psum[c] = psum[c] / (float)T;
      p_bar[col + (size_t)c * HW] = psum[c];
      const float pc = fmaxf(psum[c], eps);
      hb -= pc * logf(pc);
    }
  float best;
  preds[pix] = slu_first_argmax(psum, C, best);
  h_norm[pix] = hb / lnC;
  mi_norm[pix] = fmaxf((hb - hsum / (float)T) / lnC, 0.0f);
}

template <int CMAX>
__global__ __launch_bounds__(256) void softmax_entropy_kernel(const float* __restrict__ logits, int B, int C, int HW,
                                                              float eps, float lnC, float* __restrict__ probs,
                                                              float* __restrict__ h_norm, int64_t* __restrict__ preds) {
  const size_t npix = (size_t)B * HW;
  const size_t pix = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (pix >= npix) return;
  const size_t col = slu_pixel(pix, C, HW).col;
  float x[CMAX];
  const float m = slu_load_column(logits + col, C, HW, -INFINITY, x);
  const float lse = logf(slu_exp_sum(x, C, m));
  float h = 0.0f;
#pragma unroll
  for (int c = 0; c < CMAX; ++c)
    if (c < C) {
      x[c] = expf(x[c] - m - lse);
      if (probs) probs[col + (size_t)c * HW] = x[c];
      h -= x[c] * logf(fmaxf(x[c], eps));
    }
  float best;
  const int arg = slu_first_argmax(x, C, best);
  if (h_norm) h_norm[pix] = h / lnC;
  if (preds) preds[pix] = arg;
}

}  // namespace

extern "C" int slu_mc_reduce(const float* logits, int T, int B, int C, int HW, float eps, float* p_bar, float* h_norm,
                             float* mi_norm, int64_t* preds, slu_stream_t stream) {
  if (!logits || !p_bar || !h_norm || !mi_norm || !preds || T <= 0 || B <= 0 || C <= 0 || HW <= 0) return SLU_EINVAL;
  if (C > 32) return SLU_EUNSUPPORTED;
  const unsigned nb = slu_grid_per_pixel((size_t)B * HW);
  const float lnC = (float)log((double)C);
  slu_class_cap(C, [&](auto cmax) {
    hipLaunchKernelGGL(mc_reduce_kernel<decltype(cmax)::value>, dim3(nb), dim3(256), 0, slu_stream(stream), logits, T, B, C, HW, eps, lnC, p_bar,
                       h_norm, mi_norm, preds);
  });
  SLU_CHECK_LAUNCH();
}

extern "C" int slu_softmax_entropy(const float* logits, int B, int C, int HW, float eps, float* probs, float* h_norm,
                                   int64_t* preds, slu_stream_t stream) {
  if (!logits || B <= 0 || C <= 0 || HW <= 0) return SLU_EINVAL;
  if (C > 32) return SLU_EUNSUPPORTED;
  const unsigned nb = slu_grid_per_pixel((size_t)B * HW);
  const float lnC = (float)log((double)C);
  slu_class_cap(C, [&](auto cmax) {
    hipLaunchKernelGGL(softmax_entropy_kernel<decltype(cmax)::value>, dim3(nb), dim3(256), 0, slu_stream(stream), logits, B, C, HW, eps, lnC, probs,
                       h_norm, preds);
  });
  SLU_CHECK_LAUNCH();
}
