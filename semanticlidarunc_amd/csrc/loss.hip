// Per-pixel NLL / cross-entropy (forward + backward), and the softmax + NLL forward and the softmax backward of the fused
// "SalsaNext" loss  (reference: src/models/trainer.py:508-516, src/models/losses.py:50-73).
// One lane per pixel, class axis in registers (class_column.h): HBM-bound.
#include "class_column.h"

namespace {

enum NllKind { kLogits = 0, kProbsClamp = 1, kProbsEps = 2, kLogProbs = 3 };

template <int CMAX, int KIND>
__global__ __launch_bounds__(256) void nll_fwd_kernel(const float* __restrict__ x, const int64_t* __restrict__ labels, int B, int C,
                                                      int HW, float param, int64_t ignore, double* __restrict__ nll_sum,
                                                      unsigned long long* __restrict__ count) {
  __shared__ double s_part[4];
  __shared__ unsigned s_cnt[4];
  const size_t npix = (size_t)B * HW;
  double local = 0.0;
  unsigned n = 0;
  for (size_t pix = (size_t)blockIdx.x * blockDim.x + threadIdx.x; pix < npix; pix += (size_t)gridDim.x * blockDim.x) {
    const int64_t lab = labels[pix];
    if (slu_label_ignored(lab, ignore) || !slu_label_in_range(lab, C)) continue;
    const float* src = x + slu_pixel(pix, C, HW).col;
    float v;
    if constexpr (KIND == kLogits) {
      float xs[CMAX];
      const float m = slu_load_column(src, C, HW, -INFINITY, xs);
      float xy = 0.0f;
#pragma unroll
      for (int c = 0; c < CMAX; ++c)
        if ((int64_t)c == lab) xy = xs[c];
      v = (m + logf(slu_exp_sum(xs, C, m))) - xy;
    } else {
      const float t = src[(size_t)lab * HW];
      if constexpr (KIND == kProbsClamp) v = -logf(fmaxf(t, param));
      else if constexpr (KIND == kProbsEps) v = -logf(t + param);
      else v = -t;
    }
    local += (double)v;
    ++n;
  }
  slu_stage_wave_total(wave_sum(local), s_part);
  slu_stage_wave_total((unsigned)wave_sum((float)n), s_cnt);
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned c = slu_block_total(s_cnt);
    if (c) { atomicAdd(nll_sum, slu_block_total(s_part)); atomicAdd(count, (unsigned long long)c); }
  }
}

// grad_x = gscale[0] * d(sum of nll)/dx   (caller folds 1/count and the upstream gradient into gscale)
template <int CMAX, int KIND>
__global__ __launch_bounds__(256) void nll_bwd_kernel(const float* __restrict__ x, const int64_t* __restrict__ labels, int B, int C,
                                                      int HW, float param, int64_t ignore,
                                                      const float* __restrict__ gscale, float* __restrict__ grad_x) {
  const size_t npix = (size_t)B * HW;
  const size_t pix = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (pix >= npix) return;
  const float s = gscale[0];
  const int64_t lab = labels[pix];
  const bool valid = !(slu_label_ignored(lab, ignore) || !slu_label_in_range(lab, C));
  const size_t col = slu_pixel(pix, C, HW).col;
  const float* src = x + col;
  float* dst = grad_x + col;
  if constexpr (KIND == kLogits) {
    float xs[CMAX];
    const float m = slu_load_column(src, C, HW, -INFINITY, xs);
    const float se = slu_exp_sum_inplace(xs, C, m);
#pragma unroll
    for (int c = 0; c < CMAX; ++c)
      if (c < C) dst[(size_t)c * HW] = valid ? s * (xs[c] / se - ((int64_t)c == lab ? 1.0f : 0.0f)) : 0.0f;
  } else {
    const float t = valid ? src[(size_t)lab * HW] : 1.0f;
    float g = 0.0f;
    if (valid) {
      if constexpr (KIND == kProbsClamp) g = t >= param ? -s / t : 0.0f;
      else if constexpr (KIND == kProbsEps) g = -s / (t + param);
      else g = -s;
    }
#pragma unroll
    for (int c = 0; c < CMAX; ++c)
      if (c < C) dst[(size_t)c * HW] = ((int64_t)c == lab) ? g : 0.0f;
  }
}

// grad_logits = softmax backward of  g_c = gout * ( w_dense * dense_c  -  [c == y && p_y >= clamp] * w_nll / p_y )
template <int CMAX>
__global__ __launch_bounds__(256) void softmax_loss_bwd_kernel(const float* __restrict__ probs, const int64_t* __restrict__ labels,
                                                               const float* __restrict__ dense, float w_dense, float w_nll,
                                                               float clampv, const float* __restrict__ gout, int B, int C, int HW,
                                                               float* __restrict__ grad_logits) {
  const size_t npix = (size_t)B * HW;
  const size_t pix = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (pix >= npix) return;
  const float go = gout ? gout[0] : 1.0f;
  const int64_t lab = labels ? labels[pix] : -1;
  const size_t base = slu_pixel(pix, C, HW).col;
  float p[CMAX], g[CMAX];
  float dot = 0.0f;
#pragma unroll
  for (int c = 0; c < CMAX; ++c)
    if (c < C) {
      p[c] = probs[base + (size_t)c * HW];
      float gc = dense ? w_dense * dense[base + (size_t)c * HW] : 0.0f;
      if ((int64_t)c == lab && p[c] >= clampv) gc -= w_nll / p[c];
      g[c] = gc * go;
      dot += g[c] * p[c];
    }
#pragma unroll
  for (int c = 0; c < CMAX; ++c)
    if (c < C) grad_logits[base + (size_t)c * HW] = p[c] * (g[c] - dot);
}

// models/trainer.py:511-514 : probs = softmax(logits); -log(max(probs[y], clamp)) summed over the pixels whose label is in range
template <int CMAX>
__global__ __launch_bounds__(256) void softmax_nll_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                          int B, int C, int HW, float clampv, float* __restrict__ probs,
                                                          double* __restrict__ nll_sum) {
  __shared__ double s_part[4];
  const size_t npix = (size_t)B * HW;
  double local = 0.0;
  for (size_t pix = (size_t)blockIdx.x * blockDim.x + threadIdx.x; pix < npix; pix += (size_t)gridDim.x * blockDim.x) {
    const size_t col = slu_pixel(pix, C, HW).col;
    float x[CMAX];
    const float m = slu_load_column(logits + col, C, HW, -INFINITY, x);
    const float se = slu_exp_sum_inplace(x, C, m);
    const int64_t lab = labels[pix];
    float py = 1.0f;
#pragma unroll
    for (int c = 0; c < CMAX; ++c)
      if (c < C) {
        const float p = x[c] / se;
        if (probs) probs[col + (size_t)c * HW] = p;
        if ((int64_t)c == lab) py = p;
      }
    if (slu_label_in_range(lab, C)) local += (double)(-logf(fmaxf(py, clampv)));
  }
  slu_stage_wave_total(wave_sum(local), s_part);
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(nll_sum, slu_block_total(s_part));
}

// the kernel's KIND template argument for a runtime `kind`: f receives it as a std::integral_constant
template <class F>
int with_nll_kind(int kind, F&& f) {
  switch (kind) {
    case kLogits: return f(std::integral_constant<int, kLogits>{});
    case kProbsClamp: return f(std::integral_constant<int, kProbsClamp>{});
    case kProbsEps: return f(std::integral_constant<int, kProbsEps>{});
    case kLogProbs: return f(std::integral_constant<int, kLogProbs>{});
  }
  return SLU_EUNSUPPORTED;
}

}  // namespace

extern "C" int slu_nll_fwd(const float* x, const int64_t* labels, int B, int C, int HW, int kind, float param, int64_t ignore_index,
                           double* nll_sum, int64_t* count, slu_stream_t stream) {
  if (!x || !labels || !nll_sum || !count || B <= 0 || C <= 0 || HW <= 0) return SLU_EINVAL;
  if (C > 32) return SLU_EUNSUPPORTED;
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(count);
  const unsigned g = slu_grid_1d((size_t)B * HW, 2048);
  return with_nll_kind(kind, [&](auto k) {
    slu_class_cap(C, [&](auto cmax) {
      hipLaunchKernelGGL((nll_fwd_kernel<decltype(cmax)::value, decltype(k)::value>), dim3(g), dim3(256), 0, slu_stream(stream), x, labels, B, C, HW,
                         param, ignore_index, nll_sum, cnt);
    });
    SLU_CHECK_LAUNCH();
  });
}

extern "C" int slu_nll_bwd(const float* x, const int64_t* labels, int B, int C, int HW, int kind, float param, int64_t ignore_index,
                           const float* gscale, float* grad_x, slu_stream_t stream) {
  if (!x || !labels || !gscale || !grad_x || B <= 0 || C <= 0 || HW <= 0) return SLU_EINVAL;
  if (C > 32) return SLU_EUNSUPPORTED;
  const unsigned g = slu_grid_per_pixel((size_t)B * HW);
  return with_nll_kind(kind, [&](auto k) {
    slu_class_cap(C, [&](auto cmax) {
      hipLaunchKernelGGL((nll_bwd_kernel<decltype(cmax)::value, decltype(k)::value>), dim3(g), dim3(256), 0, slu_stream(stream), x, labels, B, C, HW,
                         param, ignore_index, gscale, grad_x);
    });
    SLU_CHECK_LAUNCH();
  });
}

extern "C" int slu_softmax_nll_fwd(const float* logits, const int64_t* labels, int B, int C, int HW, float clampv, float* probs,
                                   double* nll_sum, slu_stream_t stream) {
  if (!logits || !labels || !nll_sum || B <= 0 || C <= 0 || HW <= 0) return SLU_EINVAL;
  if (C > 32) return SLU_EUNSUPPORTED;
  const unsigned g = slu_grid_1d((size_t)B * HW, 2048);
  slu_class_cap(C, [&](auto cmax) {
    hipLaunchKernelGGL(softmax_nll_kernel<decltype(cmax)::value>, dim3(g), dim3(256), 0, slu_stream(stream), logits, labels, B, C, HW, clampv, probs,
                       nll_sum);
  });
  SLU_CHECK_LAUNCH();
}

extern "C" int slu_softmax_loss_bwd(const float* probs, const int64_t* labels, const float* dense, float w_dense, float w_nll,
                                    float clampv, const float* gout, int B, int C, int HW, float* grad_logits, slu_stream_t stream) {
  if (!probs || !grad_logits || B <= 0 || C <= 0 || HW <= 0) return SLU_EINVAL;
  if (C > 32) return SLU_EUNSUPPORTED;
  const unsigned g = slu_grid_per_pixel((size_t)B * HW);
  slu_class_cap(C, [&](auto cmax) {
    hipLaunchKernelGGL(softmax_loss_bwd_kernel<decltype(cmax)::value>, dim3(g), dim3(256), 0, slu_stream(stream), probs, labels, dense, w_dense, w_nll,
                       clampv, gout, B, C, HW, grad_logits);
  });
  SLU_CHECK_LAUNCH();
}
