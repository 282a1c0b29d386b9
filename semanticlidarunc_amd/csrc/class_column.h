// The "one lane owns one pixel, the class axis lives in registers" idiom of the per-pixel loss / metric / uncertainty kernels
// (loss, tversky, dirichlet, dirichlet_loss, metrics, uncertainty and the sample kernels of auroc / aurc), each piece stated once.
// A [B, C, HW] fp32 tensor is read one class column per lane; lanes of a wave are azimuth-adjacent, so every load and store is a
// 256-byte row segment; C <= CMAX (20 or 32, slu_class_cap) and every loop over the class axis is fully unrolled, so the column
// stays in registers.  Every helper keeps the operation order its callers had: class order for sums, strict > for the argmax.
#pragma once
#include <limits.h>
#include "slu_common.h"

// ---- host: launch shapes ----------------------------------------------------------------------------------------------------------------
// blocks of a kernel that has one thread per pixel and no grid-stride loop: all of them (a grid-stride kernel caps with slu_grid_1d itself)
static inline unsigned slu_grid_per_pixel(size_t npix) { return slu_grid_1d(npix, UINT_MAX); }

// ---- pixel split ------------------------------------------------------------------------------------------------------------------------
// pixel index -> image b, offset hw inside the image, and col = offset of the pixel's class-0 value in a contiguous [B, C, HW] tensor
// (class c is at col + c * HW).  HW and b fit an int (the entry points take them as int); col does not have to.
struct SluPixel {
  int b, hw;
  size_t col;
};
__device__ __forceinline__ SluPixel slu_pixel(size_t pix, int C, int HW) {
  const int b = (int)(pix / HW);
  const int hw = (int)(pix - (size_t)b * HW);
  return {b, hw, (size_t)b * C * (size_t)HW + hw};
}

// ---- the column -------------------------------------------------------------------------------------------------------------------------
// x[c] = src[c * HW] for c < C and `pad` above; returns the maximum over all CMAX entries, so a caller that wants the maximum of the
// column pads with -inf (a caller that pads with 0 does not use it).
template <int CMAX>
__device__ __forceinline__ float slu_load_column(const float* __restrict__ src, int C, size_t HW, float pad, float (&x)[CMAX]) {
  float m = -INFINITY;
#pragma unroll
  for (int c = 0; c < CMAX; ++c) {
    x[c] = c < C ? src[c * HW] : pad;
    m = fmaxf(m, x[c]);
  }
  return m;
}

// sum_c exp(x[c] - m) over c < C, in class order; m is the column's maximum, so every term is <= 1 and one of them is 1.
// The log-sum-exp form (p = exp(x - m - log se): uncertainty.hip, as the reference's exp(log_softmax)) keeps x.
template <int CMAX>
__device__ __forceinline__ float slu_exp_sum(const float (&x)[CMAX], int C, float m) {
  float se = 0.0f;
#pragma unroll
  for (int c = 0; c < CMAX; ++c)
    if (c < C) se += expf(x[c] - m);
  return se;
}

// the same sum, with x[c] = exp(x[c] - m) left behind for c < C (entries above keep their pad): the p = e / se form
template <int CMAX>
__device__ __forceinline__ float slu_exp_sum_inplace(float (&x)[CMAX], int C, float m) {
  float se = 0.0f;
#pragma unroll
  for (int c = 0; c < CMAX; ++c)
    if (c < C) {
      x[c] = expf(x[c] - m);
      se += x[c];
    }
  return se;
}

// First maximum of v[0 .. C), like torch.argmax / np.argmax off NaNs: the comparison is strict, so the lowest index wins a tie.
// `best` starts at -inf: a column of -inf or NaN gives index 0.
template <int CMAX>
__device__ __forceinline__ int slu_first_argmax(const float (&v)[CMAX], int C, float& best) {
  best = -INFINITY;
  int arg = 0;
#pragma unroll
  for (int c = 0; c < CMAX; ++c)
    if (c < C && v[c] > best) {
      best = v[c];
      arg = c;
    }
  return arg;
}

// Probabilities of the ECE front ends by mode (metrics/ece.py:55-67), unnormalised: returns den with p_c = x[c] / den for c < C.
// 0 alpha: x = alpha, den = sum + eps.   1 logits: x = exp(logit - max), den = sum.   2 probs: x = max(p, 0), den = max(sum, eps).
// Entries c >= C hold -inf.  auroc_score_kernel computes the same values (metrics/auroc.py:36-45) from a written-out copy: it was
// measured 5 % slower on this helper.
template <int CMAX>
__device__ __forceinline__ float slu_mode_column(const float* __restrict__ src, int C, size_t HW, int mode, float eps, float (&x)[CMAX]) {
  const float m = slu_load_column(src, C, HW, -INFINITY, x);
  if (mode == 1) return slu_exp_sum_inplace(x, C, m);
  float s = 0.0f;
#pragma unroll
  for (int c = 0; c < CMAX; ++c)
    if (c < C) {
      if (mode == 2) x[c] = fmaxf(x[c], 0.0f);
      s += x[c];
    }
  return mode == 0 ? s + eps : fmaxf(s, eps);
}

// ---- label predicates -------------------------------------------------------------------------------------------------------------------
// Which pixels count differs from kernel to kernel on purpose: each mirrors its own line of the reference.  The rules are composed
// from these at the call site and not merged:
//   nll_fwd / nll_bwd           !ignore(sentinel) && in range           tversky, dirichlet_loss     in range && !ignore(flag)
//   ece_kernel, aurc_sample     !ignore(sentinel); out of range = wrong  ece_samples, auroc_score   !ignore(flag); out of range = wrong
//   softmax_nll                 in range
__device__ __forceinline__ bool slu_label_in_range(int64_t y, int C) { return y >= 0 && y < C; }
// sentinel form: the caller without an ignore value passes INT64_MIN, which no label carries
__device__ __forceinline__ bool slu_label_ignored(int64_t y, int64_t ignore) { return y == ignore; }
// flag form: `ignore` means something only where has_ignore is set
__device__ __forceinline__ bool slu_label_ignored(int64_t y, int has_ignore, int64_t ignore) { return has_ignore && y == ignore; }

// ---- digamma / trigamma -----------------------------------------------------------------------------------------------------------------
// psi(x) = psi(x + 1) - 1 / x up to x >= 6, then the asymptotic series (|err| < 2e-7 relative there).  Two of them because the
// arguments differ: the uncertainty measures evaluate psi at alpha + 1 and alpha0 + 1 with alpha >= 1, i.e. x >= 1, which five steps
// bring to 6; the losses evaluate it at alpha itself (and at the eps-clamped alpha~ of the KL terms), any x > 0, which needs a sixth.
// For x >= 1 the two agree bit for bit; the kernels keep the one they had.
__device__ __forceinline__ float slu_digamma_steps(float x, int steps) {
  float r = 0.0f;
#pragma unroll
  for (int i = 0; i < steps; ++i)
    if (x < 6.0f) {
      r -= 1.0f / x;
      x += 1.0f;
    }
  const float inv = 1.0f / x, inv2 = inv * inv;
  return r + logf(x) - 0.5f * inv - inv2 * (1.0f / 12.0f - inv2 * (1.0f / 120.0f - inv2 * (1.0f / 252.0f)));
}
__device__ __forceinline__ float digamma_ge1(float x) { return slu_digamma_steps(x, 5); }      // x >= 1
__device__ __forceinline__ float digamma_pos(float x) { return slu_digamma_steps(x, 6); }      // x > 0

__device__ __forceinline__ float trigamma_pos(float x) {      // x > 0: psi'(x) = psi'(x + 1) + 1 / x^2; asymptotic series for x >= 6
  float r = 0.0f;
#pragma unroll
  for (int i = 0; i < 6; ++i)
    if (x < 6.0f) {
      r += 1.0f / (x * x);
      x += 1.0f;
    }
  const float inv = 1.0f / x, inv2 = inv * inv;
  return r + inv * (1.0f + 0.5f * inv + inv2 * (1.0f / 6.0f - inv2 * (1.0f / 30.0f - inv2 * (1.0f / 42.0f))));
}

// ---- block reduction of the summing kernels ---------------------------------------------------------------------------------------------
// 256 threads = 4 waves.  Every thread calls slu_stage_wave_total with its wave's total (wave_sum: the xor butterfly, all lanes hold
// it) for each quantity, the block synchronises once, and thread 0 adds the four wave totals in wave order with slu_block_total
// and issues the one atomic per quantity: inside a block the order is fixed, so a one-block launch gives the same bits every run.
template <class T>
__device__ __forceinline__ void slu_stage_wave_total(T wave_total, T (&s_part)[4]) {
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = wave_total;
}
template <class T>
__device__ __forceinline__ T slu_block_total(const T (&s_part)[4]) {
  T t = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) t += s_part[w];
  return t;
}
