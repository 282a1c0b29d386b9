// AUROC of error detection on gfx950 (replaces src/metrics/auroc.py:36-78 of the reference).
//
//   score kernel   per pixel: probabilities by mode (alpha / logits / probs, auroc.py:36-45), argmax, the uncertainty score
//                  (entropy, entropy_norm, 1-maxprob; Dirichlet mutual information for mode alpha, :47-63), validity.
//   AUROC          the reference sorts the samples by score (descending), takes cumulative sums and integrates TPR over FPR
//                  with the trapezoid rule (:65-78).  A negative sample at sorted position i advances FPR by 1/N at height
//                  TPR_i = (#positives before i) / P and a positive one advances nothing, so
//                      AUROC = sum over negatives of (#positives ranked before it) / (P N)        -- exact integers.
//                  The samples are one segment of the radix sort of radix_sort.h (key = KeyDescending of the score, value =
//                  index | error << 31); the order among equal scores is arbitrary, as it is for numpy's argsort in the reference.
#include "class_column.h"
#include "radix_sort.h"

namespace {

using namespace slu_sort;

// mode: 0 alpha, 1 logits, 2 probs.  kind: 0 entropy, 1 entropy_norm, 2 mi, 3 mi_norm, 4 1-maxprob.
// flag: 0 correct, 1 error, 2 not valid (label == ignore_index)
template <int CMAX>
__global__ __launch_bounds__(256) void auroc_score_kernel(const float* __restrict__ preds, const int64_t* __restrict__ labels,
                                                          const float* __restrict__ score_override, int B, int C, int HW, int mode, int kind,
                                                          int has_ignore, int64_t ignore, float eps, float* __restrict__ score_out,
                                                          uint8_t* __restrict__ flag_out) {
  const size_t npix = (size_t)B * HW;
  const size_t pix = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (pix >= npix) return;
  // the three-mode block is written out here and not taken from slu_mode_column (class_column.h), which ece_samples_kernel uses: same
  // bits, but this kernel ran 5 % longer with it (profiles/r18)
  const float* src = preds + slu_pixel(pix, C, HW).col;
  float x[CMAX], p[CMAX];
  float sum = 0.0f;
  const float m = slu_load_column(src, C, HW, mode == 1 ? -INFINITY : 0.0f, x);
  if (mode == 1) {
#pragma unroll
    for (int c = 0; c < CMAX; ++c)
      if (c < C) { p[c] = expf(x[c] - m); sum += p[c]; }
#pragma unroll
    for (int c = 0; c < CMAX; ++c) p[c] = c < C ? p[c] / sum : 0.0f;
  } else if (mode == 0) {
#pragma unroll
    for (int c = 0; c < CMAX; ++c)
      if (c < C) sum += x[c];
#pragma unroll
    for (int c = 0; c < CMAX; ++c) p[c] = c < C ? x[c] / (sum + eps) : 0.0f;
  } else {
#pragma unroll
    for (int c = 0; c < CMAX; ++c)
      if (c < C) { p[c] = fmaxf(x[c], 0.0f); sum += p[c]; }
    const float d = fmaxf(sum, eps);
#pragma unroll
    for (int c = 0; c < CMAX; ++c) p[c] = c < C ? p[c] / d : 0.0f;
  }
  float best;
  const int arg = slu_first_argmax(p, C, best);
  float score;
  if (score_override) {
    score = score_override[pix];
  } else if (kind == 4) {
    score = 1.0f - best;
  } else if (mode == 0 && (kind == 2 || kind == 3)) {
    // Dirichlet mutual information (auroc.py:55-63): note alpha0 carries eps here, unlike the probabilities above
    const float a0 = sum + eps;
    const float dg0 = digamma_ge1(a0 + 1.0f);
    float h = 0.0f, eh = 0.0f;
#pragma unroll
    for (int c = 0; c < CMAX; ++c)
      if (c < C) {
        const float q = x[c] / a0;
        const float qc = fmaxf(q, eps);
        h -= qc * logf(qc);
        eh -= q * (digamma_ge1(x[c] + 1.0f) - dg0);
      }
    score = h - eh;
    if (kind == 3) score /= logf((float)C);
  } else {
    float h = 0.0f;
#pragma unroll
    for (int c = 0; c < CMAX; ++c)
      if (c < C) {
        const float qc = fmaxf(p[c], eps);
        h -= qc * logf(qc);
      }
    score = (kind == 1) ? h / logf((float)C) : h;       // every other kind falls through to the plain entropy (auroc.py:53)
  }
  const int64_t lab = labels[pix];
  const bool valid = !slu_label_ignored(lab, has_ignore, ignore);      // a label outside [0, C) stays: it counts as an error
  score_out[pix] = score;
  flag_out[pix] = valid ? (uint8_t)(arg != lab ? 1 : 0) : (uint8_t)2;
}

// after the sort: sum over negatives of the number of positives ranked before them (exact, 64-bit)
__global__ __launch_bounds__(kThreads) void auroc_sum_kernel(const unsigned* __restrict__ vals, long long n, const unsigned* __restrict__ blkfg,
                                                             unsigned long long* __restrict__ total) {
  constexpr int kWaves = kThreads / 64;
  __shared__ unsigned s_w[kWaves];
  __shared__ unsigned long long s_sum[kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, blk = blockIdx.x;
  // a wave owns kItems consecutive 64-element rows of the tile (sorted order == (wave, item, lane))
  const long long base = (long long)blk * kTile + (long long)wave * (kItems * 64);
  unsigned fg[kItems];
  unsigned cnt = 0;
#pragma unroll
  for (int it = 0; it < kItems; ++it) {
    const long long i = base + it * 64 + lane;
    fg[it] = i < n ? val_flag(vals[i]) : 0u;
    cnt += (unsigned)__popcll(__ballot(fg[it]));
  }
  if (lane == 0) s_w[wave] = cnt;
  __syncthreads();
  unsigned before = blkfg[blk];
  for (int w = 0; w < wave; ++w) before += s_w[w];
  const unsigned long long lt = lanes_below(lane);
  unsigned long long acc = 0;
#pragma unroll
  for (int it = 0; it < kItems; ++it) {
    const long long i = base + it * 64 + lane;
    const unsigned long long m = __ballot(fg[it]);
    if (i < n && !fg[it]) acc += before + (unsigned)__popcll(m & lt);
    before += (unsigned)__popcll(m);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if (lane == 0) s_sum[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long t = 0;
    for (int w = 0; w < kWaves; ++w) t += s_sum[w];
    if (t) atomicAdd(total, t);
  }
}

__global__ void auroc_finalize_kernel(const unsigned long long* __restrict__ total, const unsigned* __restrict__ blkfg, const unsigned* __restrict__ vals,
                                      long long n, int nblk, double* __restrict__ out) {
  // positives = exclusive prefix of the last tile + its own count
  unsigned long long pos = blkfg[nblk - 1];
  for (long long i = (long long)(nblk - 1) * kTile; i < n; ++i) pos += val_flag(vals[i]);
  const double P = (double)pos, N = (double)(n - (long long)pos);
  out[1] = P;
  out[2] = N;
  out[0] = (pos == 0 || (long long)pos == n) ? (double)NAN : (double)*total / (P * N);
}

struct AurocWs {
  unsigned* one;                  // the sort's "segments to sort" word, written by the keygen
  unsigned long long* total;
  SluSortWs sort;
};

size_t carve(char* base, long long n, AurocWs& ws) {
  SluCarver cv{base};
  ws.one = cv.take<unsigned>(1);
  ws.total = cv.take<unsigned long long>(1);
  slu_sort_carve(cv, n, 1, ws.sort);
  return cv.off;
}

}  // namespace

extern "C" int slu_auroc_scores(const float* preds, const int64_t* labels, const float* score_override, int B, int C, int HW, int mode, int score_kind,
                                int has_ignore, int64_t ignore_index, float eps, float* scores, uint8_t* flags, slu_stream_t stream) {
  if (!preds || !labels || !scores || !flags || B <= 0 || C <= 0 || HW <= 0) return SLU_EINVAL;
  if (mode < 0 || mode > 2 || score_kind < 0 || score_kind > 4) return SLU_EINVAL;
  if (C > 32) return SLU_EUNSUPPORTED;
  const unsigned nb = slu_grid_per_pixel((size_t)B * HW);
  slu_class_cap(C, [&](auto cmax) {
    hipLaunchKernelGGL(auroc_score_kernel<decltype(cmax)::value>, dim3(nb), dim3(256), 0, slu_stream(stream), preds, labels, score_override, B, C, HW,
                       mode, score_kind, has_ignore, ignore_index, eps, scores, flags);
  });
  SLU_CHECK_LAUNCH();
}

extern "C" size_t slu_auroc_workspace_bytes(long long n) {
  if (n <= 0) return 0;
  AurocWs ws;
  return carve(nullptr, n, ws);
}

extern "C" int slu_auroc_compute(const float* scores, const uint8_t* is_error, long long n, void* workspace, size_t workspace_bytes, double* out3,
                                 float* sorted_scores, uint8_t* sorted_is_error, slu_stream_t stream) {
  if (!scores || !is_error || !workspace || !out3 || n <= 0) return SLU_EINVAL;
  if (n >= (1ll << 31)) return SLU_EUNSUPPORTED;
  if ((sorted_scores == nullptr) != (sorted_is_error == nullptr)) return SLU_EINVAL;
  AurocWs ws;
  if (carve((char*)workspace, n, ws) > workspace_bytes) return SLU_EINVAL;
  if (reinterpret_cast<uintptr_t>(workspace) & 255) return SLU_EINVAL;
  hipStream_t st = slu_stream(stream);
  const int nblk = nblk_of(n);
  const SluSortWs& s = ws.sort;
  if (hipMemsetAsync(ws.total, 0, sizeof(unsigned long long), st) != hipSuccess) return SLU_ELAUNCH;
  const unsigned kg = slu_grid_1d(n, 1024);
  hipLaunchKernelGGL(sample_keygen_kernel<KeyDescending>, dim3(kg), dim3(kThreads), 0, st, scores, is_error, n, s.keys[0], s.vals[0], ws.one);
  slu_sort_pairs(s, n, 1, ws.one, st);
  slu_sort_flag_prefix(s, n, 1, ws.one, st);
  hipLaunchKernelGGL(auroc_sum_kernel, dim3(nblk), dim3(kThreads), 0, st, s.vals[0], n, s.blkflag, ws.total);
  hipLaunchKernelGGL(auroc_finalize_kernel, dim3(1), dim3(1), 0, st, ws.total, s.blkflag, s.vals[0], n, nblk, out3);
  if (sorted_scores)      // the sorted sample list (descending score) for ROC curves: undo the key transform, keep the error flag
    hipLaunchKernelGGL(sample_unsort_kernel<KeyDescending>, dim3(kg), dim3(kThreads), 0, st, s.keys[0], s.vals[0], n, sorted_scores, sorted_is_error);
  SLU_CHECK_LAUNCH();
}
