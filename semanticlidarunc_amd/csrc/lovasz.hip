// Lovasz-Softmax on gfx950 (replaces src/losses/lovasz.py:12-88 of the reference).
//
//   for every class c present among the valid labels:
//       err_i = | 1[y_i == c] - p_c,i |            (valid pixels; ignored pixels are dropped)
//       sort err descending, fg in the same order, J_k = 1 - (G - cumfg_k) / (G + k - cumfg_k)
//       loss_c = sum_k err_(k) * (J_k - J_{k-1})
//   loss = mean over present classes
//
// Device formulation.  Ignored pixels are kept in place with err = 0 / fg = 0: they sort behind every
// positive error, so they change no J_k that multiplies a non-zero error -- the value is identical and
// no compaction pass is needed.  All classes are sorted at once: a batched LSD radix sort (4 x 8 bit)
// over [C][N] (key = 0x3F800000 - bits(err), i.e. ascending key == descending err in [0,1]; value =
// pixel index | fg << 31).  Per pass: per-tile digit histograms -> one exclusive scan per class ->
// stable scatter (the rank of an element inside its wave comes from 8 ballots over the digit bits,
// 64-lane waves; per-wave digit counters in LDS).  Classes with no foreground exit every kernel at once.
// After the sort one kernel scans the fg bits, forms J_k in fp32 exactly like the reference
// (1 - inter/union, both exact integers in fp32), accumulates loss_c in fp64 and scatters
// d loss / d p_c,i = (J_k - J_{k-1}) * (fg ? -1 : +1) back to pixel order (0 where err == 0).
// The radix passes are stable, so equal errors keep their pixel order: the gradient is the same run to run, and over a group
// of equal errors it sums to J(after the group) - J(before the group) whatever the order inside the group.
//
// Unlike the reference, keygen_kernel clamps err to [0, 1] (the key transform needs that range) and fminf/fmaxf map a NaN
// error to 0: a NaN or out-of-range probability gives a finite loss and a zero gradient at that pixel where the reference
// would propagate it.
//
// HBM-bound: ~ 4 passes x (8 B read for the histogram + 8 B read + 8 B written by the scatter) per key.
#include "slu_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kItems = 8;                       // keys per thread per tile
constexpr int kTile = kThreads * kItems;        // 2048 keys per workgroup
constexpr unsigned kOne = 0x3F800000u;          // bits(1.0f)

struct Ws {
  unsigned* keys[2];
  unsigned* vals[2];
  unsigned* hist;      // [C][256][nblk]
  unsigned* G;         // [C] foreground count per class (valid pixels)
  unsigned* blkfg;     // [C][nblk]
  double* loss_c;      // [C]
  unsigned* act;       // [C] 1 = the class is summed whether or not it is present (classes='all' / an explicit list); unused for 'present'
};

__host__ __device__ inline int nblk_of(long long n) { return (int)((n + kTile - 1) / kTile); }

// ---- keys / values / per-class foreground counts -------------------------------------------------
__global__ __launch_bounds__(kThreads) void keygen_kernel(const float* __restrict__ probs, const int64_t* __restrict__ labels,
                                                          int B, int C, int HW, int64_t ignore, unsigned* __restrict__ keys,
                                                          unsigned* __restrict__ vals, unsigned* __restrict__ G) {
  __shared__ unsigned s_cnt[32];
  const int c = blockIdx.y;
  if (threadIdx.x < 32) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const long long N = (long long)B * HW;
  unsigned local = 0;
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < N; i += (long long)gridDim.x * kThreads) {
    const int64_t y = labels[i];
    const int b = (int)(i / HW);
    const int hw = (int)(i - (long long)b * HW);
    const float p = probs[((size_t)b * C + c) * HW + hw];
    const bool valid = y != ignore;
    const bool fg = valid && y == c;
    float err = valid ? fabsf((fg ? 1.0f : 0.0f) - p) : 0.0f;
    err = fminf(fmaxf(err, 0.0f), 1.0f);
    keys[(size_t)c * N + i] = kOne - __float_as_uint(err);
    vals[(size_t)c * N + i] = (unsigned)i | (fg ? 0x80000000u : 0u);
    local += fg ? 1u : 0u;
  }
  local = (unsigned)wave_sum((float)local);     // <= 64 * iterations, exact in fp32 for any sane grid
  if ((threadIdx.x & 63) == 0 && local) atomicAdd(&s_cnt[0], local);
  __syncthreads();
  if (threadIdx.x == 0 && s_cnt[0]) atomicAdd(&G[c], s_cnt[0]);
}

// ---- radix pass: histogram ------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void hist_kernel(const unsigned* __restrict__ keys, long long N, int nblk, int shift,
                                                        const unsigned* __restrict__ G, unsigned* __restrict__ hist) {
  const int c = blockIdx.y, blk = blockIdx.x;
  if (G[c] == 0) return;
  __shared__ unsigned s_h[256];
  s_h[threadIdx.x] = 0;
  __syncthreads();
  const long long base = (long long)blk * kTile;
  const unsigned* k = keys + (size_t)c * N;
#pragma unroll
  for (int it = 0; it < kItems; ++it) {
    const long long i = base + it * kThreads + threadIdx.x;
    if (i < N) atomicAdd(&s_h[(k[i] >> shift) & 255u], 1u);
  }
  __syncthreads();
  hist[((size_t)c * nblk + blk) * 256 + threadIdx.x] = s_h[threadIdx.x];      // [class][tile][digit]: the scan reads 1 KB rows
}

// ---- radix pass: exclusive scan over (digit, tile) of one class (one workgroup per class) ---------
__global__ __launch_bounds__(256) void scan_kernel(unsigned* __restrict__ hist, int nblk, const unsigned* __restrict__ G) {
  const int c = blockIdx.x;
  if (G[c] == 0) return;
  __shared__ unsigned s_tot[256];
  // thread = digit; the tiles of a digit are 1 KB apart, the 256 digits of a tile contiguous: every iteration is one coalesced row and the
  // rows are independent loads (the [digit][tile] layout made each thread walk its own 4-byte-strided column: 98 us per pass)
  unsigned* col = hist + (size_t)c * nblk * 256 + threadIdx.x;
  unsigned tot = 0;
#pragma unroll 8
  for (int b = 0; b < nblk; ++b) tot += col[(size_t)b * 256];
  s_tot[threadIdx.x] = tot;
  __syncthreads();
  if (threadIdx.x == 0) {          // 256 values: a serial scan is a few hundred cycles
    unsigned run = 0;
    for (int d = 0; d < 256; ++d) { const unsigned t = s_tot[d]; s_tot[d] = run; run += t; }
  }
  __syncthreads();
  unsigned run = s_tot[threadIdx.x];
#pragma unroll 8
  for (int b = 0; b < nblk; ++b) { const unsigned t = col[(size_t)b * 256]; col[(size_t)b * 256] = run; run += t; }
}

// ---- radix pass: stable scatter --------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void scatter_kernel(const unsigned* __restrict__ keys_in, const unsigned* __restrict__ vals_in,
                                                           unsigned* __restrict__ keys_out, unsigned* __restrict__ vals_out,
                                                           long long N, int nblk, int shift, const unsigned* __restrict__ G,
                                                           const unsigned* __restrict__ hist) {
  const int c = blockIdx.y, blk = blockIdx.x;
  if (G[c] == 0) return;
  constexpr int kWaves = kThreads / 64;
  __shared__ unsigned s_cnt[kWaves][256];       // running count of each digit inside each wave's slice
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < kWaves * 256; i += kThreads) (&s_cnt[0][0])[i] = 0;
  __syncthreads();
  // a wave owns kItems consecutive 64-key rows of the tile: key order == (wave, item, lane)
  const long long base = (long long)blk * kTile + (long long)wave * (kItems * 64);
  const size_t seg = (size_t)c * N;
  unsigned key[kItems], val[kItems], rank[kItems];
  const unsigned long long lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
#pragma unroll
  for (int it = 0; it < kItems; ++it) {
    const long long i = base + it * 64 + lane;
    const bool in = i < N;
    key[it] = in ? keys_in[seg + i] : 0xFFFFFFFFu;
    val[it] = in ? vals_in[seg + i] : 0u;
    const unsigned d = (key[it] >> shift) & 255u;
    unsigned long long peers = __ballot(in);
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
      const unsigned long long m = __ballot((d >> bit) & 1u);
      peers &= ((d >> bit) & 1u) ? m : ~m;
    }
    const unsigned before = (unsigned)__popcll(peers & lt);
    const unsigned old = in ? s_cnt[wave][d] : 0u;
    __builtin_amdgcn_wave_barrier();
    if (in && before == 0) s_cnt[wave][d] = old + (unsigned)__popcll(peers);    // lowest lane of each digit group
    __builtin_amdgcn_wave_barrier();
    rank[it] = old + before;
  }
  __syncthreads();
  // exclusive offsets of this wave's slice inside the tile, per digit (kWaves is 4: unrolled sum)
#pragma unroll
  for (int it = 0; it < kItems; ++it) {
    const long long i = base + it * 64 + lane;
    if (i < N) {
      const unsigned d = (key[it] >> shift) & 255u;
      unsigned off = hist[((size_t)c * nblk + blk) * 256 + d];
#pragma unroll
      for (int w = 0; w < kWaves; ++w)
        if (w < wave) off += s_cnt[w][d];
      const size_t o = seg + off + rank[it];
      keys_out[o] = key[it];
      vals_out[o] = val[it];
    }
  }
}

// ---- after the sort: per-tile foreground counts, then Jaccard steps / loss / gradient scatter -------
__global__ __launch_bounds__(kThreads) void fgcount_kernel(const unsigned* __restrict__ vals, long long N, int nblk,
                                                           const unsigned* __restrict__ G, unsigned* __restrict__ blkfg) {
  const int c = blockIdx.y, blk = blockIdx.x;
  if (G[c] == 0) return;
  __shared__ unsigned s_w[kThreads / 64];
  const long long base = (long long)blk * kTile;
  unsigned n = 0;
#pragma unroll
  for (int it = 0; it < kItems; ++it) {
    const long long i = base + it * kThreads + threadIdx.x;
    if (i < N) n += vals[(size_t)c * N + i] >> 31;
  }
  n = (unsigned)wave_sum((float)n);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned t = 0;
    for (int w = 0; w < kThreads / 64; ++w) t += s_w[w];
    blkfg[(size_t)c * nblk + blk] = t;
  }
}

__global__ __launch_bounds__(256) void fgscan_kernel(unsigned* __restrict__ blkfg, int nblk, const unsigned* __restrict__ G) {
  const int c = blockIdx.x;                    // serial exclusive scan over <= a few hundred tiles
  if (G[c] == 0 || threadIdx.x != 0) return;
  unsigned run = 0;
  unsigned* row = blkfg + (size_t)c * nblk;
  for (int b = 0; b < nblk; ++b) { const unsigned t = row[b]; row[b] = run; run += t; }
}

__device__ __forceinline__ float jaccard(unsigned G, unsigned long long k, unsigned cum) {
  // lovasz.py:31-33 : 1 - (gts - cumsum(fg)) / (gts + cumsum(1 - fg)), all exact integers in fp32
  return 1.0f - (float)(G - cum) / (float)(G + (unsigned)k - cum);
}

__global__ __launch_bounds__(kThreads) void lovasz_steps_kernel(const unsigned* __restrict__ keys, const unsigned* __restrict__ vals,
                                                                long long N, int nblk, const unsigned* __restrict__ G,
                                                                const unsigned* __restrict__ act, const unsigned* __restrict__ blkfg,
                                                                double* __restrict__ loss_c, float* __restrict__ grad /* [C][N] pixel order, or null */) {
  const int c = blockIdx.y, blk = blockIdx.x;
  // an ABSENT class that is summed anyway (g = 0, lovasz.py:66-69 with classes='all'): the Jaccard steps degenerate to (1, 0, 0, ...), the term is
  // the largest error = max p_c and its gradient +1 at that pixel -- the formulas below give exactly that with g = 0
  const unsigned g = G[c];
  if (act[c] == 0) return;
  __shared__ unsigned s_wave[kThreads / 64];
  __shared__ double s_part[kThreads / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // thread t owns kItems CONSECUTIVE sorted positions, so its prefix is one block scan of its fg total
  const long long first = (long long)blk * kTile + (long long)threadIdx.x * kItems;
  const size_t seg = (size_t)c * N;
  unsigned k_[kItems], v_[kItems];
  unsigned mine = 0;
#pragma unroll
  for (int it = 0; it < kItems; ++it) {
    const long long i = first + it;
    k_[it] = i < N ? keys[seg + i] : kOne;
    v_[it] = i < N ? vals[seg + i] : 0u;
    mine += v_[it] >> 31;
  }
  // exclusive scan of `mine` over the workgroup (wave shuffle scan + wave totals)
  unsigned incl = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned t = __shfl_up(incl, o, 64);
    if (lane >= o) incl += t;
  }
  if (lane == 63) s_wave[wave] = incl;
  __syncthreads();
  unsigned cum = blkfg[(size_t)c * nblk + blk] + incl - mine;
  for (int w = 0; w < wave; ++w) cum += s_wave[w];
  double part = 0.0;
#pragma unroll
  for (int it = 0; it < kItems; ++it) {
    const long long i = first + it;
    if (i < N) {
      const unsigned fg = v_[it] >> 31;
      const float j_prev = (i == 0) ? 0.0f : jaccard(g, (unsigned long long)i, cum);
      cum += fg;
      const float step = jaccard(g, (unsigned long long)i + 1, cum) - j_prev;
      const float err = __uint_as_float(kOne - k_[it]);
      part += (double)(err * step);
      if (grad) grad[seg + (v_[it] & 0x7FFFFFFFu)] = err > 0.0f ? (fg ? -step : step) : 0.0f;
    }
  }
  part = wave_sum(part);
  if (lane == 0) s_part[wave] = part;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int w = 0; w < kThreads / 64; ++w) t += s_part[w];
    atomicAdd(&loss_c[c], t);
  }
}

__global__ void lovasz_set_active_kernel(unsigned* __restrict__ act, int C, unsigned mask) {
  if ((int)threadIdx.x < C) act[threadIdx.x] = (mask >> threadIdx.x) & 1u;
}

// loss = mean over the summed classes (G = the activity flags: the foreground counts for 'present'); grad_probs[b][c][hw] = grad[c][b*HW+hw] / n (0 for the others)
__global__ void lovasz_finalize_kernel(const unsigned* __restrict__ G, const double* __restrict__ loss_c, int C,
                                       float* __restrict__ loss_out, float* __restrict__ n_present_out) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    double s = 0.0;
    int n = 0;
    for (int c = 0; c < C; ++c)
      if (G[c]) { s += loss_c[c]; ++n; }
    loss_out[0] = n ? (float)(s / n) : 0.0f;
    n_present_out[0] = (float)n;
  }
}

__global__ __launch_bounds__(256) void lovasz_grad_layout_kernel(const float* __restrict__ grad, const unsigned* __restrict__ G,
                                                                 const float* __restrict__ n_present, int B, int C, int HW,
                                                                 float* __restrict__ grad_probs) {
  const size_t total = (size_t)B * C * HW;
  const float inv = n_present[0] > 0.0f ? 1.0f / n_present[0] : 0.0f;
  const size_t N = (size_t)B * HW;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const int hw = (int)(e % HW);
    const size_t r = e / HW;
    const int c = (int)(r % C);
    const int b = (int)(r / C);
    grad_probs[e] = G[c] ? grad[(size_t)c * N + (size_t)b * HW + hw] * inv : 0.0f;
  }
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

size_t carve(char* base, long long N, int C, Ws* ws) {
  const int nblk = nblk_of(N);
  size_t off = 0;
  auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += align256(bytes); return p; };
  // zero-initialised block first (G, loss_c): one memset covers it
  char* g = take((size_t)C * sizeof(unsigned));
  char* l = take((size_t)C * sizeof(double));
  char* k0 = take((size_t)C * N * 4); char* k1 = take((size_t)C * N * 4);
  char* v0 = take((size_t)C * N * 4); char* v1 = take((size_t)C * N * 4);
  char* h = take((size_t)C * 256 * nblk * 4);
  char* bf = take((size_t)C * nblk * 4);
  char* ac = take((size_t)C * sizeof(unsigned));
  if (ws) {
    ws->G = (unsigned*)g; ws->loss_c = (double*)l; ws->act = (unsigned*)ac;
    ws->keys[0] = (unsigned*)k0; ws->keys[1] = (unsigned*)k1; ws->vals[0] = (unsigned*)v0; ws->vals[1] = (unsigned*)v1;
    ws->hist = (unsigned*)h; ws->blkfg = (unsigned*)bf;
  }
  return off;
}

}  // namespace

extern "C" size_t slu_lovasz_workspace_bytes(int B, int C, int HW) {
  if (B <= 0 || C <= 0 || HW <= 0) return 0;
  return carve(nullptr, (long long)B * HW, C, nullptr);
}

extern "C" int slu_lovasz_fwd(const float* probs, const int64_t* labels, int B, int C, int HW, int64_t ignore_index, unsigned class_mask,
                              void* workspace, size_t workspace_bytes, float* loss, float* n_present, float* grad_probs,
                              slu_stream_t stream) {
  if (!probs || !labels || !workspace || !loss || !n_present || B <= 0 || C <= 0 || HW <= 0) return SLU_EINVAL;
  const long long N = (long long)B * HW;
  if (N >= (1ll << 31) || C > 32) return SLU_EUNSUPPORTED;
  Ws ws;
  if (carve((char*)workspace, N, C, &ws) > workspace_bytes) return SLU_EINVAL;
  if (reinterpret_cast<uintptr_t>(workspace) & 255) return SLU_EINVAL;
  hipStream_t st = slu_stream(stream);
  const int nblk = nblk_of(N);
  if (hipMemsetAsync(ws.G, 0, align256((size_t)C * sizeof(unsigned)) + (size_t)C * sizeof(double), st) != hipSuccess) return SLU_ELAUNCH;
  const unsigned kg = (unsigned)((N + kThreads - 1) / kThreads > 1024 ? 1024 : (N + kThreads - 1) / kThreads);
  hipLaunchKernelGGL(keygen_kernel, dim3(kg, C), dim3(kThreads), 0, st, probs, labels, B, C, HW, ignore_index, ws.keys[0], ws.vals[0], ws.G);
  // which classes are sorted and summed: the present ones (flag = foreground count), or the caller's set whether present or not
  const unsigned* act = ws.G;
  if (class_mask) {
    hipLaunchKernelGGL(lovasz_set_active_kernel, dim3(1), dim3(64), 0, st, ws.act, C, class_mask);
    act = ws.act;
  }
  int cur = 0;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 8 * pass;
    hipLaunchKernelGGL(hist_kernel, dim3(nblk, C), dim3(kThreads), 0, st, ws.keys[cur], N, nblk, shift, act, ws.hist);
    hipLaunchKernelGGL(scan_kernel, dim3(C), dim3(256), 0, st, ws.hist, nblk, act);
    hipLaunchKernelGGL(scatter_kernel, dim3(nblk, C), dim3(kThreads), 0, st, ws.keys[cur], ws.vals[cur], ws.keys[cur ^ 1],
                       ws.vals[cur ^ 1], N, nblk, shift, act, ws.hist);
    cur ^= 1;
  }
  hipLaunchKernelGGL(fgcount_kernel, dim3(nblk, C), dim3(kThreads), 0, st, ws.vals[cur], N, nblk, act, ws.blkfg);
  hipLaunchKernelGGL(fgscan_kernel, dim3(C), dim3(256), 0, st, ws.blkfg, nblk, act);
  // per-pixel gradient (class-major, pixel order) reuses the idle value buffer
  float* gtmp = grad_probs ? reinterpret_cast<float*>(ws.keys[cur ^ 1]) : nullptr;
  hipLaunchKernelGGL(lovasz_steps_kernel, dim3(nblk, C), dim3(kThreads), 0, st, ws.keys[cur], ws.vals[cur], N, nblk, ws.G, act, ws.blkfg,
                     ws.loss_c, gtmp);
  hipLaunchKernelGGL(lovasz_finalize_kernel, dim3(1), dim3(64), 0, st, act, ws.loss_c, C, loss, n_present);
  if (grad_probs) {
    const size_t total = (size_t)B * C * HW;
    const unsigned g = (unsigned)((total + 255) / 256 > 8192 ? 8192 : (total + 255) / 256);
    hipLaunchKernelGGL(lovasz_grad_layout_kernel, dim3(g), dim3(256), 0, st, gtmp, act, n_present, B, C, HW, grad_probs);
  }
  SLU_CHECK_LAUNCH();
}

// =====================================================================================================================
// AUROC of error detection (replaces src/metrics/auroc.py:36-78 of the reference).
//
//   score kernel   per pixel: probabilities by mode (alpha / logits / probs, auroc.py:36-45), argmax, the uncertainty score
//                  (entropy, entropy_norm, 1-maxprob; Dirichlet mutual information for mode alpha, :47-63), validity.
//   AUROC          the reference sorts the samples by score (descending), takes cumulative sums and integrates TPR over FPR
//                  with the trapezoid rule (:65-78).  A negative sample at sorted position i advances FPR by 1/N at height
//                  TPR_i = (#positives before i) / P and a positive one advances nothing, so
//                      AUROC = sum over negatives of (#positives ranked before it) / (P N)        -- exact integers.
//                  The samples go through the same batched LSD radix sort as the Lovasz loss (one "class"); the order among
//                  equal scores is arbitrary, as it is for numpy's argsort in the reference.
// =====================================================================================================================
namespace {

__device__ __forceinline__ float digamma_ge1_f(float x) {      // x >= 1: recurrence to x >= 6, then the asymptotic series
  float r = 0.0f;
#pragma unroll
  for (int i = 0; i < 5; ++i)
    if (x < 6.0f) { r -= 1.0f / x; x += 1.0f; }
  const float inv = 1.0f / x, inv2 = inv * inv;
  return r + logf(x) - 0.5f * inv - inv2 * (1.0f / 12.0f - inv2 * (1.0f / 120.0f - inv2 * (1.0f / 252.0f)));
}

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
  const int b = (int)(pix / HW);
  const int hw = (int)(pix - (size_t)b * HW);
  const float* src = preds + (size_t)b * C * HW + hw;
  float x[CMAX], p[CMAX];
  float m = -INFINITY, sum = 0.0f;
#pragma unroll
  for (int c = 0; c < CMAX; ++c) {
    x[c] = c < C ? src[(size_t)c * HW] : (mode == 1 ? -INFINITY : 0.0f);
    m = fmaxf(m, x[c]);
  }
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
  float best = -INFINITY;
  int arg = 0;
#pragma unroll
  for (int c = 0; c < CMAX; ++c)
    if (c < C && p[c] > best) { best = p[c]; arg = c; }
  float score;
  if (score_override) {
    score = score_override[pix];
  } else if (kind == 4) {
    score = 1.0f - best;
  } else if (mode == 0 && (kind == 2 || kind == 3)) {
    // Dirichlet mutual information (auroc.py:55-63): note alpha0 carries eps here, unlike the probabilities above
    const float a0 = sum + eps;
    const float dg0 = digamma_ge1_f(a0 + 1.0f);
    float h = 0.0f, eh = 0.0f;
#pragma unroll
    for (int c = 0; c < CMAX; ++c)
      if (c < C) {
        const float q = x[c] / a0;
        const float qc = fmaxf(q, eps);
        h -= qc * logf(qc);
        eh -= q * (digamma_ge1_f(x[c] + 1.0f) - dg0);
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
  const bool valid = !has_ignore || lab != ignore;
  score_out[pix] = score;
  flag_out[pix] = valid ? (uint8_t)(arg != lab ? 1 : 0) : (uint8_t)2;
}

// sort key: descending score == ascending key, any finite or infinite float (NaN sorts first)
__device__ __forceinline__ unsigned desc_key(float s) {
  const unsigned u = __float_as_uint(s);
  const unsigned asc = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ~asc;
}

__global__ __launch_bounds__(kThreads) void auroc_keygen_kernel(const float* __restrict__ scores, const uint8_t* __restrict__ is_err, long long n,
                                                                unsigned* __restrict__ keys, unsigned* __restrict__ vals, unsigned* __restrict__ G) {
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
    keys[i] = desc_key(scores[i]);
    vals[i] = (unsigned)i | (is_err[i] ? 0x80000000u : 0u);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) G[0] = 1u;          // the sort kernels skip "classes" whose count is 0
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
    fg[it] = i < n ? (vals[i] >> 31) : 0u;
    cnt += (unsigned)__popcll(__ballot(fg[it]));
  }
  if (lane == 0) s_w[wave] = cnt;
  __syncthreads();
  unsigned before = blkfg[blk];
  for (int w = 0; w < wave; ++w) before += s_w[w];
  const unsigned long long lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
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
  for (long long i = (long long)(nblk - 1) * kTile; i < n; ++i) pos += vals[i] >> 31;
  const double P = (double)pos, N = (double)(n - (long long)pos);
  out[1] = P;
  out[2] = N;
  out[0] = (pos == 0 || (long long)pos == n) ? (double)NAN : (double)*total / (P * N);
}

__global__ __launch_bounds__(kThreads) void auroc_unsort_kernel(const unsigned* __restrict__ keys, const unsigned* __restrict__ vals, long long n,
                                                                float* __restrict__ scores, uint8_t* __restrict__ is_err) {
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
    const unsigned asc = ~keys[i];
    const unsigned m = (unsigned)((int)asc >> 31);                   // all ones for a non-negative score
    reinterpret_cast<unsigned*>(scores)[i] = asc ^ ~(m & 0x7FFFFFFFu);
    is_err[i] = (uint8_t)(vals[i] >> 31);
  }
}

size_t auroc_carve(char* base, long long n, Ws* ws, unsigned long long** total) {
  const int nblk = nblk_of(n);
  size_t off = 0;
  auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += align256(bytes); return p; };
  char* g = take(sizeof(unsigned));
  char* t = take(sizeof(unsigned long long));
  char* k0 = take((size_t)n * 4); char* k1 = take((size_t)n * 4);
  char* v0 = take((size_t)n * 4); char* v1 = take((size_t)n * 4);
  char* h = take((size_t)256 * nblk * 4);
  char* bf = take((size_t)nblk * 4);
  if (ws) {
    ws->G = (unsigned*)g; ws->loss_c = nullptr;
    ws->keys[0] = (unsigned*)k0; ws->keys[1] = (unsigned*)k1; ws->vals[0] = (unsigned*)v0; ws->vals[1] = (unsigned*)v1;
    ws->hist = (unsigned*)h; ws->blkfg = (unsigned*)bf;
    *total = (unsigned long long*)t;
  }
  return off;
}

}  // namespace

extern "C" int slu_auroc_scores(const float* preds, const int64_t* labels, const float* score_override, int B, int C, int HW, int mode, int score_kind,
                                int has_ignore, int64_t ignore_index, float eps, float* scores, uint8_t* flags, slu_stream_t stream) {
  if (!preds || !labels || !scores || !flags || B <= 0 || C <= 0 || HW <= 0) return SLU_EINVAL;
  if (mode < 0 || mode > 2 || score_kind < 0 || score_kind > 4) return SLU_EINVAL;
  if (C > 32) return SLU_EUNSUPPORTED;
  const size_t npix = (size_t)B * HW;
  const unsigned nb = (unsigned)((npix + 255) / 256);
  if (C <= 20)
    hipLaunchKernelGGL(auroc_score_kernel<20>, dim3(nb), dim3(256), 0, slu_stream(stream), preds, labels, score_override, B, C, HW, mode, score_kind,
                       has_ignore, ignore_index, eps, scores, flags);
  else
    hipLaunchKernelGGL(auroc_score_kernel<32>, dim3(nb), dim3(256), 0, slu_stream(stream), preds, labels, score_override, B, C, HW, mode, score_kind,
                       has_ignore, ignore_index, eps, scores, flags);
  SLU_CHECK_LAUNCH();
}

extern "C" size_t slu_auroc_workspace_bytes(long long n) {
  if (n <= 0) return 0;
  return auroc_carve(nullptr, n, nullptr, nullptr);
}

extern "C" int slu_auroc_compute(const float* scores, const uint8_t* is_error, long long n, void* workspace, size_t workspace_bytes, double* out3,
                                 float* sorted_scores, uint8_t* sorted_is_error, slu_stream_t stream) {
  if (!scores || !is_error || !workspace || !out3 || n <= 0) return SLU_EINVAL;
  if (n >= (1ll << 31)) return SLU_EUNSUPPORTED;
  if ((sorted_scores == nullptr) != (sorted_is_error == nullptr)) return SLU_EINVAL;
  Ws ws;
  unsigned long long* total = nullptr;
  if (auroc_carve((char*)workspace, n, &ws, &total) > workspace_bytes) return SLU_EINVAL;
  if (reinterpret_cast<uintptr_t>(workspace) & 255) return SLU_EINVAL;
  hipStream_t st = slu_stream(stream);
  const int nblk = nblk_of(n);
  if (hipMemsetAsync(ws.G, 0, align256(sizeof(unsigned)) + sizeof(unsigned long long), st) != hipSuccess) return SLU_ELAUNCH;
  const unsigned kg = (unsigned)((n + kThreads - 1) / kThreads > 1024 ? 1024 : (n + kThreads - 1) / kThreads);
  hipLaunchKernelGGL(auroc_keygen_kernel, dim3(kg), dim3(kThreads), 0, st, scores, is_error, n, ws.keys[0], ws.vals[0], ws.G);
  int cur = 0;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 8 * pass;
    hipLaunchKernelGGL(hist_kernel, dim3(nblk, 1), dim3(kThreads), 0, st, ws.keys[cur], n, nblk, shift, ws.G, ws.hist);
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(256), 0, st, ws.hist, nblk, ws.G);
    hipLaunchKernelGGL(scatter_kernel, dim3(nblk, 1), dim3(kThreads), 0, st, ws.keys[cur], ws.vals[cur], ws.keys[cur ^ 1], ws.vals[cur ^ 1], n, nblk,
                       shift, ws.G, ws.hist);
    cur ^= 1;
  }
  hipLaunchKernelGGL(fgcount_kernel, dim3(nblk, 1), dim3(kThreads), 0, st, ws.vals[cur], n, nblk, ws.G, ws.blkfg);
  hipLaunchKernelGGL(fgscan_kernel, dim3(1), dim3(256), 0, st, ws.blkfg, nblk, ws.G);
  hipLaunchKernelGGL(auroc_sum_kernel, dim3(nblk), dim3(kThreads), 0, st, ws.vals[cur], n, ws.blkfg, total);
  hipLaunchKernelGGL(auroc_finalize_kernel, dim3(1), dim3(1), 0, st, total, ws.blkfg, ws.vals[cur], n, nblk, out3);
  if (sorted_scores) {
    // the sorted sample list (descending score) for ROC curves: undo the key transform, keep the error flag
    hipLaunchKernelGGL(auroc_unsort_kernel, dim3(kg), dim3(kThreads), 0, st, ws.keys[cur], ws.vals[cur], n, sorted_scores, sorted_is_error);
  }
  SLU_CHECK_LAUNCH();
}

// =====================================================================================================================
// AURC / E-AURC of selective prediction (replaces src/metrics/aurc.py:7-45 of the reference; DESIGN "AURC on the device").
//
//   samples (conf fp32, err in {0,1}), sorted ascending by conf with the radix sort above (one "class"; key = ordered-uint
//   transform of conf with -0.0 folded into +0.0, value = index | err << 31).  The passes are stable: equal confidences keep
//   their sample order.  With e_i the inclusive error count at sorted position i and E = e_{n-1}:
//       group starts  S = { i in [0, n-2] : i == 0 or c_i != c_{i-1} } = s_1 < ... < s_m,  s_0 = -1
//       R_0 = E / n,  R_k = (E - e_{s_k}) / (n - 1 - s_k),  cov_0 = 1,  cov_k = (n - 1 - s_k) / n
//       AURC     = sum_k (R_{k-1} + R_k) / 2 * (s_k - s_{k-1}) / n  +  R_m (n - 2 - s_m) / n
//       AURC_opt = (1/n) sum_{j=1..E} j / (n - E + j)
//       recall_k = e_{m_k - 1} / max(E, 1),  m_k = max(1, int(n k / 100))
//   Counts are exact integers; R, the curve and the sums are fp64.  Nothing is accumulated with floating-point atomics:
//   every workgroup writes a partial and one workgroup adds the partials in a fixed order, so a result is the same bits
//   run to run.
//
//   after the sort:  fgcount / fgscan (errors per tile)  +  group starts per tile and their scan over tiles
//                    -> one pass: e_i and the rank of every group start, compacted (s_k, R_k [, cov_k]), recall numerators
//                    -> trapezoid + optimal-curve partials -> final sum.
// =====================================================================================================================
namespace {

constexpr int kAurcMaxKs = 16;
constexpr int kAurcMaxParts = 1024;

struct AurcHdr { unsigned E, m; };                          // written by aurc_scan_kernel
struct AurcCuts { long long pos[kAurcMaxKs]; int n; };      // sorted positions m_k - 1 whose e is a recall numerator

struct AurcWs {
  Ws sort;
  AurcHdr* hdr;
  unsigned* recall_e;     // [kAurcMaxKs]
  double* part;           // [2][kAurcMaxParts] trapezoid / optimal-curve partials
  unsigned* blkgs;        // [nblk] group starts per tile, then their exclusive scan
  double* R;              // [m + 1] <= n compacted selective risks (aliases the sort's idle key/value buffers)
  int* S;                 // [m + 1] compacted group-start positions, S[0] = -1
};

// flag: 0 correct, 1 error, 2 label == ignore.  form: 0 max probability, 1 1 - clamp(ent_mc), 2 1 - clamp(H / log C)
template <int CMAX>
__global__ __launch_bounds__(256) void aurc_sample_kernel(const float* __restrict__ probs, const int64_t* __restrict__ labels,
                                                          const float* __restrict__ ent_mc, int B, int C, int HW, int64_t ignore, int form,
                                                          float logc, float* __restrict__ conf_out, uint8_t* __restrict__ flag_out) {
  const size_t npix = (size_t)B * HW;
  const size_t pix = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (pix >= npix) return;
  const int b = (int)(pix / HW);
  const int hw = (int)(pix - (size_t)b * HW);
  const float* src = probs + (size_t)b * C * HW + hw;
  float p[CMAX];
#pragma unroll
  for (int c = 0; c < CMAX; ++c) p[c] = c < C ? src[(size_t)c * HW] : 0.0f;
  float best = -INFINITY;
  int arg = 0;
#pragma unroll
  for (int c = 0; c < CMAX; ++c)
    if (c < C && p[c] > best) { best = p[c]; arg = c; }        // first argmax of the probabilities as given
  float conf;
  if (form == 0) {
    conf = best;
  } else {
    float ent;
    if (form == 1) {
      ent = ent_mc[pix];
    } else {
      float h = 0.0f;
#pragma unroll
      for (int c = 0; c < CMAX; ++c)
        if (c < C) {
          const float q = fmaxf(p[c], 1e-12f);
          h -= q * logf(q);
        }
      ent = h / logc;
    }
    conf = 1.0f - fminf(fmaxf(ent, 0.0f), 1.0f);
  }
  const int64_t lab = labels[pix];
  conf_out[pix] = conf;
  flag_out[pix] = lab == ignore ? (uint8_t)2 : (uint8_t)(arg != lab ? 1 : 0);
}

// sort key: ascending confidence == ascending key; -0.0 and +0.0 share one key
__device__ __forceinline__ unsigned asc_key(float s) {
  unsigned u = __float_as_uint(s);
  if ((u << 1) == 0u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(kThreads) void aurc_keygen_kernel(const float* __restrict__ conf, const uint8_t* __restrict__ is_err, long long n,
                                                               unsigned* __restrict__ keys, unsigned* __restrict__ vals, unsigned* __restrict__ G) {
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
    keys[i] = asc_key(conf[i]);
    vals[i] = (unsigned)i | (is_err[i] ? 0x80000000u : 0u);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) G[0] = 1u;          // the sort kernels skip "classes" whose count is 0
}

__device__ __forceinline__ bool aurc_group_start(const unsigned* __restrict__ keys, long long i, long long n) {
  return i <= n - 2 && (i == 0 || keys[i] != keys[i - 1]);     // the last sample is never a point; a tile's first key looks at the tile before
}

__global__ __launch_bounds__(kThreads) void aurc_gscount_kernel(const unsigned* __restrict__ keys, long long n, unsigned* __restrict__ blkgs) {
  __shared__ unsigned s_w[kThreads / 64];
  const long long base = (long long)blockIdx.x * kTile;
  unsigned cnt = 0;
#pragma unroll
  for (int it = 0; it < kItems; ++it) {
    const long long i = base + it * kThreads + threadIdx.x;
    cnt += (unsigned)__popcll(__ballot(aurc_group_start(keys, i, n)));
  }
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned t = 0;
    for (int w = 0; w < kThreads / 64; ++w) t += s_w[w];
    blkgs[blockIdx.x] = t;
  }
}

// one workgroup: exclusive scan of the group starts over the tiles (256 tiles per step, carried), m, and E = the scanned
// error count of the last tile + that tile's own errors
__global__ __launch_bounds__(256) void aurc_scan_kernel(unsigned* __restrict__ blkgs, int nblk, const unsigned* __restrict__ vals, long long n,
                                                        const unsigned* __restrict__ blkfg, AurcHdr* __restrict__ hdr) {
  __shared__ unsigned s_w[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned carry = 0;
  for (int b0 = 0; b0 < nblk; b0 += 256) {
    const int b = b0 + threadIdx.x;
    const unsigned mine = b < nblk ? blkgs[b] : 0u;
    unsigned incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned t = __shfl_up(incl, o, 64);
      if (lane >= o) incl += t;
    }
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    unsigned before = carry;
    for (int w = 0; w < wave; ++w) before += s_w[w];
    if (b < nblk) blkgs[b] = before + incl - mine;
    carry += s_w[0] + s_w[1] + s_w[2] + s_w[3];
    __syncthreads();
  }
  unsigned e = 0;
  for (long long i = (long long)(nblk - 1) * kTile + threadIdx.x; i < n; i += 256) e += vals[i] >> 31;
  e = (unsigned)wave_sum((float)e);                      // <= 2048: exact in fp32
  if (lane == 0) s_w[wave] = e;
  __syncthreads();
  if (threadIdx.x == 0) {
    hdr->E = blkfg[nblk - 1] + s_w[0] + s_w[1] + s_w[2] + s_w[3];
    hdr->m = carry;
  }
}

// every element's inclusive error count e_i and, for group starts, the rank k: writes the compacted (s_k, R_k) and, when asked,
// the curve; the elements at the recall cuts write their e
__global__ __launch_bounds__(kThreads) void aurc_points_kernel(const unsigned* __restrict__ keys, const unsigned* __restrict__ vals, long long n,
                                                               const unsigned* __restrict__ blkfg, const unsigned* __restrict__ blkgs,
                                                               const AurcHdr* __restrict__ hdr, AurcCuts cuts, double* __restrict__ R,
                                                               int* __restrict__ S, unsigned* __restrict__ recall_e,
                                                               double* __restrict__ cov_out, double* __restrict__ risk_out) {
  constexpr int kWaves = kThreads / 64;
  __shared__ unsigned s_we[kWaves], s_wg[kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, blk = blockIdx.x;
  const unsigned E = hdr->E;
  // a wave owns kItems consecutive 64-element rows of the tile (sorted order == (wave, item, lane))
  const long long base = (long long)blk * kTile + (long long)wave * (kItems * 64);
  unsigned fg[kItems];
  bool gs[kItems];
  unsigned ce = 0, cg = 0;
#pragma unroll
  for (int it = 0; it < kItems; ++it) {
    const long long i = base + it * 64 + lane;
    fg[it] = i < n ? (vals[i] >> 31) : 0u;
    gs[it] = aurc_group_start(keys, i, n);
    ce += (unsigned)__popcll(__ballot(fg[it]));
    cg += (unsigned)__popcll(__ballot(gs[it]));
  }
  if (lane == 0) { s_we[wave] = ce; s_wg[wave] = cg; }
  __syncthreads();
  unsigned ebefore = blkfg[blk], gbefore = blkgs[blk];
  for (int w = 0; w < wave; ++w) { ebefore += s_we[w]; gbefore += s_wg[w]; }
  bool has_cut = false;
  for (int j = 0; j < cuts.n; ++j) has_cut |= cuts.pos[j] >= (long long)blk * kTile && cuts.pos[j] < (long long)(blk + 1) * kTile;
  const unsigned long long lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  const double dn = (double)n;
#pragma unroll
  for (int it = 0; it < kItems; ++it) {
    const long long i = base + it * 64 + lane;
    const unsigned long long me = __ballot(fg[it]), mg = __ballot(gs[it]);
    const unsigned e = ebefore + (unsigned)__popcll(me & lt) + fg[it];
    if (gs[it]) {                                            // i <= n - 2: at least one sample stays
      const unsigned k = gbefore + (unsigned)__popcll(mg & lt) + 1u;
      const double rem = (double)(n - 1 - i);
      const double r = (double)(E - e) / rem;
      R[k] = r;
      S[k] = (int)i;
      if (cov_out) { cov_out[k] = rem / dn; risk_out[k] = r; }
    }
    if (has_cut && i < n)
      for (int j = 0; j < cuts.n; ++j)
        if (cuts.pos[j] == i) recall_e[j] = e;
    ebefore += (unsigned)__popcll(me);
    gbefore += (unsigned)__popcll(mg);
  }
  if (blk == 0 && threadIdx.x == 0) {
    R[0] = (double)E / dn;
    S[0] = -1;
    if (cov_out) { cov_out[0] = 1.0; risk_out[0] = (double)E / dn; }
  }
}

__device__ __forceinline__ double aurc_block_sum(double v, double* s_part) {      // fixed order: the same bits every run
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
  for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += s_part[w];
  __syncthreads();
  return t;
}

// per-workgroup partials of the trapezoid over the compacted points and of sum_j j / (n - E + j); m and E come from the device
__global__ __launch_bounds__(256) void aurc_partial_kernel(const double* __restrict__ R, const int* __restrict__ S, const AurcHdr* __restrict__ hdr,
                                                           long long n, double* __restrict__ part) {
  __shared__ double s_part[4];
  const long long m = hdr->m, E = hdr->E;
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x, stride = (long long)gridDim.x * 256;
  const double dn = (double)n;
  double trap = 0.0, opt = 0.0;
  for (long long k = 1 + gid; k <= m; k += stride) trap += (R[k - 1] + R[k]) * 0.5 * ((double)(S[k] - S[k - 1]) / dn);
  for (long long j = 1 + gid; j <= E; j += stride) opt += (double)j / (double)(n - E + j);
  trap = aurc_block_sum(trap, s_part);
  opt = aurc_block_sum(opt, s_part);
  if (threadIdx.x == 0) { part[blockIdx.x] = trap; part[kAurcMaxParts + blockIdx.x] = opt; }
}

__global__ __launch_bounds__(256) void aurc_final_kernel(const double* __restrict__ part, int nparts, const double* __restrict__ R,
                                                         const int* __restrict__ S, const AurcHdr* __restrict__ hdr, long long n,
                                                         const unsigned* __restrict__ recall_e, int nks, double* __restrict__ out,
                                                         double* __restrict__ recalls) {
  __shared__ double s_part[4];
  double trap = 0.0, opt = 0.0;
  for (int i = threadIdx.x; i < nparts; i += 256) { trap += part[i]; opt += part[kAurcMaxParts + i]; }
  trap = aurc_block_sum(trap, s_part);
  opt = aurc_block_sum(opt, s_part);
  if (threadIdx.x == 0) {
    const unsigned m = hdr->m, E = hdr->E;
    const long long sm = m ? (long long)S[m] : -1;
    const double dn = (double)n;
    if (m && n - 2 - sm > 0) trap += R[m] * ((double)(n - 2 - sm) / dn);      // the tail point (0, R_m)
    opt /= dn;
    out[0] = trap; out[1] = trap - opt; out[2] = opt;
    out[3] = (double)E; out[4] = (double)m; out[5] = (double)sm;
    for (int j = 0; j < nks; ++j) recalls[j] = (double)recall_e[j] / (double)(E > 1u ? E : 1u);
  }
}

__global__ __launch_bounds__(kThreads) void aurc_unsort_kernel(const unsigned* __restrict__ keys, const unsigned* __restrict__ vals, long long n,
                                                               float* __restrict__ conf, uint8_t* __restrict__ is_err) {
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
    const unsigned k = keys[i];
    reinterpret_cast<unsigned*>(conf)[i] = (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k;
    is_err[i] = (uint8_t)(vals[i] >> 31);
  }
}

size_t aurc_carve(char* base, long long n, AurcWs* ws) {
  const int nblk = nblk_of(n);
  size_t off = 0;
  auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += align256(bytes); return p; };
  char* g = take(sizeof(unsigned));
  char* hd = take(sizeof(AurcHdr));
  char* re = take(kAurcMaxKs * sizeof(unsigned));
  char* pa = take((size_t)2 * kAurcMaxParts * sizeof(double));
  char* k0 = take((size_t)n * 4); char* v0 = take((size_t)n * 4);
  char* k1 = take((size_t)n * 4); char* v1 = take((size_t)n * 4);      // adjacent: idle after the 4th pass, then R (8 n bytes)
  char* h = take((size_t)256 * nblk * 4);
  char* bf = take((size_t)nblk * 4);
  char* bg = take((size_t)nblk * 4);
  char* s = take((size_t)n * 4);
  if (ws) {
    ws->sort.G = (unsigned*)g; ws->sort.loss_c = nullptr; ws->sort.act = nullptr;
    ws->sort.keys[0] = (unsigned*)k0; ws->sort.keys[1] = (unsigned*)k1; ws->sort.vals[0] = (unsigned*)v0; ws->sort.vals[1] = (unsigned*)v1;
    ws->sort.hist = (unsigned*)h; ws->sort.blkfg = (unsigned*)bf;
    ws->hdr = (AurcHdr*)hd; ws->recall_e = (unsigned*)re; ws->part = (double*)pa; ws->blkgs = (unsigned*)bg;
    ws->R = (double*)k1; ws->S = (int*)s;
  }
  return off;
}

}  // namespace

extern "C" int slu_aurc_samples(const float* probs, const int64_t* labels, const float* ent_mc, int B, int C, int HW, int64_t ignore_index,
                                int use_max_prob_confidence, float* conf, uint8_t* flags, slu_stream_t stream) {
  if (!probs || !labels || !conf || !flags || B <= 0 || C <= 0 || HW <= 0) return SLU_EINVAL;
  if (C > 32) return SLU_EUNSUPPORTED;
  const int form = use_max_prob_confidence ? 0 : (ent_mc ? 1 : 2);
  const float logc = (float)log((double)C);
  const size_t npix = (size_t)B * HW;
  const unsigned nb = (unsigned)((npix + 255) / 256);
  if (C <= 20)
    hipLaunchKernelGGL(aurc_sample_kernel<20>, dim3(nb), dim3(256), 0, slu_stream(stream), probs, labels, ent_mc, B, C, HW, ignore_index, form, logc,
                       conf, flags);
  else
    hipLaunchKernelGGL(aurc_sample_kernel<32>, dim3(nb), dim3(256), 0, slu_stream(stream), probs, labels, ent_mc, B, C, HW, ignore_index, form, logc,
                       conf, flags);
  SLU_CHECK_LAUNCH();
}

extern "C" size_t slu_aurc_workspace_bytes(long long n) {
  if (n <= 0) return 0;
  return aurc_carve(nullptr, n, nullptr);
}

extern "C" int slu_aurc_compute(const float* confids, const uint8_t* is_error, long long n, void* workspace, size_t workspace_bytes,
                                const double* ks, int nks, double* out6, double* recalls, double* curve_cov, double* curve_risk,
                                float* sorted_confids, uint8_t* sorted_is_error, slu_stream_t stream) {
  if (!confids || !is_error || !workspace || !out6 || n <= 0 || nks < 0) return SLU_EINVAL;
  if (nks > 0 && (!ks || !recalls)) return SLU_EINVAL;
  if ((curve_cov == nullptr) != (curve_risk == nullptr)) return SLU_EINVAL;
  if ((sorted_confids == nullptr) != (sorted_is_error == nullptr)) return SLU_EINVAL;
  if (n >= (1ll << 31) || nks > kAurcMaxKs) return SLU_EUNSUPPORTED;
  AurcCuts cuts;
  cuts.n = nks;
  for (int j = 0; j < kAurcMaxKs; ++j) cuts.pos[j] = -1;
  for (int j = 0; j < nks; ++j) {
    if (!(ks[j] >= 0.0)) return SLU_EINVAL;                    // negative or NaN
    const double mk = (double)n * ks[j] / 100.0;               // m_k = max(1, int(n k / 100)), at most n (a slice past the end)
    const long long m = mk >= (double)n ? n : (long long)mk;
    cuts.pos[j] = (m < 1 ? 1 : m) - 1;
  }
  AurcWs ws;
  if (aurc_carve((char*)workspace, n, &ws) > workspace_bytes) return SLU_EINVAL;
  if (reinterpret_cast<uintptr_t>(workspace) & 255) return SLU_EINVAL;
  hipStream_t st = slu_stream(stream);
  const int nblk = nblk_of(n);
  Ws& s = ws.sort;
  const unsigned kg = (unsigned)((n + kThreads - 1) / kThreads > 1024 ? 1024 : (n + kThreads - 1) / kThreads);
  hipLaunchKernelGGL(aurc_keygen_kernel, dim3(kg), dim3(kThreads), 0, st, confids, is_error, n, s.keys[0], s.vals[0], s.G);
  int cur = 0;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 8 * pass;
    hipLaunchKernelGGL(hist_kernel, dim3(nblk, 1), dim3(kThreads), 0, st, s.keys[cur], n, nblk, shift, s.G, s.hist);
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(256), 0, st, s.hist, nblk, s.G);
    hipLaunchKernelGGL(scatter_kernel, dim3(nblk, 1), dim3(kThreads), 0, st, s.keys[cur], s.vals[cur], s.keys[cur ^ 1], s.vals[cur ^ 1], n, nblk,
                       shift, s.G, s.hist);
    cur ^= 1;
  }
  // cur == 0 again: keys[1] / vals[1] are idle and hold R from here on
  hipLaunchKernelGGL(fgcount_kernel, dim3(nblk, 1), dim3(kThreads), 0, st, s.vals[cur], n, nblk, s.G, s.blkfg);
  hipLaunchKernelGGL(fgscan_kernel, dim3(1), dim3(256), 0, st, s.blkfg, nblk, s.G);
  hipLaunchKernelGGL(aurc_gscount_kernel, dim3(nblk), dim3(kThreads), 0, st, s.keys[cur], n, ws.blkgs);
  hipLaunchKernelGGL(aurc_scan_kernel, dim3(1), dim3(256), 0, st, ws.blkgs, nblk, s.vals[cur], n, s.blkfg, ws.hdr);
  hipLaunchKernelGGL(aurc_points_kernel, dim3(nblk), dim3(kThreads), 0, st, s.keys[cur], s.vals[cur], n, s.blkfg, ws.blkgs, ws.hdr, cuts, ws.R, ws.S,
                     ws.recall_e, curve_cov, curve_risk);
  const int nparts = nblk > kAurcMaxParts ? kAurcMaxParts : nblk;      // a function of n alone: the summation order is fixed
  hipLaunchKernelGGL(aurc_partial_kernel, dim3(nparts), dim3(256), 0, st, ws.R, ws.S, ws.hdr, n, ws.part);
  hipLaunchKernelGGL(aurc_final_kernel, dim3(1), dim3(256), 0, st, ws.part, nparts, ws.R, ws.S, ws.hdr, n, ws.recall_e, nks, out6, recalls);
  if (sorted_confids)
    hipLaunchKernelGGL(aurc_unsort_kernel, dim3(kg), dim3(kThreads), 0, st, s.keys[cur], s.vals[cur], n, sorted_confids, sorted_is_error);
  SLU_CHECK_LAUNCH();
}
