// AURC / E-AURC of selective prediction on gfx950 (replaces src/metrics/aurc.py:7-45 of the reference; DESIGN "AURC on the device").
//
//   samples (conf fp32, err in {0,1}), sorted ascending by conf as one segment of the radix sort of radix_sort.h (key =
//   KeyAscendingFoldZero of conf, value = index | err << 31).  The passes are stable: equal confidences keep
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
//   after the sort:  the sort's flag prefix (errors per tile)  +  group starts per tile and their scan over tiles
//                    -> one pass: e_i and the rank of every group start, compacted (s_k, R_k [, cov_k]), recall numerators
//                    -> trapezoid + optimal-curve partials -> final sum.
#include "class_column.h"
#include "radix_sort.h"

namespace {

using namespace slu_sort;

constexpr int kAurcMaxKs = 16;
constexpr int kAurcMaxParts = 1024;

struct AurcHdr { unsigned E, m; };                          // written by aurc_scan_kernel
struct AurcCuts { long long pos[kAurcMaxKs]; int n; };      // sorted positions m_k - 1 whose e is a recall numerator

struct AurcWs {
  unsigned* one;          // the sort's "segments to sort" word, written by the keygen
  AurcHdr* hdr;
  unsigned* recall_e;     // [kAurcMaxKs]
  double* part;           // [2][kAurcMaxParts] trapezoid / optimal-curve partials
  SluSortWs sort;
  unsigned* blkgs;        // [nblk] group starts per tile, then their exclusive scan
  int* S;                 // [m + 1] compacted group-start positions, S[0] = -1
};                        // R [m + 1] <= n, the compacted selective risks, lives in slu_sort_idle(sort): 8 n bytes

// flag: 0 correct, 1 error, 2 label == ignore.  form: 0 max probability, 1 1 - clamp(ent_mc), 2 1 - clamp(H / log C)
template <int CMAX>
__global__ __launch_bounds__(256) void aurc_sample_kernel(const float* __restrict__ probs, const int64_t* __restrict__ labels,
                                                          const float* __restrict__ ent_mc, int B, int C, int HW, int64_t ignore, int form,
                                                          float logc, float* __restrict__ conf_out, uint8_t* __restrict__ flag_out) {
  const size_t npix = (size_t)B * HW;
  const size_t pix = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (pix >= npix) return;
  float p[CMAX], best;
  slu_load_column(probs + slu_pixel(pix, C, HW).col, C, HW, 0.0f, p);
  const int arg = slu_first_argmax(p, C, best);                // of the probabilities as given
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
  flag_out[pix] = slu_label_ignored(lab, ignore) ? (uint8_t)2 : (uint8_t)(arg != lab ? 1 : 0);
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
  for (long long i = (long long)(nblk - 1) * kTile + threadIdx.x; i < n; i += 256) e += val_flag(vals[i]);
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
    fg[it] = i < n ? val_flag(vals[i]) : 0u;
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
  const unsigned long long lt = lanes_below(lane);
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

size_t carve(char* base, long long n, AurcWs& ws) {
  const int nblk = nblk_of(n);
  SluCarver cv{base};
  ws.one = cv.take<unsigned>(1);
  ws.hdr = cv.take<AurcHdr>(1);
  ws.recall_e = cv.take<unsigned>(kAurcMaxKs);
  ws.part = cv.take<double>((size_t)2 * kAurcMaxParts);
  slu_sort_carve(cv, n, 1, ws.sort);
  ws.blkgs = cv.take<unsigned>(nblk);
  ws.S = cv.take<int>(n);
  return cv.off;
}

}  // namespace

extern "C" int slu_aurc_samples(const float* probs, const int64_t* labels, const float* ent_mc, int B, int C, int HW, int64_t ignore_index,
                                int use_max_prob_confidence, float* conf, uint8_t* flags, slu_stream_t stream) {
  if (!probs || !labels || !conf || !flags || B <= 0 || C <= 0 || HW <= 0) return SLU_EINVAL;
  if (C > 32) return SLU_EUNSUPPORTED;
  const int form = use_max_prob_confidence ? 0 : (ent_mc ? 1 : 2);
  const float logc = (float)log((double)C);
  const unsigned nb = slu_grid_per_pixel((size_t)B * HW);
  slu_class_cap(C, [&](auto cmax) {
    hipLaunchKernelGGL(aurc_sample_kernel<decltype(cmax)::value>, dim3(nb), dim3(256), 0, slu_stream(stream), probs, labels, ent_mc, B, C, HW,
                       ignore_index, form, logc, conf, flags);
  });
  SLU_CHECK_LAUNCH();
}

extern "C" size_t slu_aurc_workspace_bytes(long long n) {
  if (n <= 0) return 0;
  AurcWs ws;
  return carve(nullptr, n, ws);
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
  if (carve((char*)workspace, n, ws) > workspace_bytes) return SLU_EINVAL;
  if (reinterpret_cast<uintptr_t>(workspace) & 255) return SLU_EINVAL;
  hipStream_t st = slu_stream(stream);
  const int nblk = nblk_of(n);
  const SluSortWs& s = ws.sort;
  const unsigned kg = slu_grid_1d(n, 1024);
  hipLaunchKernelGGL(sample_keygen_kernel<KeyAscendingFoldZero>, dim3(kg), dim3(kThreads), 0, st, confids, is_error, n, s.keys[0], s.vals[0], ws.one);
  slu_sort_pairs(s, n, 1, ws.one, st);
  slu_sort_flag_prefix(s, n, 1, ws.one, st);
  double* R = static_cast<double*>(slu_sort_idle(s));
  hipLaunchKernelGGL(aurc_gscount_kernel, dim3(nblk), dim3(kThreads), 0, st, s.keys[0], n, ws.blkgs);
  hipLaunchKernelGGL(aurc_scan_kernel, dim3(1), dim3(256), 0, st, ws.blkgs, nblk, s.vals[0], n, s.blkflag, ws.hdr);
  hipLaunchKernelGGL(aurc_points_kernel, dim3(nblk), dim3(kThreads), 0, st, s.keys[0], s.vals[0], n, s.blkflag, ws.blkgs, ws.hdr, cuts, R, ws.S,
                     ws.recall_e, curve_cov, curve_risk);
  const int nparts = nblk > kAurcMaxParts ? kAurcMaxParts : nblk;      // a function of n alone: the summation order is fixed
  hipLaunchKernelGGL(aurc_partial_kernel, dim3(nparts), dim3(256), 0, st, R, ws.S, ws.hdr, n, ws.part);
  hipLaunchKernelGGL(aurc_final_kernel, dim3(1), dim3(256), 0, st, ws.part, nparts, R, ws.S, ws.hdr, n, ws.recall_e, nks, out6, recalls);
  if (sorted_confids)
    hipLaunchKernelGGL(sample_unsort_kernel<KeyAscendingFoldZero>, dim3(kg), dim3(kThreads), 0, st, s.keys[0], s.vals[0], n, sorted_confids,
                       sorted_is_error);
  SLU_CHECK_LAUNCH();
}
