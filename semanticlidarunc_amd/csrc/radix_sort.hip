// Batched LSD radix sort of (key, value) pairs on gfx950, 4 x 8 bit: the interface is radix_sort.h, the description DESIGN 3.4f.
//
// Per pass: per-tile digit histograms -> one exclusive scan per segment -> stable scatter (the rank of an element inside its wave
// comes from 8 ballots over the digit bits, 64-lane waves; per-wave digit counters in LDS).  Segments that are not to be sorted
// exit every kernel at once.
//
// HBM-bound: ~ 4 passes x (8 B read for the histogram + 8 B read + 8 B written by the scatter) per key.
#include "radix_sort.h"

namespace {

using namespace slu_sort;

// ---- radix pass: histogram ------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void hist_kernel(const unsigned* __restrict__ keys, long long N, int nblk, int shift,
                                                        const unsigned* __restrict__ sort_seg, unsigned* __restrict__ hist) {
  const int c = blockIdx.y, blk = blockIdx.x;
  if (sort_seg[c] == 0) return;
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
  hist[((size_t)c * nblk + blk) * 256 + threadIdx.x] = s_h[threadIdx.x];      // [segment][tile][digit]: the scan reads 1 KB rows
}

// ---- radix pass: exclusive scan over (digit, tile) of one segment (one workgroup per segment) ------
__global__ __launch_bounds__(256) void scan_kernel(unsigned* __restrict__ hist, int nblk, const unsigned* __restrict__ sort_seg) {
  const int c = blockIdx.x;
  if (sort_seg[c] == 0) return;
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
                                                           long long N, int nblk, int shift, const unsigned* __restrict__ sort_seg,
                                                           const unsigned* __restrict__ hist) {
  const int c = blockIdx.y, blk = blockIdx.x;
  if (sort_seg[c] == 0) return;
  constexpr int kWaves = kThreads / 64;
  __shared__ unsigned s_cnt[kWaves][256];       // running count of each digit inside each wave's slice
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < kWaves * 256; i += kThreads) (&s_cnt[0][0])[i] = 0;
  __syncthreads();
  // a wave owns kItems consecutive 64-key rows of the tile: key order == (wave, item, lane)
  const long long base = (long long)blk * kTile + (long long)wave * (kItems * 64);
  const size_t seg = (size_t)c * N;
  unsigned key[kItems], val[kItems], rank[kItems];
  const unsigned long long lt = lanes_below(lane);
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

// ---- after the sort: flagged values per tile, then their exclusive scan over the tiles of a segment ----
__global__ __launch_bounds__(kThreads) void fgcount_kernel(const unsigned* __restrict__ vals, long long N, int nblk,
                                                           const unsigned* __restrict__ sort_seg, unsigned* __restrict__ blkflag) {
  const int c = blockIdx.y, blk = blockIdx.x;
  if (sort_seg[c] == 0) return;
  __shared__ unsigned s_w[kThreads / 64];
  const long long base = (long long)blk * kTile;
  unsigned n = 0;
#pragma unroll
  for (int it = 0; it < kItems; ++it) {
    const long long i = base + it * kThreads + threadIdx.x;
    if (i < N) n += val_flag(vals[(size_t)c * N + i]);
  }
  n = (unsigned)wave_sum((float)n);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned t = 0;
    for (int w = 0; w < kThreads / 64; ++w) t += s_w[w];
    blkflag[(size_t)c * nblk + blk] = t;
  }
}

__global__ __launch_bounds__(256) void fgscan_kernel(unsigned* __restrict__ blkflag, int nblk, const unsigned* __restrict__ sort_seg) {
  const int c = blockIdx.x;                    // serial exclusive scan over <= a few hundred tiles
  if (sort_seg[c] == 0 || threadIdx.x != 0) return;
  unsigned run = 0;
  unsigned* row = blkflag + (size_t)c * nblk;
  for (int b = 0; b < nblk; ++b) { const unsigned t = row[b]; row[b] = run; run += t; }
}

}  // namespace

void slu_sort_carve(SluCarver& cv, long long n, int segs, SluSortWs& ws) {
  const int nblk = nblk_of(n);
  const size_t pairs = (size_t)segs * n;
  ws.keys[0] = cv.take<unsigned>(pairs); ws.vals[0] = cv.take<unsigned>(pairs);
  ws.keys[1] = cv.take<unsigned>(pairs); ws.vals[1] = cv.take<unsigned>(pairs);      // adjacent: slu_sort_idle
  ws.hist = cv.take<unsigned>((size_t)segs * 256 * nblk);
  ws.blkflag = cv.take<unsigned>((size_t)segs * nblk);
}

void slu_sort_pairs(const SluSortWs& ws, long long n, int segs, const unsigned* sort_seg, hipStream_t st) {
  const int nblk = nblk_of(n);
  int cur = 0;
  for (int pass = 0; pass < 4; ++pass) {      // an even number of passes: the result is back in keys[0] / vals[0]
    const int shift = 8 * pass;
    hipLaunchKernelGGL(hist_kernel, dim3(nblk, segs), dim3(kThreads), 0, st, ws.keys[cur], n, nblk, shift, sort_seg, ws.hist);
    hipLaunchKernelGGL(scan_kernel, dim3(segs), dim3(256), 0, st, ws.hist, nblk, sort_seg);
    hipLaunchKernelGGL(scatter_kernel, dim3(nblk, segs), dim3(kThreads), 0, st, ws.keys[cur], ws.vals[cur], ws.keys[cur ^ 1],
                       ws.vals[cur ^ 1], n, nblk, shift, sort_seg, ws.hist);
    cur ^= 1;
  }
}

void slu_sort_flag_prefix(const SluSortWs& ws, long long n, int segs, const unsigned* sort_seg, hipStream_t st) {
  const int nblk = nblk_of(n);
  hipLaunchKernelGGL(fgcount_kernel, dim3(nblk, segs), dim3(kThreads), 0, st, ws.vals[0], n, nblk, sort_seg, ws.blkflag);
  hipLaunchKernelGGL(fgscan_kernel, dim3(segs), dim3(256), 0, st, ws.blkflag, nblk, sort_seg);
}
