// Post-hoc temperature scaling on gfx950 (replaces src/models/temp_scaling.py:26-33,78,88-104 and :142-170 of the reference; DESIGN
// "Temperature scaling on the device").
//
//   slu_calib_rows   the calibration cache of one batch: every pixel with label != ignore as one row of C log-probabilities, appended
//                    to a device-resident [cap, C] buffer in (b, h, w) order.  A stable compaction from three plain launches:
//                      1. calib_count_kernel    valid pixels of every 256-pixel block
//                      2. calib_scan_kernel     one workgroup: exclusive scan over the blocks; base = count, count += total
//                      3. calib_scatter_kernel  one lane owns a pixel and reads its class column (a wave reads 256-byte row segments of
//                                               every class plane), the rows go to LDS at their rank inside the block, and the block's
//                                               rows -- one contiguous piece of the cache -- leave LDS in 256-byte segments
//   slu_temp_nll     sum of NLL(rows / T) and of its derivative by log T: rows reach LDS in 256-byte segments (or one row per group of C
//                    lanes under a gather index), one lane owns a row and evaluates it in fp64 (T itself is the fp32 value the
//                    reference holds), fp64 sums in a fixed order (workgroup partials, then one workgroup that adds them).
// No workgroup waits on another inside a kernel and nothing is accumulated with floating-point atomics.
#include "class_column.h"

namespace {

constexpr int kRows = 256;               // pixels (calib) or rows (nll) per workgroup step: one per thread
constexpr int kNllMaxParts = 1024;       // workgroups of temp_nll_kernel; a function of the row count alone, so the summation order is fixed

__device__ __forceinline__ unsigned long long ts_lanes_below(int lane) { return lane == 0 ? 0ull : (~0ull >> (64 - lane)); }

// LDS pitch of a row of C floats: odd, so the 64 lanes of a wave that touch 64 consecutive rows at one class hit 64 different banks
__host__ __device__ __forceinline__ constexpr int ts_pitch(int C) { return C | 1; }

// (row, class) of flat element j of a [rows, C] piece, for a thread that visits j = tid, tid + 256, ...: one division, then additions
struct TsWalk {
  unsigned r, c, dr, dc;
  __device__ __forceinline__ TsWalk(unsigned tid, unsigned C) : r(tid / C), c(tid - (tid / C) * C), dr(kRows / C), dc(kRows - (kRows / C) * C) {}
  __device__ __forceinline__ void step(unsigned C) {
    r += dr;
    c += dc;
    if (c >= C) {
      c -= C;
      ++r;
    }
  }
};

// ---- slu_calib_rows -----------------------------------------------------------------------------------------------------------------------
struct CalibWs {
  long long* base;         // [1] the row the batch starts at: count before the call
  unsigned* blk;           // [nblk] valid pixels per block, then their exclusive scan
};

__device__ __forceinline__ bool calib_valid(const int64_t* __restrict__ labels, size_t pix, size_t npix, int has_ignore, int64_t ignore, int64_t& lab) {
  if (pix >= npix) return false;
  lab = labels[pix];
  return !slu_label_ignored(lab, has_ignore, ignore);
}

__global__ __launch_bounds__(kRows) void calib_count_kernel(const int64_t* __restrict__ labels, size_t npix, int has_ignore, int64_t ignore,
                                                            unsigned* __restrict__ blk) {
  __shared__ unsigned s_w[4];
  int64_t lab;
  const bool valid = calib_valid(labels, (size_t)blockIdx.x * kRows + threadIdx.x, npix, has_ignore, ignore, lab);
  const unsigned k = (unsigned)__popcll(__ballot(valid));
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = k;
  __syncthreads();
  if (threadIdx.x == 0) blk[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// one workgroup: exclusive scan over the blocks (256 per step, carried); the batch's first row and the new row count
__global__ __launch_bounds__(256) void calib_scan_kernel(unsigned* __restrict__ blk, int nblk, long long* __restrict__ base, int64_t* __restrict__ count) {
  __shared__ unsigned s_w[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned carry = 0;
  for (int b0 = 0; b0 < nblk; b0 += 256) {
    const int b = b0 + threadIdx.x;
    const unsigned mine = b < nblk ? blk[b] : 0u;
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
    if (b < nblk) blk[b] = before + incl - mine;
    carry += s_w[0] + s_w[1] + s_w[2] + s_w[3];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const long long at = (long long)count[0];
    base[0] = at;
    count[0] = (int64_t)(at + (long long)carry);
  }
}

template <int CMAX>
__global__ __launch_bounds__(kRows) void calib_scatter_kernel(const float* __restrict__ out, int kind, const int64_t* __restrict__ labels, int B, int C,
                                                              int HW, int has_ignore, int64_t ignore, const unsigned* __restrict__ blk,
                                                              const long long* __restrict__ base, long long cap, float* __restrict__ rows,
                                                              int64_t* __restrict__ row_labels) {
  __shared__ float s_rows[kRows * ts_pitch(CMAX)];
  __shared__ unsigned s_w[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t npix = (size_t)B * HW;
  const size_t pix = (size_t)blockIdx.x * kRows + threadIdx.x;
  int64_t lab = 0;
  const bool valid = calib_valid(labels, pix, npix, has_ignore, ignore, lab);
  const unsigned long long mask = __ballot(valid);
  if (lane == 0) s_w[wave] = (unsigned)__popcll(mask);
  __syncthreads();
  const unsigned nvalid = s_w[0] + s_w[1] + s_w[2] + s_w[3];
  if (nvalid == 0) return;                                           // the whole workgroup
  unsigned rank = (unsigned)__popcll(mask & ts_lanes_below(lane));   // among the block's valid pixels, in pixel order
  for (int w = 0; w < wave; ++w) rank += s_w[w];
  const int pitch = ts_pitch(C);
  if (valid) {
    float x[CMAX];
    const float m = slu_load_column(out + slu_pixel(pix, C, HW).col, C, (size_t)HW, -INFINITY, x);
    if (kind == 0) {                                                 // p = e / sum e, in fp64, rounded once
      double e[CMAX], se = 0.0;
#pragma unroll
      for (int c = 0; c < CMAX; ++c)
        if (c < C) {
          e[c] = exp((double)x[c] - (double)m);
          se += e[c];
        }
#pragma unroll
      for (int c = 0; c < CMAX; ++c)
        if (c < C) x[c] = (float)(e[c] / se);
    } else if (kind == 2) {
#pragma unroll
      for (int c = 0; c < CMAX; ++c)
        if (c < C) x[c] = (float)exp((double)x[c]);
    }
#pragma unroll
    for (int c = 0; c < CMAX; ++c)
      if (c < C) s_rows[rank * pitch + c] = (float)log((double)fmaxf(x[c], 1e-12f));      // logf, correctly rounded
  }
  __syncthreads();
  const long long row0 = base[0] + (long long)blk[blockIdx.x];
  const long long room = cap - row0;
  if (room <= 0) return;                                             // the cache is full: nothing of this block is written
  const unsigned nw = room < (long long)nvalid ? (unsigned)room : nvalid;
  if (valid && rank < nw) row_labels[row0 + rank] = lab;
  float* __restrict__ dst = rows + (size_t)row0 * C;
  const unsigned total = nw * (unsigned)C;
  TsWalk at(threadIdx.x, (unsigned)C);
  for (unsigned j = threadIdx.x; j < total; j += kRows) {
    dst[j] = s_rows[at.r * pitch + at.c];
    at.step((unsigned)C);
  }
}

size_t calib_carve(char* base, int nblk, CalibWs& ws) {
  ws.base = reinterpret_cast<long long*>(base);
  ws.blk = reinterpret_cast<unsigned*>(base + 256);
  return 256 + (size_t)nblk * sizeof(unsigned);
}

// ---- slu_temp_nll -------------------------------------------------------------------------------------------------------------------------
struct NllWs {
  double* loss;            // [kNllMaxParts]
  double* g;               // [kNllMaxParts]
  long long* bad;          // [kNllMaxParts]
};

__device__ __forceinline__ double nll_block_sum(double v, double (&s_part)[4]) {      // fixed order: the same bits every run
  slu_stage_wave_total(wave_sum(v), s_part);
  __syncthreads();
  const double t = slu_block_total(s_part);
  __syncthreads();
  return t;
}

// T = max(exp(log_T), 1e-3f) as an fp32 value (the exponential correctly rounded); *clamped: the clamp holds T, so d T / d log_T = 0
__device__ __forceinline__ float nll_temperature(const float* __restrict__ log_T, bool* clamped) {
  const float et = (float)exp((double)log_T[0]);
  *clamped = et < 1e-3f;
  return fmaxf(et, 1e-3f);
}

template <int CMAX>
__global__ __launch_bounds__(kRows) void temp_nll_kernel(const float* __restrict__ rows, const int64_t* __restrict__ row_labels, long long N, int C,
                                                         const int64_t* __restrict__ idx, long long M, const float* __restrict__ log_T,
                                                         double* __restrict__ part_loss, double* __restrict__ part_g,
                                                         long long* __restrict__ part_bad) {
  __shared__ float s_x[kRows * ts_pitch(CMAX)];
  __shared__ long long s_src[kRows];
  __shared__ double s_part[4];
  const int tid = threadIdx.x;
  const int pitch = ts_pitch(C);
  bool clamped;
  const double rT = 1.0 / (double)nll_temperature(log_T, &clamped);
  double loss = 0.0, g = 0.0;
  long long bad = 0;
  const long long nblk = (M + kRows - 1) / kRows;
  for (long long b = blockIdx.x; b < nblk; b += gridDim.x) {
    const long long j0 = b * kRows;
    const int nr = M - j0 < kRows ? (int)(M - j0) : kRows;
    long long src = -1;
    if (tid < nr) {
      src = idx ? (long long)idx[j0 + tid] : j0 + tid;
      if (src < 0 || src >= N) src = -1;
    }
    s_src[tid] = src;
    __syncthreads();
    const unsigned total = (unsigned)nr * (unsigned)C;
    TsWalk at((unsigned)tid, (unsigned)C);
    for (unsigned j = tid; j < total; j += kRows) {
      const long long s = s_src[at.r];
      s_x[at.r * pitch + at.c] = s >= 0 ? rows[(size_t)s * C + at.c] : 0.0f;
      at.step((unsigned)C);
    }
    __syncthreads();
    if (tid < nr) {
      const int64_t y = src >= 0 ? row_labels[src] : -1;
      if (!slu_label_in_range(y, C)) {
        ++bad;
      } else {
        const float* __restrict__ xr = s_x + tid * pitch;
        float mx = -INFINITY;                        // T > 0: the largest s_c belongs to the largest x_c
#pragma unroll
        for (int c = 0; c < CMAX; ++c)
          if (c < C) mx = fmaxf(mx, xr[c]);
        const double xy = (double)xr[(int)y], m = (double)mx;
        double se = 0.0, ed = 0.0;                   // sum e_c and sum e_c (x_y - x_c), class order
#pragma unroll
        for (int c = 0; c < CMAX; ++c)
          if (c < C) {
            const double x = (double)xr[c];
            const double e = exp((x - m) * rT);
            se += e;
            ed += e * (xy - x);
          }
        loss += log(se) - (xy - m) * rT;             // m + log S - s_y, the small difference first
        if (!clamped) g += ed / se * rT;             // (x_y - sum p x) / T with sum p = 1 taken inside: no cancellation of x_y
      }
    }
    __syncthreads();                                 // before the next step overwrites the rows
  }
  loss = nll_block_sum(loss, s_part);
  g = nll_block_sum(g, s_part);
  const double nbad = nll_block_sum((double)bad, s_part);      // <= 2^53 rows: exact
  if (tid == 0) {
    part_loss[blockIdx.x] = loss;
    part_g[blockIdx.x] = g;
    part_bad[blockIdx.x] = (long long)nbad;
  }
}

__global__ __launch_bounds__(256) void temp_nll_final_kernel(const double* __restrict__ part_loss, const double* __restrict__ part_g,
                                                             const long long* __restrict__ part_bad, int nparts, double* __restrict__ loss_sum,
                                                             double* __restrict__ g_sum, int64_t* __restrict__ bad) {
  __shared__ double s_part[4];
  double loss = 0.0, g = 0.0, nbad = 0.0;
  for (int i = threadIdx.x; i < nparts; i += 256) {
    loss += part_loss[i];
    g += part_g[i];
    nbad += (double)part_bad[i];
  }
  loss = nll_block_sum(loss, s_part);
  g = nll_block_sum(g, s_part);
  nbad = nll_block_sum(nbad, s_part);
  if (threadIdx.x == 0) {
    loss_sum[0] = loss;
    g_sum[0] = g;
    bad[0] = (int64_t)nbad;
  }
}

int nll_parts(long long n) {
  const long long nblk = (n + kRows - 1) / kRows;
  return (int)(nblk > kNllMaxParts ? kNllMaxParts : nblk);
}

size_t nll_carve(char* base, NllWs& ws) {
  ws.loss = reinterpret_cast<double*>(base);
  ws.g = ws.loss + kNllMaxParts;
  ws.bad = reinterpret_cast<long long*>(ws.g + kNllMaxParts);
  return (size_t)kNllMaxParts * (2 * sizeof(double) + sizeof(long long));
}

}  // namespace

extern "C" size_t slu_calib_rows_workspace_bytes(int B, int HW) {
  if (B <= 0 || HW <= 0) return 0;
  CalibWs ws;
  return calib_carve(nullptr, (int)(((long long)B * HW + kRows - 1) / kRows), ws);
}

extern "C" int slu_calib_rows(const float* out, int kind, const int64_t* labels, int B, int C, int HW, int has_ignore, int64_t ignore_index,
                              float* rows, int64_t* row_labels, long long cap, int64_t* count, void* workspace, size_t workspace_bytes,
                              slu_stream_t stream) {
  if (!out || !labels || !rows || !row_labels || !count || !workspace || B <= 0 || C <= 0 || HW <= 0 || cap <= 0 || kind < 0 || kind > 2)
    return SLU_EINVAL;
  if (C > 32 || (long long)B * HW >= (1ll << 31)) return SLU_EUNSUPPORTED;
  const size_t npix = (size_t)B * HW;
  const int nblk = (int)((npix + kRows - 1) / kRows);
  CalibWs ws;
  if (calib_carve((char*)workspace, nblk, ws) > workspace_bytes || (reinterpret_cast<uintptr_t>(workspace) & 7)) return SLU_EINVAL;
  hipStream_t st = slu_stream(stream);
  hipLaunchKernelGGL(calib_count_kernel, dim3(nblk), dim3(kRows), 0, st, labels, npix, has_ignore, ignore_index, ws.blk);
  hipLaunchKernelGGL(calib_scan_kernel, dim3(1), dim3(256), 0, st, ws.blk, nblk, ws.base, count);
  slu_class_cap(C, [&](auto cmax) {
    hipLaunchKernelGGL(calib_scatter_kernel<decltype(cmax)::value>, dim3(nblk), dim3(kRows), 0, st, out, kind, labels, B, C, HW, has_ignore,
                       ignore_index, ws.blk, ws.base, cap, rows, row_labels);
  });
  SLU_CHECK_LAUNCH();
}

extern "C" size_t slu_temp_nll_workspace_bytes(long long n) {
  if (n <= 0) return 0;
  NllWs ws;
  return nll_carve(nullptr, ws);
}

extern "C" int slu_temp_nll(const float* rows, const int64_t* row_labels, long long N, int C, const int64_t* idx, long long M, const float* log_T,
                            double* loss_sum, double* g_sum, int64_t* bad, void* workspace, size_t workspace_bytes, slu_stream_t stream) {
  if (!rows || !row_labels || !log_T || !loss_sum || !g_sum || !bad || !workspace || N <= 0 || C <= 0 || (idx && M <= 0)) return SLU_EINVAL;
  if (C > 32) return SLU_EUNSUPPORTED;
  const long long n = idx ? M : N;
  NllWs ws;
  if (nll_carve((char*)workspace, ws) > workspace_bytes || (reinterpret_cast<uintptr_t>(workspace) & 7)) return SLU_EINVAL;
  hipStream_t st = slu_stream(stream);
  const int nparts = nll_parts(n);
  slu_class_cap(C, [&](auto cmax) {
    hipLaunchKernelGGL(temp_nll_kernel<decltype(cmax)::value>, dim3(nparts), dim3(kRows), 0, st, rows, row_labels, N, C, idx, n, log_T, ws.loss, ws.g,
                       ws.bad);
  });
  hipLaunchKernelGGL(temp_nll_final_kernel, dim3(1), dim3(256), 0, st, ws.loss, ws.g, ws.bad, nparts, loss_sum, g_sum, bad);
  SLU_CHECK_LAUNCH();
}
