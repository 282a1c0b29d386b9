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
// no compaction pass is needed.  All classes are sorted at once, one segment per class, by the radix sort of radix_sort.h
// (key = 0x3F800000 - bits(err), i.e. ascending key == descending err in [0,1]; value = pixel index | fg << 31); classes
// that are not summed are not sorted.
// After the sort one kernel scans the fg bits, forms J_k in fp32 exactly like the reference
// (1 - inter/union, both exact integers in fp32), accumulates loss_c in fp64 and scatters
// d loss / d p_c,i = (J_k - J_{k-1}) * (fg ? -1 : +1) back to pixel order (0 where err == 0).
// The radix passes are stable, so equal errors keep their pixel order: the gradient is the same run to run, and over a group
// of equal errors it sums to J(after the group) - J(before the group) whatever the order inside the group.
//
// Unlike the reference, keygen_kernel clamps err to [0, 1] (the key transform needs that range) and fminf/fmaxf map a NaN
// error to 0: a NaN or out-of-range probability gives a finite loss and a zero gradient at that pixel where the reference
// would propagate it.
#include "radix_sort.h"

namespace {

using namespace slu_sort;

constexpr unsigned kOne = 0x3F800000u;          // bits(1.0f)

struct LovaszWs {
  unsigned* G;         // [C] foreground count per class (valid pixels)
  double* loss_c;      // [C]
  SluSortWs sort;
  unsigned* act;       // [C] 1 = the class is summed whether or not it is present (classes='all' / an explicit list); unused for 'present'
};

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
    vals[(size_t)c * N + i] = make_val(i, fg);
    local += fg ? 1u : 0u;
  }
  local = (unsigned)wave_sum((float)local);     // <= 64 * iterations, exact in fp32 for any sane grid
  if ((threadIdx.x & 63) == 0 && local) atomicAdd(&s_cnt[0], local);
  __syncthreads();
  if (threadIdx.x == 0 && s_cnt[0]) atomicAdd(&G[c], s_cnt[0]);
}

// ---- after the sort: Jaccard steps / loss / gradient scatter ----------------------------------------
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
    mine += val_flag(v_[it]);
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
      const unsigned fg = val_flag(v_[it]);
      const float j_prev = (i == 0) ? 0.0f : jaccard(g, (unsigned long long)i, cum);
      cum += fg;
      const float step = jaccard(g, (unsigned long long)i + 1, cum) - j_prev;
      const float err = __uint_as_float(kOne - k_[it]);
      part += (double)(err * step);
      if (grad) grad[seg + val_index(v_[it])] = err > 0.0f ? (fg ? -step : step) : 0.0f;
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

// G and loss_c first and adjacent: one memset zeroes both
size_t carve(char* base, long long N, int C, LovaszWs& ws) {
  SluCarver cv{base};
  ws.G = cv.take<unsigned>(C);
  ws.loss_c = cv.take<double>(C);
  slu_sort_carve(cv, N, C, ws.sort);
  ws.act = cv.take<unsigned>(C);
  return cv.off;
}

}  // namespace

extern "C" size_t slu_lovasz_workspace_bytes(int B, int C, int HW) {
  if (B <= 0 || C <= 0 || HW <= 0) return 0;
  LovaszWs ws;
  return carve(nullptr, (long long)B * HW, C, ws);
}

extern "C" int slu_lovasz_fwd(const float* probs, const int64_t* labels, int B, int C, int HW, int64_t ignore_index, unsigned class_mask,
                              void* workspace, size_t workspace_bytes, float* loss, float* n_present, float* grad_probs,
                              slu_stream_t stream) {
  if (!probs || !labels || !workspace || !loss || !n_present || B <= 0 || C <= 0 || HW <= 0) return SLU_EINVAL;
  const long long N = (long long)B * HW;
  if (N >= (1ll << 31) || C > 32) return SLU_EUNSUPPORTED;
  LovaszWs ws;
  if (carve((char*)workspace, N, C, ws) > workspace_bytes) return SLU_EINVAL;
  if (reinterpret_cast<uintptr_t>(workspace) & 255) return SLU_EINVAL;
  hipStream_t st = slu_stream(stream);
  const int nblk = nblk_of(N);
  if (hipMemsetAsync(ws.G, 0, align256((size_t)C * sizeof(unsigned)) + (size_t)C * sizeof(double), st) != hipSuccess) return SLU_ELAUNCH;
  hipLaunchKernelGGL(keygen_kernel, dim3(slu_grid_1d(N, 1024), C), dim3(kThreads), 0, st, probs, labels, B, C, HW, ignore_index, ws.sort.keys[0],
                     ws.sort.vals[0], ws.G);
  // which classes are sorted and summed: the present ones (flag = foreground count), or the caller's set whether present or not
  const unsigned* act = ws.G;
  if (class_mask) {
    hipLaunchKernelGGL(lovasz_set_active_kernel, dim3(1), dim3(64), 0, st, ws.act, C, class_mask);
    act = ws.act;
  }
  slu_sort_pairs(ws.sort, N, C, act, st);
  slu_sort_flag_prefix(ws.sort, N, C, act, st);
  // per-pixel gradient (class-major, pixel order): 4 C N bytes of the sort's idle buffers
  float* gtmp = grad_probs ? static_cast<float*>(slu_sort_idle(ws.sort)) : nullptr;
  hipLaunchKernelGGL(lovasz_steps_kernel, dim3(nblk, C), dim3(kThreads), 0, st, ws.sort.keys[0], ws.sort.vals[0], N, nblk, ws.G, act,
                     ws.sort.blkflag, ws.loss_c, gtmp);
  hipLaunchKernelGGL(lovasz_finalize_kernel, dim3(1), dim3(64), 0, st, act, ws.loss_c, C, loss, n_present);
  if (grad_probs)
    hipLaunchKernelGGL(lovasz_grad_layout_kernel, dim3(slu_grid_1d((size_t)B * C * HW, 8192)), dim3(256), 0, st, gtmp, act, n_present, B, C, HW,
                       grad_probs);
  SLU_CHECK_LAUNCH();
}
