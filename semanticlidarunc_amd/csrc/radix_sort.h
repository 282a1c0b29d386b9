// The device radix sort of the losses and metrics (radix_sort.hip): `segs` independent segments of `n` (key, value)
// pairs each, [segs][n], sorted ascending by the 32-bit key, stable.  Users: lovasz.hip (one segment per class), auroc.hip and
// aurc.hip (one segment).  Internal to the library: nothing here is declared in slu.h or exported.
#pragma once
#include "slu_common.h"

namespace slu_sort {

constexpr int kThreads = 256;
constexpr int kItems = 8;                       // keys per thread per tile
constexpr int kTile = kThreads * kItems;        // 2048 keys per workgroup

__host__ __device__ inline int nblk_of(long long n) { return (int)((n + kTile - 1) / kTile); }

// value = element index | flag << 31 (n < 2^31).  The sort carries it along; slu_sort_flag_prefix counts the flag.
__device__ __forceinline__ unsigned make_val(long long i, bool flag) { return (unsigned)i | (flag ? 0x80000000u : 0u); }
__device__ __forceinline__ unsigned val_flag(unsigned v) { return v >> 31; }
__device__ __forceinline__ unsigned val_index(unsigned v) { return v & 0x7FFFFFFFu; }

// The ballot bits of the lanes before this one: with a wave on consecutive 64-element rows (sorted order == (wave, item, lane), as in
// the scatter) popcount(ballot & lanes_below) is an element's rank inside its row.
__device__ __forceinline__ unsigned long long lanes_below(int lane) { return (lane == 0) ? 0ull : (~0ull >> (64 - lane)); }

// Ordered keys of a float: key() is monotonic in the order named, bits() gives the float's bit pattern back.
struct KeyDescending {      // descending float == ascending key, any float: +NaN, +inf ... +0.0, -0.0 ... -inf, -NaN
  static __device__ __forceinline__ unsigned key(float s) {
    const unsigned u = __float_as_uint(s);
    const unsigned asc = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ~asc;
  }
  static __device__ __forceinline__ unsigned bits(unsigned key) {
    const unsigned asc = ~key;
    const unsigned m = (unsigned)((int)asc >> 31);                   // all ones for a non-negative float
    return asc ^ ~(m & 0x7FFFFFFFu);
  }
};
struct KeyAscendingFoldZero {      // ascending float == ascending key; -0.0 and +0.0 share one key, so bits() returns +0.0 for both
  static __device__ __forceinline__ unsigned key(float s) {
    unsigned u = __float_as_uint(s);
    if ((u << 1) == 0u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  }
  static __device__ __forceinline__ unsigned bits(unsigned key) { return (key & 0x80000000u) ? (key ^ 0x80000000u) : ~key; }
};

// One segment of samples (a float and a 0/1 flag each) into sort pairs, and the sorted pairs back into samples.  The keygen also
// writes the "segments to sort" word of a single-segment caller (see slu_sort_pairs): nobody else has to.  Internal linkage, as
// every kernel of the users: the library exports no kernel symbol for them.
namespace {

template <class Key>
__global__ __launch_bounds__(kThreads) void sample_keygen_kernel(const float* __restrict__ x, const uint8_t* __restrict__ flag, long long n,
                                                                 unsigned* __restrict__ keys, unsigned* __restrict__ vals,
                                                                 unsigned* __restrict__ sort_seg) {
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
    keys[i] = Key::key(x[i]);
    vals[i] = make_val(i, flag[i]);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) sort_seg[0] = 1u;
}

template <class Key>
__global__ __launch_bounds__(kThreads) void sample_unsort_kernel(const unsigned* __restrict__ keys, const unsigned* __restrict__ vals, long long n,
                                                                 float* __restrict__ x, uint8_t* __restrict__ flag) {
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
    reinterpret_cast<unsigned*>(x)[i] = Key::bits(keys[i]);
    flag[i] = (uint8_t)val_flag(vals[i]);
  }
}

}  // namespace
}  // namespace slu_sort

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// Hands out 256-byte aligned pieces of a caller-owned workspace, in call order.  base == nullptr only measures: take() returns
// nullptr and `off` ends as the size.
struct SluCarver {
  char* base;
  size_t off = 0;
  template <class T>
  T* take(size_t count) {
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += align256(count * sizeof(T));
    return p;
  }
};

// What the sort owns of a workspace.  The unsorted pairs go into keys[0] / vals[0]; slu_sort_pairs leaves the sorted ones there.
struct SluSortWs {
  unsigned* keys[2];
  unsigned* vals[2];
  unsigned* hist;          // [segs][nblk][256]
  unsigned* blkflag;       // [segs][nblk] slu_sort_flag_prefix: flagged values in the tiles before this one
};

// Carves the sort's buffers, in the order keys[0] vals[0] keys[1] vals[1] hist blkflag.
__attribute__((visibility("hidden"))) void slu_sort_carve(SluCarver& cv, long long n, int segs, SluSortWs& ws);

// After slu_sort_pairs the second buffer pair is idle: 8 * segs * n contiguous bytes from keys[1] on (keys[1] and vals[1] are carved
// back to back), free for the caller until the next sort.  Lovasz keeps its per-pixel gradient there, AURC its selective risks.
static inline void* slu_sort_idle(const SluSortWs& ws) { return ws.keys[1]; }

// Sorts every segment s with sort_seg[s] != 0 (a device array of `segs` words, read by the kernels: a workgroup of any other
// segment exits at once and that segment's buffers hold nothing defined).  A single-segment caller passes a word holding 1.
// Four 8-bit passes on `st`; launch errors are left for the caller's SLU_CHECK_LAUNCH.
__attribute__((visibility("hidden"))) void slu_sort_pairs(const SluSortWs& ws, long long n, int segs, const unsigned* sort_seg, hipStream_t st);

// Per tile of the sorted values, the exclusive prefix of the bit-31 flag over the segment's tiles -> ws.blkflag.
__attribute__((visibility("hidden"))) void slu_sort_flag_prefix(const SluSortWs& ws, long long n, int segs, const unsigned* sort_seg, hipStream_t st);
