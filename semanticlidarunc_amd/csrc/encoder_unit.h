// What the encoder unit kernels share -- shuffle_unit.hip, fire_unit.hip, regnet_unit.hip: the two-source input record (slu_cat2, include/slu.h)
// on the host and in the kernels, the overlap rule, the small-map split, the output sizes and the A-fragment weight image.  As in pixel_common.h a
// device helper has the form with which each kernel compiles to the instructions of the copy it replaced: check a change here with
// tools/h8_isa_diff.py --match kernel (profiles/r30).
#pragma once
#include "pixel_common.h"

// ---- slu_cat2 on the host ------------------------------------------------------------------------------------------------------------------
// null source, non-positive size or a channel range outside its tensor: SLU_EINVAL
inline int slu_cat2_check(const slu_cat2& s, int N, int H, int W) {
  if (!s.src0 || N <= 0 || H <= 0 || W <= 0 || s.c0 <= 0 || s.ct0 <= 0 || s.coff0 < 0 || s.coff0 + s.c0 > s.ct0) return SLU_EINVAL;
  if (s.src1 ? (s.c1 <= 0 || s.ct1 < s.c1) : s.c1 != 0) return SLU_EINVAL;
  return SLU_OK;
}
// the images are a grid dimension and a pixel index is an int: SLU_EUNSUPPORTED beyond (the tile kernels; the element walks take any size)
inline int slu_unit_grid_check(int N, int H, int W) { return N > 65535 || (long long)H * W >= 0x7fffffffLL ? SLU_EUNSUPPORTED : SLU_OK; }

// a kernel's view: base pointers with the channel offset applied, the stored channel counts as batch strides
struct Cat2Args {
  const float* src0;      // first channel read of source 0
  const float* src1;      // source 1 or nullptr
  long long bs0, bs1;     // floats between two images of each source tensor
  int c0, C;              // channels taken from source 0, channels in all
};
template <class Args>     // Cat2Args or any argument struct with these fields
inline void slu_cat2_fill(Args& a, const slu_cat2& s, size_t HW) {
  a.src0 = s.src0 + (size_t)s.coff0 * HW;
  a.src1 = s.src1;
  a.bs0 = (long long)s.ct0 * HW;
  a.bs1 = (long long)s.ct1 * HW;
  a.c0 = s.c0;
  a.C = s.c0 + s.c1;
}

// "out must not overlap an input": the whole stored tensors count, not only the channels read
inline bool slu_overlaps(const float* a, size_t na, const float* b, size_t nb) { return a < b + nb && b < a + na; }
inline bool slu_cat2_overlaps(const slu_cat2& s, int N, size_t HW, const float* out, size_t nout) {
  return slu_overlaps(out, nout, s.src0, (size_t)N * s.ct0 * HW) || (s.src1 && slu_overlaps(out, nout, s.src1, (size_t)N * s.ct1 * HW));
}

// ---- launch shapes -------------------------------------------------------------------------------------------------------------------------
// Small maps leave most of the 256 CUs idle with one workgroup per tile: split the 32-channel output blocks over up to 4 workgroups per tile
// (each recomputes the tile's on-chip intermediate, which is cheap next to an idle CU) until there are about as many workgroups as CUs.
inline int slu_cu_fill_split(long long tiles, int nblocks) {
  int split = 1;
  while (split < 4 && tiles * split < 256 && nblocks >= 2 * split) split *= 2;
  return split;
}
inline int slu_strided_out(int n, int stride) { return (n + stride - 1) / stride; }      // 3x3 / pad 1 / stride, and [::stride]: ceil(n / stride)
inline int slu_ceil_pool3s2_out(int n) { return (n - 2) / 2 + 1; }                        // MaxPool2d(3, 2, 0, ceil_mode): ceil((n - 3) / 2) + 1

// ---- slu_cat2 in a kernel --------------------------------------------------------------------------------------------------------------------
// the plane of channel c < C: img0 / img1 are the caller's pointers to this image in the two sources (base + n * batch stride, with its own
// casts), `plane` the floats of a plane, pasted as written -- H * W stays the copy's left-to-right product (size_t)c * H * W.  A macro: as a
// forced-inline function regnet_sample2_kernel and maxpool3s2_ceil_kernel came out with commuted operands and all eight shuffle_tail_kernel
// instantiations changed.
#define CAT2_PLANE(c, c0, img0, img1, plane) ((c) < (c0) ? (img0) + (size_t)(c) * plane : (img1) + (size_t)((c) - (c0)) * plane)

// one element-walk kernel over a slu_cat2 (the ceil pool, the stride-2 sampling): checks, view, launch
template <class Kernel>
inline int slu_cat2_resample(Kernel kernel, const slu_cat2* in, float* y, int N, int H, int W, int OH, int OW, hipStream_t st) {
  const size_t HW = (size_t)H * W, total = (size_t)N * (in->c0 + in->c1) * OH * OW;
  if (slu_cat2_overlaps(*in, N, HW, y, total)) return SLU_EINVAL;
  Cat2Args a;
  slu_cat2_fill(a, *in, HW);
  hipLaunchKernelGGL(kernel, dim3(slu_grid_1d(total, 16384)), dim3(256), 0, st, a.src0, a.src1, a.bs0, a.bs1, a.c0, a.C, N, H, W, OH, OW, y);
  SLU_CHECK_LAUNCH();
}

// ---- the A-fragment weight image (include/slu.h, "Packed weights") ---------------------------------------------------------------------------
// W [rows][K][taps] with K-chunk kc -> [ceil(rows / 32)][taps][afrag_ksteps][64]
__host__ __device__ inline size_t afrag_ksteps(int K, int kc) { return (size_t)((K + kc - 1) / kc) * (kc / 2); }
__host__ __device__ inline size_t afrag_floats(int rows, int K, int kc, int taps) { return (size_t)((rows + 31) / 32) * taps * afrag_ksteps(K, kc) * 64; }
// element e of the image
__device__ __forceinline__ float afrag_element(const float* __restrict__ w, size_t e, int rows, int K, int kc, int taps) {
  const size_t ks = afrag_ksteps(K, kc);
  const int l = (int)(e & 63);
  size_t r = e >> 6;
  const int k2 = (int)(r % ks);
  r /= ks;
  const int tap = (int)(r % taps), m = (int)(r / taps);
  const int row = m * 32 + (l & 31), k = 2 * k2 + (l >> 5);
  return row < rows && k < K ? w[((size_t)row * K + k) * taps + tap] : 0.0f;
}
