// Decoder kernels of the CENet ResNet-34 baseline (reference src/baselines/CENet/CENet_ResNet34.py:165-184), both HBM-bound:
//   bilinear_ac_cat_kernel       F.interpolate(x_k, size = (H, W), mode = 'bilinear', align_corners = True) of up to three maps, each written
//                                into its channel slice of ONE [N, C_tot, H, W] buffer (:165-170: three interpolations + their part of torch.cat)
//   bilinear_ac_softmax_kernel   the same interpolation of a logit map with C <= 32 classes, then softmax over the classes (:173-184)
//   bilinear_ac_sum_kernel       the sum of the same interpolation of up to three maps of equal channel count (FIDNet's commuted head)
//
// The coordinate map (ATen's area_pixel_compute_source_index with align_corners = True): src = dst * (in - 1) / (out - 1), and 0 where out == 1
// or in == 1; i0 = floor(src), i1 = min(i0 + 1, in - 1), weights l1 = src - i0, l0 = 1 - l1;
//   y = l0y * (l0x * p[y0][x0] + l1x * p[y0][x1]) + l1y * (l0x * p[y1][x0] + l1x * p[y1][x1]).
// src is a ratio of integers, so i0 and the remainder r = dst * (in - 1) - i0 * (out - 1) are found exactly (ac_taps: one float multiply, one
// integer fix-up, no integer division) and l1 = r / (out - 1) is a correctly rounded quotient: the taps never sit on the wrong side of a source
// pixel, and in == out gives l1 = 0 and the input back bit for bit.
//
// The aux heads of the model use a 1x1 conv COMMUTED with the interpolation: the reference computes softmax(conv1x1(interpolate(x_k))), the model
// runs the 1x1 conv on the low-resolution x_k and hands its logits to slu_bilinear_ac_softmax.  The interpolation is linear with weights that sum
// to 1 per output pixel, so W (sum_t a_t x_t) + b = sum_t a_t (W x_t + b): equal in exact arithmetic, and equal to the reference order up to
// rounding (the sums are taken in another order), not bit for bit.
#include "class_column.h"

namespace {

template <class T>
struct AcTapT {
  int i0, i1;
  T l0, l1;
};
typedef AcTapT<float> AcTap;

// taps of destination index dst < n_out over n_in source samples, weights of type T.  den = n_out - 1, inv_den = 1.0f / den (anything when
// den == 0).  q = (int)(num * inv_den) is within 1 of floor(num / den) (num < 2^31 and the quotient < 2^22 are the launcher's checks), the two
// comparisons put it right.
template <class T>
__device__ __forceinline__ AcTapT<T> ac_taps(int dst, int n_in, int den, float inv_den) {
  AcTapT<T> t;
  if (den == 0 || n_in == 1) {
    t.i0 = t.i1 = 0;
    t.l0 = (T)1;
    t.l1 = (T)0;
    return t;
  }
  const int num = dst * (n_in - 1);
  int q = (int)((float)num * inv_den);
  int r = num - q * den;
  if (r < 0) { --q; r += den; }
  if (r >= den) { ++q; r -= den; }
  t.i0 = q;
  t.i1 = q + (q < n_in - 1 ? 1 : 0);
  t.l1 = (T)r / (T)den;
  t.l0 = (T)1 - t.l1;
  return t;
}

struct AcCatArgs {
  const float* ptr[3];
  int C[3], h[3], w[3], c_off[3];
  int nsrc, csum;      // csum = C[0] + C[1] + C[2]: the planes written per image
};

constexpr int AC_ROWS = 4;      // output rows per thread; a workgroup of 64 x 4 threads covers 256 columns x 16 rows of one plane

// horizontal pass of one source row for a thread's 4 columns
__device__ __forceinline__ float4 ac_hrow(const float* __restrict__ row, const AcTap (&tx)[4]) {
  float4 v;
  v.x = tx[0].l0 * row[tx[0].i0] + tx[0].l1 * row[tx[0].i1];
  v.y = tx[1].l0 * row[tx[1].i0] + tx[1].l1 * row[tx[1].i1];
  v.z = tx[2].l0 * row[tx[2].i0] + tx[2].l1 * row[tx[2].i1];
  v.w = tx[3].l0 * row[tx[3].i0] + tx[3].l1 * row[tx[3].i1];
  return v;
}

// grid (column tiles of 256, row tiles of 16, N * csum planes); a lane owns 4 adjacent columns (one 16-byte store where `vec`) of AC_ROWS
// consecutive rows and keeps the horizontally interpolated source rows y0 / y1 across them: going up by 2, 4 or 8 most output rows share
// theirs with the row above.
__global__ __launch_bounds__(256) void bilinear_ac_cat_kernel(AcCatArgs a, float* __restrict__ out, int C_tot, int H, int W, int vec) {
  const int n = blockIdx.z / a.csum;
  int c = blockIdx.z - n * a.csum;
  int k = 0;
  if (a.nsrc > 1 && c >= a.C[0]) { c -= a.C[0]; k = 1; }
  if (a.nsrc > 2 && k == 1 && c >= a.C[1]) { c -= a.C[1]; k = 2; }
  const int h = a.h[k], w = a.w[k];
  const float* __restrict__ p = a.ptr[k] + ((size_t)n * a.C[k] + c) * (size_t)h * w;
  float* __restrict__ q = out + ((size_t)n * C_tot + a.c_off[k] + c) * (size_t)H * W;

  const int ox = (blockIdx.x * 64 + threadIdx.x) * 4;
  if (ox >= W) return;
  const int denx = W - 1, deny = H - 1;
  const float inv_dx = 1.0f / (float)denx, inv_dy = 1.0f / (float)deny;
  AcTap tx[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) tx[j] = ac_taps<float>(min(ox + j, W - 1), w, denx, inv_dx);      // a column past W is computed in bounds and not stored

  const int oy0 = (blockIdx.y * 4 + threadIdx.y) * AC_ROWS;
  int cy0 = -1, cy1 = -1;
  float4 h0 = {}, h1 = {};
#pragma unroll
  for (int j = 0; j < AC_ROWS; ++j) {
    const int oy = oy0 + j;
    if (oy >= H) break;
    const AcTap ty = ac_taps<float>(oy, h, deny, inv_dy);
    if (ty.i0 != cy0) {
      if (ty.i0 == cy1) h0 = h1;
      else h0 = ac_hrow(p + (size_t)ty.i0 * w, tx);
      cy0 = ty.i0;
    }
    if (ty.i1 != cy1) {
      if (ty.i1 == cy0) h1 = h0;
      else h1 = ac_hrow(p + (size_t)ty.i1 * w, tx);
      cy1 = ty.i1;
    }
    float4 v;
    v.x = ty.l0 * h0.x + ty.l1 * h1.x;
    v.y = ty.l0 * h0.y + ty.l1 * h1.y;
    v.z = ty.l0 * h0.z + ty.l1 * h1.z;
    v.w = ty.l0 * h0.w + ty.l1 * h1.w;
    float* d = q + (size_t)oy * W + ox;
    if (vec) {
      *reinterpret_cast<float4*>(d) = v;
    } else {
      d[0] = v.x;
      if (ox + 1 < W) d[1] = v.y;
      if (ox + 2 < W) d[2] = v.z;
      if (ox + 3 < W) d[3] = v.w;
    }
  }
}

// out[n, c] = sum over k of the interpolation of src_k[n, c]: the walk of bilinear_ac_cat_kernel per source -- the same taps, the same two
// nested lerps -- with the terms added in source order in registers.  grid (column tiles of 256, row tiles of 16,
// N * C planes); every source has the C channels of `out`.  FIDNet's head (fidnet.py) runs its 1x1 conv over the three interpolated pyramid maps
// at their own low resolutions and sums the interpolated results here: the conv commutes with the interpolation (head of this file).
__global__ __launch_bounds__(256) void bilinear_ac_sum_kernel(AcCatArgs a, float* __restrict__ out, int H, int W, int vec) {
  const size_t plane = blockIdx.z;
  const int ox = (blockIdx.x * 64 + threadIdx.x) * 4;
  if (ox >= W) return;
  const int denx = W - 1, deny = H - 1;
  const float inv_dx = 1.0f / (float)denx, inv_dy = 1.0f / (float)deny;
  const int oy0 = (blockIdx.y * 4 + threadIdx.y) * AC_ROWS;
  float4 acc[AC_ROWS] = {};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (k < a.nsrc) {
      const int h = a.h[k], w = a.w[k];
      const float* __restrict__ p = a.ptr[k] + plane * (size_t)h * w;
      AcTap tx[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) tx[j] = ac_taps<float>(min(ox + j, W - 1), w, denx, inv_dx);
      int cy0 = -1, cy1 = -1;
      float4 h0 = {}, h1 = {};
#pragma unroll
      for (int j = 0; j < AC_ROWS; ++j) {
        const int oy = oy0 + j;
        if (oy < H) {
          const AcTap ty = ac_taps<float>(oy, h, deny, inv_dy);
          if (ty.i0 != cy0) {
            if (ty.i0 == cy1) h0 = h1;
            else h0 = ac_hrow(p + (size_t)ty.i0 * w, tx);
            cy0 = ty.i0;
          }
          if (ty.i1 != cy1) {
            if (ty.i1 == cy0) h1 = h0;
            else h1 = ac_hrow(p + (size_t)ty.i1 * w, tx);
            cy1 = ty.i1;
          }
          float4 v;
          v.x = ty.l0 * h0.x + ty.l1 * h1.x;
          v.y = ty.l0 * h0.y + ty.l1 * h1.y;
          v.z = ty.l0 * h0.z + ty.l1 * h1.z;
          v.w = ty.l0 * h0.w + ty.l1 * h1.w;
          if (k == 0) {
            acc[j] = v;      // not 0 + v: a single source at the output size comes back bit for bit, -0 included
          } else {
            acc[j].x += v.x, acc[j].y += v.y, acc[j].z += v.z, acc[j].w += v.w;
          }
        }
      }
    }
  }
  float* __restrict__ q = out + plane * (size_t)H * W;
#pragma unroll
  for (int j = 0; j < AC_ROWS; ++j) {
    const int oy = oy0 + j;
    if (oy < H) {
      float* d = q + (size_t)oy * W + ox;
      if (vec) {
        *reinterpret_cast<float4*>(d) = acc[j];
      } else {
        d[0] = acc[j].x;
        if (ox + 1 < W) d[1] = acc[j].y;
        if (ox + 2 < W) d[2] = acc[j].z;
        if (ox + 3 < W) d[3] = acc[j].w;
      }
    }
  }
}

// grid (column tiles of 256, H, N); a lane owns one output pixel and its class column (class_column.h), lanes of a wave are azimuth-adjacent.
// The interpolated logits and their maximum are kept in fp64 up to the subtraction of the maximum: a logit of magnitude 80 carries an fp32
// rounding of 4e-6, which the softmax turns into up to 1e-6 of a probability wherever two classes are close; v - max is small where the
// probability is not, so fp32 is enough from expf on.  The kernel is bound by its stores, the fp64 arithmetic hides behind them.
// same = (h == H && w == W): the logits are read directly (the main head).
template <int CMAX>
__global__ __launch_bounds__(256) void bilinear_ac_softmax_kernel(const float* __restrict__ x, float* __restrict__ y, int C, int h, int w, int H, int W,
                                                                  int same) {
  const int ox = blockIdx.x * 256 + threadIdx.x, oy = blockIdx.y;
  if (ox >= W) return;
  const size_t hw = (size_t)h * w, HW = (size_t)H * W;
  const float* __restrict__ p = x + (size_t)blockIdx.z * C * hw;
  float e[CMAX];
  if (same) {
    const float m = slu_load_column(p + (size_t)oy * w + ox, C, hw, -INFINITY, e);
#pragma unroll
    for (int c = 0; c < CMAX; ++c) e[c] -= m;
  } else {
    const AcTapT<double> ty = ac_taps<double>(oy, h, H - 1, 1.0f / (float)(H - 1));
    const AcTapT<double> tx = ac_taps<double>(ox, w, W - 1, 1.0f / (float)(W - 1));
    const float* __restrict__ r0 = p + (size_t)ty.i0 * w;
    const float* __restrict__ r1 = p + (size_t)ty.i1 * w;
    double v[CMAX];
    double m = -INFINITY;
#pragma unroll
    for (int c = 0; c < CMAX; ++c) {
      v[c] = -INFINITY;
      if (c < C) {
        const size_t o = c * hw;
        v[c] = ty.l0 * (tx.l0 * (double)r0[o + tx.i0] + tx.l1 * (double)r0[o + tx.i1]) +
               ty.l1 * (tx.l0 * (double)r1[o + tx.i0] + tx.l1 * (double)r1[o + tx.i1]);
      }
      m = fmax(m, v[c]);
    }
#pragma unroll
    for (int c = 0; c < CMAX; ++c) e[c] = (float)(v[c] - m);
  }
  const float se = slu_exp_sum_inplace(e, C, 0.0f);      // e[c] = expf(logit - max) for c < C
  float* __restrict__ d = y + (size_t)blockIdx.z * C * HW + (size_t)oy * W + ox;
#pragma unroll
  for (int c = 0; c < CMAX; ++c)
    if (c < C) d[c * HW] = e[c] / se;
}

// what ac_taps needs of one axis: dst * (in - 1) < 2^31 and a quotient below 2^22
inline bool ac_axis_ok(int n_in, int n_out) { return n_in >= 1 && n_out >= 1 && n_in < (1 << 22) && (long long)(n_out - 1) * (n_in - 1) < 0x7fffffffLL; }

}  // namespace

extern "C" int slu_bilinear_ac_cat(const slu_bilinear_src* srcs, int nsrc, float* out, int N, int C_tot, int H, int W, slu_stream_t stream) {
  if (!srcs || !out || nsrc < 1 || nsrc > 3 || N <= 0 || C_tot <= 0 || H <= 0 || W <= 0) return SLU_EINVAL;
  AcCatArgs a = {};
  a.nsrc = nsrc;
  for (int k = 0; k < nsrc; ++k) {
    const slu_bilinear_src& s = srcs[k];
    if (!s.ptr || s.C <= 0 || s.h <= 0 || s.w <= 0 || s.c_off < 0 || (long long)s.c_off + s.C > C_tot) return SLU_EINVAL;
    for (int j = 0; j < k; ++j)      // two sources writing one channel would race
      if (s.c_off < srcs[j].c_off + srcs[j].C && srcs[j].c_off < s.c_off + s.C) return SLU_EINVAL;
    if (!ac_axis_ok(s.h, H) || !ac_axis_ok(s.w, W)) return SLU_EUNSUPPORTED;
    a.ptr[k] = s.ptr;
    a.C[k] = s.C, a.h[k] = s.h, a.w[k] = s.w, a.c_off[k] = s.c_off;
    a.csum += s.C;
  }
  const long long planes = (long long)N * a.csum;
  const unsigned gy = (unsigned)((H + 4 * AC_ROWS - 1) / (4 * AC_ROWS));
  if (planes > 65535 || gy > 65535) return SLU_EUNSUPPORTED;
  const int vec = W % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
  const dim3 grid((unsigned)((W + 255) / 256), gy, (unsigned)planes);
  hipLaunchKernelGGL(bilinear_ac_cat_kernel, grid, dim3(64, 4), 0, slu_stream(stream), a, out, C_tot, H, W, vec);
  SLU_CHECK_LAUNCH();
}

extern "C" int slu_bilinear_ac_sum(const slu_bilinear_src* srcs, int nsrc, float* out, int N, int C, int H, int W, slu_stream_t stream) {
  if (!srcs || !out || nsrc < 1 || nsrc > 3 || N <= 0 || C <= 0 || H <= 0 || W <= 0) return SLU_EINVAL;
  AcCatArgs a = {};
  a.nsrc = nsrc;
  a.csum = C;
  for (int k = 0; k < nsrc; ++k) {
    const slu_bilinear_src& s = srcs[k];
    if (!s.ptr || s.C != C || s.h <= 0 || s.w <= 0 || s.c_off != 0) return SLU_EINVAL;
    if (!ac_axis_ok(s.h, H) || !ac_axis_ok(s.w, W)) return SLU_EUNSUPPORTED;
    a.ptr[k] = s.ptr;
    a.C[k] = C, a.h[k] = s.h, a.w[k] = s.w;
  }
  const long long planes = (long long)N * C;
  const unsigned gy = (unsigned)((H + 4 * AC_ROWS - 1) / (4 * AC_ROWS));
  if (planes > 65535 || gy > 65535) return SLU_EUNSUPPORTED;
  const int vec = W % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
  const dim3 grid((unsigned)((W + 255) / 256), gy, (unsigned)planes);
  hipLaunchKernelGGL(bilinear_ac_sum_kernel, grid, dim3(64, 4), 0, slu_stream(stream), a, out, H, W, vec);
  SLU_CHECK_LAUNCH();
}

extern "C" int slu_bilinear_ac_softmax(const float* x, float* y, int N, int C, int h, int w, int H, int W, slu_stream_t stream) {
  if (!x || !y || N <= 0 || C <= 0 || C > 32 || h <= 0 || w <= 0 || H <= 0 || W <= 0) return SLU_EINVAL;
  if (!ac_axis_ok(h, H) || !ac_axis_ok(w, W) || N > 65535 || H > 65535) return SLU_EUNSUPPORTED;
  const dim3 grid((unsigned)((W + 255) / 256), (unsigned)H, (unsigned)N);
  const int same = h == H && w == W;
  slu_class_cap(C, [&](auto cap) {
    hipLaunchKernelGGL(bilinear_ac_softmax_kernel<decltype(cap)::value>, grid, dim3(256), 0, slu_stream(stream), x, y, C, h, w, H, W, same);
  });
  SLU_CHECK_LAUNCH();
}
