// The middle of an EfficientNetV2 MBConv block (torchvision's MBConv: 1x1 expansion, depthwise 3x3, SqueezeExcitation with SiLU, 1x1 projection) in
// two launches; the 1x1 convs around it are the fused conv kernel.  The composed route (effnet_ops.hip: dwconv3x3_kernel, global_avgpool_kernel,
// then slu_se_gate) reads the expanded map -- the largest tensor of the block -- a second time only to average it.  The second launch, the gate
// over the tile sums, is slu_se_gate_psum in se_gate.hip.
//
//   dwconv3x3_se_kernel<S, VEC>   y[n, c, oy, ox] = silu(bias[c] + sum_{a, b} w[c, 3 a + b] x[n, c, S oy - 1 + a, S ox - 1 + b])   (pad 1, S = 1 / 2)
//                                 psum[n, c, t]   = sum of y[n, c] over the rows of output tile t
//     A workgroup of 256 owns one (image, channel, tile); a tile is a run of `rows` whole output rows (dwse_rows: about 2048 outputs, so the
//     8 x 256 plane of features[4] on a 64 x 2048 scan is ONE tile and the grid is N C workgroups).  The tile's receptive field -- (rows - 1) S + 3
//     input rows, zero outside the image -- goes through LDS once: 16-byte loads where W % 4 == 0 and x is 16-byte aligned, scalar loads
//     otherwise; an LDS row is [4 floats, the last one column -1 = 0][W columns][zeros up to a multiple of 4 + 4], so column x sits at x + 4 and
//     every row starts 16-byte aligned.  Only the row halo between two tiles is read twice.  VEC (OW % 4 == 0, y 16-byte aligned): a lane
//     computes four adjacent outputs of a row from one ds_read_b128 (two at S = 2) + the edge columns per input row and stores them as one
//     dwordx4; otherwise one output per step.  The nine weights and the bias are uniform over the workgroup: one scalar fetch.  Exact fp32: the
//     fmaf chain of dwconv3x3_kernel in the same (a, b) order (a padding tap adds w * 0), the same silu().
//     The sum: every lane adds what it stores in a fixed order, wave_sum, one LDS slot per wave, the four slots added in wave order by one
//     lane, one float per tile -- no atomics and no order between workgroups, so y and psum are bit-identical run to run.
#include "encoder_unit.h"

namespace {

constexpr int DWSE_TILE_OUTPUTS = 2048;      // outputs per tile aimed at: 8 per lane
constexpr size_t DWSE_MAX_LDS = 60 * 1024;      // of the 64 KiB a workgroup gets without opting in to more; the rest holds the wave slots

__host__ __device__ inline int dwse_pitch(int W) { return ((W + 3) & ~3) + 8; }

// output rows per tile: whole rows, about DWSE_TILE_OUTPUTS outputs, and a receptive field that fits DWSE_MAX_LDS (0: not even one row does)
int dwse_rows(int W, int OH, int OW, int stride) {
  int rows = DWSE_TILE_OUTPUTS / OW;
  rows = rows < 1 ? 1 : rows;
  rows = rows > OH ? OH : rows;
  const size_t row_bytes = (size_t)dwse_pitch(W) * 4;
  const size_t fit = DWSE_MAX_LDS / row_bytes;      // input rows that fit
  if (fit < 3) return 0;
  const int cap = (int)((fit - 3) / stride) + 1;
  return rows < cap ? rows : cap;
}

template <int S, bool VEC>
__global__ __launch_bounds__(256) void dwconv3x3_se_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                           float* __restrict__ y, float* __restrict__ psum, int C, int H, int W, int OH, int OW, int rows,
                                                           int T, int vec_load) {
  extern __shared__ __align__(16) float s_in[];      // [(rows - 1) S + 3][P]
  __shared__ float s_red[4];
  const int tid = threadIdx.x;
  const int t = blockIdx.x, c = blockIdx.y, n = blockIdx.z;
  const int P = dwse_pitch(W);
  const int oy0 = t * rows;
  const int nrows = min(rows, OH - oy0);      // the last tile may be ragged
  const int IR = (nrows - 1) * S + 3;
  const int iy0 = oy0 * S - 1;
  const size_t plane = (size_t)n * C + c;
  const float* __restrict__ xp = x + plane * (size_t)H * W;

  // the pads of every row: columns -4 .. -1 and W .. P - 5
  const int pw = P - W;
  for (int e = tid; e < IR * pw; e += 256) {
    const int r = e / pw, k = e - r * pw;
    s_in[r * P + (k < 4 ? k : W + k)] = 0.0f;
  }
  if (vec_load) {
    const int W4 = W >> 2;
    for (int e = tid; e < IR * W4; e += 256) {
      const int r = e / W4, q = e - r * W4;
      const int iy = iy0 + r;
      float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (iy >= 0 && iy < H) v = *reinterpret_cast<const float4*>(xp + (size_t)iy * W + 4 * q);
      *reinterpret_cast<float4*>(s_in + r * P + 4 + 4 * q) = v;
    }
  } else {
    for (int e = tid; e < IR * W; e += 256) {
      const int r = e / W, q = e - r * W;
      const int iy = iy0 + r;
      s_in[r * P + 4 + q] = (iy >= 0 && iy < H) ? xp[(size_t)iy * W + q] : 0.0f;
    }
  }
  float wt[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) wt[k] = w[(size_t)c * 9 + k];
  const float b = bias[c];
  __syncthreads();

  float* __restrict__ yp = y + plane * (size_t)OH * OW + (size_t)oy0 * OW;
  float part = 0.0f;
  if (VEC) {
    const int G = OW >> 2;
    for (int e = tid; e < nrows * G; e += 256) {
      const int ly = e / G, g = e - ly * G;
      // input columns S 4 g - 1 .. S (4 g + 3) + 1 of rows S ly .. S ly + 2 of the staged field; column x sits at x + 4
      const float* __restrict__ sp = s_in + (ly * S) * P + 4 * S * g + 3;
      float a0 = b, a1 = b, a2 = b, a3 = b;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const float* __restrict__ r = sp + a * P;
        const float l = r[0];
        const float4 m = *reinterpret_cast<const float4*>(r + 1);
        if (S == 1) {
          const float e5 = r[5];
          a0 = fmaf(wt[3 * a], l, a0);   a0 = fmaf(wt[3 * a + 1], m.x, a0); a0 = fmaf(wt[3 * a + 2], m.y, a0);
          a1 = fmaf(wt[3 * a], m.x, a1); a1 = fmaf(wt[3 * a + 1], m.y, a1); a1 = fmaf(wt[3 * a + 2], m.z, a1);
          a2 = fmaf(wt[3 * a], m.y, a2); a2 = fmaf(wt[3 * a + 1], m.z, a2); a2 = fmaf(wt[3 * a + 2], m.w, a2);
          a3 = fmaf(wt[3 * a], m.z, a3); a3 = fmaf(wt[3 * a + 1], m.w, a3); a3 = fmaf(wt[3 * a + 2], e5, a3);
        } else {
          const float4 h = *reinterpret_cast<const float4*>(r + 5);
          a0 = fmaf(wt[3 * a], l, a0);   a0 = fmaf(wt[3 * a + 1], m.x, a0); a0 = fmaf(wt[3 * a + 2], m.y, a0);
          a1 = fmaf(wt[3 * a], m.y, a1); a1 = fmaf(wt[3 * a + 1], m.z, a1); a1 = fmaf(wt[3 * a + 2], m.w, a1);
          a2 = fmaf(wt[3 * a], m.w, a2); a2 = fmaf(wt[3 * a + 1], h.x, a2); a2 = fmaf(wt[3 * a + 2], h.y, a2);
          a3 = fmaf(wt[3 * a], h.y, a3); a3 = fmaf(wt[3 * a + 1], h.z, a3); a3 = fmaf(wt[3 * a + 2], h.w, a3);
        }
      }
      const float4 o = make_float4(silu(a0), silu(a1), silu(a2), silu(a3));
      *reinterpret_cast<float4*>(yp + (size_t)ly * OW + 4 * g) = o;
      part += (o.x + o.y) + (o.z + o.w);
    }
  } else {
    for (int e = tid; e < nrows * OW; e += 256) {
      const int ly = e / OW, ox = e - ly * OW;
      const float* __restrict__ sp = s_in + (ly * S) * P + S * ox + 3;
      float acc = b;
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int k = 0; k < 3; ++k) acc = fmaf(wt[3 * a + k], sp[a * P + k], acc);
      const float o = silu(acc);
      yp[e] = o;
      part += o;
    }
  }
  BLOCK_PUT(wave_sum, part, s_red);
  __syncthreads();
  if (tid == 0) psum[plane * T + t] = BLOCK_TOTAL4(s_red);
}

template <int S>
int launch_dwse(const float* x, const float* w, const float* bias, float* y, float* psum, int N, int C, int H, int W, int OH, int OW, int rows, int T,
                hipStream_t st) {
  const size_t lds = (size_t)((rows - 1) * S + 3) * dwse_pitch(W) * 4;
  const int vec_load = (W % 4 == 0 && ((uintptr_t)x & 15) == 0) ? 1 : 0;
  const bool vec = OW % 4 == 0 && ((uintptr_t)y & 15) == 0;
  const dim3 grid((unsigned)T, (unsigned)C, (unsigned)N);
  if (vec)
    hipLaunchKernelGGL((dwconv3x3_se_kernel<S, true>), grid, dim3(256), lds, st, x, w, bias, y, psum, C, H, W, OH, OW, rows, T, vec_load);
  else
    hipLaunchKernelGGL((dwconv3x3_se_kernel<S, false>), grid, dim3(256), lds, st, x, w, bias, y, psum, C, H, W, OH, OW, rows, T, vec_load);
  SLU_CHECK_LAUNCH();
}

}  // namespace

extern "C" int slu_dwconv3x3_se_tiles(int H, int W, int stride) {
  if (H <= 0 || W <= 0 || (stride != 1 && stride != 2)) return 0;
  const int OH = slu_strided_out(H, stride), OW = slu_strided_out(W, stride);
  const int rows = dwse_rows(W, OH, OW, stride);
  return rows <= 0 ? 0 : (OH + rows - 1) / rows;
}

extern "C" int slu_dwconv3x3_se_fwd(const float* x, const float* w, const float* bias, float* y, float* psum, int N, int C, int H, int W, int stride,
                                    slu_stream_t stream) {
  if (!x || !w || !bias || !y || !psum || N <= 0 || C <= 0 || H <= 0 || W <= 0 || (stride != 1 && stride != 2)) return SLU_EINVAL;
  if (N > 65535 || C > 65535 || (long long)H * W >= 0x7fffffffLL) return SLU_EUNSUPPORTED;
  const int OH = slu_strided_out(H, stride), OW = slu_strided_out(W, stride);
  const int rows = dwse_rows(W, OH, OW, stride);
  if (rows <= 0) return SLU_EUNSUPPORTED;      // three input rows do not fit the LDS budget
  const int T = (OH + rows - 1) / rows;
  hipStream_t st = slu_stream(stream);
  return stride == 1 ? launch_dwse<1>(x, w, bias, y, psum, N, C, H, W, OH, OW, rows, T, st)
                     : launch_dwse<2>(x, w, bias, y, psum, N, C, H, W, OH, OW, rows, T, st);
}
