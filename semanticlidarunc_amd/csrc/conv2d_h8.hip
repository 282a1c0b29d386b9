// Half-precision storage path ("h8"): activations live in HBM as fp16 in channel blocks of 8,
//     x[N][G = C/8][H][W][8]         (16 bytes per (pixel, block); azimuth-adjacent pixels are adjacent records)
// and every conv multiplies fp16 x fp16 on v_mfma_f32_32x32x16_f16 with fp32 accumulation and an fp32 epilogue
// (bias, LeakyReLU, folded BatchNorm, residual) before rounding the result to fp16 once.  The layout makes ONE
// 16-byte record = ONE MFMA B operand of one lane (lane (pixel r, half h) holds the 8 channels of block 2k+h), so
// staging a tile is a plain 16-byte copy (no conversion, no transpose), a wave's global loads / stores are 1 KB
// contiguous along the azimuth, and HBM traffic is half of the fp32 path.  BASELINE.json configs[2],[4] name this
// storage precision ("bf16"); fp16 is used instead because the activations of the range-image stack are O(1..100)
// and fp16's 11-bit mantissa keeps the logits within the 1e-3 parity bar (bf16 does not).
//
// This file: weight packing, the checks every conv shares (fill_h8) and the dispatch.  One file per kernel family, in dispatch order, each
// with its gate, launchers and one entry point (conv_h8.h, which also has what they share):
//   gemm1x1_h8.hip      gemm1x1_h8_kernel     wide 1x1 convs as a GEMM ring: 256 outputs, and 384 -> 128 with a residual
//   conv1x1_h8.h        conv1x1_h8_kernel     the other 1x1 convs, streaming: no halo => B operands straight from global memory, weights
//                                             through LDS; conv1x1_h8_res_kernel: <= 64 outputs, weights resident (also the fp32 logits head).
//                                             Compiled as part of conv_h8_tiled.hip (conv1x1_h8.h says why)
//   ring3_h8.hip        ring3_h8_kernel       full-resolution 3x3 convs with 32 / 64 channels: resident weights, deep input ring
//   conv_h8_tiled.hip   conv_h8_kernel        every other 3x3 / dilated / 2x2 / 1x1 conv: LDS tile [blocks][rows+halo][cols+halo] of 16-byte
//                                             records; conv_h8_late_kernel: the activation after the residual add (ResNet BasicBlock)
//   The layout / pooling / pixel-shuffle kernels around the convs are in layout_h8.hip.
#include "conv_h8.h"

using namespace slu_h8;

namespace {

// wpack[mblk][kstep][tap][lane][8]: lane (r, h) holds W[co = 32 mblk + r][ci = 16 kstep + 8 h + j][tap], j = 0..7, as fp16
__global__ void pack_h8_kernel(const float* __restrict__ w, int cout, int cin, int ks, int nks, size_t total, uint4* __restrict__ out) {
  const int T = ks * ks;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const int lane = (int)(e & 63);
    size_t r = e >> 6;
    const int tap = (int)(r % T);
    r /= T;
    const int k = (int)(r % nks);
    const int m = (int)(r / nks);
    const int co = m * 32 + (lane & 31);
    float x[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int ci = k * 16 + 8 * (lane >> 5) + j;
      x[j] = (co < cout && ci < cin) ? w[((size_t)co * cin + ci) * T + tap] : 0.0f;
    }
    out[e] = h8_pack8(x);
  }
}

// the one traversal of the h8 forward dispatch: slu_conv2d_h8_fwd launches at its leaf, slu_conv2d_h8_kernel_name has the leaf name itself
int conv_h8_dispatch(const slu_conv_h8_desc* d, const SluEmit& e) {
  H8Args a{};
  const int rc = fill_h8(d, a);
  if (rc != SLU_OK) return rc;
  if (d->act_after_resid) return h8_tiled(a, d, e);      // the late activation: one family implements it, none ignores it
  int st = -1;
  if (!a.src[0].shuf) {      // a source read through PixelShuffle in place: the ring or the tiled SCALED 3x3 kernels only
    st = h8_gemm1x1(a, d, e);
    if (st == -1) st = h8_conv1x1(a, d, e);
  }
  if (st == -1) st = h8_ring3(a, d, e);
  return st != -1 ? st : h8_tiled(a, d, e);
}

}  // namespace

int slu_h8::fill_h8(const slu_conv_h8_desc* d, H8Args& a) {
  if (!d || !d->out || !d->wpack || d->nsrc < 1 || d->nsrc > SLU_MAX_SRC) return SLU_EINVAL;
  if (d->N <= 0 || d->H <= 0 || d->W <= 0 || d->Cout <= 0) return SLU_EINVAL;
  if (d->bn_a && !d->bn_b) return SLU_EINVAL;
  if (d->has_act != 0 && d->has_act != 1) return SLU_EINVAL;
  if (d->has_act && !(d->slope >= 0.0f && d->slope <= 1.0f)) return SLU_EINVAL;      // LeakyReLU is evaluated as max(v, slope v)
  int g = 0;
  for (int s = 0; s < d->nsrc; ++s) {
    const slu_h8_src& S = d->src[s];
    if (!S.ptr || S.G <= 0 || S.nbatch < 0 || (S.shuffle != 0 && S.shuffle != 1)) return SLU_EINVAL;
    if (((uintptr_t)S.ptr & 15) || ((uintptr_t)S.scale & 15)) return SLU_EINVAL;
    // a shuffled source: the first one, whole groups of 64 stored channels (an even number of contributed blocks), even output size
    if (S.shuffle && (s != 0 || S.G % 8 || (d->H & 1) || (d->W & 1) || S.nbatch)) return SLU_EINVAL;
    const int gc = S.shuffle ? S.G / 4 : S.G;      // blocks this source contributes to the concatenated input
    a.src[s] = H8Src{reinterpret_cast<const uint4*>(S.ptr), S.scale, gc, g, S.nbatch, S.shuffle};
    g += gc;
  }
  for (int s = d->nsrc; s < SLU_MAX_SRC; ++s) a.src[s] = H8Src{nullptr, nullptr, 0, 0x7fffffff, 0, 0};
  if (((uintptr_t)d->out & 15) || ((uintptr_t)d->resid & 15) || ((uintptr_t)d->wpack & 15)) return SLU_EINVAL;
  if (d->resid && d->out_f32_nchw) return SLU_EINVAL;
  if (d->act_after_resid != 0 && d->act_after_resid != 1) return SLU_EINVAL;
  a.nsrc = d->nsrc;
  a.N = d->N; a.H = d->H; a.W = d->W;
  a.Gin = g;
  a.Cout = d->Cout;
  a.Gout = (d->Cout + 7) / 8;
  a.nmblk = (d->Cout + 31) / 32;
  a.nks = (g + 1) / 2;
  a.wpack = reinterpret_cast<const uint4*>(d->wpack);
  a.bias = d->bias; a.bn_a = d->bn_a; a.bn_b = d->bn_b;
  a.has_act = d->has_act; a.slope = d->slope;
  a.out_f32 = d->out_f32_nchw ? 1 : 0;
  a.tiles_x = a.tiles_y = 0;
#ifdef SLU_H8_AB
  static const int dbg = slu_env_int("SLU_GEMM_DBG", 0);
  a.dbg = dbg;
#endif
  return SLU_OK;
}

extern "C" size_t slu_packed_weight_bytes_h8(int cout, int cin, int ksize) {
  if (cout <= 0 || cin <= 0 || ksize <= 0) return 0;
  const size_t nmblk = (cout + 31) / 32, nks = (cin + 15) / 16;
  return nmblk * nks * (size_t)(ksize * ksize) * 64 * 16;
}

extern "C" int slu_pack_conv_weight_h8(const float* w, int cout, int cin, int ksize, void* out, slu_stream_t stream) {
  if (!w || !out) return SLU_EINVAL;
  const size_t bytes = slu_packed_weight_bytes_h8(cout, cin, ksize);
  if (bytes == 0) return SLU_EINVAL;
  const size_t total = bytes / 16;      // > 0: whole 1 KB fragments
  hipLaunchKernelGGL(pack_h8_kernel, dim3(slu_grid_1d(total, 32768)), dim3(256), 0, slu_stream(stream), w, cout, cin, ksize, (cin + 15) / 16, total,
                     reinterpret_cast<uint4*>(out));
  SLU_CHECK_LAUNCH();
}

extern "C" int slu_conv2d_h8_fwd(const slu_conv_h8_desc* d, slu_stream_t stream) { return conv_h8_dispatch(d, SluEmit{slu_stream(stream), nullptr, 0}); }

// name of the kernel instantiation slu_conv2d_h8_fwd launches for `d` (as rocprofv3 prints it), or the status with which it refuses `d`
extern "C" int slu_conv2d_h8_kernel_name(const slu_conv_h8_desc* d, char* buf, size_t n) {
  return buf ? conv_h8_dispatch(d, SluEmit{nullptr, buf, n}) : SLU_EINVAL;
}
