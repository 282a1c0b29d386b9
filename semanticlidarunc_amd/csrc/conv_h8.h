// What more than one h8 conv kernel family names (conv2d_h8.hip has the map of the families): the argument structs, the source selection, the
// shared epilogues and the families' entry points.  Internal to the library: nothing here is declared in slu.h or exported.
#pragma once
#include "h8_common.h"

namespace slu_h8 {      // named: the structs are parameter types of functions that cross translation units

struct H8Src {
  const uint4* ptr;    // [nimg][G][H][W] records
  const float* scale;  // [N][8 G] fp32 multiplier per (output image, channel) or nullptr
  int G;               // channel blocks of the stored tensor
  int gbeg;            // first block of this source in the concatenated input
  int nb;              // 0: holds N images; k > 0: holds k images, output image n reads n % k
  int shuf;            // 1: read through PixelShuffle(2) in place: ptr is [nimg][4 G][H/2][W/2] with its channels stored in shuffle order (slu.h)
};

struct H8Args {
  H8Src src[SLU_MAX_SRC];
  int nsrc;
  int N, H, W, Gin, Cout, Gout, nmblk, nks;   // nks = 16-channel K-steps = ceil(Gin / 2)
  const uint4* wpack;
  const float *bias, *bn_a, *bn_b;
  int has_act;
  float slope;
  int out_f32;         // 1: `out` is fp32 NCHW [N][Cout][H][W] (the logits head); 0: h8
  int tiles_x, tiles_y;
  int order;                 // 0: each workgroup walks a contiguous run of tiles; 1: tiles interleaved across workgroups
#ifdef SLU_H8_AB
  int dbg;                   // ablation switches of gemm1x1_h8_kernel (SLU_GEMM_DBG, -DSLU_H8_AB builds only): 1 no input DMA, 2 no weight DMA, 4 no MFMA
#endif
};

// descriptor -> H8Args after the checks every family shares (conv2d_h8.hip)
__attribute__((visibility("hidden"))) int fill_h8(const slu_conv_h8_desc* d, H8Args& a);

// One entry per family: the status of its launch (or, with e.name, of writing the name of the instantiation it would launch), a refusal
// status, or -1 for "not mine, try the next".  h8_tiled is the last resort and never answers -1; it also owns the late activation
// (slu_conv_h8_desc.act_after_resid) and the SCALED 3x3 form of a source read through PixelShuffle in place.
__attribute__((visibility("hidden"))) int h8_gemm1x1(H8Args& a, const slu_conv_h8_desc* d, const SluEmit& e);      // gemm1x1_h8.hip
__attribute__((visibility("hidden"))) int h8_conv1x1(H8Args& a, const slu_conv_h8_desc* d, const SluEmit& e);      // conv1x1_h8.h
__attribute__((visibility("hidden"))) int h8_ring3(H8Args& a, const slu_conv_h8_desc* d, const SluEmit& e);        // ring3_h8.hip
__attribute__((visibility("hidden"))) int h8_tiled(H8Args& a, const slu_conv_h8_desc* d, const SluEmit& e);        // conv_h8_tiled.hip

inline bool any_scale(const slu_conv_h8_desc* d) {
  for (int s = 0; s < d->nsrc; ++s)
    if (d->src[s].scale) return true;
  return false;
}

inline bool h8_one_plain_source(const H8Args& a) { return a.nsrc == 1 && a.src[0].nb == 0 && !a.src[0].scale; }

namespace {

// While all families were one translation unit, ring3_h8_kernel's staging lambda (which names h8_zero_rec itself) made the compiler treat the
// record as used by host code: it got external linkage and every kernel of the unit reads its address from the GOT.  This host-side use
// keeps that linkage, and with it each kernel's instruction stream (tools/h8_isa_diff.py, profiles/r17), in the units that no longer hold
// that lambda.  Dropping it saves the kernels one scalar load in their prologue: a kernel change, to be measured as one.
[[maybe_unused]] const void* const h8_zero_rec_host_use = &h8_zero_rec;

struct SrcSel {
  const uint4* ptr;
  const float* scale;
  int G, gl, ns;
};

__device__ __forceinline__ SrcSel select_src(const H8Args& a, const int (&img)[SLU_MAX_SRC], int g) {
  SrcSel p{a.src[0].ptr, a.src[0].scale, a.src[0].G, g, img[0]};
#pragma unroll
  for (int s = 1; s < SLU_MAX_SRC; ++s)
    if (s < a.nsrc && g >= a.src[s].gbeg) p = SrcSel{a.src[s].ptr, a.src[s].scale, a.src[s].G, g - a.src[s].gbeg, img[s]};
  return p;
}

// Epilogue shared by both kernels: one 32-channel x 32-pixel accumulator tile of a lane -> 4 x (4 channels)
//   chan0: first channel of the 32-block; se: LDS constants bias | bn_a | bn_b indexed by `cl0 + ...`
template <int STRIDE>
__device__ __forceinline__ void store_tile(const H8Args& a, const f32x16& acc, const float* se, int cl0, int co0, int hh, bool pix_ok,
                                           size_t n, size_t pix, size_t HW, const void* __restrict__ resid, void* __restrict__ out,
                                           float slope_pre) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int cl = cl0 + 8 * q + 4 * hh + k;
      float t = acc[4 * q + k] + se[cl];
      t = t > 0.0f ? t : t * slope_pre;
      v[k] = t * se[STRIDE + cl] + se[2 * STRIDE + cl];
    }
    const int co = co0 + 8 * q + 4 * hh;           // first of this lane's 4 channels
    if (a.out_f32) {
      float* o = reinterpret_cast<float*>(out);
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (pix_ok && co + k < a.Cout) o[(n * a.Cout + co + k) * HW + pix] = v[k];
    } else {
      const int go = co >> 3;
      const bool ok = pix_ok && go < a.Gout;
      const size_t idx = ok ? ((n * a.Gout + go) * HW + pix) * 2 + hh : 0;   // 8-byte half records
      if (resid) {
        const uint2 rv = reinterpret_cast<const uint2*>(resid)[idx];
        const half2v r0 = __builtin_bit_cast(half2v, rv.x), r1 = __builtin_bit_cast(half2v, rv.y);
        v[0] += (float)r0[0]; v[1] += (float)r0[1]; v[2] += (float)r1[0]; v[3] += (float)r1[1];
      }
      if (ok) reinterpret_cast<uint2*>(out)[idx] = make_uint2(pack2(v[0], v[1]), pack2(v[2], v[3]));
    }
  }
}

// Epilogue of the persistent kernel (h8 output): EVERY lane issues its 4 stores (and its 4 residual loads when they were
// not prefetched) -- lanes outside the image / past the last channel block read the zero record and store to a scratch
// record -- so the number of vector-memory operations per tile is a compile-time constant the kernel's counted waits rely on.
// LATE (conv_h8_late_kernel): the activation comes AFTER the residual add, out = leaky(conv + bias + resid) with slope `slope_late`; the caller
// passes slope_pre = 1 and the layer carries no folded BatchNorm (its constants are the defaults 1 / 0).
template <int STRIDE, bool PRE, bool LATE = false>
__device__ __forceinline__ void store_tile_full(const H8Args& a, const f32x16& acc, const float* se, int cl0, int go0, int hh, bool pix_ok, size_t n,
                                                size_t pix, size_t HW, const uint2* __restrict__ resid, const uint2 (&rv)[4],
                                                uint2* __restrict__ out, float slope_pre, uintptr_t zero_addr, uintptr_t trash_addr,
                                                float slope_late = 1.0f) {
  const float4* se4 = reinterpret_cast<const float4*>(se);
  const float2v sl = {slope_pre, slope_pre};
  const size_t plane2 = HW * 2;
  const size_t idx0 = ((n * a.Gout + go0) * HW + pix) * 2 + hh;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int c4 = (cl0 + 8 * q) / 4 + hh;
    H8Quad t = h8_epilogue(acc, q, se4[c4], se4[STRIDE / 4 + c4], se4[2 * STRIDE / 4 + c4], sl);
    const bool ok = pix_ok && go0 + q < a.Gout;
    const size_t idx = idx0 + q * plane2;
    if (resid) h8_add_resid(t, PRE ? rv[q] : *(ok ? resid + idx : reinterpret_cast<const uint2*>(zero_addr)));
    if constexpr (LATE) h8_leaky(t, float2v{slope_late, slope_late});
    *(ok ? out + idx : reinterpret_cast<uint2*>(trash_addr)) = pack4(t);
  }
}

// The same epilogue with whole 16-byte records on the way out (h8_swap16): lane half 0 stores the record of block 2 pr and lane half 1
// that of block 2 pr + 1 -- 2 store instructions per accumulator tile instead of 4.  The residual is added before the exchange from 8-byte
// loads of the lane's own channels, each waited for in full where it is used: rare on the layers the TILED kernel serves; the GEMM, whose
// 768 -> 256 layers all carry one, has its own form (gemm_store_tile) and keeps this one as its A/B fallback.  The tensor-or-trash choice
// goes through an integer, so the loads and stores here are FLAT operations (they count in lgkmcnt as well as vmcnt).
template <int STRIDE, bool LATE = false>
__device__ __forceinline__ void store_tile_swap16(const H8Args& a, const f32x16& acc, const float* se, int cl0, int go0, int hh, bool pix_ok, size_t n,
                                                  size_t pix, size_t HW, const uint2* __restrict__ resid, uint4* __restrict__ out, float slope_pre,
                                                  uintptr_t zero_addr, uintptr_t trash_addr, float slope_late = 1.0f) {
  const float4* se4 = reinterpret_cast<const float4*>(se);
  const float2v sl = {slope_pre, slope_pre};
#pragma unroll
  for (int pr = 0; pr < 2; ++pr) {
    unsigned hw[4];
#pragma unroll
    for (int q2 = 0; q2 < 2; ++q2) {
      const int q = 2 * pr + q2;
      const int c4 = (cl0 + 8 * q) / 4 + hh;
      H8Quad t = h8_epilogue(acc, q, se4[c4], se4[STRIDE / 4 + c4], se4[2 * STRIDE / 4 + c4], sl);
      if (resid) {
        const bool okq = pix_ok && go0 + q < a.Gout;
        h8_add_resid(t, *(okq ? resid + (((n * a.Gout + go0 + q) * HW + pix) * 2 + hh) : reinterpret_cast<const uint2*>(zero_addr)));
      }
      if constexpr (LATE) h8_leaky(t, float2v{slope_late, slope_late});
      hw[2 * q2] = pack2(t.t0);
      hw[2 * q2 + 1] = pack2(t.t1);
    }
    const uint4 rec = h8_swap16(hw[0], hw[1], hw[2], hw[3]);
    const int go = go0 + 2 * pr + hh;
    *((pix_ok && go < a.Gout) ? out + ((n * a.Gout + go) * HW + pix) : reinterpret_cast<uint4*>(trash_addr)) = rec;
  }
}

}  // namespace

}  // namespace slu_h8
