// GroupNorm apply + ReLU + 1x1 segmentation head + MC-dropout reduction in one pass (exact-fp32 path; the fp32 / f16x3 FPN models):
//   v_t      = relu((x_t - mean) * rstd * gamma + beta)      (groupnorm_apply_kernel's expression, fpn_ops.hip; statistics from
//                                                              slu_groupnorm_stats)
//   logits_t = W v_t + b                                      (semanticFCN_opt.py:296, a 1x1 conv over the UpsampleBlock output)
//   p_t      = exp(log_softmax(logits_t));  p_bar = mean_t p_t;  H = -sum clamp(p_bar) log clamp(p_bar) / ln C
//   MI       = max((H_bar - mean_t H[p_t]) / ln C, 0);  preds = argmax_c p_bar          (mc_reduce_kernel, uncertainty.hip)
// Unfused, every pass writes the normalised tensor and C fp32 logit maps that the next kernel reads back; here x is read once and nothing
// but the four results is written.  A wave owns 128 pixels of one scan and walks its T passes.  The product runs on
// v_mfma_f32_32x32x2_f32 (== a k-ordered fmaf chain): classes padded to M = 32, pixels on N, channels in K-steps of 2; lane l feeds channel
// 2 s + (l >> 5) of pixel column l & 31.  With 16-byte loads a lane holds 4 adjacent pixels, which are the same column of 4 accumulators,
// so the results leave as 16-byte stores too.  The class axis of a pixel lies in TWO lanes (l and l ^ 32 hold classes 8 q + 4 h + k), so
// max / sum / entropy / argmax finish with one cross-half exchange each.  The weights ([Cin][32], zero-padded), gamma / beta and the
// group of every channel sit in LDS; x and its statistics are requested a chunk of channels ahead of the arithmetic.
#include <math.h>
#include "slu_common.h"

namespace {

constexpr int HM_KC = 4;          // K-steps (channel pairs) per chunk: what a lane keeps in flight ahead of the MFMAs
constexpr int HM_CMAX = 128;      // head input channels covered
constexpr int HM_TILE = 128;      // pixels per wave

struct HmChunk {
  float x[HM_KC][4];
  float mean[HM_KC], rstd[HM_KC];
};

// the expression of groupnorm_apply_kernel, compiled under the same contraction rules
__device__ __forceinline__ float hm_norm(float x, float mean, float rstd, float gamma, float beta) { return (x - mean) * rstd * gamma + beta; }

// NQ = ceil(C / 8): accumulator groups of 8 classes with a live class (rows r < 4 NQ kept; dead rows of the last group get logit -inf).
// VEC: pixel of accumulator q, column j is 4 j + q (one float4 per lane and channel); else 32 q + j (four dword loads).
template <int NQ, bool VEC, bool GN>
__global__ __launch_bounds__(256) void head_mc_f32_kernel(const float* __restrict__ x, int T, int B, int Cin, int HW, const float* __restrict__ gn_mean,
                                                          const float* __restrict__ gn_rstd, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, int groups, int relu, const float* __restrict__ w,
                                                          const float* __restrict__ bias, int C, float eps, float lnC, float* __restrict__ p_bar,
                                                          float* __restrict__ h_norm, float* __restrict__ mi_norm, int64_t* __restrict__ preds) {
#pragma clang fp contract(off)
  constexpr int NR = 4 * NQ, R0 = NR - 4;
  __shared__ float wl[HM_CMAX * 32];          // wl[k][i] = w[i][k], 0 for i >= C or k >= Cin
  __shared__ float2 gb[HM_CMAX];              // gamma, beta (1, 0 where absent or k >= Cin)
  __shared__ int grp[HM_CMAX];                // group of channel k (clamped to a valid one for k >= Cin)
  for (int e = threadIdx.x; e < HM_CMAX * 32; e += 256) {
    const int k = e >> 5, i = e & 31;
    wl[e] = (i < C && k < Cin) ? w[(size_t)i * Cin + k] : 0.0f;
  }
  if (threadIdx.x < HM_CMAX) {
    const int k = threadIdx.x, kc = k < Cin ? k : Cin - 1;
    gb[k] = make_float2((gamma && k < Cin) ? gamma[k] : 1.0f, (beta && k < Cin) ? beta[k] : 0.0f);
    grp[k] = GN ? kc / (Cin / groups) : 0;
  }
  __syncthreads();

  const int lane = threadIdx.x & 63, hh = lane >> 5, jj = lane & 31;
  const int nch = (Cin + 2 * HM_KC - 1) / (2 * HM_KC);
  const int tiles = (HW + HM_TILE - 1) / HM_TILE;
  const long long nblk = (long long)B * tiles;
  const long long wave0 = (long long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nwave = (long long)gridDim.x * 4;
  float bs[NR];
  bool live[4];
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    const int c = slu_frag_row(0, r, hh);
    const bool ok = c < C;
    if (r >= R0) live[r - R0] = ok;
    bs[r] = (ok && bias) ? bias[c] : 0.0f;
  }
  const float invT = 1.0f / (float)T, eps_log_eps = eps > 0.0f ? eps * logf(eps) : 0.0f;

  for (long long blk = wave0; blk < nblk; blk += nwave) {
    const int b = (int)(blk / tiles);
    const int p0 = (int)(blk - (long long)b * tiles) * HM_TILE;
    int pix[4];
    bool pok[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      pix[q] = p0 + (VEC ? 4 * jj + q : 32 * q + jj);
      pok[q] = pix[q] < HW;
    }
    // chunk ch of pass t: channels 2 HM_KC ch + 2 k + hh.  A masked element reads element 0 of x (always mapped) and counts as 0.
    auto load_chunk = [&](HmChunk& d, int t, int ch) {
      const size_t n = (size_t)t * B + b;
#pragma unroll
      for (int k = 0; k < HM_KC; ++k) {
        const int c = 2 * HM_KC * ch + 2 * k + hh;
        const bool cok = c < Cin;
        const size_t base = (n * Cin + c) * (size_t)HW;
        if constexpr (VEC) {
          const bool ok = cok && pok[0];
          const float4 v = *reinterpret_cast<const float4*>(x + (ok ? base + pix[0] : 0));
          d.x[k][0] = ok ? v.x : 0.0f; d.x[k][1] = ok ? v.y : 0.0f; d.x[k][2] = ok ? v.z : 0.0f; d.x[k][3] = ok ? v.w : 0.0f;
        } else {
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const bool ok = cok && pok[q];
            const float v = x[ok ? base + pix[q] : 0];
            d.x[k][q] = ok ? v : 0.0f;
          }
        }
        if constexpr (GN) {
          const size_t gi = n * groups + grp[c];
          d.mean[k] = gn_mean[gi];
          d.rstd[k] = gn_rstd[gi];
        }
      }
    };

    float psum[4][NR], hsum[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      hsum[q] = 0.0f;
#pragma unroll
      for (int r = 0; r < NR; ++r) psum[q][r] = 0.0f;
    }
    HmChunk nx;
    load_chunk(nx, 0, 0);
    for (int t = 0; t < T; ++t) {
      f32x16 acc[4];
      SLU_ZERO_ACC(acc, 4);
      for (int ch = 0; ch < nch; ++ch) {
        const HmChunk cur = nx;
        const bool wrap = ch + 1 == nch;
        if (!wrap || t + 1 < T) load_chunk(nx, wrap ? t + 1 : t, wrap ? 0 : ch + 1);   // uniform; the chunk after the last does not exist
#pragma unroll
        for (int k = 0; k < HM_KC; ++k) {
          const int c = 2 * HM_KC * ch + 2 * k + hh;
          const float a = wl[c * 32 + jj];
          const float2 g = gb[c];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            float v = cur.x[k][q];
            if constexpr (GN) v = hm_norm(v, cur.mean[k], cur.rstd[k], g.x, g.y);
            v = relu ? fmaxf(v, 0.0f) : v;
            acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, v, acc[q], 0, 0, 0);
          }
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float z[NR], m = -INFINITY;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
          z[r] = acc[q][r] + bs[r];
          if (r >= R0) z[r] = live[r - R0] ? z[r] : -INFINITY;
          m = fmaxf(m, z[r]);
        }
        m = fmaxf(m, __shfl_xor(m, 32, 64));
        // one exp per class and pass: p = e / sum(e), and log p = (z - m) - log(sum e) is already known (the clamp at eps, which the
        // reference applies before the log, only matters for p < eps: there the term is the constant eps log eps)
        float e[NR], se = 0.0f;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
          e[r] = expf(z[r] - m);                           // a dead row: exp(-inf) = 0
          se += e[r];
        }
        se += __shfl_xor(se, 32, 64);
        const float lse = logf(se), rse = 1.0f / se;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
          const float p = e[r] * rse;
          psum[q][r] = __builtin_fmaf(e[r], rse, psum[q][r]);
          // -p log p added the way the final entropy adds its terms (one rounding each), so equal passes give MI = 0, not a rounding residue
          const float ht = p >= eps ? __builtin_fmaf(-p, z[r] - m - lse, hsum[q]) : hsum[q] - eps_log_eps;
          hsum[q] = (r >= R0 && !live[r - R0]) ? hsum[q] : ht;   // a dead row has p = 0 < eps but is no class: it adds nothing
        }
      }
    }

    float hn[4], mi[4];
    int arg[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float hb = 0.0f, best = -INFINITY;
      int ar = 0;
#pragma unroll
      for (int r = 0; r < NR; ++r)
        if (r < R0 || live[r - R0]) {
          const float p = psum[q][r] * invT;
          psum[q][r] = p;
          if (p > best) { best = p; ar = slu_frag_row(0, r, hh); }   // classes ascend with r: the first maximum of this lane's share
          const float pc = fmaxf(p, eps);
          hb = __builtin_fmaf(-pc, logf(pc), hb);
        }
      hb += __shfl_xor(hb, 32, 64);
      const float hs = hsum[q] + __shfl_xor(hsum[q], 32, 64);
      const float ob = __shfl_xor(best, 32, 64);
      const int oa = __shfl_xor(ar, 32, 64);
      if (ob > best || (ob == best && oa < ar)) ar = oa;             // first maximum over all classes, like argmax
      hn[q] = hb / lnC;
      mi[q] = fmaxf(__builtin_fmaf(-hs, invT, hb) / lnC, 0.0f);
      arg[q] = ar;
    }
    if constexpr (VEC) {
      if (pok[0]) {
#pragma unroll
        for (int r = 0; r < NR; ++r)
          if (r < R0 || live[r - R0])
            *reinterpret_cast<float4*>(p_bar + ((size_t)b * C + slu_frag_row(0, r, hh)) * HW + pix[0]) =
                make_float4(psum[0][r], psum[1][r], psum[2][r], psum[3][r]);
        const size_t o = (size_t)b * HW + pix[0];
        if (hh == 0) {
          *reinterpret_cast<float4*>(h_norm + o) = make_float4(hn[0], hn[1], hn[2], hn[3]);
          *reinterpret_cast<float4*>(mi_norm + o) = make_float4(mi[0], mi[1], mi[2], mi[3]);
        } else {
          *reinterpret_cast<longlong2*>(preds + o) = make_longlong2(arg[0], arg[1]);
          *reinterpret_cast<longlong2*>(preds + o + 2) = make_longlong2(arg[2], arg[3]);
        }
      }
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (pok[q]) {
#pragma unroll
          for (int r = 0; r < NR; ++r)
            if (r < R0 || live[r - R0]) p_bar[((size_t)b * C + slu_frag_row(0, r, hh)) * HW + pix[q]] = psum[q][r];
          const size_t o = (size_t)b * HW + pix[q];
          if (hh == 0) {
            h_norm[o] = hn[q];
            mi_norm[o] = mi[q];
          } else {
            preds[o] = arg[q];
          }
        }
    }
  }
}

template <int NQ, bool VEC>
void launch_head_mc_f32(bool gn, dim3 grid, hipStream_t st, const float* x, int T, int B, int Cin, int HW, const float* mean, const float* rstd,
                        const float* gamma, const float* beta, int groups, int relu, const float* w, const float* bias, int C, float eps, float lnC,
                        float* p_bar, float* h_norm, float* mi_norm, int64_t* preds) {
  if (gn)
    hipLaunchKernelGGL((head_mc_f32_kernel<NQ, VEC, true>), grid, dim3(256), 0, st, x, T, B, Cin, HW, mean, rstd, gamma, beta, groups, relu, w, bias, C,
                       eps, lnC, p_bar, h_norm, mi_norm, preds);
  else
    hipLaunchKernelGGL((head_mc_f32_kernel<NQ, VEC, false>), grid, dim3(256), 0, st, x, T, B, Cin, HW, mean, rstd, gamma, beta, groups, relu, w, bias, C,
                       eps, lnC, p_bar, h_norm, mi_norm, preds);
}

}  // namespace

extern "C" int slu_head_mc_f32(const float* x, int T, int B, int Cin, int HW, const float* gn_mean, const float* gn_rstd, const float* gn_gamma,
                               const float* gn_beta, int groups, int relu, const float* w, const float* bias, int C, float eps, float* p_bar,
                               float* h_norm, float* mi_norm, int64_t* preds, slu_stream_t stream) {
  if (!x || !w || !p_bar || !h_norm || !mi_norm || !preds || T <= 0 || B <= 0 || Cin <= 0 || HW <= 0 || C <= 0 || C > 32 || !(eps >= 0.0f))
    return SLU_EINVAL;
  if ((gn_mean == nullptr) != (gn_rstd == nullptr)) return SLU_EINVAL;
  const bool gn = gn_mean != nullptr;
  if (gn && (groups <= 0 || Cin % groups)) return SLU_EINVAL;
  if (Cin > HM_CMAX || (long long)T * B * (gn ? groups : 1) > 0x7fffffffLL) return SLU_EUNSUPPORTED;
  const bool vec = HW % 4 == 0 && !(((uintptr_t)x | (uintptr_t)p_bar | (uintptr_t)h_norm | (uintptr_t)mi_norm | (uintptr_t)preds) & 15);
  const long long nblk = (long long)B * ((HW + HM_TILE - 1) / HM_TILE);
  long long nb = (nblk + 3) / 4;
  if (nb > 256 * 8) nb = 256 * 8;                                     // grid-stride: the chip sweeps the T*B images as one front per pass
  const float lnC = (float)log((double)C);
  hipStream_t st = slu_stream(stream);
  const dim3 grid((unsigned)nb);
  const int NQ = (C + 7) / 8;                                          // live groups of 8 classes, 1 .. 4
#define SLU_HEAD_MC_F32(NQ_)                                                                                                                      \
  do {                                                                                                                                            \
    if (vec) launch_head_mc_f32<NQ_, true>(gn, grid, st, x, T, B, Cin, HW, gn_mean, gn_rstd, gn_gamma, gn_beta, groups, relu, w, bias, C, eps, lnC, \
                                           p_bar, h_norm, mi_norm, preds);                                                                        \
    else launch_head_mc_f32<NQ_, false>(gn, grid, st, x, T, B, Cin, HW, gn_mean, gn_rstd, gn_gamma, gn_beta, groups, relu, w, bias, C, eps, lnC,   \
                                        p_bar, h_norm, mi_norm, preds);                                                                           \
  } while (0)
  if (NQ == 1) SLU_HEAD_MC_F32(1);
  else if (NQ == 2) SLU_HEAD_MC_F32(2);
  else if (NQ == 3) SLU_HEAD_MC_F32(3);
  else SLU_HEAD_MC_F32(4);
#undef SLU_HEAD_MC_F32
  SLU_CHECK_LAUNCH();
}
