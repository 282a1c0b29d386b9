// A chain of 1 .. 4 per-pixel 1x1 convs, each with bias and LeakyReLU, in ONE launch -- the point-MLP stem of FIDNet's ResNet34_point backbone
// (reference src/baselines/FIDNet/ResNet.py:469-502, 563-576: Cin -> 64 -> 128 -> 256 -> 512 with eval BatchNorm folded into each conv):
//
//   y = act(W_L . ... act(W_1 . x + b_1) ... + b_L)      per pixel;  act(v) = v > 0 ? v : slope * v, optional on the last layer
//
// A 1x1 chain has no spatial structure: a workgroup owns PM_P = 32 NB consecutive pixels of the flattened H W index of one image (NB = 2, or 1
// where two activation maps of 64 pixels do not fit the LDS) and masks the tail.  The input tile is staged into LDS once ([channel][pixel], the
// channels zero-filled up to a multiple of PM_KC); layer l reads its B operand from one LDS buffer and writes act(.) into the other, the last
// layer writes to global memory: the intermediate maps never leave the chip.  LDS = (widest map held by buffer 0 + widest held by buffer 1) x
// PM_P x 4 B: 128 + 256 channels x 64 pixels = 96 KB for the model's chain.
//
//   point_mlp_kernel<NB>   256 threads = 4 waves.  Per layer, wave w owns the 32-channel output blocks w, w + 4, .. and all NB pixel blocks of
//                          each: acc[NB].  A from the packed weight image (streamed from L2: the chain's 690 KB do not fit the LDS) and B from
//                          LDS (lane -> consecutive floats: conflict-free) are loaded one chunk of PM_KS K-steps ahead of the MFMAs.  A
//                          workgroup-wide barrier separates the layers.
//   point_mlp_pack_kernel  W [Co][Ci] -> its A-fragment image (encoder_unit.h) with K-chunk PM_KC.
// Products are v_mfma_f32_32x32x2_f32 (exact fp32: a k-ordered fmaf chain); no atomics: results are bit-identical run to run.
#include "encoder_unit.h"

namespace {

constexpr int PM_KS = 8;                 // K-steps (of 2 channels) per chunk
constexpr int PM_KC = 2 * PM_KS;         // channels per chunk: the input channels are padded to it in LDS and in the packed image
constexpr int PM_MAX_L = 4, PM_MAX_C0 = 32, PM_MAX_W = 512;
constexpr size_t PM_LDS_MAX = 160 * 1024;

struct PmArgs {
  const float* x;
  const float* w;         // packed images of the layers, one after the other
  const float* b;         // biases of the layers, one after the other
  float* out;
  long long HW;
  int C0, C0P, nl;        // C0P = C0 rounded up to PM_KC
  int width[PM_MAX_L];
  int off1;               // floats from LDS buffer 0 to LDS buffer 1
  float slope, slope_last;   // slope_last = 1 without the last activation: v * 1.0f == v
};

template <int NB>
__global__ __launch_bounds__(256) void point_mlp_kernel(const PmArgs a) {
  extern __shared__ float s_pm[];
  constexpr int P = 32 * NB;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hh = lane >> 5, jj = lane & 31;
  const size_t n = blockIdx.y, HW = (size_t)a.HW;
  const size_t pix0 = (size_t)blockIdx.x * P;

  // ---- the input tile: [C0P][P], 0 in the padded channels (their weights are 0 too, and 0 x NaN must not get in) and past the image ----
  {
    const float* __restrict__ px = a.x + n * a.C0 * HW;
    for (int e = tid; e < a.C0P * P; e += 256) {
      const int c = e / P, p = e - c * P;
      const size_t pix = pix0 + p;
      s_pm[e] = c < a.C0 && pix < HW ? px[(size_t)c * HW + pix] : 0.0f;
    }
  }
  __syncthreads();

  const float* __restrict__ wl = a.w;
  const float* __restrict__ bl = a.b;
  float* s_in = s_pm;
  float* s_out = s_pm + a.off1;
  int K = a.C0P;
  for (int l = 0; l < a.nl; ++l) {
    const int Co = a.width[l], M = Co >> 5, ksteps = K >> 1, nch = K / PM_KC;
    const bool last = l == a.nl - 1;
    const float slope = last ? a.slope_last : a.slope;
    for (int mb = w; mb < M; mb += 4) {
      const float* __restrict__ wblk = wl + (size_t)mb * ksteps * 64 + lane;
      f32x16 acc[NB];
      SLU_ZERO_ACC(acc, NB);
      float bz[16];      // this lane's 16 biases, loaded ahead of the K loop
#pragma unroll
      for (int r = 0; r < 16; ++r) bz[r] = bl[slu_frag_row(mb * 32, r, hh)];
      // chunk q's operands: A from the packed image, B from the input map in LDS
      auto load = [&](int q, float (&av)[PM_KS], float (&bv)[PM_KS][NB]) __attribute__((always_inline)) {
#pragma unroll
        for (int kk = 0; kk < PM_KS; ++kk) av[kk] = wblk[((size_t)q * PM_KS + kk) * 64];
        const float* sb = s_in + (q * PM_KC + hh) * P + jj;
#pragma unroll
        for (int kk = 0; kk < PM_KS; ++kk)
#pragma unroll
          for (int i = 0; i < NB; ++i) bv[kk][i] = sb[2 * kk * P + 32 * i];
      };
      float av[PM_KS], bv[PM_KS][NB];
      load(0, av, bv);
      for (int q = 0; q < nch; ++q) {
        // the next chunk's operands are requested before this chunk's MFMAs (fire_unit.hip: the scheduling barriers keep the loads there)
        float an[PM_KS], bn[PM_KS][NB];
        load(q + 1 < nch ? q + 1 : q, an, bn);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int kk = 0; kk < PM_KS; ++kk) {
#pragma unroll
          for (int i = 0; i < NB; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[kk], bv[kk][i], acc[i], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int kk = 0; kk < PM_KS; ++kk) {
          av[kk] = an[kk];
#pragma unroll
          for (int i = 0; i < NB; ++i) bv[kk][i] = bn[kk][i];
        }
      }
      // bias, LeakyReLU; the next layer's B operand, or the result
      // (LDS stores: a 32-lane half writes 32 consecutive floats of one row; the other half's row is 4 P floats further, on the same banks, but
      // ds_write_b32 is serviced per half, and only lanes of one group conflict)
      if (last) {
        float* __restrict__ po = a.out + (n * Co + (size_t)mb * 32) * HW;
#pragma unroll
        for (int i = 0; i < NB; ++i) {
          const size_t pix = pix0 + 32 * i + jj;
          if (pix < HW) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const float v = acc[i][r] + bz[r];
              po[(size_t)slu_frag_row(0, r, hh) * HW + pix] = v > 0.0f ? v : v * slope;
            }
          }
        }
      } else {
#pragma unroll
        for (int i = 0; i < NB; ++i)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const float v = acc[i][r] + bz[r];
            s_out[slu_frag_row(mb * 32, r, hh) * P + 32 * i + jj] = v > 0.0f ? v : v * slope;
          }
      }
    }
    __syncthreads();
    wl += (size_t)M * ksteps * 64;
    bl += Co;
    K = Co;
    float* t = s_in;
    s_in = s_out;
    s_out = t;
  }
}

__global__ __launch_bounds__(256) void point_mlp_pack_kernel(const float* __restrict__ w, int cout, int cin, size_t total, float* __restrict__ out) {
  PIX_GRID_STRIDE(e, total) out[e] = afrag_element(w, e, cout, cin, PM_KC, 1);
}

template <int NB>
int launch_point_mlp(const PmArgs& a, dim3 grid, size_t lds, hipStream_t st) {
  static SluLdsGrant grant;
  return slu_launch_lds(point_mlp_kernel<NB>, grid, dim3(256), lds, st, grant, a);
}

}  // namespace

extern "C" int slu_point_mlp_pack(const float* w, int cout, int cin, float* out, slu_stream_t stream) {
  if (!w || !out || cout <= 0 || cin <= 0) return SLU_EINVAL;
  if (cout % 32 || cout > PM_MAX_W || cin > PM_MAX_W) return SLU_EUNSUPPORTED;
  const size_t total = afrag_floats(cout, cin, PM_KC, 1);
  hipLaunchKernelGGL(point_mlp_pack_kernel, dim3(slu_grid_1d(total, 4096)), dim3(256), 0, slu_stream(stream), w, cout, cin, total, out);
  SLU_CHECK_LAUNCH();
}

extern "C" int slu_point_mlp(const float* x, const float* wpack, const float* bias, const int* widths, int nlayers, int N, int C0, long long HW,
                             float slope, int act_last, float* out, slu_stream_t stream) {
  if (!x || !wpack || !bias || !widths || !out || nlayers < 1 || nlayers > PM_MAX_L || N <= 0 || C0 <= 0 || HW <= 0) return SLU_EINVAL;
  for (int l = 0; l < nlayers; ++l)
    if (widths[l] <= 0) return SLU_EINVAL;
  if (C0 > PM_MAX_C0 || N > 65535 || HW >= 0x7fffffffLL) return SLU_EUNSUPPORTED;
  PmArgs a = {};
  a.x = x, a.w = wpack, a.b = bias, a.out = out;
  a.HW = HW, a.C0 = C0, a.nl = nlayers;
  a.C0P = (C0 + PM_KC - 1) / PM_KC * PM_KC;
  a.slope = slope, a.slope_last = act_last ? slope : 1.0f;
  // buffer 0 holds the input tile and the outputs of layers 2, 4, ..; buffer 1 those of layers 1, 3, ..; the last layer's output is not held
  int wide[2] = {a.C0P, 0};
  for (int l = 0; l < nlayers; ++l) {
    if (widths[l] % 32 || widths[l] > PM_MAX_W) return SLU_EUNSUPPORTED;
    a.width[l] = widths[l];
    if (l + 1 < nlayers && widths[l] > wide[(l + 1) & 1]) wide[(l + 1) & 1] = widths[l];
  }
  const int ch = wide[0] + wide[1];
  const int nb = (size_t)ch * 64 * sizeof(float) <= PM_LDS_MAX ? 2 : 1;      // 1024 channels x 32 pixels x 4 B = 128 KB always fit
  const int P = 32 * nb;
  a.off1 = wide[0] * P;
  const size_t lds = (size_t)ch * P * sizeof(float);
  const dim3 grid((unsigned)((HW + P - 1) / P), (unsigned)N);
  return nb == 2 ? launch_point_mlp<2>(a, grid, lds, slu_stream(stream)) : launch_point_mlp<1>(a, grid, lds, slu_stream(stream));
}
