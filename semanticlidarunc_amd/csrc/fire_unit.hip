// A SqueezeNet Fire module (torchvision's Fire: squeeze 1x1 -> ReLU -> {expand 1x1, expand 3x3 / pad 1} -> ReLU -> concat) in ONE launch, and the
// ceil-mode max-pool that sits between the Fires:
//
//   s[n,k]       = relu(bsq[k] + sum_c wsq[k,c] src[n,c])                              k < S
//   out[n,j]     = relu(b1[j] + sum_k w1[j,k] s[n,k])                                  j < E1
//   out[n,E1+j]  = relu(b3[j] + sum_{k,a,b} w3[j,k,a,b] s[n,k,y-1+a,x-1+b])            j < E3        (s = 0 outside the image)
//
// The squeeze map never leaves the chip: a workgroup computes it for one 4 x 32 output tile plus a one-pixel halo (6 x 34 = 204 positions,
// seven 32-pixel MFMA column blocks) into LDS -- [S rounded up to 16][204] floats, 52 224 B at S = 64 -- and both expand convs read it from
// there; the concat is the store address.  Halo positions outside the image are stored as 0 (the 3x3's padding); those inside the image but
// outside the tile are computed from the real input, so the halo costs 224 / 128 = 1.75 x the squeeze arithmetic of the tile.
//
//   fire_kernel<MS, NBW>    256 threads = 4 waves.  Squeeze: wave w owns halo column blocks w and w + 4 and all MS = ceil(S / 32) row blocks; the
//                           B operand (32 input channels x 32 positions per chunk) comes straight from global memory, the A operand from the
//                           packed weight image (L2); both are loaded one chunk ahead.  Expand: the 32-channel output blocks of the two convs
//                           are dealt to the waves as (row group of NBW tile rows) x (block phase): NBW = 4 -- a wave holds all four rows of a
//                           block, blocks w, w + 4, ..; NBW = 2 -- two rows, blocks (w >> 1) + 2 i; NBW = 1 -- one row, every block.  A from the
//                           packed image one chunk (8 K-steps) ahead, B from LDS (lane -> consecutive floats: conflict-free).  Small maps are
//                           split over blockIdx.z by output blocks (slu_cu_fill_split; each z recomputes the squeeze) and take the smaller NBW.
//   fire_pack_kernel        wsq [S][Cin], w1 [E1][S], w3 [E3][S][3][3] -> their three A-fragment images (encoder_unit.h), one after the other.
//   maxpool3s2_ceil_kernel  nn.MaxPool2d(3, 2, padding=0, ceil_mode=True) over the same slu_cat2.
// Products are v_mfma_f32_32x32x2_f32 (exact fp32: a k-ordered fmaf chain); no atomics: results are bit-identical run to run.
#include "encoder_unit.h"

namespace {

constexpr int FT_H = 4, FT_W = 32;                    // output tile
constexpr int FH_H = FT_H + 2, FH_W = FT_W + 2;       // with the halo
constexpr int FH_PIX = FH_H * FH_W;                   // 204 squeeze positions = LDS floats per squeeze channel
constexpr int FH_NB = (FH_PIX + 31) / 32;             // 7 column blocks
constexpr int F_KS = 8;                               // expand: K-steps (of 2 squeeze channels) per chunk
constexpr int F_KC = 2 * F_KS;                        //         channels per chunk: S is padded to it in the packed images and in LDS
constexpr int FQ_KS = 16;                             // squeeze: K-steps per chunk -- 32 MS MFMAs per wave, long enough to cover the round trip
constexpr int FQ_KC = 2 * FQ_KS;                      //          of the next chunk's input loads; Cin is padded to it in the packed image
constexpr int F_MAX_S = 64, F_MAX_E = 256;

struct FireArgs {
  const float* src0;      // the fields of Cat2Args (slu_cat2_fill), flat: as a member struct the kernels' argument loads change
  const float* src1;
  long long bs0, bs1;
  int c0, C;
  int H, W, tx;           // tx = tiles per row of tiles
  int S, SP, E1, E3;      // SP = S rounded up to F_KC
  int nb1, nb3, mps1, mps3;   // 32-channel output blocks of the two expand convs; blocks per blockIdx.z
  int nchq;               // squeeze chunks = ceil(C / FQ_KC)
  const float *wsq, *w1, *w3;   // packed images
  const float *bsq, *b1, *b3;
  float* out;
};

// The B operands of squeeze chunk q: 32 channels x this lane's two halo positions.  Every load is unconditional and its value is used as it
// comes (a select on a loaded value makes the compiler branch around the load and wait for it: eight serial round trips per chunk).  A position
// outside the image reads pixel 0 of the channel: its column of the product is discarded when the squeeze map is stored.  A channel past Cin (the
// ragged last chunk, whose weights are zero) reads `zero`, a 0.0f of the packed image's own padding: 0 x NaN from a neighbouring tensor must not
// get in.
__device__ __forceinline__ void fire_load_b(const FireArgs& a, const float* s0, const float* s1, const float* zero, size_t HW, int q, int hh,
                                            const int (&off)[2], float (&bv)[2][FQ_KS]) {
#pragma unroll
  for (int kk = 0; kk < FQ_KS; ++kk) {
    const int c = q * FQ_KC + 2 * kk + hh;
    const float* p = CAT2_PLANE(c, a.c0, s0, s1, HW);
#pragma unroll
    for (int u = 0; u < 2; ++u) bv[u][kk] = *(c < a.C ? p + off[u] : zero);
  }
}

template <int MS>
__device__ __forceinline__ void fire_load_a(const float* wq, int kp2, int q, float (&av)[MS][FQ_KS]) {
#pragma unroll
  for (int m = 0; m < MS; ++m)
#pragma unroll
    for (int kk = 0; kk < FQ_KS; ++kk) av[m][kk] = wq[((size_t)m * kp2 + (size_t)q * FQ_KS + kk) * 64];
}

// One 32-channel output block of an expand conv for NBW tile rows: TAPS = 1 (the 1x1: the centre of the halo window) or 9.
template <int NBW, int TAPS>
__device__ __forceinline__ void fire_expand_block(const FireArgs& a, const float* __restrict__ s_s, const float* __restrict__ wblk,
                                                  const float* __restrict__ bias, int co0, int cn, float* __restrict__ po, int y0, int x0, int row0,
                                                  int lane) {
  const int hh = lane >> 5, jj = lane & 31;
  const int cps = a.SP / F_KC, nch = TAPS * cps;
  f32x16 acc[NBW];
  SLU_ZERO_ACC(acc, NBW);
  // this lane's 16 biases, loaded ahead of the K loop from clamped indices (a load inside the guarded stores below would be a serial round trip
  // per register)
  float bz[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) bz[r] = bias[min(slu_frag_row(0, r, hh), cn - 1)];
  // chunk q's operands: A from the packed image, B from the squeeze map at the chunk's tap
  auto load = [&](int q, float (&av)[F_KS], float (&bv)[F_KS][NBW]) __attribute__((always_inline)) {
#pragma unroll
    for (int kk = 0; kk < F_KS; ++kk) av[kk] = wblk[((size_t)q * F_KS + kk) * 64 + lane];
    const int tap = TAPS == 1 ? 4 : q / cps, kc = TAPS == 1 ? q : q - tap * cps;
    const int ta = tap / 3, tb = tap - 3 * ta;
    const float* sb = s_s + (kc * F_KC + hh) * FH_PIX + (row0 + ta) * FH_W + tb + jj;
#pragma unroll
    for (int kk = 0; kk < F_KS; ++kk)
#pragma unroll
      for (int i = 0; i < NBW; ++i) bv[kk][i] = sb[2 * kk * FH_PIX + i * FH_W];
  };
  float av[F_KS], bv[F_KS][NBW];
  load(0, av, bv);
  for (int q = 0; q < nch; ++q) {
    // the next chunk's operands are requested before this chunk's MFMAs; the scheduling barriers keep the compiler from sinking each load to
    // its use (one exposed round trip per K-step instead of per chunk)
    float an[F_KS], bn[F_KS][NBW];
    load(q + 1 < nch ? q + 1 : q, an, bn);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int kk = 0; kk < F_KS; ++kk) {
#pragma unroll
      for (int i = 0; i < NBW; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[kk], bv[kk][i], acc[i], 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int kk = 0; kk < F_KS; ++kk) {
      av[kk] = an[kk];
#pragma unroll
      for (int i = 0; i < NBW; ++i) bv[kk][i] = bn[kk][i];
    }
  }
  const size_t HW = (size_t)a.H * a.W;
  const int x = x0 + jj;
#pragma unroll
  for (int i = 0; i < NBW; ++i) {
    const int y = y0 + row0 + i;
    if (y < a.H && x < a.W) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int j = slu_frag_row(0, r, hh);
        if (j < cn) {
          const float v = acc[i][r] + bz[r];
          po[(size_t)(co0 + j) * HW + (size_t)y * a.W + x] = v > 0.0f ? v : 0.0f;
        }
      }
    }
  }
}

template <int MS, int NBW>
__global__ __launch_bounds__(256) void fire_kernel(const FireArgs a) {
  extern __shared__ float s_s[];      // [SP][FH_PIX]
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hh = lane >> 5, jj = lane & 31;
  const int n = blockIdx.y;
  const int ty = blockIdx.x / a.tx;
  const int y0 = ty * FT_H, x0 = (blockIdx.x - ty * a.tx) * FT_W;
  const size_t HW = (size_t)a.H * a.W;

  // ---- squeeze: halo column blocks w and w + 4 (the eighth does not exist: wave 3 computes it like the others and stores nothing), every row
  // block ----
  {
    int off[2], pp[2];
    bool ok[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int p = (w + 4 * u) * 32 + jj;
      const int hy = p / FH_W, hx = p - hy * FH_W;
      const int iy = y0 - 1 + hy, ix = x0 - 1 + hx;
      pp[u] = p;
      ok[u] = p < FH_PIX && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
      off[u] = ok[u] ? iy * a.W + ix : 0;
    }
    const float* s0 = a.src0 + (size_t)n * a.bs0;
    const float* s1 = a.src1 ? a.src1 + (size_t)n * a.bs1 : s0;
    const float* wq = a.wsq + lane;
    const int kp2 = a.nchq * FQ_KS;
    // the last K-step's second channel of row 0 in the packed squeeze image: 0.0f whenever Cin is no multiple of 32, and only read then
    const float* zero = a.wsq + ((size_t)kp2 - 1) * 64 + 32;
    f32x16 acc[MS][2];
    SLU_ZERO_ACC2(acc, MS, 2);
    // this lane's squeeze biases, loaded ahead of the K loop from clamped indices: rows S .. SP - 1 (zero weights) get a finite value that the
    // zero-filled expand weights ignore
    float bq[MS][16];
#pragma unroll
    for (int m = 0; m < MS; ++m)
#pragma unroll
      for (int r = 0; r < 16; ++r) bq[m][r] = a.bsq[min(slu_frag_row(32 * m, r, hh), a.S - 1)];
    float bv[2][FQ_KS], av[MS][FQ_KS];
    fire_load_b(a, s0, s1, zero, HW, 0, hh, off, bv);
    fire_load_a<MS>(wq, kp2, 0, av);
    for (int q = 0; q < a.nchq; ++q) {
      float bn[2][FQ_KS], an[MS][FQ_KS];
      const int qn = q + 1 < a.nchq ? q + 1 : q;
      fire_load_b(a, s0, s1, zero, HW, qn, hh, off, bn);
      fire_load_a<MS>(wq, kp2, qn, an);
      __builtin_amdgcn_sched_barrier(0);      // the next chunk's loads stay ahead of this chunk's MFMAs
#pragma unroll
      for (int kk = 0; kk < FQ_KS; ++kk)
#pragma unroll
        for (int m = 0; m < MS; ++m) {
#pragma unroll
          for (int u = 0; u < 2; ++u) acc[m][u] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[m][kk], bv[u][kk], acc[m][u], 0, 0, 0);
        }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int kk = 0; kk < FQ_KS; ++kk) {
#pragma unroll
        for (int u = 0; u < 2; ++u) bv[u][kk] = bn[u][kk];
#pragma unroll
        for (int m = 0; m < MS; ++m) av[m][kk] = an[m][kk];
      }
    }
    // bias, ReLU, 0 outside the image
#pragma unroll
    for (int m = 0; m < MS; ++m)
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        if (pp[u] < FH_PIX) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int k = slu_frag_row(32 * m, r, hh);
            if (k < a.SP) {
              const float v = acc[m][u][r] + bq[m][r];
              s_s[k * FH_PIX + pp[u]] = ok[u] && v > 0.0f ? v : 0.0f;
            }
          }
        }
      }
  }
  __syncthreads();

  // ---- expand: the output blocks of this blockIdx.z, dealt to the waves as (row group) x (block phase) ----
  constexpr int RG = FT_H / NBW;
  const int rg = w % RG, bp = w / RG;
  const int row0 = rg * NBW;
  float* __restrict__ po = a.out + (size_t)n * (a.E1 + a.E3) * HW;
  const int z = blockIdx.z;
  const size_t k1 = (size_t)(a.SP / 2) * 64, k3 = 9 * k1;      // floats of one block in the packed images
  {
    const int lo = z * a.mps3, hi = min(a.nb3, lo + a.mps3);
    for (int mb = lo + bp; mb < hi; mb += NBW)
      fire_expand_block<NBW, 9>(a, s_s, a.w3 + (size_t)mb * k3, a.b3 + mb * 32, a.E1 + mb * 32, min(32, a.E3 - mb * 32), po, y0, x0, row0, lane);
  }
  {
    const int lo = z * a.mps1, hi = min(a.nb1, lo + a.mps1);
    for (int mb = lo + bp; mb < hi; mb += NBW)
      fire_expand_block<NBW, 1>(a, s_s, a.w1 + (size_t)mb * k1, a.b1 + mb * 32, mb * 32, min(32, a.E1 - mb * 32), po, y0, x0, row0, lane);
  }
}

// out = [wsq image | w1 image | w3 image]; see the head of the file
__global__ __launch_bounds__(256) void fire_pack_kernel(const float* __restrict__ wsq, const float* __restrict__ w1, const float* __restrict__ w3, int cin,
                                                        int s, int e1, int e3, size_t nq, size_t n1, size_t total, float* __restrict__ out) {
  PIX_GRID_STRIDE(e, total) {
    out[e] = e < nq        ? afrag_element(wsq, e, s, cin, FQ_KC, 1)
             : e < nq + n1 ? afrag_element(w1, e - nq, e1, s, F_KC, 1)
                           : afrag_element(w3, e - nq - n1, e3, s, F_KC, 9);
  }
}

// nn.MaxPool2d(3, 2, padding=0, ceil_mode=True): windows start at (2 oy, 2 ox) and are clipped at the far edge
__global__ __launch_bounds__(256) void maxpool3s2_ceil_kernel(const float* __restrict__ s0, const float* __restrict__ s1, long long bs0, long long bs1,
                                                              int c0, int C, int N, int H, int W, int OH, int OW, float* __restrict__ y) {
  const size_t total = (size_t)N * C * OH * OW;
  PIX_GRID_STRIDE(e, total) {
    const PixXYCN o = pix_xycn(e, OW, OH, C);
    const float* p = CAT2_PLANE(o.c, c0, s0 + o.n * (size_t)bs0, s1 + o.n * (size_t)bs1, H * W);
    float m = -INFINITY;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const int iy = 2 * o.y + i, ix = 2 * o.x + j;
        if (iy < H && ix < W) m = fmaxf(m, p[(size_t)iy * W + ix]);
      }
    y[e] = m;
  }
}

struct FireSizes {
  size_t nq, n1, n3;
};
bool fire_sizes(int cin, int s, int e1, int e3, FireSizes& z) {
  if (cin <= 0 || s <= 0 || e1 <= 0 || e3 <= 0 || s > F_MAX_S || e1 > F_MAX_E || e3 > F_MAX_E) return false;
  z.nq = afrag_floats(s, cin, FQ_KC, 1);
  z.n1 = afrag_floats(e1, s, F_KC, 1);
  z.n3 = afrag_floats(e3, s, F_KC, 9);
  return true;
}

template <int MS>
int launch_fire(const FireArgs& a, dim3 grid, size_t lds, int nbw, hipStream_t st) {
  if (nbw == 4) hipLaunchKernelGGL((fire_kernel<MS, 4>), grid, dim3(256), lds, st, a);
  else if (nbw == 2) hipLaunchKernelGGL((fire_kernel<MS, 2>), grid, dim3(256), lds, st, a);
  else hipLaunchKernelGGL((fire_kernel<MS, 1>), grid, dim3(256), lds, st, a);
  SLU_CHECK_LAUNCH();
}

}  // namespace

extern "C" size_t slu_fire_packed_floats(int cin, int s, int e1, int e3) {
  FireSizes z;
  return fire_sizes(cin, s, e1, e3, z) ? z.nq + z.n1 + z.n3 : 0;
}

extern "C" int slu_fire_pack(const float* wsq, const float* w1, const float* w3, int cin, int s, int e1, int e3, float* out, slu_stream_t stream) {
  if (!wsq || !w1 || !w3 || !out || cin <= 0 || s <= 0 || e1 <= 0 || e3 <= 0) return SLU_EINVAL;
  FireSizes z;
  if (!fire_sizes(cin, s, e1, e3, z)) return SLU_EUNSUPPORTED;
  const size_t total = z.nq + z.n1 + z.n3;
  hipLaunchKernelGGL(fire_pack_kernel, dim3(slu_grid_1d(total, 4096)), dim3(256), 0, slu_stream(stream), wsq, w1, w3, cin, s, e1, e3, z.nq, z.n1, total,
                     out);
  SLU_CHECK_LAUNCH();
}

extern "C" int slu_fire_fwd(const slu_fire_desc* d, slu_stream_t stream) {
  if (!d || !d->wpack || !d->bsq || !d->b1 || !d->b3 || !d->out || slu_cat2_check(d->in, d->N, d->H, d->W)) return SLU_EINVAL;
  if (d->S <= 0 || d->E1 <= 0 || d->E3 <= 0) return SLU_EINVAL;
  FireSizes z;
  if (!fire_sizes(d->in.c0 + d->in.c1, d->S, d->E1, d->E3, z) || slu_unit_grid_check(d->N, d->H, d->W)) return SLU_EUNSUPPORTED;
  const size_t HW = (size_t)d->H * d->W;
  if (slu_cat2_overlaps(d->in, d->N, HW, d->out, (size_t)d->N * (d->E1 + d->E3) * HW)) return SLU_EINVAL;
  FireArgs a;
  slu_cat2_fill(a, d->in, HW);
  a.H = d->H; a.W = d->W;
  a.tx = (d->W + FT_W - 1) / FT_W;
  a.S = d->S;
  a.SP = (d->S + F_KC - 1) / F_KC * F_KC;
  a.E1 = d->E1; a.E3 = d->E3;
  a.nb1 = (d->E1 + 31) / 32;
  a.nb3 = (d->E3 + 31) / 32;
  a.nchq = (a.C + FQ_KC - 1) / FQ_KC;
  a.wsq = d->wpack; a.w1 = d->wpack + z.nq; a.w3 = d->wpack + z.nq + z.n1;
  a.bsq = d->bsq; a.b1 = d->b1; a.b3 = d->b3;
  a.out = d->out;
  const long long tiles = (long long)a.tx * ((d->H + FT_H - 1) / FT_H) * d->N;
  if (tiles > 0x7fffffffLL) return SLU_EUNSUPPORTED;
  const int split = slu_cu_fill_split(tiles, a.nb3);
  a.mps3 = (a.nb3 + split - 1) / split;
  a.mps1 = (a.nb1 + split - 1) / split;
  const int nbw = a.mps3 >= 4 ? 4 : a.mps3 >= 2 ? 2 : 1;
  const dim3 grid((unsigned)(tiles / d->N), (unsigned)d->N, (unsigned)split);
  const size_t lds = (size_t)a.SP * FH_PIX * sizeof(float);
  return d->S > 32 ? launch_fire<2>(a, grid, lds, nbw, slu_stream(stream)) : launch_fire<1>(a, grid, lds, nbw, slu_stream(stream));
}

extern "C" int slu_maxpool3s2_ceil_fwd(const slu_cat2* in, float* y, int N, int H, int W, slu_stream_t stream) {
  if (!in || !y || slu_cat2_check(*in, N, H, W) || H < 3 || W < 3) return SLU_EINVAL;
  return slu_cat2_resample(maxpool3s2_ceil_kernel, in, y, N, H, W, slu_ceil_pool3s2_out(H), slu_ceil_pool3s2_out(W), slu_stream(stream));
}
