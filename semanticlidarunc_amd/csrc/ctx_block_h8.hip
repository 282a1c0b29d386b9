// Fused ResContextBlock of SalsaNext on the half-precision ("h8") path (reference SalsaNext.py:10-39):
//
//     s   = leaky(conv1x1(x) + b1)                                   (conv1 + act1; the block's shortcut)
//     a1  = bn1(leaky(conv3x3_pad1(s) + b2))                          (conv2, act2, bn1)
//     out = s + bn2(leaky(conv3x3_dil2_pad2(a1) + b3))                (conv3, act3, bn2, + shortcut)
//
// Unfused that is three launches moving 7 full-resolution tensor passes (x -> s; s -> a1; a1, s -> out); here s and a1 never leave
// the CU: the block reads x and writes out -- 2 passes.  All three layers have 32 output channels (the three context blocks of the
// network run at full resolution, where they are HBM-bound).
//
// Persistent workgroup of 8 waves.  A work item is one image x one STRIP of 64 output columns x a segment of rows, walked DOWN in bands
// of R = 8 output rows; items dealt round-robin, XCD-aware (h8_tile_run, h8_common.h).  s and a1 live in LDS row RINGS of R + 6 = 14 and
// R + 4 = 12 rows (s with 3 halo columns each side, a1 with 2): a band [b, b + 8) needs s rows [b - 3, b + 11) and a1 rows [b - 2, b + 10),
// of which all but R rows of each were computed by the band above, so a band computes only R new rows of each.  The first band of a
// segment fills both rings (14 rows of s, 12 of a1: the old 8 x 64 tile).  Rows outside the image are written as zeros: conv2's and
// conv3's padding.  Per band three phases, each an implicit GEMM on v_mfma_f32_32x32x16_f16 over a FLATTENED pixel range of the band's
// new rows (32 consecutive pixels of the region's row-major order = one MFMA N-block; ds_read_b128 addresses are per lane, so a block
// may straddle rows and the ring's wrap):
//   P1  s on the new rows x 70 columns (8 x 70 = 560 px, 18 N-blocks): B operands straight from global memory -- loaded into registers
//       one band AHEAD (issued at the start of the previous band's P3, so their latency hides under the MFMAs); epilogue -> fp16 -> ring S.
//   P2  a1 on the new rows x 68 columns (8 x 68 = 544 px, 17 N-blocks) from S; epilogue -> fp16 -> ring A1.
//   P3  out on the band (8 x 64, 16 N-blocks: one row per wave) from A1; epilogue adds the centre of S and stores h8.
// Lanes past a region's last pixel compute on garbage and write a per-channel-block trash row of the ring (32 records).
// Rounding points (fp16 for s and a1, fp32 accumulation in the same k-step / tap order) are those of the unfused kernels, so the
// two paths agree to the last bit of fp16 except where an FMA contraction differs; every value is computed by the same instruction
// sequence whichever band or segment computes it, so the output does not depend on how the launch is segmented.
// Segments: a strip is split into row segments (each recomputing its first band's 6 + 4 halo rows) only when there are fewer strips
// than CUs.  LDS: S 64.8 KB + A1 54.3 KB + all weights resident 38 KB + epilogue constants = 159 KB (one workgroup per CU).
#include <algorithm>
#include <type_traits>
#include "h8_common.h"

namespace {

struct CtxArgs {
  const uint4* x;              // h8 [N][Gin][H][W], or [nb][Gin][H][W] when nb > 0
  const uint4 *w1, *w2, *w3;   // packed weights: [nks1][1][64], [2][9][64], [2][9][64] records
  const float *b1, *b2, *bn1_a, *bn1_b, *b3, *bn2_a, *bn2_b;      // [32] fp32 or nullptr
  float slope;                 // LeakyReLU slope of the three activations
  uint2* out;                  // h8 [N][4][H][W] as 8-byte half records
  int N, H, W, Gin;
  int nb;                      // > 0: x holds nb images and output image n reads image n % nb (the stacked MC passes of one batch)
  int strips_x, nseg, seg_rows;  // strips of TW columns; row segments of seg_rows rows (a multiple of R) per strip
};

constexpr int R = 8, TW = 64;                                   // band height, strip width
constexpr int SW = TW + 6, SROWS = R + 6;                       // s: 3 halo columns each side; ring rows
constexpr int AW = TW + 4, AROWS = R + 4;                       // a1: 2 halo columns each side; ring rows
constexpr int SRING = SROWS * SW + 32, ARING = AROWS * AW + 32; // records per channel block: the ring, then 32 trash records
constexpr int NB1F = (SROWS * SW + 31) / 32, NB1 = (R * SW + 31) / 32;   // N-blocks of P1: first band of a segment (14 rows) / later bands
constexpr int NB2F = (AROWS * AW + 31) / 32, NB2 = (R * AW + 31) / 32;   // the same for P2 (12 rows / 8 rows)
constexpr int NWAVE = 8;
#ifndef SLU_CTX_RING
#define SLU_CTX_RING 4
#endif
constexpr int RING = SLU_CTX_RING;                             // B-operand ring: an LDS read is issued RING - 1 MFMAs before its use
constexpr int PW1 = (NB1F + NWAVE - 1) / NWAVE, PW2 = (NB2F + NWAVE - 1) / NWAVE, PW3 = 2;
// LDS map in 16-byte records from offset 0 (the kernel has no static LDS): the two rings first, so that every access is
// "opaque per-lane record index + a constant below 64 KB" and needs no address register of its own
constexpr int OFF_S = 0, OFF_A = OFF_S + 4 * SRING, OFF_W1 = OFF_A + 4 * ARING;
template <int NKS1> constexpr int off_w2() { return OFF_W1 + NKS1 * 64; }
template <int NKS1> constexpr int off_w3() { return off_w2<NKS1>() + 18 * 64; }
template <int NKS1> constexpr int off_epi() { return off_w3<NKS1>() + 18 * 64; }      // 7 x 32 floats = 56 records
template <int NKS1> constexpr size_t lds_bytes() { return (size_t)(off_epi<NKS1>() + 56) * 16; }

#ifdef SLU_CTX_PROF      // development aid: shader clocks of wave 0 of every workgroup per phase (P1 | barrier | P2 | barrier | P3 | barrier)
__device__ unsigned long long g_ctx_prof[8];
#define CTX_PROF_MARK(i)                                             \
  {                                                                  \
    const unsigned long long t_now = __builtin_amdgcn_s_memtime();  \
    asm volatile("" ::: "memory");                                   \
    prof_acc[i] += t_now - prof_t;                                   \
    prof_t = t_now;                                                  \
  }
#else
#define CTX_PROF_MARK(i)
#endif

// a value the optimiser must treat as unknown: keeps "index + constant" LDS addresses in base-register + immediate form
__device__ __forceinline__ int opaque(int v) {
  asm volatile("" : "+v"(v));
  return v;
}

// LeakyReLU(t) = max(t, slope t) for 0 <= slope <= 1: a multiply + one v_max_f32 per element (the builtin max first canonicalises
// both operands with a v_max v, v, v each; accumulator values need no quieting)
__device__ __forceinline__ float2v leaky2(float2v t, float2v sl) {
  const float2v m = t * sl;
  float2v r;
  asm("v_max_f32 %0, %1, %2" : "=v"(r[0]) : "v"(t[0]), "v"(m[0]));
  asm("v_max_f32 %0, %1, %2" : "=v"(r[1]) : "v"(t[1]), "v"(m[1]));
  return r;
}

// ring slot of v in [0, 2 n)
__device__ __forceinline__ int wrap(int v, int n) { return v >= n ? v - n : v; }

template <int NKS1>
__global__ __launch_bounds__(64 * NWAVE, 2) void ctx_h8_kernel(const CtxArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint4* lds = reinterpret_cast<uint4*>(smem);
  uint2* lds2 = reinterpret_cast<uint2*>(smem);
  float4* lds4 = reinterpret_cast<float4*>(smem);
  constexpr int OFF_W2 = off_w2<NKS1>(), OFF_W3 = off_w3<NKS1>(), OFF_EPI = off_epi<NKS1>();

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int hh = lane >> 5, jj = lane & 31;
  const size_t HW = (size_t)a.H * a.W;

  const H8Run run = h8_tile_run(a.strips_x, a.nseg, a.N);
  const int t_beg = run.beg, t_end = run.end, t_step = run.step;
  if (t_beg >= t_end) return;

  {
    float* s_epi = reinterpret_cast<float*>(lds + OFF_EPI);      // b1 | b2 | bn1_a | bn1_b | b3 | bn2_a | bn2_b   (7 x 32 floats)
    if (tid < 32) {
      s_epi[tid] = a.b1 ? a.b1[tid] : 0.0f;
      s_epi[32 + tid] = a.b2 ? a.b2[tid] : 0.0f;
      s_epi[64 + tid] = a.bn1_a ? a.bn1_a[tid] : 1.0f;
      s_epi[96 + tid] = a.bn1_a ? a.bn1_b[tid] : 0.0f;
      s_epi[128 + tid] = a.b3 ? a.b3[tid] : 0.0f;
      s_epi[160 + tid] = a.bn2_a ? a.bn2_a[tid] : 1.0f;
      s_epi[192 + tid] = a.bn2_a ? a.bn2_b[tid] : 0.0f;
    }
    for (int e = tid; e < NKS1 * 64; e += 64 * NWAVE) lds[OFF_W1 + e] = a.w1[e];
    for (int e = tid; e < 18 * 64; e += 64 * NWAVE) {
      lds[OFF_W2 + e] = a.w2[e];
      lds[OFF_W3 + e] = a.w3[e];
    }
  }

  // Per-lane position inside the region of the N-blocks this wave owns (band independent: the regions of the first and the later bands
  // of a segment have the same width).  P1 / P2: blocks wave, wave + 8, ... of the flattened region, r | c << 8.  P3: row `wave`.
  int p1_rc[PW1], p1_goff[PW1], p2_rc[PW2];
#pragma unroll
  for (int i = 0; i < PW1; ++i) {
    const int e = 32 * (wave + NWAVE * i) + jj, r = e / SW, c = e - r * SW;
    p1_rc[i] = r | (c << 8);
    p1_goff[i] = r * a.W + c;
  }
#pragma unroll
  for (int i = 0; i < PW2; ++i) {
    const int e = 32 * (wave + NWAVE * i) + jj, r = e / AW, c = e - r * AW;
    p2_rc[i] = r | (c << 8);
  }
  const int i_w1 = opaque(OFF_W1 + lane), i_w2 = opaque(OFF_W2 + lane), i_w3 = opaque(OFF_W3 + lane), i_epi = opaque(OFF_EPI + hh);

  // one band: image n, strip columns [x0, x0 + 64), output rows [y0, y0 + R), band j of the segment that ends at row r1
  struct Band { int x0, y0, n, xn, j, r1; };      // xn: the image of x that output image n reads
  auto decode = [&](int t) {
    Band p;
    const int tx = t % a.strips_x;
    t /= a.strips_x;
    p.x0 = tx * TW;
    p.y0 = (t % a.nseg) * a.seg_rows;
    p.n = t / a.nseg;
    p.xn = a.nb > 0 ? p.n % a.nb : p.n;
    p.j = 0;
    p.r1 = min(a.H, p.y0 + a.seg_rows);
    return p;
  };
  // B operands of P1 for band bd: lane (pixel jj, half hh) of block i, K-step k holds channel block 2 k + hh of its pixel (zero
  // outside the image / past the region / past the last channel block).  The first band of a segment computes s rows [y0 - 3, y0 + 11),
  // a later one the new rows [y0 + 3, y0 + 11).
  // Every lane issues all PW1 x NKS1 loads of every band (a lane without a pixel reads the zero record): with a fixed count per band
  // the wait at P1 covers these loads only, not the output stores of the band before, which were issued after them.
  uint4 xr[PW1][NKS1];
  auto load_x = [&](const Band& bd) {
    const bool first = bd.j == 0;
    const int ys = first ? bd.y0 - 3 : bd.y0 + 3, nr = first ? SROWS : R;
    const long long org = (long long)ys * a.W + (bd.x0 - 3);
#pragma unroll
    for (int i = 0; i < PW1; ++i) {
      const int rc = p1_rc[i];
      const int gy = ys + (rc & 255), gx = bd.x0 - 3 + (rc >> 8);
      const bool in = (rc & 255) < nr && (unsigned)gy < (unsigned)a.H && (unsigned)gx < (unsigned)a.W;
#pragma unroll
      for (int k = 0; k < NKS1; ++k) {
        const int g = 2 * k + hh;
        const bool ok = in && g < a.Gin;
        xr[i][k] = *(ok ? a.x + (long long)(((size_t)bd.xn * a.Gin + g) * HW) + org + p1_goff[i] : &h8_zero_rec);
      }
    }
  };

  const float2v sl = {a.slope, a.slope};
  // this lane's 16 biases of a layer (channel 8 q + 4 hh + k at [4 q + k]): the C operand of a block's first MFMA
  auto lane_bias = [&](int first_f4) {
    f32x16 v;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 t = lds4[i_epi + first_f4 + 2 * q];
      v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
    }
    return v;
  };

  auto run_p1 = [&](const Band& bd) {
    const bool first = bd.j == 0;
    const int jr = R * bd.j;                                     // rows of this segment above the band
    // ---------------- P1: s = leaky(conv1x1(x) + b1) on the band's new rows -> ring S (zero outside the image: conv2's padding) ----------------
    // S row y of the segment starting at row y_seg sits in ring row (y - y_seg + 3) mod 14
    {
      const int ys = first ? bd.y0 - 3 : bd.y0 + 3, nr = first ? SROWS : R, u0 = first ? 0 : (jr + 6) % SROWS;
      auto phase1 = [&](auto nl_c) {
        constexpr int NL = decltype(nl_c)::value;
        const f32x16 biasv = lane_bias(0);
        half8 af[NKS1];
#pragma unroll
        for (int k = 0; k < NKS1; ++k) af[k] = __builtin_bit_cast(half8, lds[i_w1 + k * 64]);
        f32x16 acc[NL];
#pragma unroll
        for (int i = 0; i < NL; ++i)
#pragma unroll
          for (int k = 0; k < NKS1; ++k)
            acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[k], __builtin_bit_cast(half8, xr[i][k]), k == 0 ? biasv : acc[i], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < NL; ++i) {
          const int r = p1_rc[i] & 255, c = p1_rc[i] >> 8;
          const int gy = ys + r, gx = bd.x0 - 3 + c;
          const bool in = (unsigned)gy < (unsigned)a.H && (unsigned)gx < (unsigned)a.W;
          const int wi = opaque(((OFF_S + (r < nr ? wrap(u0 + r, SROWS) * SW + c : SROWS * SW + jj)) << 1) + hh);
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float2v t0 = leaky2(float2v{acc[i][4 * q], acc[i][4 * q + 1]}, sl), t1 = leaky2(float2v{acc[i][4 * q + 2], acc[i][4 * q + 3]}, sl);
            lds2[wi + q * SRING * 2] = in ? make_uint2(pack2(t0), pack2(t1)) : make_uint2(0u, 0u);
          }
        }
      };
      static_assert(NB1F > (PW1 - 1) * NWAVE && NB1 > (PW1 - 2) * NWAVE && NB1 <= (PW1 - 1) * NWAVE, "P1 block counts per wave: 4 / 3 / 2");
      const int nl = (first ? NB1F - wave + NWAVE - 1 : NB1 - wave + NWAVE - 1) / NWAVE;
      if (nl == PW1) phase1(std::integral_constant<int, PW1>{});
      else if (nl == PW1 - 1) phase1(std::integral_constant<int, PW1 - 1>{});
      else phase1(std::integral_constant<int, PW1 - 2>{});
    }
  };

  int item = t_beg;
  Band cur = decode(item);
  load_x(cur);
  __syncthreads();                                               // weights + constants visible
#ifdef SLU_CTX_PROF
  unsigned long long prof_acc[6] = {0, 0, 0, 0, 0, 0}, prof_t = __builtin_amdgcn_s_memtime();
#endif
  // P1 of the first band is peeled off the loop, and every x load is retired here: inside the loop the x loads are always followed by
  // the previous band's 8 output stores, so each wait on them counts those stores instead of draining them (vmcnt counts both)
  run_p1(cur);
#pragma unroll
  for (int i = 0; i < PW1; ++i)
#pragma unroll
    for (int k = 0; k < NKS1; ++k) asm volatile("" ::"v"(xr[i][k].x));

  for (;;) {
    const bool first = cur.j == 0;
    const int jr = R * cur.j;                                    // rows of this segment above the band
    CTX_PROF_MARK(0)
    __syncthreads();
    CTX_PROF_MARK(1)

    // ---------------- P2: a1 = bn1(leaky(conv3x3(s) + b2)) on the band's new rows -> ring A1 (zero outside the image) ----------------
    // A1 row y of the segment starting at row y_seg sits in ring row (y - y_seg + 2) mod 12.
    // The 18 weight fragments live in registers for the phase (one LDS read per MFMA: the B operand, issued 3 MFMAs ahead into a ring
    // of 4).  Blocks run one after the other on two alternating accumulator tiles; the epilogue of block i - 1 is cut into 16 pieces of
    // 2 - 5 vector instructions that are issued behind the first 16 MFMAs of block i, in program order pinned by sched_barrier: the
    // matrix pipe never waits for an epilogue and the epilogue never waits for the matrix pipe (hipcc does not find this interleave).
    {
      const int ya = first ? cur.y0 - 2 : cur.y0 + 2, nr = first ? AROWS : R, v0 = first ? 0 : jr + 4;
      const int vs = v0 % SROWS, va = v0 % AROWS;                // ring rows of the region's first row: in S (tap row 0) and in A1
      // FIRST: the first band of a segment, whose tap rows never wrap (one S base per block; a later band holds one per tap row)
      auto phase2 = [&](auto nl_c, auto first_c) {
        constexpr int NL = decltype(nl_c)::value, G = 18 * NL;
        constexpr bool FIRST = decltype(first_c)::value;
        constexpr int NTY = FIRST ? 1 : 3;
        const f32x16 biasv = lane_bias(8);
        int rb[NL][NTY], wi[NL];                                     // S record of tap row ty, column 0 in channel block hh ; uint2 index written in A1
#pragma unroll
        for (int i = 0; i < NL; ++i) {
          const int r = p2_rc[i] & 255, c = p2_rc[i] >> 8;
#pragma unroll
          for (int ty = 0; ty < NTY; ++ty) rb[i][ty] = opaque(OFF_S + hh * SRING + wrap(vs + r + ty, SROWS) * SW + c);
          wi[i] = opaque(((OFF_A + (r < nr ? wrap(va + r, AROWS) * AW + c : AROWS * AW + jj)) << 1) + hh);
        }
        half8 af[18];                                                  // read behind the MFMAs of block 0 (no 18 KB burst per wave at the phase start)
        auto read_a = [&](int t) { af[t] = __builtin_bit_cast(half8, lds[i_w2 + t * 64]); };
        f32x16 acc[2];
        half8 bq[RING];
        unsigned hp[8];                                                // the block's 16 results as 8 packed fp16 pairs
        float4 ba4[2], bb4[2];                                         // folded BatchNorm of the q being finished and of the next one (LDS table)
        float2v tp2;
        auto read_b = [&](int g) {
          const int i = g / 18, m = g % 18, k = m / 9, tap = m % 9;
          if constexpr (FIRST) bq[g % RING] = __builtin_bit_cast(half8, lds[rb[i][0] + 2 * k * SRING + (tap / 3) * SW + (tap % 3)]);
          else bq[g % RING] = __builtin_bit_cast(half8, lds[rb[i][tap / 3] + 2 * k * SRING + (tap % 3)]);
        };
        // the per-channel constants a q needs are read four pieces (= MFMA slots) before their first use: an LDS round trip under load
        // is longer than one slot, and a wait in the epilogue stream stalls the MFMAs behind it
        auto prefetch_q = [&](int q) {
          ba4[q & 1] = lds4[i_epi + 16 + 2 * q];
          bb4[q & 1] = lds4[i_epi + 24 + 2 * q];
        };
        // piece m (0..15) of block ib's epilogue: pair p = m / 2; even m: LeakyReLU, odd m: BatchNorm + fp16 pair (+ the LDS write of a finished q)
        auto epi_piece = [&](int ib, int m) {
          const int pr = m >> 1, q = pr >> 1;
          const f32x16& ac = acc[ib & 1];
          if ((m & 1) == 0) {
            if ((pr & 1) == 0 && q < 3) prefetch_q(q + 1);
            tp2 = leaky2(float2v{ac[2 * pr], ac[2 * pr + 1]}, sl);
          } else {
            const float4 ba = ba4[q & 1], bb = bb4[q & 1];
            tp2 = (pr & 1) ? tp2 * float2v{ba.z, ba.w} + float2v{bb.z, bb.w} : tp2 * float2v{ba.x, ba.y} + float2v{bb.x, bb.y};
            hp[pr] = pack2(tp2);
            if (pr & 1) {
              const int rc = p2_rc[ib];
              const int gy = ya + (rc & 255), gx = cur.x0 - 2 + (rc >> 8);
              const bool in = (unsigned)gy < (unsigned)a.H && (unsigned)gx < (unsigned)a.W;
              lds2[wi[ib] + q * ARING * 2] = in ? make_uint2(hp[pr - 1], hp[pr]) : make_uint2(0u, 0u);
            }
          }
        };
#pragma unroll
        for (int g = 0; g < RING - 1; ++g) { read_a(g); read_b(g); }
#pragma unroll
        for (int g = 0; g < G; ++g) {
          const int i = g / 18, m = g % 18;
          if (g + RING - 1 < 18) read_a(g + RING - 1);
          if (g + RING - 1 < G) read_b(g + RING - 1);
          acc[i & 1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[m], bq[g % RING], m == 0 ? biasv : acc[i & 1], 0, 0, 0);
          if (i > 0 && m < 16) epi_piece(i - 1, m);
          if (m == 16) prefetch_q(0);                                  // for the epilogue of block i, which starts two slots from here
          __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int m = 0; m < 16; ++m) epi_piece(NL - 1, m);
      };
      static_assert(NB2F > (PW2 - 1) * NWAVE && NB2 > (PW2 - 2) * NWAVE && NB2 <= (PW2 - 1) * NWAVE, "P2 block counts per wave: 4 / 3 / 2");
      using std::integral_constant;
      if (first) {
        if (wave < NB2F - (PW2 - 1) * NWAVE) phase2(integral_constant<int, PW2>{}, integral_constant<bool, true>{});
        else phase2(integral_constant<int, PW2 - 1>{}, integral_constant<bool, true>{});
      } else {
        if (wave < NB2 - (PW2 - 2) * NWAVE) phase2(integral_constant<int, PW2 - 1>{}, integral_constant<bool, false>{});
        else phase2(integral_constant<int, PW2 - 2>{}, integral_constant<bool, false>{});
      }
    }
    CTX_PROF_MARK(2)
    __syncthreads();
    CTX_PROF_MARK(3)

    // the next band's x goes into registers now: its latency hides under P3
    Band nxt = cur;
    bool more = true;
    if (cur.y0 + R < cur.r1) {
      nxt.y0 += R;
      ++nxt.j;
    } else if (item + t_step < t_end) {
      item += t_step;
      nxt = decode(item);
    } else {
      more = false;
    }
    load_x(nxt);                                                 // after the last band: loads of its own rows, unused

    // ---------------- P3: out = s + bn2(leaky(conv3x3_dil2(a1) + b3)) on the 8 x 64 band (same pipeline, two blocks) ----------------
    {
      constexpr int G = 18 * PW3;
      const f32x16 biasv = lane_bias(32);
      int rb[3];                                                     // A1 record of tap row ty, column jj of the strip in channel block hh
#pragma unroll
      for (int ty = 0; ty < 3; ++ty) rb[ty] = opaque(OFF_A + hh * ARING + ((jr + wave + 2 * ty) % AROWS) * AW + jj);
      const int p3_s = opaque(((OFF_S + ((jr + wave + 3) % SROWS) * SW + jj + 3) << 1) + hh);  // the same pixel's half record in S (the shortcut)
      half8 af[18];
      auto read_a = [&](int t) { af[t] = __builtin_bit_cast(half8, lds[i_w3 + t * 64]); };
      f32x16 acc[2];
      half8 bq[RING];
      unsigned hp[8];
      float4 ba4[2], bb4[2];
      uint2 sv[2];
      float2v tp2;
      const int gy = cur.y0 + wave;
      auto read_b = [&](int g) {
        const int i = g / 18, m = g % 18, k = m / 9, tap = m % 9;
        bq[g % RING] = __builtin_bit_cast(half8, lds[rb[tap / 3] + 2 * k * ARING + 32 * i + (tap % 3) * 2]);
      };
      auto prefetch_q = [&](int ib, int q) {
        sv[q & 1] = lds2[p3_s + (q * SRING + 32 * ib) * 2];         // shortcut values of this q (two pairs)
        ba4[q & 1] = lds4[i_epi + 40 + 2 * q];
        bb4[q & 1] = lds4[i_epi + 48 + 2 * q];
      };
      auto epi_piece = [&](int ib, int m) {
        const int pr = m >> 1, q = pr >> 1;
        const f32x16& ac = acc[ib & 1];
        if ((m & 1) == 0) {
          if ((pr & 1) == 0 && q < 3) prefetch_q(ib, q + 1);
          tp2 = leaky2(float2v{ac[2 * pr], ac[2 * pr + 1]}, sl);
        } else {
          const float4 ba = ba4[q & 1], bb = bb4[q & 1];
          tp2 = (pr & 1) ? tp2 * float2v{ba.z, ba.w} + float2v{bb.z, bb.w} : tp2 * float2v{ba.x, ba.y} + float2v{bb.x, bb.y};
          tp2 += unpack2((pr & 1) ? sv[q & 1].y : sv[q & 1].x);
          hp[pr] = pack2(tp2);
          if (pr & 1) {
            const int gx = cur.x0 + 32 * ib + jj;
            const bool ok = gy < a.H && gx < a.W;
            uint2* dst = ok ? a.out + (((((size_t)cur.n * 4 + q) * HW + (size_t)gy * a.W + gx) << 1) + hh) : reinterpret_cast<uint2*>(&h8_trash_rec);
            *dst = make_uint2(hp[pr - 1], hp[pr]);
          }
        }
      };
#pragma unroll
      for (int g = 0; g < RING - 1; ++g) { read_a(g); read_b(g); }
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const int i = g / 18, m = g % 18;
        if (g + RING - 1 < 18) read_a(g + RING - 1);
        if (g + RING - 1 < G) read_b(g + RING - 1);
        acc[i & 1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[m], bq[g % RING], m == 0 ? biasv : acc[i & 1], 0, 0, 0);
        if (i > 0 && m < 16) epi_piece(i - 1, m);
        if (m == 16) prefetch_q(i, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int m = 0; m < 16; ++m) epi_piece(PW3 - 1, m);
    }
    CTX_PROF_MARK(4)
    __syncthreads();                                             // the ring rows this band read are free for the next band
    CTX_PROF_MARK(5)
    if (!more) break;
    cur = nxt;
    run_p1(cur);
  }
#ifdef SLU_CTX_PROF
  if (tid == 0) {
    for (int i = 0; i < 6; ++i) atomicAdd(&g_ctx_prof[i], prof_acc[i]);
    atomicAdd(&g_ctx_prof[6], 1ull);
  }
#endif
}

template <int NKS1>
int launch_ctx(CtxArgs& a, hipStream_t st) {
  constexpr size_t lds = lds_bytes<NKS1>();
  static_assert(lds <= 160 * 1024, "rings do not fit in LDS");
  constexpr long long NCU = 256;                                 // one 8-wave workgroup per CU (LDS)
  const long long strips = (long long)((a.W + TW - 1) / TW) * a.N;
  const int bands = (a.H + R - 1) / R;
  int per = bands;                                               // bands per segment: whole strips unless CUs would idle
  if (strips < NCU) {
    const int nseg = (int)std::min<long long>(bands, (NCU + strips - 1) / strips);
    per = (bands + nseg - 1) / nseg;
  }
  a.strips_x = (a.W + TW - 1) / TW;
  a.nseg = (bands + per - 1) / per;
  a.seg_rows = per * R;
  const long long nt = strips * a.nseg;
  if (nt <= 0 || nt > 0x7fffffffLL || (long long)bands * R + 2 * R > 0x7fffffffLL) return SLU_EUNSUPPORTED;
  long long gx = NCU;
  if (gx > nt) gx = nt;
  static SluLdsGrant grant;
  return slu_launch_lds(ctx_h8_kernel<NKS1>, dim3((unsigned)gx), dim3(64 * NWAVE), lds, st, grant, a);
}

}  // namespace

#ifdef SLU_CTX_PROF
extern "C" int slu_ctx_prof_read(unsigned long long* out8) {
  if (hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_ctx_prof), sizeof(unsigned long long) * 8) != hipSuccess) return SLU_ELAUNCH;
  unsigned long long z[8] = {};
  return hipMemcpyToSymbol(HIP_SYMBOL(g_ctx_prof), z, sizeof(z)) == hipSuccess ? SLU_OK : SLU_ELAUNCH;
}
#endif

extern "C" int slu_ctx_block_h8_supported(int Cin, int C, int H, int W) { return (Cin >= 1 && Cin <= 32 && C == 32 && H > 0 && W > 0 && W < (1 << 20)) ? 1 : 0; }

extern "C" int slu_ctx_block_h8_fwd(const slu_ctx_block_h8_desc* d, slu_stream_t stream) {
  if (!d || !d->x || !d->w1 || !d->w2 || !d->w3 || !d->out || d->N <= 0 || d->H <= 0 || d->W <= 0) return SLU_EINVAL;
  if (((uintptr_t)d->x | (uintptr_t)d->out | (uintptr_t)d->w1 | (uintptr_t)d->w2 | (uintptr_t)d->w3) & 15) return SLU_EINVAL;
  if ((d->bn1_a == nullptr) != (d->bn1_b == nullptr) || (d->bn2_a == nullptr) != (d->bn2_b == nullptr)) return SLU_EINVAL;
  if (!slu_ctx_block_h8_supported(d->Cin, d->C, d->H, d->W)) return SLU_EUNSUPPORTED;
  if (!(d->slope >= 0.0f && d->slope <= 1.0f)) return SLU_EINVAL;      // LeakyReLU as max(t, slope t)
  if (d->x == d->out) return SLU_EINVAL;                                  // strips read their neighbours' halo
  if (d->nbatch < 0 || (d->nbatch > 0 && d->N % d->nbatch)) return SLU_EINVAL;
  CtxArgs a{};
  a.x = reinterpret_cast<const uint4*>(d->x);
  a.w1 = reinterpret_cast<const uint4*>(d->w1);
  a.w2 = reinterpret_cast<const uint4*>(d->w2);
  a.w3 = reinterpret_cast<const uint4*>(d->w3);
  a.b1 = d->bias1; a.b2 = d->bias2; a.bn1_a = d->bn1_a; a.bn1_b = d->bn1_b; a.b3 = d->bias3; a.bn2_a = d->bn2_a; a.bn2_b = d->bn2_b;
  a.slope = d->slope;
  a.out = reinterpret_cast<uint2*>(d->out);
  a.N = d->N; a.H = d->H; a.W = d->W; a.Gin = (d->Cin + 7) / 8;
  a.nb = d->nbatch;
  hipStream_t st = slu_stream(stream);
  return d->Cin <= 16 ? launch_ctx<1>(a, st) : launch_ctx<2>(a, st);
}
