// h8 convs, the deep-ring 3x3 family (ring3_h8_kernel): the full-resolution 3x3 layers with 32 / 64 (80 -> 32) channels, among them the one
// that reads its first source through PixelShuffle in place.  The map of the families is in conv2d_h8.hip.
#include "conv_h8.h"

using namespace slu_h8;

namespace {

// -----------------------------------------------------------------------------------------------------------
// 3x3 convs of the full-resolution layers with 32 / 64 input and output channels, ONE plain source: the deep-ring form.
// conv_h8_kernel keeps one 16-channel chunk (~21-43 KB) of DMA in flight per CU while it multiplies the previous one; at
// 5.5 TB/s x ~2 us of loaded latency a CU needs ~43 KB in flight ALL the time, and these layers have too little MFMA work
// per chunk to cover one round trip.  Here (the structure of tail2_h8_kernel, conv_tail_h8.hip):
//   * all weights resident in LDS for the life of the persistent workgroup (<= 72 KB);
//   * the rest of the LDS is a ring of D input chunks (16 channels with halo), D - 1 of them in flight;
//   * one wave owns ALL output channels of its pixels (MB blocks) and RPW rows; fragments double-buffered in source order;
//   * counted vmcnt waits: every wave issues the same VM operations at every position of every tile (surplus DMA slots
//     copy the zero record to a trash block, beyond the last tile whole chunks do);
//   * whole 16-byte records per lane on the way out (v_permlane32_swap between lanes jj and jj + 32).
// One tile = NKS positions: wait(chunk s) | barrier | DMA(chunk s + P) | 9 taps of chunk s ; after the last: epilogue, NST stores.
// -----------------------------------------------------------------------------------------------------------
struct RingArgs {
  const uint4 *x, *x1;         // h8 [N][G0][H][W] (+ a second plain source [N][G1][H][W], G0 + G1 = 2 NKS, G0 even: the concatenation)
  int G0, G1;
  const uint4* wpack;          // [MB][NKS][9][64]
  const float *bias, *bn_a, *bn_b;
  float slope;                 // 1 = no activation
  uint4* out;                  // h8 [N][4 MB][H][W]
  int N, H, W, tiles_x, tiles_y;
  // x read through PixelShuffle(2) in place (NKS = 5 only): x is [N][4 G0][H/2][W/2] with channels stored in shuffle order, so the record of
  // contributed block g at pixel (gy, gx) is the stored record of plane 4 g + 2 (gy & 1) + (gx & 1) at (gy >> 1, gx >> 1)
  int shuf;
  const float* sc0;            // shuf: [N][32 G0] fp32 multipliers per stored channel (stored order) or nullptr
};

template <int NKS, int NIB, int P, int NST>
constexpr int ring3_younger(int c) {             // VM operations issued after the DMA of chunk c and before the top of position c
  const int s0 = ((c - P) % NKS + NKS) % NKS;
  int n = s0 == NKS - 1 ? NST : 0;
  for (int d = 1; d < P; ++d) n += NIB + ((s0 + d) % NKS == NKS - 1 ? NST : 0);
  return n;
}

template <int DIL, int MB, int NKS, int RPW, int D>
__global__ __launch_bounds__(512, 2) void ring3_h8_kernel(const RingArgs a) {
  constexpr int NWAVE = 8, KS = 3, T = 9, PAD = DIL, P = D - 1;
  constexpr int C = 32 * MB, GO = 4 * MB;
  constexpr int TW = 64, TH = NWAVE * RPW, NB = 2 * RPW;
  constexpr int LW = TW + 2 * PAD, LH = TH + 2 * PAD, REC = LH * LW;
  constexpr int NBLK_B = (2 * REC + 63) / 64, NIB = (NBLK_B + NWAVE - 1) / NWAVE;
  constexpr int BUFREC = NBLK_B * 64;
  constexpr int NST = MB * NB * 2;
  static_assert(P >= 1 && P <= NKS, "ring depth");

  // static array + native vector loads: see tail2_h8_kernel (reads without a TBAA tag are guarded with vmcnt(0) by the compiler)
  __shared__ __attribute__((aligned(16))) float s_epi[3 * C];
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint4* s_w = reinterpret_cast<uint4*>(smem);                      // [MB][NKS][9][64]
  uint4* s_ring = s_w + MB * NKS * T * 64;                          // [D][BUFREC]
  uint4* s_trash = s_ring + D * BUFREC;                             // [64]
  uint4* s_mul = s_trash + 64;                                      // shuf with multipliers: [N][4 G0] fp16 records, one per stored block

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), wn = wave;
  const int hh = lane >> 5, jj = lane & 31;
  const size_t HW = (size_t)a.H * a.W;

  const H8Run run = h8_tile_run(a.tiles_x, a.tiles_y, a.N);
  const int t_beg = run.beg, t_end = run.end, t_step = run.step;
  if (t_beg >= t_end) return;

  if (tid < C) H8_FILL_EPI(s_epi, 0, C, tid, true, tid, a.bias, a.bn_a, a.bn_b);
  for (int blk = wave; blk < MB * NKS * T; blk += NWAVE) SLU_GLDS16(a.wpack + (size_t)blk * 64 + lane, s_w + blk * 64);
  const bool mul0 = NKS == 5 && a.shuf && a.sc0;
  if constexpr (NKS == 5) {
    // the multiplier table goes to LDS once, here: the tile loop's VM operations (and ring3_younger) stay what they are
    if (mul0) {
      for (int e = tid; e < a.N * 4 * a.G0; e += 64 * NWAVE) {
        s_mul[e] = __builtin_bit_cast(uint4, h8_multipliers(a.sc0 + (size_t)e * 8));
      }
    }
  }
  const int hw4 = (a.H >> 1) * (a.W >> 1), w2 = a.W >> 1;

  struct TilePos { int x0, y0, n; };
  auto decode = [&](int t) {
    TilePos p;
    const int tx = t % a.tiles_x;
    t /= a.tiles_x;
    p.x0 = tx * TW;
    p.y0 = (t % a.tiles_y) * TH;
    p.n = t / a.tiles_y;
    return p;
  };
  int pc_rc[NIB], pc_off[NIB];
#pragma unroll
  for (int i = 0; i < NIB; ++i) {
    const int e = (i * NWAVE + wave) * 64 + lane;
    const int g2 = e / REC, rem = e - g2 * REC, r = rem / LW, c = rem - r * LW;
    pc_rc[i] = r | (c << 8) | ((g2 & 1) << 16) | ((e < 2 * REC ? 1 : 0) << 17);
    pc_off[i] = (r * a.W + c) * 16;
  }
  auto stage = [&](const TilePos& tp, int c, int slot, bool valid) {
    uint4* db = s_ring + slot * BUFREC;
    const uintptr_t zero = reinterpret_cast<uintptr_t>(&h8_zero_rec);
    const bool second = 2 * c >= a.G0;                  // a K-step never straddles the two sources (G0 is even)
    const uint4* src = second ? a.x1 : a.x;
    const int gs = second ? a.G1 : a.G0, g = second ? 2 * c - a.G0 : 2 * c;
    const bool sh = NKS == 5 && a.shuf && !second;      // the 4 stored planes of a contributed block span HW records, as a plain block does
    const uintptr_t base0 = reinterpret_cast<uintptr_t>(src) +
                            16 * ((long long)(((size_t)tp.n * gs + g) * HW) + (sh ? 0ll : (long long)(tp.y0 - PAD) * a.W + (tp.x0 - PAD)));
    const uintptr_t base1 = base0 + 16 * (long long)HW;
#pragma unroll
    for (int i = 0; i < NIB; ++i) {
      const int blk = i * NWAVE + wave;
      const int rc = pc_rc[i];
      const int gy = tp.y0 - PAD + (rc & 255), gx = tp.x0 - PAD + ((rc >> 8) & 255);
      const bool ok = valid && (rc >> 17) && (unsigned)gy < (unsigned)a.H && (unsigned)gx < (unsigned)a.W;
      int off = pc_off[i];
      if constexpr (NKS == 5) {
        if (sh) off = 16 * ((2 * (gy & 1) + (gx & 1)) * hw4 + (gy >> 1) * w2 + (gx >> 1));
      }
      const uintptr_t p = ok ? (((rc >> 16) & 1) ? base1 : base0) + (long long)off : zero;
      SLU_GLDS16(reinterpret_cast<const uint4*>(p), (NBLK_B % NWAVE == 0 || blk < NBLK_B) ? db + blk * 64 : s_trash);
    }
    asm volatile("" ::: "memory");
  };

  const int bbase = hh * REC + (wn * RPW) * LW + jj;
  TilePos cur = decode(t_beg), nxt = cur;
  bool has_next = t_beg + t_step < t_end;
  if (has_next) nxt = decode(t_beg + t_step);
#pragma unroll
  for (int c = 0; c < P; ++c) stage(cur, c, c, true);
  int rslot = 0, wslot = P % D;
  bool first = true;
  const float2v sl = {a.slope, a.slope};
  const f32x4v* se4p = reinterpret_cast<const f32x4v*>(s_epi) + hh;

  for (int tile = t_beg; tile < t_end; tile += t_step) {
    f32x16 acc[MB][NB];
    h8_zero(acc);

    auto position = [&](auto cc) {
      constexpr int c = decltype(cc)::value;
      constexpr int YOUNG = ring3_younger<NKS, NIB, P, NST>(c);
      static_assert(YOUNG <= 63, "vmcnt is a 6-bit counter");
      if (first && c < P) h8_vmcnt<0>();          // the first tile's prologue (and the resident weights)
      else h8_vmcnt<YOUNG>();
      h8_lds_barrier();
      {
        constexpr int cn = (c + P) % NKS;
        if (c + P < NKS) stage(cur, cn, wslot, true);
        else stage(nxt, cn, wslot, has_next);
        wslot = wslot + 1 == D ? 0 : wslot + 1;
      }
      const uint4* sb = s_ring + rslot * BUFREC + bbase;
      rslot = rslot + 1 == D ? 0 : rslot + 1;
      half8 fa[2][MB], fb[2][NB];
      // K-step 0 of a shuffled source with multipliers: the lane's B fragment at tap (ty, tx) is input pixel (y0 + wn + ty - 1, x0 + 32 b + jj + tx - 1)
      // of contributed block hh = stored block 4 hh + 2 (row parity) + (column parity); y0 and x0 are even, so the lane needs four records of
      // its image's table: msc[ty & 1][tx & 1]
      constexpr bool MUL = NKS == 5 && c == 0 && RPW == 1 && DIL == 1;
      half8 msc[MUL ? 2 : 1][MUL ? 2 : 1];
      if constexpr (MUL) {
        if (mul0) {
#pragma unroll
          for (int ty = 0; ty < 2; ++ty)
#pragma unroll
            for (int tx = 0; tx < 2; ++tx)
              msc[ty][tx] = __builtin_bit_cast(half8, s_mul[cur.n * 4 * a.G0 + 4 * hh + 2 * ((wn + ty + 1) & 1) + ((jj + tx + 1) & 1)]);
        }
      }
      auto rd = [&](int tap, int buf) {
        const int dy = (tap / KS) * DIL, dx = (tap % KS) * DIL;
#pragma unroll
        for (int i = 0; i < MB; ++i) fa[buf][i] = __builtin_bit_cast(half8, s_w[((i * NKS + c) * T + tap) * 64 + lane]);
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          fb[buf][b] = __builtin_bit_cast(half8, sb[((b >> 1) + dy) * LW + (b & 1) * 32 + dx]);
          if constexpr (MUL) {
            if (mul0) fb[buf][b] *= msc[(tap / KS) & 1][(tap % KS) & 1];
          }
        }
      };
      rd(0, 0);
#pragma unroll
      for (int tap = 0; tap < T; ++tap) {
        if (tap + 1 < T) rd(tap + 1, (tap + 1) & 1);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
          for (int i = 0; i < MB; ++i) acc[i][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[tap & 1][i], fb[tap & 1][b], acc[i][b], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
    };
    h8_static_for(position, std::make_integer_sequence<int, NKS>{});
    first = false;

#pragma unroll
    for (int i = 0; i < MB; ++i)
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const int gy = cur.y0 + wn * RPW + (b >> 1), gx = cur.x0 + (b & 1) * 32 + jj;
        const bool ok = gy < a.H && gx < a.W;
        const size_t idx0 = ok ? ((size_t)cur.n * GO + i * 4 + hh) * HW + (size_t)gy * a.W + gx : 0;
#pragma unroll
        for (int pr = 0; pr < 2; ++pr) {
          unsigned hw[4];
#pragma unroll
          for (int q2 = 0; q2 < 2; ++q2) {
            const int q = 2 * pr + q2;
            const int c4 = (i * 32 + 8 * q) / 4;
            const H8Quad t = h8_epilogue(acc[i][b], q, se4p[c4], se4p[C / 4 + c4], se4p[2 * C / 4 + c4], sl);
            hw[2 * q2] = pack2(t.t0);
            hw[2 * q2 + 1] = pack2(t.t1);
          }
          const uint4 rec = h8_swap16(hw[0], hw[1], hw[2], hw[3]);
          *(ok ? a.out + idx0 + (size_t)(2 * pr) * HW : &h8_trash_rec) = rec;
        }
      }
    asm volatile("" ::: "memory");
    cur = nxt;
    has_next = tile + 2 * t_step < t_end;
    if (has_next) nxt = decode(tile + 2 * t_step);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // zero-record DMAs issued for the tile after the last: LDS must not be released under them
}

template <int DIL, int MB, int NKS, int RPW, int D>
int launch_ring3(const H8Args& h, const slu_conv_h8_desc* d, const SluEmit& e) {
  constexpr int TH = 8 * RPW, PAD = DIL;
  constexpr size_t nblk_b = (size_t)(2 * (TH + 2 * PAD) * (64 + 2 * PAD) + 63) / 64;
  constexpr size_t lds0 = ((size_t)MB * NKS * 9 * 64 + (size_t)D * nblk_b * 64 + 64) * 16;      // + 3 * 32 MB floats static
  static_assert(lds0 + 3 * 32 * MB * 4 <= 160 * 1024, "ring does not fit in LDS");
  // a shuffled first source (NKS = 5: UpBlock.conv1 at full resolution): its multiplier table [N][4 G0] records joins the ring in LDS
  const bool shuf = h.src[0].shuf != 0;
  if (shuf && (NKS != 5 || RPW != 1 || DIL != 1 || h.src[0].G != 2)) return SLU_EUNSUPPORTED;      // K-step 0 is the only one multiplied
  const size_t lds = lds0 + ((shuf && h.src[0].scale) ? (size_t)h.N * 4 * h.src[0].G * 16 : 0);
  if (lds + 3 * 32 * MB * 4 > 160 * 1024) return -1;      // the table does not fit: the tiled SCALED kernel
  RingArgs a{};
  a.shuf = shuf ? 1 : 0;
  a.sc0 = shuf ? h.src[0].scale : nullptr;
  a.x = h.src[0].ptr; a.G0 = h.src[0].G;
  a.x1 = h.nsrc > 1 ? h.src[1].ptr : h.src[0].ptr; a.G1 = h.nsrc > 1 ? h.src[1].G : 0;
  a.wpack = h.wpack; a.bias = h.bias; a.bn_a = h.bn_a; a.bn_b = h.bn_b;
  a.slope = (h.has_act & 3) == 1 ? h.slope : 1.0f;
  a.out = reinterpret_cast<uint4*>(d->out);
  a.N = h.N; a.H = h.H; a.W = h.W;
  a.tiles_x = (a.W + 63) / 64;
  a.tiles_y = (a.H + TH - 1) / TH;
  const long long nt = (long long)a.tiles_x * a.tiles_y * a.N;
  if (nt < 256) return -1;      // too few tiles to fill the chip: the tiled kernel
  if (nt > 0x7fffffffLL) return SLU_EUNSUPPORTED;
  if (e.name) return slu_emit_name(e, "ring3_h8_kernel<%d, %d, %d, %d, %d>", DIL, MB, NKS, RPW, D);
  static SluLdsGrant grant;
  return slu_launch_lds(ring3_h8_kernel<DIL, MB, NKS, RPW, D>, dim3(256), dim3(512), lds, e.st, grant, a);
}

// the layers ring3_h8_kernel covers: 3x3 (dil 1 / 2), one or two plain sources of 32 / 64 (80 -> 32: dil 1) channels in all, 32 / 64 output
// channels, h8 output, no residual, activation before BN only
bool ring3_ok(const slu_conv_h8_desc* d, const H8Args& a) {
  static const bool off = slu_env_int("SLU_H8_RING3", 1) == 0;      // A/B switch
  if (off || d->ksize != 3 || d->pad != d->dil || (d->dil != 1 && d->dil != 2) || a.nsrc < 1 || a.nsrc > 2) return false;
  int gsum = 0;
  for (int s = 0; s < a.nsrc; ++s) {
    if ((a.src[s].scale && !a.src[s].shuf) || a.src[s].nb) return false;
    gsum += a.src[s].G;
  }
  // in-place PixelShuffle: the 80 -> 32 instantiation with exactly ONE shuffled K-step (64 stored channels -> blocks 0, 1): the kernel
  // stages any K-step of source 0 through the shuffle but multiplies K-step 0 only
  if (a.src[0].shuf && !(a.nsrc == 2 && a.Gin == 10 && a.src[0].G == 2)) return false;
  if (gsum != a.Gin || (a.nsrc == 2 && (a.src[0].G & 1)) || a.out_f32 || d->resid || (a.has_act & ~1)) return false;
  if ((a.has_act & 1) && !(a.slope >= 0.0f && a.slope <= 1.0f)) return false;      // LeakyReLU as max(t, slope t)
  return (a.Cout == 32 || a.Cout == 64) && ((a.Gin == 4 || a.Gin == 8) || (a.Gin == 10 && a.Cout == 32 && d->dil == 1));
}

// <DIL, MB, NKS, RPW, D>: 16-row tiles (RPW 2) where the weights and the ring fit in LDS; -1 when the layer has fewer than 256 tiles of that height
int launch_ring3_any(const H8Args& a, const slu_conv_h8_desc* d, const SluEmit& e) {
  const int mb = a.Cout / 32, nks = a.Gin / 2;
  if (nks == 5) return launch_ring3<1, 1, 5, 1, 4>(a, d, e);                       // 80 -> 32: PixelShuffle output | skip (UpBlock.conv1, full resolution)
  if (mb == 2 && nks == 4) return d->dil == 1 ? launch_ring3<1, 2, 4, 1, 3>(a, d, e) : launch_ring3<2, 2, 4, 1, 3>(a, d, e);
  if (mb == 2 && nks == 2) return d->dil == 1 ? launch_ring3<1, 2, 2, 2, 3>(a, d, e) : launch_ring3<2, 2, 2, 1, 3>(a, d, e);
  if (mb == 1 && nks == 4) return d->dil == 1 ? launch_ring3<1, 1, 4, 2, 3>(a, d, e) : launch_ring3<2, 1, 4, 1, 3>(a, d, e);
  return d->dil == 1 ? launch_ring3<1, 1, 2, 2, 3>(a, d, e) : launch_ring3<2, 1, 2, 2, 3>(a, d, e);
}

}  // namespace

int slu_h8::h8_ring3(H8Args& a, const slu_conv_h8_desc* d, const SluEmit& e) { return ring3_ok(d, a) ? launch_ring3_any(a, d, e) : -1; }
