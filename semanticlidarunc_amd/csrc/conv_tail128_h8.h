// The C = 128 member of the tail2_h8_kernel family (conv_tail_h8.hip; included there, after TailArgs), reported as tail2_h8_kernel<4, 2, 3, RES>.
//
// At 128 channels the two accumulator sets of the other members (acc3 and acc_out side by side) leave a 2x2 register tile, one LDS
// fragment read per MFMA: the whole LDS bandwidth.  Here ONE set is live at a time, so a wave owns 64 output channels x 128 pixels
// (2 x 4 accumulator tiles, 128 registers, 6 fragment reads per 8 MFMAs as in conv_h8_kernel), the workgroup's tile is 8 rows x 64 columns,
// 8 waves = 2 (channel halves, wm) x 4 (row pairs, wn), and the tile runs in two phases:
//   phase A  8 positions, one K-step (16 channels) of a2 each: the a2 chunk with its halo (2 x 10 x 66 records) and the chunk's 16 tap-weight
//            fragments come by LDS-DMA into a ring of 3 slots, 2 chunks in flight; 4 dilated taps -> acc3
//   epilogue A   acc3 -> bias, LeakyReLU, BN -> fp16 (the rounding the unfused path applies when it stores a3) -> the a3 image in LDS,
//            B-operand layout [16 channel blocks][8 rows][64 columns], 128 KB.  The image is dead during phase A: the ring lives in it.
//   phase B  12 positions of 2 K-steps of the 1x1 over cat(a1, a2, a3), in that order, -> acc_out.  Only the 1x1 weight fragments go through
//            LDS (a ring of 3 x 8 KB beside the image); a1 and a2 are pixel-local, so a lane loads exactly the h8 records that are its B
//            operands straight into registers, 2 K-steps (8 records) a group, two groups in flight; a3 comes from the image.
//   epilogue B   bias, LeakyReLU, BN, + residual, whole 16-byte records both ways (h8_swap16)
// Every wait of the tile loop is a counted vmcnt.  Each wave issues the same vector-memory operations at every position of every tile (surplus
// DMA slots copy the zero record to a trash block, lanes outside the image load pixel 0 of their image and store to the trash record), the
// register loads are inline asm the compiler does not track.  In issue order, per wave and tile (S = one phase-A chunk, NIB = 5 DMAs;
// W = one pair of 1x1 weight K-steps, 1 DMA; R = one register group, 8 loads; Xa / Xb = the residual halves, 8 loads each; ST = 8 stores):
//   S0 S1 | A0: S2 | A1: S3 | ... | A5: S7 | A6: W0 W1 | A7: .. R0 R1 | B0: W2 .. R2 | B1: W3 .. R3 | ... | B5: W7 .. R7 | B6: W8 | B7: W9 |
//   B8: W10 Xa | B9: W11 | B10: Xb | B11 | epilogue B: ST ST
// and "what position p needs has landed" is vmcnt(number of operations issued after it), the constants named below.
// Nothing is in flight across tiles but the stores, so the first tile needs no special case and the exit no wait (the price: the first
// chunk's latency is exposed once per tile, about 2 us of 40).  Without a residual B11 waits in full: nothing is younger than W11.
// Registers: 2 waves per SIMD (one 8-wave workgroup per CU: the LDS), up to 256 VGPRs a wave: 128 accumulators + 64 of register groups (or the
// residual) + fragments.  Splitting into VGPR + AGPR halves at 1 wave per SIMD would leave the MFMA pipe without a second wave to cover the
// barriers of the two rings.

template <bool HASRES>
__device__ __forceinline__ void tail128_h8_body(const TailArgs& a) {
  constexpr int NWAVE = 8, WN = 4, MBW = 2, RPW = 2, T = 4, PAD = 1, DIL = 2, D = 3;
  constexpr int C = 128, NKS = 8, MBLK = 4;
  constexpr int TW = 64, TH = WN * RPW, NB = 2 * RPW;
  constexpr int LW = TW + 2 * PAD, LH = TH + 2 * PAD, REC = LH * LW;
  constexpr int NBLK_B = (2 * REC + 63) / 64, NBLK_A = MBLK * T, NBLK = NBLK_B + NBLK_A;      // 64-record blocks of a chunk: a2 | tap weights
  constexpr int NIB = (NBLK + NWAVE - 1) / NWAVE;                                             // DMA slots per wave and chunk
  constexpr int SLOTREC = NBLK * 64;
  constexpr int IMGREC = (C / 8) * TH * 64;                                                   // the a3 image
  constexpr int NPAIR = 3 * NKS / 2, NRG = NKS;                                               // phase-B positions; register groups (a1: 4, a2: 4)
  constexpr int WPREC = 2 * MBLK * 64;                                                        // one pair of 1x1 weight K-steps
  static_assert(D * SLOTREC <= IMGREC, "the phase-A ring lives inside the a3 image");
  static_assert(NBLK_B == 21 && NIB == 5 && NB == 4 && MBW * NB == 8, "the counted waits below name their registers and counts");
  // counted waits: operations issued after the one waited for (see the schedule above)
  constexpr int W_A = NIB;            // A0 .. A6: the next chunk
  constexpr int W_A7 = 2;             // A7: W0 W1
  constexpr int W_B0 = 8;             // B0: R1
  constexpr int W_BR = 9;             // B1 .. B6: W(j + 1) R(j + 1)
  constexpr int W_B7 = 1;             // B7: W8
  constexpr int W_B8 = 1;             // B8: W9
  constexpr int W_B9 = 9;             // B9: W10 Xa  (without a residual: W10)
  constexpr int W_B10 = 9;            // B10: Xa W11 (W11)
  constexpr int W_B11 = 8;            // B11: Xb     (nothing: the full wait)
  constexpr int W_XA = 8, W_XB = 8;   // epilogue B: Xa under Xb; Xb under the stores of the first half

  __shared__ __attribute__((aligned(16))) float s_epi[6 * C];       // native vector reads, see tail2_h8_kernel
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint4* s_a3 = reinterpret_cast<uint4*>(smem);                     // [C / 8][TH][64]; phase A: the ring [D][SLOTREC]
  uint4* s_wb = s_a3 + IMGREC;                                      // [3][WPREC]
  uint4* s_trash = s_wb + 3 * WPREC;                                // [64]

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), wm = wave >> 2, wn = wave & 3;
  const int hh = lane >> 5, jj = lane & 31;
  const size_t HW = (size_t)a.H * a.W;

  const H8Run run = h8_tile_run(a.tiles_x, a.tiles_y, a.N);
  const int t_beg = run.beg, t_end = run.end, t_step = run.step;
  if (t_beg >= t_end) return;

  if (tid < C) {
    H8_FILL_EPI(s_epi, 0, C, tid, true, tid, a.biasA, a.bnA_a, a.bnA_b);
    H8_FILL_EPI(s_epi, 3 * C, C, tid, true, tid, a.biasB, a.bnB_a, a.bnB_b);
  }

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
  H8_OPAQUE_ADDR(zero, h8_zero_rec);
  H8_OPAQUE_ADDR(trash, h8_trash_rec);
  // DMA slot i of a wave copies block i * 8 + wave of the chunk: an a2 block (records e of [2][LH][LW]), a tap-weight block, or nothing.
  // Whatever a slot derives from the lane alone is tile-invariant, and the compiler would keep all of it (record coordinates, 64-bit
  // addresses of every weight block of every chunk) in registers across the tile loop and spill: the lane is made opaque at every use and
  // the coordinates are computed again, a dozen VALU operations per DMA
  auto lane_again = [&]() {
    int l = lane;
    asm volatile("" : "+v"(l));
    return l;
  };
  auto stage = [&](const TilePos& tp, int c, int slot) {
    uint4* db = s_a3 + slot * SLOTREC;
    const uintptr_t base0 = reinterpret_cast<uintptr_t>(a.a2) +
                            16 * ((long long)(((size_t)tp.n * a.G + 2 * c) * HW) + (long long)(tp.y0 - PAD) * a.W + (tp.x0 - PAD));
    const int l = lane_again();
#pragma unroll
    for (int i = 0; i < NIB; ++i) {
      const int blk = i * NWAVE + wave;
      uintptr_t p = zero;
      if (i * NWAVE < NBLK_B) {      // an a2 block
        const int e = blk * 64 + l;
        const int g2 = e / REC, rem = e - g2 * REC, r = rem / LW, cc = rem - r * LW;
        const int gy = tp.y0 - PAD + r, gx = tp.x0 - PAD + cc;
        const bool ok = e < 2 * REC && (unsigned)gy < (unsigned)a.H && (unsigned)gx < (unsigned)a.W;
        const long long off = (long long)(g2 ? HW : 0) + r * a.W + cc;
        p = ok ? base0 + 16 * off : zero;
      }
      if ((i + 1) * NWAVE > NBLK_B && blk >= NBLK_B) {      // block m * 4 + tap of the chunk's weights (packed [MBLK][NKS][4][64]), or surplus
        const int ab = blk - NBLK_B, m = ab >> 2, tap = ab & 3;
        uintptr_t wsrc = reinterpret_cast<uintptr_t>(a.w2 + (((size_t)m * NKS + c) * T + tap) * 64);
        asm volatile("" : "+s"(wsrc));
        p = blk < NBLK ? wsrc + 16 * l : zero;
      }
      SLU_GLDS16(reinterpret_cast<const uint4*>(p), blk < NBLK ? db + blk * 64 : s_trash);
    }
    asm volatile("" ::: "memory");
  };
  // K-steps 2 j, 2 j + 1 of the 1x1 weights (packed [MBLK][3 NKS][64], cat order (a1, a2, a3)): wave w copies K-step 2 j + (w >> 2), block w & 3
  auto stage_w = [&](int j) {
    uintptr_t wsrc = reinterpret_cast<uintptr_t>(a.w1 + ((size_t)(wave & 3) * 3 * NKS + 2 * j + (wave >> 2)) * 64);
    asm volatile("" : "+s"(wsrc));
    const uintptr_t p = wsrc + 16 * lane_again();
    SLU_GLDS16(reinterpret_cast<const uint4*>(p), s_wb + (j % 3) * WPREC + wave * 64);
    asm volatile("" ::: "memory");
  };

  const int bbase2 = hh * REC + (wn * RPW) * LW + jj;
  const float2v slA = {a.slopeA, a.slopeA}, slB = {a.slopeB, a.slopeB};
  // The wave's share of the epilogue constants and of the a3 image as ONE opaque index each, so that every access is that register plus an
  // immediate offset: left to itself the compiler keeps a register per (channel block, row, group) address across the tile loop and spills
  int se_i = hh + wm * MBW * 8, s3_i = ((((wm * MBW * 4) * TH + wn * RPW) * 64 + jj) << 1) + hh;
  int a3_lo = (hh * TH + wn * RPW) * 64 + jj, a3_hi = a3_lo + IMGREC / 2;      // phase B reads: K-steps 0 .. 3 / 4 .. 7 of a3 (64 KB of offsets each)
  asm volatile("" : "+v"(se_i), "+v"(a3_lo), "+v"(a3_hi));
  const unsigned s3_addr = (unsigned)(uintptr_t)((__attribute__((address_space(3))) char*)smem) + s3_i * 8;      // LDS byte address
  auto se4 = [&](int k) { return reinterpret_cast<const f32x4v*>(s_epi)[se_i + k]; };      // k: float4 index of the wave's channel block i, group q
  __syncthreads();      // the epilogue constants; every later barrier is h8_lds_barrier

  for (int tile = t_beg; tile < t_end; tile += t_step) {
    const TilePos cur = decode(tile);
    f32x16 acc[MBW][NB];
    u32x4v rg[2][2][NB];                       // register groups: [buffer][K-step of the pair][pixel block]
    u32x4v res[HASRES ? MBW : 1][HASRES ? NB : 1][2];
    h8_zero(acc);
    // this lane's records inside image cur.n: channel block hh, pixel of accumulator block b; lanes outside the image read pixel 0.  The
    // channel block pair of a load goes into its scalar base
    unsigned voff[NB];
    bool okb[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const int gy = cur.y0 + wn * RPW + (b >> 1), gx = cur.x0 + (b & 1) * 32 + jj;
      okb[b] = gy < a.H && gx < a.W;
      voff[b] = (unsigned)(((okb[b] ? (size_t)gy * a.W + gx : 0) + hh * HW) << 4);
    }
    const unsigned long long img16 = 16ull * ((size_t)cur.n * a.G * HW);
    // register group j: K-steps 2 j, 2 j + 1 of cat(a1, a2); K-step k of pixel block b = the record of channel block 2 k + hh
    auto load_group = [&](auto jc) {
      constexpr int j = decltype(jc)::value;
      auto& dst = rg[j & 1];                   // named outside the asm: an asm operand alone does not capture
      const unsigned long long base = reinterpret_cast<unsigned long long>(j < NRG / 2 ? a.a1 : a.a2) + img16;
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          const unsigned vo = voff[b];
          const unsigned long long sb = base + 32ull * ((2 * j + kk) % NKS) * HW;
          asm volatile("global_load_dwordx4 %0, %1, %2" : "=&v"(dst[kk][b]) : "v"(vo), "s"(sb) : "memory");
        }
    };
    auto load_resid = [&](auto ic) {           // whole records: lane (jj, hh) loads record 2 pr + hh of channel block i (un-swapped in epilogue B)
      constexpr int i = decltype(ic)::value;
      if constexpr (HASRES) {
        auto& dst = res[i];
        const unsigned long long base = reinterpret_cast<unsigned long long>(a.resid) + img16;
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
          for (int pr = 0; pr < 2; ++pr) {
            const unsigned vo = voff[b];
            const unsigned long long sb = base + 16ull * ((wm * MBW + i) * 4 + 2 * pr) * HW;
            asm volatile("global_load_dwordx4 %0, %1, %2" : "=&v"(dst[b][pr]) : "v"(vo), "s"(sb) : "memory");
          }
      }
    };

    // ---- phase A ----
    h8_lds_barrier();                          // every wave has read the previous tile's a3 image: the ring may overwrite it
    stage(cur, 0, 0);
    stage(cur, 1, 1);
    auto position_a = [&](auto cc) {
      constexpr int c = decltype(cc)::value;
      h8_vmcnt<(c < NKS - 1 ? W_A : W_A7)>();
      h8_lds_barrier();
      if constexpr (c + 2 < NKS) stage(cur, c + 2, (c + 2) % D);
      if constexpr (c == NKS - 2) { stage_w(0); stage_w(1); }
      const uint4* sb = s_a3 + (c % D) * SLOTREC + bbase2;
      const uint4* sa = s_a3 + (c % D) * SLOTREC + (NBLK_B + wm * MBW * T) * 64 + lane;
      // 4 dilated taps, fragments double-buffered: the reads of tap s + 1 are issued before the MFMAs of tap s (as in tail2_h8_kernel)
      half8 fa[2][MBW], fb[2][NB];
      auto rd = [&](int st, int buf) {
        const int dy = (st >> 1) * DIL, dx = (st & 1) * DIL;
#pragma unroll
        for (int i = 0; i < MBW; ++i) fa[buf][i] = __builtin_bit_cast(half8, sa[(i * T + st) * 64]);
#pragma unroll
        for (int b = 0; b < NB; ++b) fb[buf][b] = __builtin_bit_cast(half8, sb[((b >> 1) + dy) * LW + (b & 1) * 32 + dx]);
      };
      rd(0, 0);
#pragma unroll
      for (int st = 0; st < T; ++st) {
        if (st + 1 < T) rd(st + 1, (st + 1) & 1);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
          for (int i = 0; i < MBW; ++i) acc[i][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[st & 1][i], fb[st & 1][b], acc[i][b], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
      if constexpr (c == NKS - 1) {      // after the last fragments: the registers of phase A's double buffer are free
        load_group(std::integral_constant<int, 0>{});
        load_group(std::integral_constant<int, 1>{});
      }
    };
    h8_static_for(position_a, std::make_integer_sequence<int, NKS>{});

    // ---- epilogue A: the a3 image over the ring, once every wave has left it ----
    h8_lds_barrier();
    // The writes are inline asm: a ds_write the compiler sees is guarded with s_waitcnt vmcnt(0) while an LDS-DMA it issued (W0, W1) may be in
    // flight, which would drain the register groups R0 and R1 too.  The barrier at the top of phase B waits for them (lgkmcnt(0)).
#pragma unroll
    for (int i = 0; i < MBW; ++i)
#pragma unroll
      for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int c4 = (i * 32 + 8 * q) / 4;
          const uint2 v = pack4(h8_epilogue(acc[i][b], q, se4(c4), se4(C / 4 + c4), se4(2 * C / 4 + c4), slA));
          const unsigned long long v64 = (unsigned long long)v.x | ((unsigned long long)v.y << 32);
          asm volatile("ds_write_b64 %0, %1 offset:%2" ::"v"(s3_addr), "v"(v64), "n"(((((i * 4 + q) * TH + (b >> 1)) * 64 + (b & 1) * 32) << 1) * 8) : "memory");
        }
    h8_zero(acc);

    // ---- phase B ----
    auto position_b = [&](auto jc) {
      constexpr int j = decltype(jc)::value;
      constexpr int XA = HASRES ? 8 : 0;
      if constexpr (j < NRG) {                 // weights pair j and register group j
        constexpr int n = j == 0 ? W_B0 : (j == NRG - 1 ? W_B7 : W_BR);
        asm volatile("s_waitcnt vmcnt(%8)"
                     : "+v"(rg[j & 1][0][0]), "+v"(rg[j & 1][0][1]), "+v"(rg[j & 1][0][2]), "+v"(rg[j & 1][0][3]),
                       "+v"(rg[j & 1][1][0]), "+v"(rg[j & 1][1][1]), "+v"(rg[j & 1][1][2]), "+v"(rg[j & 1][1][3])
                     : "n"(n)
                     : "memory");
      } else {
        h8_vmcnt<(j == 8 ? W_B8 : j == 9 ? W_B9 - 8 + XA : j == 10 ? W_B10 - 8 + XA : W_B11 - 8 + XA)>();
      }
      h8_lds_barrier();
      if constexpr (j + 2 < NPAIR) stage_w(j + 2);
      if constexpr (j == 8) load_resid(std::integral_constant<int, 0>{});
      if constexpr (j == 10) load_resid(std::integral_constant<int, 1>{});
      const uint4* sw = s_wb + (j % 3) * WPREC + (wm * MBW) * 64 + lane;
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        half8 af[MBW], bf[NB];
#pragma unroll
        for (int i = 0; i < MBW; ++i) af[i] = __builtin_bit_cast(half8, sw[(kk * MBLK + i) * 64]);
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          if constexpr (j < NRG) bf[b] = __builtin_bit_cast(half8, rg[j & 1][kk][b]);
          else bf[b] = __builtin_bit_cast(half8, s_a3[(j < NRG + 2 ? a3_lo : a3_hi) + ((2 * ((2 * (j - NRG) + kk) & 3)) * TH + (b >> 1)) * 64 + (b & 1) * 32]);
        }
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
          for (int i = 0; i < MBW; ++i) acc[i][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[i], bf[b], acc[i][b], 0, 0, 0);
        if constexpr (j >= NRG) __builtin_amdgcn_sched_barrier(0);      // one K-step of a3 fragments at a time: the residual is in registers
      }
      if constexpr (j + 2 < NRG) {
        __builtin_amdgcn_sched_barrier(0);      // the group's buffer is free once the MFMAs that read it have been issued
        load_group(std::integral_constant<int, j + 2>{});
      }
    };
    h8_static_for(position_b, std::make_integer_sequence<int, NPAIR>{});

    // ---- epilogue B: 16 stores per lane, whole records (see tail2_h8_kernel); the residual's second half lands under the first half's stores ----
    auto epilogue_b = [&](auto ic) {
      constexpr int i = decltype(ic)::value;
      if constexpr (HASRES) {
        asm volatile("s_waitcnt vmcnt(%8)"
                     : "+v"(res[i][0][0]), "+v"(res[i][0][1]), "+v"(res[i][1][0]), "+v"(res[i][1][1]),
                       "+v"(res[i][2][0]), "+v"(res[i][2][1]), "+v"(res[i][3][0]), "+v"(res[i][3][1])
                     : "n"(i == 0 ? W_XA : W_XB)
                     : "memory");
      }
#pragma unroll
      for (int b = 0; b < NB; ++b) {
#pragma unroll
        for (int pr = 0; pr < 2; ++pr) {
          uint4 rw = make_uint4(0u, 0u, 0u, 0u);       // residual words: x, y for q = 2 pr; z, w for q = 2 pr + 1
          if constexpr (HASRES) rw = h8_swap16(res[i][b][pr].x, res[i][b][pr].y, res[i][b][pr].z, res[i][b][pr].w);
          unsigned hw[4];
#pragma unroll
          for (int q2 = 0; q2 < 2; ++q2) {
            const int q = 2 * pr + q2;
            const int c4 = (i * 32 + 8 * q) / 4;
            H8Quad t = h8_epilogue(acc[i][b], q, se4(3 * C / 4 + c4), se4(4 * C / 4 + c4), se4(5 * C / 4 + c4), slB);
            if constexpr (HASRES) h8_add_resid(t, q2 ? make_uint2(rw.z, rw.w) : make_uint2(rw.x, rw.y));
            hw[2 * q2] = pack2(t.t0);
            hw[2 * q2 + 1] = pack2(t.t1);
          }
          const uint4 rec = h8_swap16(hw[0], hw[1], hw[2], hw[3]);
          const uintptr_t dst = reinterpret_cast<uintptr_t>(a.out) + img16 + 16ull * ((wm * MBW + i) * 4 + 2 * pr) * HW;      // scalar, as for the loads
          *reinterpret_cast<__attribute__((address_space(1))) u32x4v*>(okb[b] ? dst + voff[b] : trash) = u32x4v{rec.x, rec.y, rec.z, rec.w};      // global_store, not FLAT
        }
      }
      asm volatile("" ::: "memory");
    };
    h8_static_for(epilogue_b, std::make_integer_sequence<int, MBW>{});
  }
}

// The symbol is tail128_h8_kernel<HASRES>; the dispatch reports it as the family member it is, tail2_h8_kernel<4, 2, 3, RES> (MB = 4 channel
// blocks of 32, 2 rows per wave, ring depth 3).  tools/check_counted_waits.py scans both spellings.
template <bool HASRES>
__global__ __launch_bounds__(512, 2) void tail128_h8_kernel(const TailArgs a) { tail128_h8_body<HASRES>(a); }

// one 8-wave workgroup per CU; `fits`: the register loads address an image with 32-bit offsets
inline bool tail128_fits(int G, int H, int W) { return (unsigned long long)G * H * W * 16ull < (1ull << 32); }
constexpr size_t tail128_lds_bytes() { return ((size_t)16 * 8 * 64 + 3 * 2 * 4 * 64 + 64) * 16; }      // + 6 C floats static
