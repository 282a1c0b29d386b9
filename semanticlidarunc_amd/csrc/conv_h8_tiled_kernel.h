// The tiled h8 conv kernel's definition (see "Tiled kernel" in conv_h8_tiled.hip, which includes this file; what it names is there and in conv_h8.h).
// No include guard: conv_h8_tiled.hip includes it once per kernel symbol, with
//   H8_TILED_KERNEL   the symbol: conv_h8_kernel, conv_h8_late_kernel
//   H8_TILED_LATE     false: out = [resid +] bn(act(conv + bias));  true: out = act(conv + bias + resid), the activation after the residual add
// Two symbols from one text rather than one more template parameter or a shared __device__ body: either of those changes the name or the
// instruction stream of every existing instantiation (tools/h8_isa_diff.py), and the tests and profiles name those.
template <int KS, int DIL, int PAD, int MB, int WM, int WN, int RPW, bool SCALED, bool WRES, bool F32OUT, int KPC = 1, int OPT = 0, bool ONE = false>
__global__ __launch_bounds__(64 * WM * WN, h8_waves_per_simd(MB, WM * WN, RPW)) void H8_TILED_KERNEL(const H8Args a, const void* __restrict__ resid,
                                                                                                       void* __restrict__ out) {
  constexpr bool LATE = H8_TILED_LATE;
  static_assert(!LATE || (KS == 3 && DIL == 1 && PAD == 1 && !SCALED && !F32OUT && KPC == 1), "late activation: the plain 3x3 / dil 1 family, h8 output");
  constexpr int NWAVE = WM * WN;
  constexpr int T = KS * KS, TS = KPC * T;          // taps per K-step, tap-steps per chunk
  constexpr int TW = 64, TH = WN * RPW, NB = 2 * RPW;
  constexpr int LW = TW + 2 * PAD, LH = TH + 2 * PAD;
  constexpr int REC = LH * LW;                      // records per channel block
  constexpr int MBLK = WM * MB;
  constexpr int NREC_B = KPC * 2 * REC, NBLK_B = (NREC_B + 63) / 64;    // 64-record pieces of the input tile of a chunk
  constexpr int NB_ALLOC = NBLK_B * 64;
  constexpr int NREC_A = MBLK * TS * 64, NBLK_A = MBLK * TS;            // weight fragments of a chunk
  constexpr int NIB = (NBLK_B + NWAVE - 1) / NWAVE, NIA = (NBLK_A + NWAVE - 1) / NWAVE;
  static_assert(KPC == 1 || (!WRES && !SCALED && MB == 2 && WM == 2 && WN == 4), "multi-K-step chunks: the 8-wave 128-channel configuration only");
  static_assert(OPT == 0 || (MB == 2 && WM == 2 && WN == 4 && !F32OUT), "OPT: the 8-wave 128-channel configuration only");
  static_assert(KPC <= 2, "pc_rc carries 2 bits of channel block");
  static_assert(KPC == 1 || ONE, "multi-K-step chunks: single-source layers only");
  // SHUF: the instantiations that can read source 0 through PixelShuffle(2) in place (H8Src.shuf, a runtime property: UpBlock.conv1 with
  // multipliers).  The K-steps of source 0 fetch, for tile-image pixel (gy, gx) of contributed block g, the stored record of plane
  // 4 g + 2 (gy & 1) + (gx & 1) at (gy >> 1, gx >> 1) -- a block's four stored planes span H W records like a plain block, so only the
  // per-lane offset differs -- and their multiplier is the one of that STORED block: selected by the parity of the pixel a B fragment reads.
  constexpr bool SHUF = SCALED && KS == 3 && DIL == 1 && PAD == 1 && !ONE && KPC == 1;
  static_assert(!SHUF || (WN * RPW) % 2 == 0, "tile rows start on even image rows");

  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* s_epi = reinterpret_cast<float*>(smem);                        // bias | bn_a | bn_b
  uint4* s_scale = reinterpret_cast<uint4*>(s_epi + 3 * MBLK * 32);     // [2][64] fp16 multipliers per channel block (SCALED)
  uint4* s_b = s_scale + (SCALED ? 128 : 0);                            // [2][NB_ALLOC]
  uint4* s_a = s_b + 2 * NB_ALLOC;                                      // WRES: [MBLK][nks][T][64]; else [2][MBLK][KPC][T][64]

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
  const bool late_half = wave >= NWAVE / 2;      // waves 4..7 share their SIMDs with waves 0..3
  const int mblk0 = blockIdx.y * MBLK;
  // h8_tile_run's numbering with the `order` switch, written out: as a branch of the helper (by value, by reference, as a returned struct)
  // the interleaved form re-associated the t_end arithmetic of every instantiation
  int t_beg, t_end, t_step = 1;
  {
    const int nwg = gridDim.x, b = blockIdx.x, xcd = b & 7, qq = nwg >> 3, rr = nwg & 7;
    const int w = (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + (b >> 3);
    const long long nt = (long long)a.tiles_x * a.tiles_y * a.N;
    if (a.order) {      // interleaved (the default)
      t_step = nwg;
      t_beg = w;
      t_end = w < nt ? w + (int)((nt - w + nwg - 1) / nwg) * nwg : w;
    } else {            // contiguous run [nt w / nwg, nt (w + 1) / nwg), kept for A/B runs
      t_beg = (int)(nt * w / nwg);
      t_end = (int)(nt * (w + 1) / nwg);
    }
  }
  t_beg = __builtin_amdgcn_readfirstlane(t_beg);
  t_end = __builtin_amdgcn_readfirstlane(t_end);
  t_step = __builtin_amdgcn_readfirstlane(t_step);
  if (t_beg >= t_end) return;

  if (tid < MBLK * 32) {
    const int co = mblk0 * 32 + tid;
    const bool ok = co < a.Cout;
    H8_FILL_EPI(s_epi, 0, MBLK * 32, tid, ok, co, a.bias, a.bn_a, a.bn_b);
  }

  const int hh = lane >> 5, jj = lane & 31;
  const size_t HW = (size_t)a.H * a.W;
  const float slope_act = (a.has_act & 3) == 1 ? a.slope : 1.0f;
  const float slope_pre = LATE ? 1.0f : slope_act;      // LATE: the activation follows the residual add (slope_act goes to the store)
  const int nks = a.nks;
  const int nchunk = (nks + KPC - 1) / KPC;
  const int a_stride = WRES ? nks * T * 64 : TS * 64;                   // uint4 per channel block in s_a
  const int abase = (wm * MB) * a_stride + lane;
  const int bbase = hh * REC + (wn * RPW) * LW + jj;                    // + (rr + dy)*LW + cb*32 + dx

  // Tile bookkeeping stays on the scalar unit: the position of the first tile comes from one division, every later one from adding the
  // (pre-divided) tile stride with carries.  Integer division runs on the vector ALU even for uniform operands; left to itself hipcc
  // kept the whole per-chunk staging set-up that depends on it in VGPRs (and in scratch, reloaded behind a vmcnt(0) that also drained
  // the DMA queue) -- readfirstlane pins the results to SGPRs.
  struct TilePos { int tx, ty, x0, y0, n, i0, i1, i2; };      // i_s: the image of source s that output image n reads (once per tile, not per chunk)
  auto rfl = [](int v) __attribute__((always_inline)) { return __builtin_amdgcn_readfirstlane(v); };
  const int step_tx = rfl(t_step % a.tiles_x), step_ty = rfl((t_step / a.tiles_x) % a.tiles_y), step_n = rfl(t_step / (a.tiles_x * a.tiles_y));
  auto finish = [&](TilePos& p) __attribute__((always_inline)) {
    p.x0 = p.tx * TW;
    p.y0 = p.ty * TH;
    p.i0 = p.i1 = p.i2 = p.n;
    if constexpr (!ONE) {
      if (a.src[0].nb) p.i0 = rfl(p.n % a.src[0].nb);
      if (a.nsrc > 1 && a.src[1].nb) p.i1 = rfl(p.n % a.src[1].nb);
      if (a.nsrc > 2 && a.src[2].nb) p.i2 = rfl(p.n % a.src[2].nb);
    }
  };
  auto decode = [&](int t) __attribute__((always_inline)) {
    TilePos p;
    p.tx = rfl(t % a.tiles_x);
    t /= a.tiles_x;
    p.ty = rfl(t % a.tiles_y);
    p.n = rfl(t / a.tiles_y);
    finish(p);
    return p;
  };
  auto advance = [&](TilePos p) __attribute__((always_inline)) {      // the tile t_step after p
    p.tx += step_tx;
    if (p.tx >= a.tiles_x) p.tx -= a.tiles_x, p.ty += 1;
    p.ty += step_ty;
    if (p.ty >= a.tiles_y) p.ty -= a.tiles_y, p.n += 1;
    p.n += step_n;
    finish(p);
    return p;
  };
  static_assert(SLU_MAX_SRC == 3, "TilePos carries one image index per source");
  H8_OPAQUE_ADDR(zero_addr, h8_zero_rec);
  H8_OPAQUE_ADDR(trash_addr, h8_trash_rec);
  // Per-lane description of the input-tile pieces this wave copies (the same for every chunk and tile): piece i covers
  // records [64 (i NWAVE + wave), +64) of the [2 KPC][LH][LW] tile image; pc_rc = row | col << 8 | block << 16 | inside << 20.
  int pc_rc[NIB], pc_off[NIB];
#pragma unroll
  for (int i = 0; i < NIB; ++i) {
    const int e = (i * NWAVE + wave) * 64 + lane;
    const int g2 = e / REC;
    const int rem = e - g2 * REC;
    const int r = rem / LW;
    const int c = rem - r * LW;
    pc_rc[i] = r | (c << 8) | ((g2 & (2 * KPC - 1)) << 16) | ((e < NREC_B ? 1 : 0) << 20);
    pc_off[i] = r * a.W + c + (g2 & (2 * KPC - 1)) * (int)HW;      // block g of the chunk starts g planes after block 0 (same source)
  }
  // LDS-DMA of chunk q of tile tp into input buffer `buf` (and, unless WRES, its weight fragments into weight buffer `buf`),
  // in NPIECE pieces per wave: stage_begin fixes the wave-uniform part, stage_piece(i) issues one global_load_lds.  The
  // pieces of chunk c+1 are issued BETWEEN the taps of chunk c (see the tap loops): when all of them came in one burst
  // right after the barrier, the eight waves queued on the CU's single address pipe while the matrix cores idled
  // (measured with -DSLU_H8_PROF: 25 % of the kernel in that burst, another 20 % in the barrier behind it).
  constexpr int NPIECE = NIB + (WRES ? 0 : NIA);
  constexpr int PPT = (NPIECE + TS - 1) / TS;        // pieces issued after each tap-step
  // st_b0: byte address of the record at tile-image position (0, 0) of the chunk's first block; st_b1: the same for its second block
  // MINUS one plane (pc_off carries the plane offset of the block), which equals st_b0 unless the K-step straddles two sources
  uintptr_t st_b0 = 0, st_b1 = 0;
  bool st_sh = false;                                  // SHUF: the chunk belongs to the shuffled source 0 (an even number of blocks: never straddles)
  const int hw4 = (a.H >> 1) * (a.W >> 1), w2 = a.W >> 1;
  int st_g0 = 0;                                       // first channel block of the chunk (a block g is live while st_g0 + g < Gin)
  bool st_on = false;
  int st_x0 = 0, st_y0 = 0, st_q = 0, st_wave = wave;
  uint4 *st_db = s_b, *st_da = s_a;
  auto stage_begin = [&](const TilePos& tp, int q, int buf) __attribute__((always_inline)) {
    const int img[SLU_MAX_SRC] = {tp.i0, tp.i1, tp.i2};
    long long org = (long long)(tp.y0 - PAD) * a.W + (tp.x0 - PAD);
    st_g0 = 2 * KPC * q;
    if constexpr (SHUF) {
      st_sh = a.src[0].shuf && st_g0 < a.src[0].G;
      if (st_sh) org = 0;                              // the pieces carry the whole in-image offset
    }
    if constexpr (ONE) {
      st_b0 = reinterpret_cast<uintptr_t>(a.src[0].ptr) + 16 * ((long long)(((size_t)tp.n * a.src[0].G + st_g0) * HW) + org);
      st_b1 = st_b0;
    } else {
      const SrcSel p0 = select_src(a, img, st_g0 < a.Gin ? st_g0 : 0), p1 = select_src(a, img, st_g0 + 1 < a.Gin ? st_g0 + 1 : 0);
      st_b0 = reinterpret_cast<uintptr_t>(p0.ptr) + 16 * ((long long)(((size_t)p0.ns * p0.G + p0.gl) * HW) + org);
      st_b1 = reinterpret_cast<uintptr_t>(p1.ptr) + 16 * ((long long)(((size_t)p1.ns * p1.G + p1.gl) * HW) + org - (long long)HW);
    }
    st_x0 = tp.x0 - PAD;
    st_y0 = tp.y0 - PAD;
    st_q = q;
    st_db = s_b + buf * NB_ALLOC;
    st_da = s_a + buf * NREC_A;
    st_on = true;
    // an opaque copy of the wave number per chunk: otherwise every piece's LDS address and bounds test is hoisted out of the tile loop
    // as a loop invariant, ~100 SGPRs live across it, spilled to VGPR lanes (and, in the two-K-step form, to scratch)
    st_wave = wave;
    asm volatile("" : "+s"(st_wave));
  };
  auto stage_piece = [&](int i) __attribute__((always_inline)) {
    if (i < NIB) {
      const int blk = i * NWAVE + st_wave;
      if (NBLK_B % NWAVE == 0 || blk < NBLK_B) {
        const int rc = pc_rc[i];
        const int gy = st_y0 + (rc & 255), gx = st_x0 + ((rc >> 8) & 255);
        const int gsel = (rc >> 16) & 3;
        const uintptr_t gb = (!ONE && gsel == 1) ? st_b1 : st_b0;
        const bool ok = (rc >> 20) && st_g0 + gsel < a.Gin && (unsigned)gy < (unsigned)a.H && (unsigned)gx < (unsigned)a.W;
        int off = pc_off[i];                           // records; one image's blocks of a chunk stay far below 2^31 / 16
        if constexpr (SHUF) {
          if (st_sh) off = gsel * (int)HW + (2 * (gy & 1) + (gx & 1)) * hw4 + (gy >> 1) * w2 + (gx >> 1);
        }
        const uintptr_t src = ok ? gb + 16 * (long long)off : zero_addr;
        SLU_GLDS16(reinterpret_cast<const uint4*>(src), st_db + blk * 64);
      }
    } else if constexpr (!WRES) {
      const int blk = (i - NIB) * NWAVE + st_wave;                      // = (m * KPC + j) * T + tap
      if (NBLK_A % NWAVE == 0 || blk < NBLK_A) {
        const int m = blk / TS, r = blk - m * TS;                         // r = j * T + tap: K-step j of the chunk
        const bool live = mblk0 + m < a.nmblk && (KPC == 1 || KPC * st_q + r / T < nks);
        const uint4* src = live ? a.wpack + (((size_t)(mblk0 + m) * nks + KPC * st_q) * T + r) * 64 + lane : reinterpret_cast<const uint4*>(zero_addr);
        SLU_GLDS16(src, st_da + blk * 64);
      }
    }
  };
  // the pieces that go with tap-step `tap` (compile-time indices once the tap loop is unrolled)
  auto stage_after_tap = [&](int tap) __attribute__((always_inline)) {
    if (st_on) {
#pragma unroll
      for (int k = 0; k < PPT; ++k)
        if (tap * PPT + k < NPIECE) stage_piece(tap * PPT + k);
    }
  };
  // per-channel multipliers of image n as fp16, one record per channel block (SCALED)
  auto stage_scales = [&](int n, int par) __attribute__((always_inline)) {
    if (tid < 64) {
      half8 h;
#pragma unroll
      for (int k = 0; k < 8; ++k) h[k] = (_Float16)1.0f;
      // table position -> block: plain, position g = block g of the concatenated input; with a shuffled source 0 of G0 contributed
      // blocks, positions [0, 4 G0) = its STORED blocks and position 3 G0 + g = block g >= G0 of the other sources
      int g = tid;
      bool stored0 = false;
      if constexpr (SHUF) {
        if (a.src[0].shuf) {
          stored0 = tid < 4 * a.src[0].G;
          g = stored0 ? 0 : tid - 3 * a.src[0].G;
        }
      }
      if (stored0) {
        if (a.src[0].scale) {
          h = h8_multipliers(a.src[0].scale + ((size_t)n * 4 * a.src[0].G + tid) * 8);
        }
      } else if (g < a.Gin) {
        int img[SLU_MAX_SRC] = {0, 0, 0};
        const SrcSel p = select_src(a, img, g);
        if (p.scale) {
          h = h8_multipliers(p.scale + ((size_t)n * p.G + p.gl) * 8);
        }
      }
      s_scale[par * 64 + tid] = __builtin_bit_cast(uint4, h);
    }
  };

  if constexpr (WRES) {      // all weight fragments of this channel-block group, once
    const int per_m = nks * T;
    for (int blk = wave; blk < MBLK * per_m; blk += NWAVE) {
      const int m = blk / per_m;
      const uint4* src = mblk0 + m < a.nmblk ? a.wpack + ((size_t)(mblk0 + m) * per_m + (blk - m * per_m)) * 64 + lane : &h8_zero_rec;
      SLU_GLDS16(src, s_a + blk * 64);
    }
  }
  TilePos cur = decode(t_beg), nxt = cur;
  stage_begin(cur, 0, 0);
#pragma unroll
  for (int i = 0; i < NPIECE; ++i) stage_piece(i);
  int buf = 0;
  constexpr bool SWAP16 = (OPT & 8) != 0;            // whole 16-byte records per lane on the way out
  constexpr int NST = MB * NB * (SWAP16 ? 2 : 4);    // stores of a tile's epilogue, per wave (h8 output: every lane stores)
  constexpr bool PRE = MB == 1 && !F32OUT;           // residual of the tile prefetched before its last MFMA phase
  const uint2* resid2 = reinterpret_cast<const uint2*>(resid);
  uint2 rv[PRE ? NB : 1][4];
  // the staging set-up of the chunk after (tile, q): the next chunk of this tile, or the first of the next tile
  auto setup_next = [&](int tile, int q) __attribute__((always_inline)) {
    st_on = false;
    if (q + 1 < nchunk) {
      stage_begin(cur, q + 1, buf ^ 1);
    } else if (tile + t_step < t_end) {
      nxt = advance(cur);
      stage_begin(nxt, 0, buf ^ 1);
    }
  };

#ifdef SLU_H8_PROF
  unsigned long long prof_acc[6] = {0, 0, 0, 0, 0, 0}, prof_t = __builtin_amdgcn_s_memtime();
#endif
  int tile_no = 0;
  for (int tile = t_beg; tile < t_end; tile += t_step, ++tile_no) {
    f32x16 acc[MB][NB];                                // per tile (not carried around the loop: keeps it in the MFMA registers)
    // written out: with h8_zero the fp32-output instantiation takes one VGPR more
#pragma unroll
    for (int i = 0; i < MB; ++i)
#pragma unroll
      for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][b][r] = 0.0f;
    const int spar = tile_no & 1;
    if constexpr (SCALED) stage_scales(cur.n, spar);
    for (int q = 0; q < nchunk; ++q) {
      // (OPT & 4) every piece of chunk (tile, q) was issued during the previous MFMA phase, so the staging state may move on to the
      // chunk after it while this wave waits for its DMA and for the other waves
      if constexpr ((OPT & 4) != 0) setup_next(tile, q);
      // Chunk (tile, q) has landed and nobody reads the other buffer any more.  vmcnt counts loads, LDS-DMA and stores in
      // issue order: at a tile's first chunk the only operations younger than the DMA we wait for are the NST stores of the
      // previous tile's epilogue, which may stay in flight (waiting for them would expose the HBM write latency per tile).
      if (!F32OUT && q == 0 && tile != t_beg) h8_vmcnt<(NST < 63 ? NST : 63)>();
      else h8_vmcnt<0>();
      h8_lgkmcnt0();
      H8_PROF_MARK(0)                                    // waiting for the chunk's DMA (and, at q = 0, the epilogue before it)
      h8_barrier();
      H8_PROF_MARK(1)                                    // barrier
      if constexpr ((OPT & 4) == 0) setup_next(tile, q);
      if constexpr (PRE) {
        if (resid && q == nchunk - 1) {
#pragma unroll
          for (int b = 0; b < NB; ++b) {
            const int gy = cur.y0 + wn * RPW + (b >> 1), gx = cur.x0 + (b & 1) * 32 + jj;
            const bool pix_ok = gy < a.H && gx < a.W;
            const size_t pix = (size_t)gy * a.W + gx;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              const int go = (mblk0 + wm) * 4 + k;
              rv[b][k] = *((pix_ok && go < a.Gout) ? resid2 + (((size_t)cur.n * a.Gout + go) * HW + pix) * 2 + hh
                                                   : reinterpret_cast<const uint2*>(zero_addr));
            }
          }
        }
      }
      H8_PROF_MARK(2)                                    // issuing the next chunk's DMA (+ residual prefetch)
      const uint4* sb = s_b + buf * NB_ALLOC + bbase;
      const uint4* sa = s_a + abase + (WRES ? q * T * 64 : buf * NREC_A);
      // scm[yr][xr]: the multiplier of the B fragment of accumulator block b at tap (dy, dx), yr = ((b >> 1) + dy) & 1, xr = dx & 1.  A plain
      // chunk has one record for all four; a shuffled one the stored block 4 g + 2 (row parity) + (column parity) of the pixel read: row
      // y0 + wn RPW + (b >> 1) + dy - 1 with y0 even, column x0 + 32 (b & 1) + jj + dx - 1 with x0 a multiple of 64
      half8 scm[SHUF ? 2 : 1][SHUF ? 2 : 1];
      if constexpr (SHUF) {
        const int g0s = a.src[0].shuf ? a.src[0].G : 0;
        if (2 * q < g0s) {
#pragma unroll
          for (int yr = 0; yr < 2; ++yr)
#pragma unroll
            for (int xr = 0; xr < 2; ++xr)
              scm[yr][xr] = __builtin_bit_cast(half8, s_scale[spar * 64 + 4 * (2 * q + hh) + 2 * ((yr + wn * RPW + 1) & 1) + ((jj + xr + 1) & 1)]);
        } else {
          scm[0][0] = __builtin_bit_cast(half8, s_scale[spar * 64 + 3 * g0s + 2 * q + hh]);
          scm[0][1] = scm[1][0] = scm[1][1] = scm[0][0];
        }
      } else if constexpr (SCALED) {
        scm[0][0] = __builtin_bit_cast(half8, s_scale[spar * 64 + 2 * q + hh]);
      }
      auto sc_of = [&](int b, int dy, int dx) __attribute__((always_inline)) -> half8 { return SHUF ? scm[((b >> 1) + dy) & 1][dx & 1] : scm[0][0]; };
      {
        if constexpr (MB == 2 && WM == 2 && WN == 4) {
          // the 8-wave 128-channel configuration (MFMA-bound layers): fragments of tap-step t+1 are read before the MFMAs of tap-step t
          // issue, in THIS order -- sched_barrier pins it; with sched_group_barrier hints (below) the compiler still emits read, wait,
          // MFMA, read, ... (+3 % on these layers; the other configurations spill with a second fragment set)
          half8 af[2][MB], bf[2][NB];
          auto read_frags = [&](int set, int ts) __attribute__((always_inline)) {
            const int j = ts / T, tap = ts % T;          // K-step of the chunk, tap
            const int dy = (tap / KS) * DIL, dx = (tap % KS) * DIL;
#pragma unroll
            for (int i = 0; i < MB; ++i) af[set][i] = __builtin_bit_cast(half8, sa[i * a_stride + ts * 64]);
#pragma unroll
            for (int b = 0; b < NB; ++b) {
              bf[set][b] = __builtin_bit_cast(half8, sb[j * 2 * REC + ((b >> 1) + dy) * LW + (b & 1) * 32 + dx]);
              if constexpr (SCALED) bf[set][b] *= sc_of(b, dy, dx);
            }
          };
          read_frags(0, 0);
#pragma unroll
          for (int ts = 0; ts < TS; ++ts) {
            if (ts + 1 < TS) read_frags((ts + 1) & 1, ts + 1);
            __builtin_amdgcn_sched_barrier(0);
            if constexpr ((OPT & 1) != 0) {
              if (late_half) stage_after_tap(ts);
              __builtin_amdgcn_sched_barrier(0);
            }
            if constexpr ((OPT & 2) != 0) __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int b = 0; b < NB; ++b)
#pragma unroll
              for (int i = 0; i < MB; ++i) acc[i][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[ts & 1][i], bf[ts & 1][b], acc[i][b], 0, 0, 0);
            if constexpr ((OPT & 2) != 0) __builtin_amdgcn_s_setprio(0);
            __builtin_amdgcn_sched_barrier(0);
            if constexpr ((OPT & 1) != 0) {
              if (!late_half) stage_after_tap(ts);
            } else {
              stage_after_tap(ts);
            }
          }
        } else if constexpr (MB == 1) {
          // fragments of tap t+1 are read from LDS while the MFMAs of tap t issue (two register sets, one DS read per MFMA
          // slot); with MB = 2 the second set does not fit in 256 VGPRs next to the 128 accumulator registers
          half8 af[2][MB], bf[2][NB];
          auto read_frags = [&](int set, int tap) __attribute__((always_inline)) {
            const int dy = (tap / KS) * DIL, dx = (tap % KS) * DIL;
#pragma unroll
            for (int i = 0; i < MB; ++i) af[set][i] = __builtin_bit_cast(half8, sa[i * a_stride + tap * 64]);
#pragma unroll
            for (int b = 0; b < NB; ++b) {
              bf[set][b] = __builtin_bit_cast(half8, sb[((b >> 1) + dy) * LW + (b & 1) * 32 + dx]);
              if constexpr (SCALED) bf[set][b] *= sc_of(b, dy, dx);
            }
          };
          read_frags(0, 0);
#pragma unroll
          for (int tap = 0; tap < T; ++tap) {
            if (tap + 1 < T) read_frags((tap + 1) & 1, tap + 1);
#pragma unroll
            for (int b = 0; b < NB; ++b)
#pragma unroll
              for (int i = 0; i < MB; ++i) acc[i][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[tap & 1][i], bf[tap & 1][b], acc[i][b], 0, 0, 0);
            if (tap + 1 < T) {
#pragma unroll
              for (int k = 0; k < MB * NB; ++k) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, (MB + NB + MB * NB - 1) / (MB * NB), 0);
              }
            }
            stage_after_tap(tap);
          }
        } else {
#pragma unroll
          for (int tap = 0; tap < T; ++tap) {
            const int dy = (tap / KS) * DIL, dx = (tap % KS) * DIL;
            half8 af[MB];
#pragma unroll
            for (int i = 0; i < MB; ++i) af[i] = __builtin_bit_cast(half8, sa[i * a_stride + tap * 64]);
#pragma unroll
            for (int b = 0; b < NB; ++b) {
              half8 bf = __builtin_bit_cast(half8, sb[((b >> 1) + dy) * LW + (b & 1) * 32 + dx]);
              if constexpr (SCALED) bf *= sc_of(b, dy, dx);
#pragma unroll
              for (int i = 0; i < MB; ++i) acc[i][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[i], bf, acc[i][b], 0, 0, 0);
            }
            // ask for an MFMA / LDS-read interleave: each tap's fragment reads are spread between the previous tap's MFMAs
#pragma unroll
            for (int k = 0; k < MB * NB; ++k) {
              __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
              __builtin_amdgcn_sched_group_barrier(0x100, (MB + NB + MB * NB - 1) / (MB * NB), 0);
            }
            stage_after_tap(tap);
          }
        }
      }
      buf ^= 1;
      H8_PROF_MARK(3)                                    // LDS reads + MFMAs of the chunk
    }
    {
#pragma unroll
      for (int i = 0; i < MB; ++i) {
        const int ml = wm * MB + i;
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          const int gy = cur.y0 + wn * RPW + (b >> 1), gx = cur.x0 + (b & 1) * 32 + jj;
          const bool pix_ok = gy < a.H && gx < a.W;
          const size_t pix = pix_ok ? (size_t)gy * a.W + gx : 0;
          if constexpr (F32OUT)
            store_tile<MBLK * 32>(a, acc[i][b], s_epi, ml * 32, (mblk0 + ml) * 32, hh, pix_ok, (size_t)cur.n, pix, HW, resid, out, slope_pre);
          else if constexpr (SWAP16 && LATE)
            store_tile_swap16<MBLK * 32, true>(a, acc[i][b], s_epi, ml * 32, (mblk0 + ml) * 4, hh, pix_ok, (size_t)cur.n, pix, HW, resid2,
                                               reinterpret_cast<uint4*>(out), slope_pre, zero_addr, trash_addr, slope_act);
          else if constexpr (LATE)
            store_tile_full<MBLK * 32, PRE, true>(a, acc[i][b], s_epi, ml * 32, (mblk0 + ml) * 4, hh, pix_ok, (size_t)cur.n, pix, HW, resid2,
                                                  rv[PRE ? b : 0], reinterpret_cast<uint2*>(out), slope_pre, zero_addr, trash_addr, slope_act);
          else if constexpr (SWAP16)
            store_tile_swap16<MBLK * 32>(a, acc[i][b], s_epi, ml * 32, (mblk0 + ml) * 4, hh, pix_ok, (size_t)cur.n, pix, HW, resid2,
                                         reinterpret_cast<uint4*>(out), slope_pre, zero_addr, trash_addr);
          else
            store_tile_full<MBLK * 32, PRE>(a, acc[i][b], s_epi, ml * 32, (mblk0 + ml) * 4, hh, pix_ok, (size_t)cur.n, pix, HW, resid2,
                                            rv[PRE ? b : 0], reinterpret_cast<uint2*>(out), slope_pre, zero_addr, trash_addr);
          __builtin_amdgcn_sched_barrier(0);     // one accumulator tile at a time (register pressure)
        }
      }
    }
    H8_PROF_MARK(4)                                      // epilogue
    cur = nxt;
  }
#ifdef SLU_H8_PROF
  if (tid == 0) {
    for (int i = 0; i < 5; ++i) atomicAdd(&g_h8_prof[i], prof_acc[i]);
    atomicAdd(&g_h8_prof[5], 1ull);
  }
#endif
}
