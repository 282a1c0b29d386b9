// h8 convs, the 1x1 GEMM ring (gemm1x1_h8_kernel and its A/B form gemm1x1_h8_kernel_v1): the wide 1x1 convs with 256 output channels and the
// 384 -> 128 concat convs with a residual.  The map of the families is in conv2d_h8.hip.
#include "conv_h8.h"

using namespace slu_h8;

namespace {

// gemm1x1_h8_kernel's form of the same epilogue.  Every lane of every tile is live there (H W % 256 == 0, Cout = 64 MB), so there is no trash
// record and the address keeps its address space: global_store_dwordx4 at `obase` (wave-uniform: the tile's first record of the accumulator
// tile's first block) plus the lane's 32-bit byte offset `vo` (half hh, pixel), record 2 pr + hh; pr = 0 / 1 are `plane2` bytes (two planes of
// H W records) apart, added on the scalar side.  RES: res[pr] is the residual's record 2 pr + hh, loaded whole by the caller (the same offsets
// from the residual's base) and retired by a counted wait before the call; h8_swap16 gives the lane back its halves of records 2 pr and 2 pr + 1.  Same arithmetic, in the same order, as
// store_tile_swap16: h8_epilogue, h8_add_resid, pack2, swap.
template <int STRIDE, bool RES>
__device__ __forceinline__ void gemm_store_tile(const f32x16& acc, const float* se, int cl0, int hh, const u32x4v (&res)[2], char* obase, unsigned vo,
                                                unsigned plane2, float slope_pre) {
  const float4* se4 = reinterpret_cast<const float4*>(se);
  const float2v sl = {slope_pre, slope_pre};
#pragma unroll
  for (int pr = 0; pr < 2; ++pr) {
    uint4 rw = make_uint4(0u, 0u, 0u, 0u);       // residual words: x, y for q = 2 pr; z, w for q = 2 pr + 1
    if constexpr (RES) rw = h8_swap16(res[pr].x, res[pr].y, res[pr].z, res[pr].w);
    unsigned hw[4];
#pragma unroll
    for (int q2 = 0; q2 < 2; ++q2) {
      const int q = 2 * pr + q2;
      const int c4 = (cl0 + 8 * q) / 4 + hh;
      H8Quad t = h8_epilogue(acc, q, se4[c4], se4[STRIDE / 4 + c4], se4[2 * STRIDE / 4 + c4], sl);
      if constexpr (RES) h8_add_resid(t, q2 ? make_uint2(rw.z, rw.w) : make_uint2(rw.x, rw.y));
      hw[2 * q2] = pack2(t.t0);
      hw[2 * q2 + 1] = pack2(t.t1);
    }
    *reinterpret_cast<uint4*>(obase + (size_t)pr * plane2 + vo) = h8_swap16(hw[0], hw[1], hw[2], hw[3]);
  }
}

// -----------------------------------------------------------------------------------------------------------
// Wide 1x1 convs with 256 output channels (768 -> 256 concat convs and the 128 / 256 -> 256 shortcuts of the U-Net's lower levels) as a plain
// GEMM, out[Cout][pixels] = W[Cout][Cin] x[Cin][pixels]: BOTH operands go global -> LDS by global_load_lds into a ring of D chunks of KC K-steps,
// D - 1 in flight, issued as one burst behind the barrier that frees the slot; one barrier per chunk; every wave issues the same number of DMAs
// at every position (beyond the end: the zero record), so "chunk c has landed" is the constant vmcnt((D - 2) NPIECE).  A workgroup of 8 waves
// (2 along the channels x 4 along the pixels) owns 256 consecutive pixels of one image plane and all channels: the weights stream once per 256
// pixels (the streaming conv1x1_h8_kernel re-reads them per 128 and stages them through registers + two barriers per 64 channels).
// Measured (N = 64, tools/h8_1x1_bench.py, profiles/r10; streaming kernel -> this one): 768 -> 256 + residual at 16x512 502 -> 372 us, at 8x256
// 131 -> 90, 128 -> 256 at 16x512 118 -> 89, 256 -> 256 at 8x256 46 -> 37; the 128-output instantiation <2, 4, 3> 543 -> 478 us on 384 -> 128 +
// residual at 32x1024 (149 -> 137 at 16x512) and is dispatched for exactly those layers (gemm1x1_ok).  With the epilogue before r10 (below) the
// 768 -> 256 layer took 449 us and the 128-output form 618: its residual cost 159 of the 449 us, now 86 of 372.  What the r03 ablation
// switches (SLU_GEMM_DBG in -DSLU_H8_AB builds) showed on 768 -> 256: no input DMA 399 us, no weight DMA 413, no MFMA 354, none of the three STILL 306 of
// 481 -- the time is in the per-chunk skeleton (32 DMA instructions per CU and chunk, barrier, fragment reads) and the epilogue, not in HBM,
// L2 or the matrix cores; a deeper ring of smaller chunks (KC 2, D 4) was slower (484) than two 64-channel chunks (459).
// The residual (AHEAD, the default).  The 768 -> 256 layers all carry one.  It is loaded in whole 16-byte records (lane (jj, hh): record
// 2 pr + hh of each accumulator tile, un-swapped by h8_swap16 before the add) by inline-asm global_load_dwordx4 the compiler does not
// track, so it places no wait of its own: the records of the first two M-blocks (8 loads, 32 registers) are issued behind the barrier of the
// tile's LAST chunk, BEFORE that chunk's stage_next(), and retired at the top of the epilogue by vmcnt(NPIECE) -- vmcnt retires in issue order,
// and the only younger operations are the NPIECE DMAs of that stage_next(), the next tile's burst, which stays in flight.  With MB = 4 the
// records of M-blocks 2, 3 are issued at the top of the epilogue, into the registers the fragments have left, and retired by vmcnt(8) behind
// the 8 stores of M-blocks 0, 1 (which retires the burst too: it has had the last chunk's MFMA phase and half an epilogue to land).  Every
// wave issues the same vector-memory operations at every tile, and all of them are global_*: nothing counts in lgkmcnt but LDS reads.
// The chunk wait vmcnt((D - 2) NPIECE) assumes that only DMA pieces are younger than the chunk it waits for; residual loads and stores issued
// in between make it stricter (the chunk is then older than the (D - 2) NPIECE youngest operations by more), never wrong.  With D = 2 it is a
// full wait anyway.
// The form before that (AHEAD = false, SLU_GEMM1X1_RES_AHEAD=0, kept for A/B runs and the bit-equality test: gemm1x1_h8_kernel_v1) is
// store_tile_swap16: 4 FLAT 8-byte loads per accumulator tile, each followed by the compiler's vmcnt(0) lgkmcnt(0) -- 32 serial round trips per
// wave and tile in <4, 4, 2>, each draining the next tile's burst and the stores just issued, with all eight waves in the epilogue together.
// Needs: Cout = 64 MB, H W % 256 == 0 (so every lane of every tile is live), nks % KC == 0, every source a whole number of chunks, no
// multipliers / batch broadcast, 16 Gout H W < 2^32 (the lane's byte offset inside one image of the output is 32-bit).
// -----------------------------------------------------------------------------------------------------------
template <int MB, int KC, int D, bool AHEAD, bool RES>
__device__ __forceinline__ void gemm1x1_h8_body(const H8Args& a, const void* __restrict__ resid, void* __restrict__ out) {
  constexpr int NWAVE = 8, MBLK = 2 * MB, TP = 256, NB = 2;
  constexpr int NREC_A = MBLK * KC * 64, NREC_B = 2 * KC * TP;           // records per chunk: weight fragments, input tile [2 KC blocks][256 px]
  constexpr int NPA = MBLK * KC, NPB = 2 * KC * 4;                       // 64-record pieces
  constexpr int NIA = (NPA + NWAVE - 1) / NWAVE, NIB = NPB / NWAVE;
  constexpr int NPIECE = NIA + NIB;
  static_assert(NPB % NWAVE == 0 && NPA % NWAVE == 0 && D >= 2 && (D - 2) * NPIECE <= 63, "pieces divide over the waves; vmcnt is 6 bits");

  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* s_epi = reinterpret_cast<float*>(smem);                         // bias | bn_a | bn_b
  uint4* s_b = reinterpret_cast<uint4*>(s_epi + 3 * MBLK * 32);          // [D][NREC_B]
  uint4* s_a = s_b + D * NREC_B;                                         // [D][MBLK][KC][64]

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3, hh = lane >> 5, jj = lane & 31;
  const size_t HW = (size_t)a.H * a.W;
  const int tiles_per_img = (int)(HW / TP);
  const int ntiles = tiles_per_img * a.N, nch = a.nks / KC;
  const int t_step = gridDim.x, t_beg = (int)blockIdx.x;
  if (t_beg >= ntiles) return;

  if (tid < MBLK * 32) {
    const bool ok = tid < a.Cout;
    H8_FILL_EPI(s_epi, 0, MBLK * 32, tid, ok, tid, a.bias, a.bn_a, a.bn_b);
  }
  H8_OPAQUE_ADDR(zero_addr, h8_zero_rec);
  H8_OPAQUE_ADDR(trash_addr, h8_trash_rec);

  // the staging cursor runs D - 1 chunks ahead of the compute cursor: (s_tile, s_q) = the next chunk to copy, into ring slot s_slot
  int s_tile = t_beg, s_q = 0, s_slot = 0;
  auto stage_next = [&]() __attribute__((always_inline)) {
    const bool valid = s_tile < ntiles;
    int wv = wave;
    asm volatile("" : "+s"(wv));                                        // (keeps the per-piece address arithmetic out of the loop-invariant set)
    uintptr_t base = zero_addr;
    if (valid) {
      const int n = s_tile / tiles_per_img, p0 = (s_tile - n * tiles_per_img) * TP;
      const int g = 2 * KC * s_q;                                        // first channel block of the chunk: one source holds the whole chunk
      const uint4* ptr = a.src[0].ptr;
      int G = a.src[0].G, gl = g;
#pragma unroll
      for (int s = 1; s < SLU_MAX_SRC; ++s)
        if (s < a.nsrc && g >= a.src[s].gbeg) ptr = a.src[s].ptr, G = a.src[s].G, gl = g - a.src[s].gbeg;
      base = reinterpret_cast<uintptr_t>(ptr) + 16 * (((size_t)n * G + gl) * HW + p0);
    }
    uint4* db = s_b + s_slot * NREC_B;
    uint4* da = s_a + s_slot * NREC_A;
#pragma unroll
    for (int i = 0; i < NIB; ++i) {
      const int p = i * NWAVE + wv;                                      // block = p / 4, pixel quarter = p % 4
      const uintptr_t src = (valid && !SLU_ABLATE(a, 1)) ? base + 16 * ((size_t)(p >> 2) * HW + (size_t)((p & 3) * 64 + lane)) : zero_addr;
      SLU_GLDS16(reinterpret_cast<const uint4*>(src), db + p * 64);
    }
#pragma unroll
    for (int i = 0; i < NIA; ++i) {
      const int p = i * NWAVE + wv;                                      // = m * KC + ks
      const int m = p / KC, ks = p - m * KC;
      const uint4* src = (valid && !SLU_ABLATE(a, 2)) ? a.wpack + ((size_t)m * a.nks + KC * s_q + ks) * 64 + lane : reinterpret_cast<const uint4*>(zero_addr);
      SLU_GLDS16(src, da + p * 64);
    }
    asm volatile("" ::: "memory");
    s_slot = s_slot + 1 == D ? 0 : s_slot + 1;
    if (++s_q == nch) s_q = 0, s_tile += t_step;
  };
#pragma unroll
  for (int c = 0; c < D - 1; ++c) stage_next();

  int r_slot = 0;
  const float slope_pre = (a.has_act & 3) == 1 ? a.slope : 1.0f;
  [[maybe_unused]] const uint2* resid2 = reinterpret_cast<const uint2*>(resid);
  const int abase = (wm * MB) * KC * 64 + lane;
  const int bbase = hh * TP + wn * 64 + jj;

  // AHEAD: byte offset of the lane's record (block hh, pixel of accumulator column b) from the tile's first record of block 0, the same in the
  // residual and in the output; the wave's M-block i and pair pr add (4 (wm MB + i) + 2 pr) planes to the scalar base, which keeps the sixteen
  // offsets of a tile out of the vector registers.  Two sets of 8 residual records: M-blocks 0, 1 / 2, 3.
  static_assert(!AHEAD || MB == 2 || MB == 4, "the residual waits name 8 registers per set");
  const unsigned plane = (unsigned)(HW * 16);
  unsigned voff[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) voff[b] = (unsigned)(hh * HW * 16) + (unsigned)((wn * 64 + b * 32 + jj) * 16);
  unsigned long long rbase = 0;
  auto load_resid = [&](u32x4v (&r)[2][NB][2], int i0) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int pr = 0; pr < 2; ++pr) {
          const unsigned long long base = rbase + (unsigned long long)((wm * MB + i0 + i) * 4 + 2 * pr) * plane;
          asm volatile("global_load_dwordx4 %0, %1, %2" : "=&v"(r[i][b][pr]) : "v"(voff[b]), "s"(base) : "memory");
        }
  };

  for (int tile = t_beg; tile < ntiles; tile += t_step) {
    f32x16 acc[MB][NB];
    h8_zero(acc);
    u32x4v ra[2][NB][2], rb[2][NB][2];
    const int n = tile / tiles_per_img, p0 = (tile - n * tiles_per_img) * TP;
    const size_t tile16 = 16 * ((size_t)n * a.Gout * HW + p0);        // the tile's first record of block 0, in bytes
    if constexpr (AHEAD) rbase = reinterpret_cast<unsigned long long>(resid) + tile16;
    for (int q = 0; q < nch; ++q) {
      // the oldest chunk in flight has landed once at most the (D - 2) younger chunks' pieces are outstanding (residual loads and stores of an
      // epilogue in between only make the wait stricter); then every wave is past its reads of the slot that is re-filled next
      h8_chunk_landed<(D - 2) * NPIECE>();
      if constexpr (AHEAD && RES)
        if (q == nch - 1) load_resid(ra, 0);      // older than the burst below: vmcnt(NPIECE) retires them and not the burst
      stage_next();
      const uint4* sb = s_b + r_slot * NREC_B + bbase;
      const uint4* sa = s_a + r_slot * NREC_A + abase;
      r_slot = r_slot + 1 == D ? 0 : r_slot + 1;
      half8 af[2][MB], bf[2][NB];
      auto read_frags = [&](int set, int ks) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < MB; ++i) af[set][i] = __builtin_bit_cast(half8, sa[(i * KC + ks) * 64]);
#pragma unroll
        for (int b = 0; b < NB; ++b) bf[set][b] = __builtin_bit_cast(half8, sb[2 * ks * TP + b * 32]);
      };
      read_frags(0, 0);
#pragma unroll
      for (int ks = 0; ks < KC; ++ks) {
        if (ks + 1 < KC) read_frags((ks + 1) & 1, ks + 1);
        __builtin_amdgcn_sched_barrier(0);
        if (!SLU_ABLATE(a, 4)) {
#pragma unroll
          for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int i = 0; i < MB; ++i) acc[i][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[ks & 1][i], bf[ks & 1][b], acc[i][b], 0, 0, 0);
        } else {
#pragma unroll
          for (int i = 0; i < MB; ++i) asm volatile("" ::"v"(af[ks & 1][i]));
#pragma unroll
          for (int b = 0; b < NB; ++b) asm volatile("" ::"v"(bf[ks & 1][b]));
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    if constexpr (AHEAD) {
      char* obase = reinterpret_cast<char*>(out) + tile16;
      {
        auto blocks = [&](const u32x4v (&r)[2][NB][2], int i0) __attribute__((always_inline)) {
#pragma unroll
          for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int b = 0; b < NB; ++b) {
              gemm_store_tile<MBLK * 32, RES>(acc[i0 + i][b], s_epi, (wm * MB + i0 + i) * 32, hh, r[i][b], obase + (size_t)((wm * MB + i0 + i) * 4) * plane,
                                              voff[b], 2 * plane, slope_pre);
              __builtin_amdgcn_sched_barrier(0);
            }
        };
        // M-blocks 0, 1: their records were issued before the last chunk's stage_next(), whose NPIECE DMAs are all that is younger
        if constexpr (RES)
          asm volatile("s_waitcnt vmcnt(%8)"
                       : "+v"(ra[0][0][0]), "+v"(ra[0][0][1]), "+v"(ra[0][1][0]), "+v"(ra[0][1][1]), "+v"(ra[1][0][0]), "+v"(ra[1][0][1]),
                         "+v"(ra[1][1][0]), "+v"(ra[1][1][1])
                       : "n"(NPIECE));
        if constexpr (RES && MB == 4) load_resid(rb, 2);
        blocks(ra, 0);
        if constexpr (MB == 4) {
          // M-blocks 2, 3: younger than their records are the 2 NB 2 stores above
          if constexpr (RES)
            asm volatile("s_waitcnt vmcnt(%8)"
                         : "+v"(rb[0][0][0]), "+v"(rb[0][0][1]), "+v"(rb[0][1][0]), "+v"(rb[0][1][1]), "+v"(rb[1][0][0]), "+v"(rb[1][0][1]),
                           "+v"(rb[1][1][0]), "+v"(rb[1][1][1])
                         : "n"(2 * NB * 2));
          blocks(rb, 2);
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < MB; ++i) {
        const int ml = wm * MB + i;
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          const size_t pix = (size_t)p0 + wn * 64 + b * 32 + jj;
          store_tile_swap16<MBLK * 32>(a, acc[i][b], s_epi, ml * 32, ml * 4, hh, true, (size_t)n, pix, HW, resid2, reinterpret_cast<uint4*>(out), slope_pre,
                                       zero_addr, trash_addr);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // zero-record DMAs issued beyond the last chunk: LDS must not be released under them
}

template <int MB, int KC, int D>
__global__ __launch_bounds__(512, 2) void gemm1x1_h8_kernel(const H8Args a, const void* __restrict__ resid, void* __restrict__ out) {
  // with and without a residual: two whole tile loops (one uniform branch per launch, and the registers of the residual records stay out of
  // the loop that has none)
  if (resid) gemm1x1_h8_body<MB, KC, D, true, true>(a, resid, out);
  else gemm1x1_h8_body<MB, KC, D, true, false>(a, resid, out);
}
// the epilogue before the residual was loaded ahead (SLU_GEMM1X1_RES_AHEAD=0)
template <int MB, int KC, int D>
__global__ __launch_bounds__(512, 2) void gemm1x1_h8_kernel_v1(const H8Args a, const void* __restrict__ resid, void* __restrict__ out) {
  gemm1x1_h8_body<MB, KC, D, false, false>(a, resid, out);      // (RES is not read: store_tile_swap16 tests `resid` per tile)
}

// the layers gemm1x1_h8_kernel covers; SLU_H8_GEMM1X1=0 is the A/B switch back to the streaming kernels
constexpr int GEMM1X1_KC = 4, GEMM1X1_D256 = 2, GEMM1X1_D128 = 3;      // chunk = 64 channels; ring: 2 x 64 KB (256 outputs), 3 x 48 KB (128)
bool gemm1x1_ok(const slu_conv_h8_desc* d, const H8Args& a) {
  // 256 output channels: measured (tools/h8_1x1_bench.py, N = 64, profiles/r10) 502 -> 372 us against the streaming kernel on 768->256 at 16x512.
  // 128 outputs: only the 384 -> 128 concat convs that carry a residual (three sources, 24 K-steps): 543 -> 478 us at 32x1024 and 149 -> 137 at
  // 16x512 since the residual is loaded ahead (with the epilogue before that the GEMM was the slower one, 618 us); the other 128-output
  // layers stay on the streaming kernel, and SLU_H8_GEMM1X1=2 sends every 128-output layer within reach here (tests, A/B runs)
  static const int mode = slu_env_int("SLU_H8_GEMM1X1", 1);
  const bool off = mode == 0, all = mode == 2;
  const bool concat128 = a.Cout == 128 && d->resid && a.nsrc == 3 && a.nks == 24;
  if (off || d->ksize != 1 || d->pad != 0 || a.out_f32 || (a.Cout != 256 && !(a.Cout == 128 && (all || concat128)))) return false;
  if (((long long)a.H * a.W) % 256 || a.nks % GEMM1X1_KC || a.Gin != 2 * a.nks) return false;
  if ((a.has_act & ~1) || ((a.has_act & 1) && !(a.slope >= 0.0f && a.slope <= 1.0f))) return false;
  for (int s = 0; s < a.nsrc; ++s)
    if (a.src[s].scale || a.src[s].nb || a.src[s].G % (2 * GEMM1X1_KC)) return false;
  if (16LL * a.Gout * a.H * a.W > 0xffffffffLL) return false;      // a lane's byte offset inside one image of the output / residual is 32-bit
  return (long long)a.N * a.H * a.W / 256 <= 0x7fffffffLL;
}

template <int MB, int D>
int launch_gemm1x1(H8Args& a, const slu_conv_h8_desc* d, const SluEmit& e) {
  constexpr int KC = GEMM1X1_KC, MBLK = 2 * MB;
  constexpr size_t lds = (size_t)3 * MBLK * 32 * 4 + (size_t)D * (2 * KC * 256) * 16 + (size_t)D * (MBLK * KC * 64) * 16;
  static_assert(lds <= 160 * 1024, "gemm1x1 LDS");
  const long long nt = (long long)a.N * a.H * a.W / 256;
  const long long gx = nt < 256 ? nt : 256;
  // A/B switch: SLU_GEMM1X1_RES_AHEAD=0 is the epilogue that loads the residual where it is used (gemm1x1_h8_kernel_v1)
  static const bool v1 = slu_env_int("SLU_GEMM1X1_RES_AHEAD", 1) == 0;
  if (e.name) return slu_emit_name(e, v1 ? "gemm1x1_h8_kernel_v1<%d, %d, %d>" : "gemm1x1_h8_kernel<%d, %d, %d>", MB, KC, D);
  static SluLdsGrant grant, grant_v1;
  if (v1) return slu_launch_lds(gemm1x1_h8_kernel_v1<MB, KC, D>, dim3((unsigned)gx), dim3(512), lds, e.st, grant_v1, a, d->resid, d->out);
  return slu_launch_lds(gemm1x1_h8_kernel<MB, KC, D>, dim3((unsigned)gx), dim3(512), lds, e.st, grant, a, d->resid, d->out);
}

}  // namespace

int slu_h8::h8_gemm1x1(H8Args& a, const slu_conv_h8_desc* d, const SluEmit& e) {
  if (!gemm1x1_ok(d, a)) return -1;
  return a.Cout == 128 ? launch_gemm1x1<2, GEMM1X1_D128>(a, d, e) : launch_gemm1x1<4, GEMM1X1_D256>(a, d, e);
}
