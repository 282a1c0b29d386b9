// h8 convs, the tiled family (conv_h8_kernel, conv_h8_late_kernel: conv_h8_tiled_kernel.h): every 3x3 / dilated / 2x2 layer and every 1x1 the
// other families leave, in the tile configuration choose_h8 picks.  The map of the families is in conv2d_h8.hip.
#include "conv_h8.h"

// scheduling options of the 8-wave 128-channel configuration (conv_h8_kernel's OPT), as measured with tools/h8_ab.py (one process,
// interleaved rounds, N = 64, single-source form): 15 is +1 ... +3 % on the 3x3 layers and +3 ... +7 % on the 2x2-dilated ones; two K-steps
// per barrier paid (+6 ... +8 %) only while the per-chunk set-up was expensive and costs 2 ... 4 % since it is one scalar multiply-add
#ifndef H8_M128_OPT_3X3
#define H8_M128_OPT_3X3 15
#endif
#ifndef H8_M128_OPT_2X2
#define H8_M128_OPT_2X2 15
#endif
#ifndef H8_M128_KPC2_DEFAULT
#define H8_M128_KPC2_DEFAULT 0      // 2x2-dilated 128 / 256-channel layers: two K-steps per barrier (kept as an A/B switch, SLU_H8_KPC2=1)
#endif

using namespace slu_h8;

namespace {

#ifdef SLU_H8_PROF      // development aid: per-phase shader-clock totals of wave 0 of every workgroup of the tiled kernel
__device__ unsigned long long g_h8_prof[8];
#define H8_PROF_MARK(i)                                         \
  {                                                             \
    const unsigned long long t_now = __builtin_amdgcn_s_memtime(); \
    asm volatile("" ::: "memory");                              \
    prof_acc[i] += t_now - prof_t;                              \
    prof_t = t_now;                                             \
  }
#else
#define H8_PROF_MARK(i)
#endif

// -----------------------------------------------------------------------------------------------------------
// Tiled kernel, persistent, LDS-DMA staged.  Workgroup = WM x WN waves; output tile = TH rows x 64 columns x
// (32 WM MB) channels.  Tiles are dealt to the resident workgroups round-robin (tile = w + i * #workgroups, the 32
// workgroups of an XCD side by side along the azimuth), so at any moment the chip works on one compact band of the
// image: neighbouring halos meet in L2 and DRAM sees long contiguous rows.  The unit of staging is a chunk = one
// K-step (16 channels): the input tile (2 channel blocks, halo included) and the weight fragments are copied
// global -> LDS by global_load_lds (no staging registers), into the buffer the previous chunk is not using, piece
// by piece BETWEEN the taps of the current chunk's MFMA phase; the chunk after a tile's last one is the first
// chunk of the NEXT tile, so loads stay in flight across the epilogue.
// One barrier per chunk.  WRES: the weight fragments of ALL K-steps stay in LDS for the whole kernel (small
// layers).  SCALED: per-(image, channel) multipliers (Dropout2d on a concatenated input) are applied to the B
// fragments after the LDS read.
// -----------------------------------------------------------------------------------------------------------
// KPC: K-steps (16 channels each) per chunk = per barrier (2 for the 2x2-dilated 128-channel layers, whose 4 taps per K-step are too
// little MFMA work per barrier).  OPT (bit mask, the 8-wave 128-channel configuration): 1 = waves 4..7 (the SIMD partners of waves
// 0..3) issue a tap's LDS-DMA pieces BEFORE its MFMAs, waves 0..3 after them, so the two waves of a SIMD stop stalling on the
// address pipe at the same moment; 2 = s_setprio 1 around the MFMA cluster; 4 = the next chunk's staging set-up runs before the
// wait + barrier instead of after; 8 = whole 16-byte records per lane on the way out (v_permlane32_swap).
// ONE: the layer has ONE plain source (no concatenation, no batch broadcast): the staging set-up of a chunk is one 64-bit multiply-add on
// the scalar unit instead of the source-selection chains of the general form.
// waves per SIMD the registers allow: the kernel's __launch_bounds__ and launch_h8_k's persistent grid
constexpr int h8_waves_per_simd(int mb, int nwave, int rpw) { return (mb * rpw >= 8) ? 1 : ((nwave >= 8 || mb >= 2 || rpw >= 2) ? 2 : 3); }

// The kernel's text is conv_h8_tiled_kernel.h, compiled into two symbols.  conv_h8_late_kernel: the 3x3 / dil 1 / pad 1 layer with the activation
// AFTER the residual add, out = leaky(conv + bias + resid) -- the second conv of a ResNet BasicBlock (BatchNorm folded into weight and bias,
// ReLU = slope 0); same template parameters, tile walk, staging and counted waits, no SCALED / fp32-output / multi-K-step forms.
#define H8_TILED_KERNEL conv_h8_kernel
#define H8_TILED_LATE false
#include "conv_h8_tiled_kernel.h"
#undef H8_TILED_KERNEL
#undef H8_TILED_LATE
#define H8_TILED_KERNEL conv_h8_late_kernel
#define H8_TILED_LATE true
#include "conv_h8_tiled_kernel.h"
#undef H8_TILED_KERNEL
#undef H8_TILED_LATE

template <int KS, int DIL, int PAD, int MB, int WM, int WN, int RPW, bool SCALED, bool WRES, bool F32OUT = false, int KPC = 1, int OPT = 0, bool ONE = false,
          bool LATE = false>
int launch_h8_k(H8Args& a, const slu_conv_h8_desc* d, const SluEmit& e) {
  constexpr int TH = WN * RPW, MBLK = WM * MB, T = KS * KS, NWAVE = WM * WN;
  constexpr size_t nb_alloc = (size_t)((KPC * 2 * (TH + 2 * PAD) * (64 + 2 * PAD) + 63) / 64) * 64;
  const size_t lds = (size_t)3 * MBLK * 32 * 4 + (SCALED ? 2048 : 0) + 2 * nb_alloc * 16 + (size_t)MBLK * (WRES ? a.nks : 2 * KPC) * T * 64 * 16;
  if (lds > 160 * 1024) return SLU_EUNSUPPORTED;
  if (SCALED && a.Gin > 64) return SLU_EUNSUPPORTED;
  if (a.src[0].shuf) {      // a source read through PixelShuffle in place: the SCALED 3x3 kernels only; one table record per stored block of it
    if (!(SCALED && KS == 3 && DIL == 1 && PAD == 1 && !ONE && KPC == 1 && !F32OUT)) return SLU_EUNSUPPORTED;
    if (3 * a.src[0].G + a.Gin > 64) return SLU_EUNSUPPORTED;
  }
  a.tiles_x = (a.W + 63) / 64;
  a.tiles_y = (a.H + TH - 1) / TH;
  static const int order = slu_env_int("SLU_H8_ORDER", 1);      // 0 is kept for A/B runs
  a.order = order;
  const long long nt = (long long)a.tiles_x * a.tiles_y * a.N;
  const int gy = (a.nmblk + MBLK - 1) / MBLK;
  if (nt <= 0 || nt > 0x7fffffffLL || gy > 65535) return SLU_EUNSUPPORTED;
  if (e.name) {
    return slu_emit_name(e, LATE ? "conv_h8_late_kernel<%d, %d, %d, %d, %d, %d, %d, %s, %s, %s, %d, %d, %s>"
                                 : "conv_h8_kernel<%d, %d, %d, %d, %d, %d, %d, %s, %s, %s, %d, %d, %s>",
                         KS, DIL, PAD, MB, WM, WN, RPW, slu_tf(SCALED), slu_tf(WRES), slu_tf(F32OUT), KPC, OPT, slu_tf(ONE));
  }
  // persistent grid: as many workgroups as fit on the 256 CUs at once (registers / LDS), never more than tiles
  long long per_cu = h8_waves_per_simd(MB, NWAVE, RPW) * 4 / NWAVE;
  const long long by_lds = (long long)(160 * 1024 / lds);
  if (by_lds < per_cu) per_cu = by_lds;
  if (per_cu < 1) per_cu = 1;
  long long gx = (256 * per_cu + gy - 1) / gy;
  if (gx < 8) gx = 8;
  if (gx > nt) gx = nt;
  static SluLdsGrant grant;
  if constexpr (LATE)
    return slu_launch_lds(conv_h8_late_kernel<KS, DIL, PAD, MB, WM, WN, RPW, SCALED, WRES, F32OUT, KPC, OPT, ONE>, dim3((unsigned)gx, (unsigned)gy),
                          dim3(64 * NWAVE), lds, e.st, grant, a, d->resid, d->out);
  else
    return slu_launch_lds(conv_h8_kernel<KS, DIL, PAD, MB, WM, WN, RPW, SCALED, WRES, F32OUT, KPC, OPT, ONE>, dim3((unsigned)gx, (unsigned)gy),
                          dim3(64 * NWAVE), lds, e.st, grant, a, d->resid, d->out);
}

constexpr size_t WRES_MAX_BYTES = 24 * 1024;

// weights of all K-steps stay resident in LDS when they are small (full-resolution 32-channel layers)
template <int KS, int DIL, int PAD, int MB, int WM, int WN, int RPW, bool SCALED>
int launch_h8(H8Args& a, const slu_conv_h8_desc* d, const SluEmit& e) {
  const size_t wbytes = (size_t)WM * MB * a.nks * KS * KS * 64 * 16;
  if (wbytes <= WRES_MAX_BYTES) return launch_h8_k<KS, DIL, PAD, MB, WM, WN, RPW, SCALED, true>(a, d, e);
  return launch_h8_k<KS, DIL, PAD, MB, WM, WN, RPW, SCALED, false>(a, d, e);
}

inline long long wg_count(const H8Args& a, int th, int mblk) {
  return (long long)a.N * ((a.H + th - 1) / th) * ((a.W + 63) / 64) * ((a.nmblk + mblk - 1) / mblk);
}

// tile configurations {MB, WM, WN, RPW}: 8-wave workgroups (16 or 8 rows) when the layer has enough tiles for
// every CU, 4-wave ones with 8 / 4 rows for the small feature maps at the bottom of the U-Net
enum { CFG_M32_TH16 = 0, CFG_M64_TH16, CFG_M128_TH8, CFG_M32_TH8, CFG_M64_TH8, CFG_M128_TH4, CFG_M32_TH4, CFG_M64_TH4, CFG_COUNT };

// ... as a type for the launcher templates: f receives the shape of `cfg` (conv_tile_shape of conv_common.h is the fp32 side's)
template <int CFG_, int MB_, int WM_, int WN_, int RPW_>
struct H8TileShape {
  static constexpr int CFG = CFG_, MB = MB_, WM = WM_, WN = WN_, RPW = RPW_;
};
template <class F>
int h8_tile_shape(int cfg, F&& f) {
  switch (cfg) {
    case CFG_M32_TH16: return f(H8TileShape<CFG_M32_TH16, 1, 1, 8, 2>{});
    case CFG_M64_TH16: return f(H8TileShape<CFG_M64_TH16, 2, 1, 8, 2>{});
    case CFG_M128_TH8: return f(H8TileShape<CFG_M128_TH8, 2, 2, 4, 2>{});
    case CFG_M32_TH8:  return f(H8TileShape<CFG_M32_TH8, 1, 1, 4, 2>{});
    case CFG_M64_TH8:  return f(H8TileShape<CFG_M64_TH8, 2, 1, 4, 2>{});
    case CFG_M128_TH4: return f(H8TileShape<CFG_M128_TH4, 2, 2, 2, 2>{});
    case CFG_M32_TH4:  return f(H8TileShape<CFG_M32_TH4, 1, 1, 4, 1>{});
    case CFG_M64_TH4:  return f(H8TileShape<CFG_M64_TH4, 2, 1, 4, 1>{});
  }
  return SLU_EUNSUPPORTED;
}

int choose_h8(const H8Args& a) {
  const long long want = 256;
  static const int forced = slu_env_int("SLU_H8_CFG", -1);      // development aid
  if (forced >= 0 && forced < CFG_COUNT) return forced;
  if (a.nmblk >= 4) {
    if (a.H >= 8 && wg_count(a, 8, 4) >= want) return CFG_M128_TH8;
    if (wg_count(a, 4, 4) >= want) return CFG_M128_TH4;
    if (wg_count(a, 4, 2) >= want) return CFG_M64_TH4;
    return CFG_M32_TH4;
  }
  if (a.nmblk >= 2) {
    if (a.H >= 16 && wg_count(a, 16, 2) >= want) return CFG_M64_TH16;
    if (a.H >= 8 && wg_count(a, 8, 2) >= want) return CFG_M64_TH8;
    if (wg_count(a, 4, 2) >= want) return CFG_M64_TH4;
    return CFG_M32_TH4;
  }
  if (a.H >= 16 && wg_count(a, 16, 1) >= want) return CFG_M32_TH16;
  if (a.H >= 8 && wg_count(a, 8, 1) >= want) return CFG_M32_TH8;
  return CFG_M32_TH4;
}

// The 8-wave 128-channel configuration (the MFMA-bound 128 / 256-channel layers of the U-Net's lower levels) with its scheduling
// options (conv_h8_kernel's OPT / KPC).  SLU_H8_OPT / SLU_H8_KPC2 (environment) and, in -DSLU_H8_AB builds, slu_h8_dev_set_opt()
// are A/B switches of the development tools.
int g_h8_opt = slu_env_int("SLU_H8_OPT", -1);
int g_h8_kpc2 = slu_env_int("SLU_H8_KPC2", H8_M128_KPC2_DEFAULT);

constexpr size_t h8_m128_weight_bytes(int nks, int T) { return (size_t)4 * nks * T * 64 * 16; }

template <int KS, int DIL, int PAD, bool SCALED>
int launch_h8_m128(H8Args& a, const slu_conv_h8_desc* d, const SluEmit& e) {
  if (h8_m128_weight_bytes(a.nks, KS * KS) <= WRES_MAX_BYTES) return launch_h8_k<KS, DIL, PAD, 2, 2, 4, 2, SCALED, true>(a, d, e);
  if constexpr (!SCALED) {
    if (h8_one_plain_source(a)) {
      if constexpr (KS == 2) {
        if (g_h8_kpc2 && a.nks >= 2) {
#ifdef SLU_H8_AB
          if (g_h8_opt == 0) return launch_h8_k<KS, DIL, PAD, 2, 2, 4, 2, false, false, false, 2, 0, true>(a, d, e);
#endif
          return launch_h8_k<KS, DIL, PAD, 2, 2, 4, 2, false, false, false, 2, H8_M128_OPT_2X2, true>(a, d, e);
        }
      }
#ifdef SLU_H8_AB
      switch (g_h8_opt) {
        case 0: return launch_h8_k<KS, DIL, PAD, 2, 2, 4, 2, false, false, false, 1, 0, true>(a, d, e);
        case 8: return launch_h8_k<KS, DIL, PAD, 2, 2, 4, 2, false, false, false, 1, 8, true>(a, d, e);
        case 15: return launch_h8_k<KS, DIL, PAD, 2, 2, 4, 2, false, false, false, 1, 15, true>(a, d, e);
        case 100: return launch_h8_k<KS, DIL, PAD, 2, 2, 4, 2, false, false, false, 1, 0, false>(a, d, e);      // the general form, for comparison
      }
#endif
      return launch_h8_k<KS, DIL, PAD, 2, 2, 4, 2, false, false, false, 1, KS == 2 ? H8_M128_OPT_2X2 : H8_M128_OPT_3X3, true>(a, d, e);
    }
  }
  return launch_h8_k<KS, DIL, PAD, 2, 2, 4, 2, SCALED, false>(a, d, e);
}

template <int KS, int DIL, int PAD, bool SCALED>
int launch_h8_tiles(H8Args& a, const slu_conv_h8_desc* d, int cfg, const SluEmit& e) {
  return h8_tile_shape(cfg, [&](auto s) {
    using S = decltype(s);
    if constexpr (S::CFG == CFG_M128_TH8) return launch_h8_m128<KS, DIL, PAD, SCALED>(a, d, e);
    else return launch_h8<KS, DIL, PAD, S::MB, S::WM, S::WN, S::RPW, SCALED>(a, d, e);
  });
}

// out = leaky(conv3x3 + bias + resid) (slu_conv_h8_desc.act_after_resid): conv_h8_late_kernel in the tile configuration choose_h8 picks, weights
// streamed per chunk (a BasicBlock's 64 .. 512-channel weights never fit the resident form); the 128-channel configuration with the
// scheduling options of its plain 3x3 form where the layer has one plain source
template <int MB, int WM, int WN, int RPW, int OPT = 0, bool ONE = false>
int launch_h8_late_k(H8Args& a, const slu_conv_h8_desc* d, const SluEmit& e) {
  return launch_h8_k<3, 1, 1, MB, WM, WN, RPW, false, false, false, 1, OPT, ONE, true>(a, d, e);
}
int launch_h8_late(H8Args& a, const slu_conv_h8_desc* d, int cfg, const SluEmit& e) {
  return h8_tile_shape(cfg, [&](auto s) {
    using S = decltype(s);
    if constexpr (S::CFG == CFG_M128_TH8)
      if (h8_one_plain_source(a)) return launch_h8_late_k<S::MB, S::WM, S::WN, S::RPW, H8_M128_OPT_3X3, true>(a, d, e);
    return launch_h8_late_k<S::MB, S::WM, S::WN, S::RPW>(a, d, e);
  });
}

template <int KS, int DIL, int PAD>
int launch_h8_family(H8Args& a, const slu_conv_h8_desc* d, int cfg, bool scaled, const SluEmit& e) {
  return scaled ? launch_h8_tiles<KS, DIL, PAD, true>(a, d, cfg, e) : launch_h8_tiles<KS, DIL, PAD, false>(a, d, cfg, e);
}

}  // namespace

int slu_h8::h8_tiled(H8Args& a, const slu_conv_h8_desc* d, const SluEmit& e) {
  const bool sc = any_scale(d);
  if (d->act_after_resid) {      // one family implements the late activation; every other path refuses the flag, none ignores it
    if (d->ksize != 3 || d->dil != 1 || d->pad != 1 || !d->resid || !d->has_act || d->bn_a || a.out_f32 || a.src[0].shuf || sc) return SLU_EUNSUPPORTED;
    return launch_h8_late(a, d, choose_h8(a), e);
  }
  if (a.src[0].shuf) {      // read in place by ring3_h8_kernel<1, 1, 5, 1, 4> or, here, by the SCALED 3x3 kernels; anything else: slu_pixel_shuffle_h8
    if (!sc || d->ksize != 3 || d->dil != 1 || d->pad != 1 || a.out_f32) return SLU_EUNSUPPORTED;
    return launch_h8_family<3, 1, 1>(a, d, choose_h8(a), true, e);
  }
  if (a.out_f32) {      // fp32 NCHW output outside the streaming kernel's reach (odd H*W): 1x1 head only
    if (d->ksize != 1 || d->dil != 1 || d->pad != 0 || sc) return SLU_EUNSUPPORTED;
    return launch_h8_k<1, 1, 0, 1, 1, 4, 1, false, false, true>(a, d, e);
  }
  const int cfg = choose_h8(a);
  return slu_conv_family(d->ksize, d->dil, d->pad, [&](auto g) -> int {
    using G = decltype(g);
    // taps at offsets -1 and 0: a 3x3 / stride 2 / pad 1 conv over the space-to-depth image of its input (slu_space_to_depth2_h8); no multipliers
    if constexpr (G::KS == 2 && G::DIL == 1) return sc ? SLU_EUNSUPPORTED : launch_h8_tiles<2, 1, 1, false>(a, d, cfg, e);
    else return launch_h8_family<G::KS, G::DIL, G::PAD>(a, d, cfg, sc, e);
  });
}

#ifdef SLU_H8_AB
extern "C" void slu_h8_dev_set_opt(int opt, int kpc2) { g_h8_opt = opt; g_h8_kpc2 = kpc2; }
#endif

#include "conv1x1_h8.h"      // the streaming 1x1 family: compiled in this unit (see there)

#ifdef SLU_H8_PROF
extern "C" int slu_h8_prof_read(unsigned long long* out8) {
  if (hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_h8_prof), sizeof(unsigned long long) * 8) != hipSuccess) return SLU_ELAUNCH;
  unsigned long long z[8] = {};
  return hipMemcpyToSymbol(HIP_SYMBOL(g_h8_prof), z, sizeof(z)) == hipSuccess ? SLU_OK : SLU_ELAUNCH;
}
#endif
