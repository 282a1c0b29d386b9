/*
 * slu.h -- C ABI of libslu_hip.so: the MI355X (gfx950) kernels behind the SemanticLiDARUnc
 * range-image hot path.
 *
 * The reference (kav-institute/SemanticLiDARUnc) is pure Python on torch: it has no FFI layer, so
 * there is no reference-side binding to replace one-for-one.  Each entry point below names the
 * reference Python code whose arithmetic it replaces (path:line under the reference's src/), and
 * INTEGRATION.md shows the ctypes stub a maintainer adds to call it.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer unless the comment says HOST; tensors are dense NCHW fp32
 *    (W = azimuth fastest), labels / predictions int64, exactly the layouts the reference uses;
 *  - the library never allocates, frees or synchronises: outputs and scratch are caller-owned,
 *    every launch is asynchronous on `stream` (a hipStream_t passed as void*; NULL = default);
 *  - return value 0 = launched, negative = SLU_E* (nothing was launched); never throws/exits;
 *  - re-entrant, no mutable global state.
 */
#ifndef SLU_H_
#define SLU_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SLU_ABI_VERSION 46

#define SLU_OK            0
#define SLU_EINVAL       -1   /* null pointer / non-positive size / inconsistent descriptor   */
#define SLU_EUNSUPPORTED -2   /* shape or kernel family outside what the library instantiates */
#define SLU_ELAUNCH      -3   /* hipGetLastError() != hipSuccess right after the launch       */

typedef void* slu_stream_t;

int slu_abi_version(void);
const char* slu_strerror(int code);

/* ------------------------------------------------------------------------------------------
 * Convolution (replaces nn.Conv2d + nn.LeakyReLU + eval nn.BatchNorm2d + residual add +
 * torch.cat + nn.PixelShuffle(2) + nn.Dropout2d of  baselines/SalsaNext/SalsaNext.py:25-39,
 * :73-109, :142-170, :213)
 *
 *   out[n,co,y,x] = resid[n,co,y,x]
 *                 + bn_a[co] * leaky( bias[co] + sum_{ci,i,j} w[co,ci,i,j] * in[n,ci,y-pad+i*dil,x-pad+j*dil] ) + bn_b[co]
 *
 * `in` is the channel concatenation of up to 3 sources; a source may be read through
 * PixelShuffle(2) and multiplied by a per-(n, source-channel) factor (folded Dropout2d).
 * `out` must not overlap any input (sources, resid).  Stride 1, "same" output size; kernel families (ksize,dil,pad) = (1,1,0) (3,1,1) (3,2,2) (2,2,1).
 * ------------------------------------------------------------------------------------------ */
#define SLU_MAX_SRC 3

typedef struct slu_conv_src {
  const float* ptr;    /* [N, C, H, W]  or, when pixel_shuffle, [N, C, H/2, W/2]                */
  const float* scale;  /* [N, C] multiplier per (sample, source channel), or NULL               */
  int32_t C;           /* channels of the stored tensor                                          */
  int32_t pixel_shuffle; /* 1: contributes C/4 channels, in[c,y,x] = ptr[4c+2(y&1)+(x&1), y/2, x/2] */
  int32_t nbatch;      /* 0: the tensor holds N images; k > 0: it holds k images and output image n reads image n % k
                          (a deterministic skip tensor shared by the stacked MC passes); `scale` stays [N, C]      */
  int32_t cuse;        /* 0: every channel contributes; k > 0: only the first k channels do (the reference overwrites the
                          last meta_channel_dim channels of a stage output: x[:, :-m], semanticFCN.py:309-313).  Only
                          allowed on the LAST source, without pixel_shuffle                                          */
} slu_conv_src;

typedef struct slu_conv_desc {   /* HOST struct */
  slu_conv_src src[SLU_MAX_SRC];
  int32_t nsrc;
  int32_t N, H, W;       /* output (= input) spatial size                                        */
  int32_t Cin, Cout;     /* Cin = sum of contributed channels                                    */
  int32_t ksize, dil, pad;
  int32_t ck;            /* K-chunk the weights were packed with (slu_conv_ck)                   */
  const float* wpack;    /* slu_pack_conv_weight output                                          */
  const float* bias;     /* [Cout] or NULL                                                       */
  int32_t has_act;       /* 0 none; 1: leaky(v) = v > 0 ? v : slope * v (slope 0 = ReLU); 2: tanh(v); 3: SiLU v * sigmoid(v);
                            +4 (with 1 only): apply it after bn_a/bn_b and the residual add (ResNet BasicBlock) instead of before */
  float slope;
  const float* bn_a;     /* [Cout] or NULL (then bn_b ignored): folded eval BatchNorm            */
  const float* bn_b;
  const float* resid;    /* [N, Cout, H, W] or NULL                                              */
  float* out;            /* [N, Cout, H, W]                                                      */
  int32_t precision;     /* SLU_CONV_FP32 (exact fp32 MFMA) or SLU_CONV_F16X3 (split-fp16, see below)             */
  double* stats;         /* NULL, or f64 [2][Cout] (zero it first): the kernel adds the per-channel sum and sum of squares of the values it
                            stores -- the batch statistics of a train-mode BatchNorm that follows (SalsaNext.py:30-36) without a second pass
                            over the output.  SLU_CONV_FP32 only.                                                                        */
} slu_conv_desc;

/* precision of the multiply-accumulate inside slu_conv2d_fwd (inputs, outputs and accumulation are fp32 either way):
 *   SLU_CONV_FP32  : v_mfma_f32_32x32x2_f32, bit-for-bit a k-ordered fmaf chain; wpack from slu_pack_conv_weight, ck = slu_conv_ck
 *   SLU_CONV_F16X3 : every fp32 operand x is split x = hi + lo (two fp16), products hi*hi + hi*lo + lo*hi on
 *                    v_mfma_f32_32x32x16_f16 (fp32 accumulate): ~2^-22 relative error per product while lo is a normal
 *                    fp16 (|x| >= 2^-3), an absolute operand error of 2^-24 below that (2e-5 of the output scale holds while
 *                    both operands have rms >= 2^-8), hi saturates above 65504 and lo carries the rest up to 131008
 *                    (DESIGN 3.1b); 5.3x fewer MFMA cycles; wpack from slu_pack_conv_weight_f16x3, ck = 16 */
#define SLU_CONV_FP32  0
#define SLU_CONV_F16X3 1

/* K-chunk (input channels staged per LDS round) used for a kernel family. */
int slu_conv_ck(int ksize);
/* number of floats of the packed (MFMA A-fragment ordered, zero padded) weight image */
size_t slu_packed_weight_floats(int cout, int cin, int ksize, int ck);
/* w: [cout, cin, ksize, ksize] (torch OIHW) -> out: packed image.  Re-run after every weight update. */
int slu_pack_conv_weight(const float* w, int cout, int cin, int ksize, int ck, float* out, slu_stream_t stream);
/* many weights in one launch (a training step repacks all of them after the optimizer step).  jobs_dev: DEVICE array; job i packs w
 * [cout][cin][k][k] into `out` (slu_packed_weight_floats(cout, cin, k, ck) floats) as slu_pack_conv_weight does, or -- dgrad = 1 -- the weights
 * of the data-gradient conv (slu_dgrad_weight + slu_pack_conv_weight: slu_packed_weight_floats(cin, cout, k, ck) floats); begin = sum of the
 * output sizes of the jobs before it (ascending), total = sum over all jobs. */
typedef struct slu_pack_job {
  const float* w;
  float* out;
  int32_t cout, cin, ksize, ck;
  int32_t dgrad, reserved;
  uint64_t begin;
} slu_pack_job;
int slu_pack_conv_weights_multi(const slu_pack_job* jobs_dev, int njobs, size_t total, slu_stream_t stream);
int slu_conv2d_fwd(const slu_conv_desc* desc, slu_stream_t stream);
/* split-fp16 weight image (bytes) and its packer (w: [cout,cin,k,k] fp32 OIHW) */
size_t slu_packed_weight_bytes_f16x3(int cout, int cin, int ksize);
int slu_pack_conv_weight_f16x3(const float* w, int cout, int cin, int ksize, void* out, slu_stream_t stream);
/* Name of the kernel instantiation slu_conv2d_fwd launches for `desc` (as rocprofv3 prints it), into HOST buf (64 bytes hold every name).
 * The launch's own dispatch with a leaf that prints instead of launching: no HIP call, and the status is the one slu_conv2d_fwd returns
 * for `desc` (a refused descriptor gets that error, not a name); SLU_EINVAL for a null or too short buf. */
int slu_conv2d_kernel_name(const slu_conv_desc* desc, char* buf, size_t buflen);

/* a = gamma / sqrt(var + eps), b = beta - mean * a   (eval-mode nn.BatchNorm2d, SalsaNext.py:32,36,...) */
int slu_bn_fold(const float* gamma, const float* beta, const float* mean, const float* var, float eps,
                int C, float* a, float* b, slu_stream_t stream);

/* nn.AvgPool2d(3, stride=2, padding=1) (count_include_pad) of x * scale[n,c]  (SalsaNext.py:69,98-101).
 * x [N,C,H,W] -> y [N,C,(H+1)/2,(W+1)/2]; scale [N,C] or NULL. */
int slu_avgpool3s2_fwd(const float* x, const float* scale, float* y, int N, int C, int H, int W,
                       slu_stream_t stream);
/* same, but x holds only `in_batch` images and output image n pools x[n % in_batch] (scale is [N,C]) */
int slu_avgpool3s2_bcast_fwd(const float* x, const float* scale, float* y, int N, int in_batch, int C, int H, int W,
                             slu_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * MC-dropout reduction (replaces models/trainer.py:1105-1136,1143-1154 = tester.py:412-451)
 *   probs_t = exp(log_softmax(logits_t)); p_bar = mean_t probs_t;
 *   H_norm = -sum_c clamp(p_bar,eps) ln clamp(p_bar,eps) / ln C
 *   MI_norm = max(0, (H - mean_t H[probs_t]) / ln C);  preds = argmax_c p_bar (first max wins)
 * logits [T,B,C,HW]; p_bar [B,C,HW]; h_norm, mi_norm [B,HW]; preds int64 [B,HW].  C <= 32.
 * ------------------------------------------------------------------------------------------ */
int slu_mc_reduce(const float* logits, int T, int B, int C, int HW, float eps,
                  float* p_bar, float* h_norm, float* mi_norm, int64_t* preds, slu_stream_t stream);

/* Single-pass eval (replaces models/trainer.py:1180-1184,1211-1214):
 *   probs = exp(log_softmax(logits)); preds = argmax; H_norm = -sum p ln max(p, eps) / ln C */
int slu_softmax_entropy(const float* logits, int B, int C, int HW, float eps,
                        float* probs, float* h_norm, int64_t* preds, slu_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Metrics
 * ------------------------------------------------------------------------------------------ */
/* confmat[t*C+p] += 1 for every pixel with 0 <= t,p < C   (models/evaluator.py:45-53; rows = GT) */
int slu_confusion_update(const int64_t* preds, const int64_t* targets, int64_t n, int C,
                         int64_t* confmat, slu_stream_t stream);

/* Top-label calibration bins (metrics/ece.py:55-84,136-140), mode 'probs':
 *   p = max(probs,0) / max(sum_c, 1e-12); conf = clamp(max_c p, 0, 1); correct = argmax == label;
 *   pixels with label == ignore_index are skipped (pass INT64_MIN for "no ignore");
 *   bin b = [b/n_bins, (b+1)/n_bins) on float32 edges linspace(0,1,n_bins+1), last bin closed.
 * Accumulates: count int64[n_bins], sum_correct f64[n_bins], sum_conf f64[n_bins]. */
int slu_ece_update(const float* probs, const int64_t* labels, int B, int C, int HW, int64_t ignore_index,
                   int n_bins, int64_t* count, double* sum_correct, double* sum_conf, slu_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Loss (models/trainer.py:511-514): probs = softmax(logits);
 *   nll_sum += sum_pixels -ln max(probs[label], clamp)     (caller divides by the pixel count)
 * logits [B,C,HW], labels int64 [B,HW] in [0,C); probs out [B,C,HW] (may be NULL); nll_sum f64[1].
 * ------------------------------------------------------------------------------------------ */
int slu_softmax_nll_fwd(const float* logits, const int64_t* labels, int B, int C, int HW, float clamp,
                        float* probs, double* nll_sum, slu_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Per-pixel NLL / cross-entropy (models/losses.py:55-73, trainer.py:514).  x [B,C,HW]; pixels whose label is
 * == ignore_index or outside [0,C) are skipped.  kind: 0 logits (nll = logsumexp - x_y, i.e. CrossEntropyLoss),
 * 1 probs, -ln max(p_y, param);  2 probs, -ln(p_y + param);  3 log-probs, -x_y.
 * fwd: nll_sum f64[1] += sum, count int64[1] += #pixels (caller zeroes both, divides).
 * bwd: grad_x[B,C,HW] = gscale[0] * d(sum nll)/dx   (gscale: DEVICE scalar = upstream grad / count).
 * ------------------------------------------------------------------------------------------ */
int slu_nll_fwd(const float* x, const int64_t* labels, int B, int C, int HW, int kind, float param, int64_t ignore_index,
                double* nll_sum, int64_t* count, slu_stream_t stream);
int slu_nll_bwd(const float* x, const int64_t* labels, int B, int C, int HW, int kind, float param, int64_t ignore_index,
                const float* gscale, float* grad_x, slu_stream_t stream);

/* Softmax backward of the fused SalsaNext loss (trainer.py:511-516):
 *   g_c = gout[0] * ( w_dense * dense[c]  -  [c == y and p_y >= clamp] * w_nll / p_y ),  grad_logits_c = p_c (g_c - sum_k g_k p_k)
 * probs, dense (nullable), grad_logits [B,C,HW]; labels nullable; gout DEVICE scalar or NULL (= 1). */
int slu_softmax_loss_bwd(const float* probs, const int64_t* labels, const float* dense, float w_dense, float w_nll, float clamp,
                         const float* gout, int B, int C, int HW, float* grad_logits, slu_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Lovasz-Softmax (losses/lovasz.py:12-88).  probs [B,C,HW] (rows sum to 1), labels int64 [B,HW];
 * pixels with label == ignore_index are dropped (pass INT64_MIN for none).
 * class_mask: 0 = classes='present' (the classes that occur among the valid labels); else bit c set = class c is summed whether it occurs
 *   or not (classes='all': all C bits; classes=[...]: those) -- an absent class contributes its largest probability (lovasz.py:62-75).
 *   loss[1]      : mean over the summed classes of  sum_k err_(k) * (J_k - J_{k-1})   (errors sorted descending)
 *   n_present[1] : number of summed classes (float)
 *   grad_probs   : [B,C,HW] d loss / d probs, or NULL
 * workspace: slu_lovasz_workspace_bytes(B,C,HW) bytes, 256-byte aligned, caller-owned scratch.
 * ------------------------------------------------------------------------------------------ */
size_t slu_lovasz_workspace_bytes(int B, int C, int HW);
int slu_lovasz_fwd(const float* probs, const int64_t* labels, int B, int C, int HW, int64_t ignore_index, unsigned class_mask,
                   void* workspace, size_t workspace_bytes, float* loss, float* n_present, float* grad_probs,
                   slu_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Training side of the conv stack (autograd of SalsaNext.py:25-39,73-109,142-170; nn.BatchNorm2d train mode).
 * All tensors dense fp32; [N,C,HW] = NCHW with H*W flattened.  f64 accumulators are caller-zeroed, += semantics.
 * ------------------------------------------------------------------------------------------ */
/* sum[c] += sum y, sumsq[c] += sum y^2 over (N,HW) */
int slu_bn_stats(const float* y, int N, int C, int HW, double* sum, double* sumsq, slu_stream_t stream);
/* s1[c] += sum dz, s2[c] += sum dz * (y - mean[c]) * invstd[c] */
int slu_bn_bwd_reduce(const float* dz, const float* y, const float* mean, const float* invstd, int N, int C, int HW,
                      double* s1, double* s2, slu_stream_t stream);
/* per-channel BatchNorm coefficients in one launch (fp64 inside).  train != 0: statistics from sum/sumsq over `count` elements
 * (biased variance), running_mean/var updated in place with `momentum` and the unbiased variance (nullable: no update);
 * train == 0: statistics = running_mean/var.  Outputs mean, invstd, a = gamma*invstd, b = beta - mean*a (all [C]). */
int slu_bn_coeffs_fwd(const double* sum, const double* sumsq, double count, const float* gamma, const float* beta, float eps,
                      float momentum, int train, float* running_mean, float* running_var, int C, float* mean, float* invstd,
                      float* a, float* b, slu_stream_t stream);
/* backward coefficients for slu_act_affine_bwd from slu_bn_bwd_reduce sums: k1 = gamma*invstd; train: k3 = -gamma*invstd^2*s2/count,
 * k2 = -gamma*invstd*s1/count - k3*mean; eval: k2 = k3 = 0; dgamma = s2, dbeta = s1 */
int slu_bn_coeffs_bwd(const double* s1, const double* s2, double count, const float* gamma, const float* mean, const float* invstd,
                      int train, int C, float* k1, float* k2, float* k3, float* dgamma, float* dbeta, slu_stream_t stream);
/* z = a[c]*y + b[c] + resid   (a, b, resid nullable: 1, 0, 0) */
int slu_affine_fwd(const float* y, const float* a, const float* b, const float* resid, float* z, int N, int C, int HW,
                   slu_stream_t stream);
/* da = (k1[c]*dz + k2[c] + k3[c]*y) * (has_act && y <= 0 ? slope : 1);  dbias[c] += sum da  (k*, y, dbias nullable) */
int slu_act_affine_bwd(const float* dz, const float* y, const float* k1, const float* k2, const float* k3, float slope,
                       int has_act, int N, int C, int HW, float* da, double* dbias, slu_stream_t stream);
/* The two BatchNorm passes of a layer with their coefficient launches folded in (a training step has 42 such layers):
 * slu_bn_apply_fwd = slu_bn_coeffs_fwd + slu_affine_fwd: z = gamma (y - mean) invstd + beta [+ resid]; mean / invstd [C] are written for the
 *   backward, the running statistics updated as slu_bn_coeffs_fwd does.
 * slu_bn_act_bwd = slu_bn_coeffs_bwd + slu_act_affine_bwd + the fp64 -> fp32 rounding of the bias gradient: has_bn = 0: k1 = 1, k2 = k3 = 0.
 *   acc64 [C] fp64 and ticket [C] uint32 are caller-ZEROED scratch (the last workgroup of a channel to add its partial sum writes dbias[c]);
 *   dbias nullable (then acc64 / ticket are unused); dgamma / dbeta [C] fp32 (has_bn only). */
int slu_bn_apply_fwd(const float* y, const double* sum, const double* sumsq, double count, const float* gamma, const float* beta, float eps,
                     float momentum, int train, float* running_mean, float* running_var, const float* resid, float* z, int N, int C, int HW,
                     float* mean, float* invstd, slu_stream_t stream);
int slu_bn_act_bwd(const float* dz, const float* y, const double* s1, const double* s2, double count, const float* gamma, const float* mean,
                   const float* invstd, int has_bn, int train, float slope, int has_act, int N, int C, int HW, float* da, double* acc64,
                   unsigned* ticket, float* dbias, float* dgamma, float* dbeta, slu_stream_t stream);
/* src [N,C,HW] -> dst [N,HW,Cp], Cp = C rounded up to 32, padding channels zero */
int slu_nchw_to_nhwc(const float* src, int N, int C, int HW, float* dst, slu_stream_t stream);
/* the conv input described by `src` (concat / PixelShuffle / multipliers applied) as [N,H*W,Cp] */
int slu_gather_nhwc(const slu_conv_src* src, int nsrc, int N, int H, int W, float* dst, slu_stream_t stream);
/* gradient of one source: dsrc = (channels [cbeg, cbeg+contributed) of dcat [N,Ccat,H,W], un-shuffled) * scale[n,cs] */
int slu_split_grad(const float* dcat, int N, int Ccat, int cbeg, int H, int W, int Csrc, int pixel_shuffle, const float* scale,
                   float* dsrc, slu_stream_t stream);
/* backward of slu_avgpool3s2_fwd: dy [N,C,(H+1)/2,(W+1)/2] -> dx [N,C,H,W] */
int slu_avgpool3s2_bwd(const float* dy, const float* scale, float* dx, int N, int C, int H, int W, slu_stream_t stream);
/* weights of the data-gradient conv: wd[ci][co][k-1-i][k-1-j] = w[co][ci][i][j]; feed to slu_pack_conv_weight and run
 * slu_conv2d_fwd on da with Cin/Cout swapped (the four kernel families are symmetric: 2*pad == (k-1)*dil) */
int slu_dgrad_weight(const float* w, int cout, int cin, int ksize, float* wd, slu_stream_t stream);
/* dW [cout,cin,k,k] = sum_pixels da * shifted input; da_t [N,HW,Cop], in_t [N,HW,Cip] channel-last (padded to 32);
 * dWp: scratch of slu_wgrad_packed_floats floats.  W must be even.  fp32 atomics: not bit-reproducible. */
size_t slu_wgrad_packed_floats(int cout, int cin, int ksize);
int slu_conv2d_wgrad(const float* da_t, const float* in_t, int N, int H, int W, int Cout, int Cin, int ksize, int dil, int pad,
                     float* dWp, float* dW, slu_stream_t stream);
/* weight gradient of a 1x1 conv straight from the NCHW tensors (no channel-last copies): da [N,Cout,HW], the conv's sources as in
 * slu_conv2d_fwd (plain tensors only: no PixelShuffle / multiplier / broadcast; every source but the last a multiple of 32 channels; HW a
 * multiple of 32; 16-byte aligned bases) -> dW [Cout, sum of source channels].  SLU_EUNSUPPORTED otherwise (use slu_conv2d_wgrad).
 * prezeroed != 0: the caller hands over an accumulator that is already zero (dW here, dWp below) and the launcher skips its fill -- a
 * training step issues ~50 of these calls, one fill each was 0.2 ms of it. */
int slu_conv1x1_wgrad_nchw(const float* da, const slu_conv_src* src, int nsrc, int N, int HW, int Cout, float* dW, int prezeroed, slu_stream_t stream);
/* the 3x3 (dil 1 / 2, pad = dil) and 2x2 (dil 2, pad 1) families: da [N,Cout,H,W]; sources as in slu_conv2d_fwd including PixelShuffle and
 * multipliers (no broadcast / channel cut), any channel counts; W a multiple of 16 (PixelShuffle sources: H even);
 * dWp: scratch of slu_wgrad_packed_floats floats -> dW [Cout, Cin, k, k].  SLU_EUNSUPPORTED otherwise (use slu_conv2d_wgrad). */
int slu_conv2d_wgrad_nchw(const float* da, const slu_conv_src* src, int nsrc, int N, int H, int W, int Cout, int ksize, int dil, int pad,
                          float* dWp, float* dW, int prezeroed, slu_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * ResNet-FPN pieces (models/semanticFCN.py:145-153, 230-245, 266-354): data movement around the conv kernel.
 * ------------------------------------------------------------------------------------------ */
/* nn.MaxPool2d(3, 2, 1): x [N,C,H,W] -> y [N,C,(H+1)/2,(W+1)/2] */
int slu_maxpool3s2_fwd(const float* x, float* y, int N, int C, int H, int W, slu_stream_t stream);
/* F.interpolate(mode='nearest', scale_factor=1/factor): y[..,oy,ox] = x[..,oy*factor,ox*factor] */
int slu_nearest_down(const float* x, float* y, int N, int C, int H, int W, int factor, slu_stream_t stream);
/* y[n,(2p+q)*C+c,oy,ox] = x[n,c,2oy+p,2ox+q]: a stride-2 3x3/p1 conv on x == a (2,1,1) conv on y with re-indexed weights */
int slu_space_to_depth2(const float* x, float* y, int N, int C, int H, int W, slu_stream_t stream);
/* the same of cat(a[:, :ca], b) (a [N,Ca,H,W], b [N,Cb,H,W]) -> y [N, 4*(ca+Cb), H/2, W/2] */
int slu_space_to_depth2_cat(const float* a, int Ca, int ca, const float* b, int Cb, float* y, int N, int H, int W, slu_stream_t stream);
/* nn.PixelShuffle(r) of x [N,Cout*r*r,H,W], optionally followed by ELU(v)+1, written into channels [c_off, c_off+Cout) of
 * y [N,Ctot,H*r,W*r] (c_off = 0, Ctot = Cout: a plain PixelShuffle; otherwise several maps share one concatenated buffer) */
int slu_depth_to_space(const float* x, float* y, int N, int Cout, int H, int W, int r, int elu_plus_one, int c_off, int Ctot,
                       slu_stream_t stream);
/* out = value * softmax(score, dim=-1): score [N,1,H,W], value/out [N,C,H,W]; W <= 4096 (AttentionModule :32-38) */
int slu_row_softmax_mul(const float* score, const float* value, float* out, int N, int C, int H, int W, slu_stream_t stream);

/* ---- pieces of the `semanticFCN_opt` variant (baselines/Reichert/semanticFCN_opt.py) -----------------------------
 * slu_bilinear_upsample: F.interpolate(x, scale_factor = scale, mode = 'bilinear', align_corners = False) (UpsampleBlock :24-27):
 *   x [N,C,H,W] -> y [N,C,H*scale,W*scale].
 * slu_groupnorm_fwd: nn.GroupNorm(groups, C, eps) [+ ReLU] (:20,66-70): statistics per (sample, group) over (C/groups)*HW (biased
 *   variance, accumulated in fp64), y = (x - mean) * rstd * gamma[c] + beta[c]; mean / rstd fp32 [N*groups] are outputs; y may be x.
 * slu_spatial_softmax_gate: SpatialAttention's gate (:80-85): w = softmax(score[n] over H*W); out = x * w + x.  x, out [N,C,HW];
 *   score [N,1,HW]; stats fp32 [2 N] scratch (max, 1 / sum). */
int slu_bilinear_upsample(const float* x, float* y, int N, int C, int H, int W, int scale, slu_stream_t stream);
int slu_groupnorm_fwd(const float* x, const float* gamma, const float* beta, int N, int C, int HW, int groups, float eps, int relu, float* mean,
                      float* rstd, float* y, slu_stream_t stream);
int slu_spatial_softmax_gate(const float* x, const float* score, float* stats, float* out, int N, int C, int HW, slu_stream_t stream);
/* the statistics launch of slu_groupnorm_fwd alone: mean / rstd fp32 [N*groups], the same numbers */
int slu_groupnorm_stats(const float* x, int N, int C, int HW, int groups, float eps, float* mean, float* rstd, slu_stream_t stream);

/* GroupNorm apply [+ ReLU] + 1x1 segmentation head + MC-dropout reduction in one pass, exact fp32 (semanticFCN_opt.py:286-296 +
 * trainer.py:1143-1154): x fp32 [T*B][Cin][HW], pass-major (image t*B + b = pass t of scan b);
 * v = (x - mean[n*groups + c/(Cin/groups)]) * rstd[..] * gamma[c] + beta[c] (mean / rstd from slu_groupnorm_stats, [T*B*groups] each; both NULL:
 * v = x; gamma / beta [Cin] or NULL), max(v, 0) if relu; logits = w v + bias with w [C][Cin] row-major (the Conv2d weight as stored), bias [C] or
 * NULL.  Outputs as slu_mc_reduce: p_bar fp32 [B][C][HW], h_norm / mi_norm fp32 [B][HW], preds int64 [B][HW].  1 <= C <= 32 (SLU_EINVAL
 * otherwise); Cin <= 128 (SLU_EUNSUPPORTED above); any HW (16-byte accesses when HW % 4 == 0 and every base is 16-byte aligned). */
int slu_head_mc_f32(const float* x, int T, int B, int Cin, int HW, const float* gn_mean, const float* gn_rstd, const float* gn_gamma,
                    const float* gn_beta, int groups, int relu, const float* w, const float* bias, int C, float eps, float* p_bar, float* h_norm,
                    float* mi_norm, int64_t* preds, slu_stream_t stream);

/* ---- fp16 channel-blocked ("h8") inference path: BASELINE.json configs[2],[4] (half-precision storage, fp32 accumulate): conv2d_h8.hip (dispatch) and the kernel families of conv_h8.h ----
 * Activation layout: x[N][G = ceil(C/8)][H][W][8] fp16, pad channels = 0, base pointers 16-byte aligned.
 * Replaces the same reference arithmetic as slu_conv2d_fwd (SalsaNext.py:25-39,73-109,142-170,197-215) with fp16 operands. */
typedef struct slu_h8_src {
  const void* ptr;     /* h8 tensor [nimg][G][H][W][8]                                                              */
  const float* scale;  /* [N][8 G] fp32 multiplier per (output image, channel) (Dropout2d), or NULL; 16-byte aligned  */
  int32_t G;           /* channel blocks                                                                             */
  int32_t nbatch;      /* 0: nimg = N; k > 0: the tensor holds k images, output image n reads image n % k            */
  int32_t shuffle;     /* 1 (first source only): the source is nn.PixelShuffle(2) of ptr, read in place.  ptr is h8
                          [N][G][H/2][W/2][8] whose channels are STORED IN SHUFFLE ORDER -- stored block 4 go + sub, slot k
                          holds channel 32 go + 4 k + sub of the tensor PixelShuffle is applied to (sub = 2 i + j), so that
                          the record of shuffled block go at output pixel (y, x) is the stored record of block
                          4 go + 2 (y & 1) + (x & 1) at (y >> 1, x >> 1).  The source contributes G / 4 blocks; G a multiple
                          of 8 (SLU_EINVAL otherwise), H and W even; scale is [N][8 G] per STORED channel in stored order.
                          COVERED: (a) G == 8 (64 stored channels = one shuffled K-step) as the first of two sources of
                          the 80 -> 32 3x3 layer that ring3_h8_kernel<1, 1, 5, 1, 4> runs (second source plain: no
                          scale, no nbatch; at least 256 tiles of 8 x 64; N <= 237 with a scale); (b) any 3x3 / dil 1 /
                          pad 1 layer with h8 output in which SOME source carries a scale (the SCALED conv_h8_kernel
                          instantiations), with 3 G / 4 + input blocks <= 64 (one multiplier record per stored block).
                          Anything else is SLU_EUNSUPPORTED: materialise the shuffle with slu_pixel_shuffle_h8.
                          Each multiplier is rounded to fp16 and the fp16 product rounds once; slu_pixel_shuffle_h8
                          multiplies by the fp32 value and rounds once.  The two agree bit for bit when the multipliers
                          are exact in fp16 (0 and products of 1 / (1 - p) for p = 0.2: powers of 1.25); for other
                          values they may differ in the last fp16 bit of the scaled input                              */
  int32_t reserved;
} slu_h8_src;

typedef struct slu_conv_h8_desc {   /* HOST struct */
  slu_h8_src src[SLU_MAX_SRC];  /* concatenated along channels, block-wise (torch.cat(dim=1) of 8-aligned tensors)   */
  int32_t nsrc;
  int32_t N, H, W, Cout, ksize, dil, pad;
  const void* wpack;     /* slu_pack_conv_weight_h8 output                                                           */
  const float* bias;     /* [Cout] fp32 or NULL                                                                      */
  int32_t has_act;       /* 0 none; 1: leaky(v) = v > 0 ? v : slope * v                                              */
  float slope;
  const float* bn_a;     /* [Cout] fp32 or NULL: folded eval BatchNorm                                               */
  const float* bn_b;
  const void* resid;     /* h8 [N][ceil(Cout/8)][H][W][8] or NULL                                                    */
  void* out;             /* h8 [N][ceil(Cout/8)][H][W][8], or fp32 [N][Cout][H][W] when out_f32_nchw                  */
  int32_t out_f32_nchw;  /* 1: the logits head (SalsaNext.py:213) keeps the reference's fp32 NCHW output; 1x1 convs only */
  int32_t act_after_resid; /* 1: out = act(conv + bias + resid), the tail of a torchvision BasicBlock with its BatchNorm folded
                            (semanticFCN.py:145-153 builds on it; out = relu(bn2(conv2(.)) + identity)).  Needs resid, has_act and
                            no bn_a; (k,dil,pad) = (3,1,1), h8 output, no scale, no shuffled source (conv_h8_late_kernel).
                            Anything else with the flag set is SLU_EUNSUPPORTED: it is never ignored.  0: the order above      */
} slu_conv_h8_desc;

size_t slu_packed_weight_bytes_h8(int cout, int cin, int ksize);
/* w: OIHW fp32 [cout][cin][k][k] (cin = real channels of the concatenated input; only the LAST source may be padded) */
int slu_pack_conv_weight_h8(const float* w, int cout, int cin, int ksize, void* out, slu_stream_t stream);
/* out = [resid +] bn_a * act(conv(cat(src * scale)) + bias) + bn_b, rounded to fp16 once.
 * Families: (k,dil,pad) = (1,1,0), (3,1,1), (3,2,2), (2,2,1) as in slu_conv2d_fwd, and (2,1,1) without scales: taps at offsets -1 and 0,
 * which is a 3x3 / stride 2 / pad 1 conv (the first conv of a ResNet stage) over slu_space_to_depth2_h8 of its input. */
int slu_conv2d_h8_fwd(const slu_conv_h8_desc* desc, slu_stream_t stream);
/* name of the kernel instantiation the call above launches (as rocprofv3 prints it), by the same rules as slu_conv2d_kernel_name
 * (96 bytes hold every name) */
int slu_conv2d_h8_kernel_name(const slu_conv_h8_desc* desc, char* buf, size_t n);
/* ---- h8 layout and pooling around the convs: layout_h8.hip ---------------------------------------------------------------------- */
/* fp32 NCHW <-> h8 (set_model_inputs' tensor on the way in, utils/inputs.py:4-34; scale [N][C] optional) */
int slu_nchw_to_h8(const float* x, const float* scale, void* y, int N, int C, int H, int W, slu_stream_t stream);
int slu_h8_to_nchw(const void* x, float* y, int N, int C, int H, int W, slu_stream_t stream);
/* AvgPool2d(3, 2, 1) of x * scale[n][c] (SalsaNext.py:69,98-101); in_batch > 0: x holds in_batch images shared by all n */
int slu_avgpool3s2_h8(const void* x, const float* scale, void* y, int N, int in_batch, int G, int H, int W, slu_stream_t stream);
/* nn.PixelShuffle(2) (SalsaNext.py:143): y[n][c][2h+i][2w+j] = x[n][4c+2i+j][h][w] * scale_in[n][4c+2i+j] * scale_out[n][c];
 * x: h8 with Gin blocks at HxW; y: h8 with ceil(2 Gin / 8) blocks at 2Hx2W; scales fp32 [N][8 Gin] / [N][2 Gin] or NULL */
int slu_pixel_shuffle_h8(const void* x, const float* scale_in, const float* scale_out, void* y, int N, int Gin, int H, int W,
                         slu_stream_t stream);

/* ---- h8 data movement of the ResNet-FPN model (models/semanticFCN.py): fpn_h8.hip ------------------------------------------ */
/* MaxPool2d(3, 2, 1) (the stem's backbone.maxpool, semanticFCN.py:149): x h8 [N][G][H][W][8] -> y h8 [N][G][ceil(H/2)][ceil(W/2)][8];
 * taps outside the image are -inf (never chosen), pad channels stay 0 */
int slu_maxpool3s2_h8(const void* x, void* y, int N, int G, int H, int W, slu_stream_t stream);
/* Space-to-depth by 2 ahead of a stage's stride-2 convs (semanticFCN.py:309-313 + torchvision BasicBlock.conv1 / downsample[0]):
 * x h8 [N][G][H][W][8] (H, W even) -> y h8 [N][4 G][H/2][W/2][8], phase-major: channel (2 p + q) 8 G + c = x[c][2 y + p][2 x + q], so the
 * 3x3 / stride 2 / pad 1 conv is the (2,1,1) conv of y, and y00 (h8 [N][G][H/2][W/2][8] or NULL) = phase (0, 0) on its own, which the
 * 1x1 / stride 2 downsample conv reads as a plain 1x1.  meta != NULL: channels C - m .. C - 1 of x are replaced on the way by
 * meta[n][.][f (2 y + p)][f (2 x + q)] rounded to fp16 -- torch.cat([x[:, :-m], F.interpolate(meta, scale_factor=1/f, mode="nearest")], 1)
 * (semanticFCN.py:283-285) -- with meta fp32 [N][m][f H][f W], f in {1, 2, 4, 8}, 0 < m <= C, 8 (G - 1) < C <= 8 G */
int slu_space_to_depth2_h8(const void* x, const float* meta, int m, int C, int f, void* y, void* y00, int N, int G, int H, int W,
                           slu_stream_t stream);
/* The tail of AttentionModule.forward (semanticFCN.py:25-40) in one launch: tv = h8 [N][2 C / 8][H][W][8], the output of ONE 1x1 conv with
 * the stacked weights [W_q + W_k ; W_v] (channels 0 .. C - 1 = t = q + k, C .. 2 C - 1 = v).  Per image row:
 * s[w] = b_a[0] + sum_c w_a[c] tanh(t[c][w]) in fp32, p = softmax_w(s), out[c][w] = v[c][w] p[w] rounded to fp16 once.
 * w_a fp32 [C], b_a fp32 [1] (device memory); out h8 [N][C / 8][H][W][8]; C % 8 == 0, W <= 4096 */
int slu_attention_row_h8(const void* tv, const float* w_a, const float* b_a, void* out, int N, int C, int H, int W, slu_stream_t stream);
/* ConvTranspose2d(kernel = stride = s) (upsample_layer_x2 / x3 / x4, semanticFCN.py:230-232) after its 1x1 conv: y = h8
 * [N][s s Cout / 8][H][W][8] with channels ordered (i, j, cout), Cout % 8 == 0, so every output record is a whole input record:
 * out[n][g_off + g][s h + i][s w + j] = y[n][(i s + j) Cout / 8 + g][h][w], out = h8 [N][Gtot][s H][s W][8] (a block slice of the
 * concatenated up-sampled maps that decoder_semantic reads); s in {2, 4, 8} */
int slu_depth_to_space_h8(const void* y, void* out, int N, int Cout, int s, int H, int W, int Gtot, int g_off, slu_stream_t stream);
/* The end of decoder_semantic (ConvTranspose2d(k 4, s 2, p 1) + ELU, semanticFCN.py:244-245, and the + 1 of forward's return) after its 3x3 conv to
 * 4 `classes` sub-pixel channels ordered (class, i, j): out[n][c][2 h + i][2 w + j] = elu(y[n][4 c + 2 i + j][h][w]) + 1;
 * y = h8 [N][ceil(4 classes / 8)][H][W][8], out fp32 NCHW [N][classes][2 H][2 W] */
int slu_depth_to_space2_elu_h8(const void* y, float* out, int N, int classes, int H, int W, slu_stream_t stream);

/* ---- h8 forms of what `semanticFCN_opt` puts between its convs (baselines/Reichert/semanticFCN_opt.py): fpn_opt_h8.hip -------------
 * All tensors h8 [N][G][H][W][8] fp16 with zero pad channels and 16-byte aligned bases; fp32 arithmetic (fp64 sums in GroupNorm), every
 * stored value rounded to fp16 once; no float atomics: two runs of a call give the same bits.
 * slu_bilinear_upsample_h8: F.interpolate(x, scale_factor = s, mode = 'bilinear', align_corners = False) (UpsampleBlock :24-27):
 *   x [N][G][H][W][8] -> y [N][G][s H][s W][8]; source coordinate (dst + 0.5) / s - 0.5 clamped at 0, upper neighbour clamped at H - 1 /
 *   W - 1; s in {2, 4, 8} (SLU_EINVAL otherwise).
 * slu_groupnorm_stats_h8: mean and 1 / sqrt(var + eps) (biased variance) per (image, group) of the STORED fp16 values of x [N][ceil(C/8)][HW][8]
 *   -> mean / rstd fp32 [N groups].  The values and their squares are summed exactly in fp64 (per-workgroup partials in `workspace`,
 *   slu_groupnorm_stats_h8_workspace_bytes(N, C, HW) bytes, 8-byte aligned; then one wave per group in a fixed order), so the variance
 *   survives |mean| >> std.  C / groups in {1, 2, 4, 8}: a group lies inside one record (every GroupNorm resnet18 / resnet34 build is 1, 2
 *   or 4 wide); anything else is SLU_EUNSUPPORTED.
 * slu_groupnorm_apply_h8: out[n][g_off + g] = (x - mean) * rstd * gamma[c] + beta[c], max(., 0) if relu, into blocks [g_off, g_off + ceil(C/8))
 *   of out [N][Gtot][HW][8] (the three UpsampleBlocks share one buffer, as slu_depth_to_space_h8's callers); gamma / beta fp32 [C] or NULL;
 *   pad channels of the last block are written 0; out == x is allowed when Gtot == ceil(C/8) and g_off == 0 (SLU_EINVAL otherwise).
 * slu_spatial_softmax_gate_h8: SpatialAttention's gate (:80-85): w = softmax(score[n] over H W) in fp32, out = x w + x.  score fp32 [N][HW]
 *   (the fp32 NCHW output of the `score` conv); stats fp32 [2 N] scratch (max, 1 / sum), reduced by one workgroup per image. */
int slu_bilinear_upsample_h8(const void* x, void* y, int N, int G, int H, int W, int s, slu_stream_t stream);
size_t slu_groupnorm_stats_h8_workspace_bytes(int N, int C, int HW);
int slu_groupnorm_stats_h8(const void* x, int N, int C, int HW, int groups, float eps, float* mean, float* rstd, void* workspace,
                           slu_stream_t stream);
int slu_groupnorm_apply_h8(const void* x, const float* mean, const float* rstd, const float* gamma, const float* beta, int relu, void* out, int N,
                           int C, int HW, int groups, int Gtot, int g_off, slu_stream_t stream);
int slu_spatial_softmax_gate_h8(const void* x, const float* score, float* stats, void* out, int N, int C, int HW, slu_stream_t stream);

/* Fused tail of a SalsaNext block on the h8 path (ResBlock.conv4 + conv5, SalsaNext.py:59-68; UpBlock.conv3 + conv4, :157-167):
 *   a3  = bnA_a * actA(conv2x2_dil2_pad1(a2) + biasA) + bnA_b          (kept on chip, rounded to fp16 like the stored tensor would be)
 *   out = [resid +] bnB_a * actB(conv1x1(cat(a1, a2, a3)) + biasB) + bnB_b
 * a1, a2, resid, out: h8 [N][C/8][H][W][8]; w2x2 = slu_pack_conv_weight_h8 of [C][C][2][2]; w1x1 = the same of [C][3C][1][1].
 * C in {32, 64, 128} (slu_conv_tail_h8_supported); anything else: run the two layers through slu_conv2d_h8_fwd. */
typedef struct slu_conv_tail_h8_desc {   /* HOST struct */
  const void *a1, *a2;
  int32_t N, H, W, C;
  const void *w2x2, *w1x1;
  const float *biasA, *bnA_a, *bnA_b;   /* [C] fp32 or NULL */
  int32_t hasactA;
  float slopeA;
  const float *biasB, *bnB_a, *bnB_b;
  int32_t hasactB;
  float slopeB;
  const void* resid;
  void* out;
  /* shortcut mode (exclusive with resid): the residual is LeakyReLU(conv1x1(sc_x) + sc_bias), rounded to fp16 -- the shortcut branch of a
   * ResBlock (SalsaNext.py:52-53) computed inside the tail from the block's input instead of being written and read back.
   * sc_x: h8 [N][sc_cin/8][H][W][8]; sc_w = slu_pack_conv_weight_h8 of [C][sc_cin][1][1]; slu_conv_tail_h8_shortcut_supported(C, sc_cin). */
  const void *sc_x, *sc_w;
  const float* sc_bias;
  int32_t sc_cin, sc_hasact;
  float sc_slope;
} slu_conv_tail_h8_desc;
int slu_conv_tail_h8_supported(int C, int H, int W);
int slu_conv_tail_h8_shortcut_supported(int C, int sc_cin);
int slu_conv_tail_h8_fwd(const slu_conv_tail_h8_desc* desc, slu_stream_t stream);
/* name of the kernel instantiation the call above launches, by the same rules as slu_conv2d_kernel_name */
int slu_conv_tail_h8_kernel_name(const slu_conv_tail_h8_desc* desc, char* buf, size_t n);

/* Fused ResContextBlock on the h8 path (SalsaNext.py:10-39: conv1 1x1 + act -> shortcut; conv2 3x3 + act + bn1; conv3 3x3 dil 2 +
 * act + bn2; + shortcut), the three full-resolution blocks at the head of the network:
 *   s = act(conv1x1(x) + bias1);  a1 = bn1(act(conv3x3_pad1(s) + bias2));  out = s + bn2(act(conv3x3_dil2_pad2(a1) + bias3))
 * s and a1 stay on chip (rounded to fp16 exactly where the three separate slu_conv2d_h8_fwd launches would store them).
 * x: h8 [N][ceil(Cin/8)][H][W][8]; out: h8 [N][4][H][W][8]; w1 / w2 / w3 = slu_pack_conv_weight_h8 of [32][Cin][1][1] / [32][32][3][3] /
 * [32][32][3][3]; act = LeakyReLU(slope), 0 <= slope <= 1.  Cin <= 32, C == 32 (slu_ctx_block_h8_supported).
 * nbatch > 0: x holds nbatch images and output image n is the block of x[n % nbatch] (N a multiple of nbatch): the T stacked passes of an
 * MC-dropout evaluation read the B distinct input images in place instead of T copies of them. */
typedef struct slu_ctx_block_h8_desc {   /* HOST struct */
  const void* x;
  int32_t N, H, W, Cin, C;
  const void *w1, *w2, *w3;
  const float* bias1;                    /* [32] fp32 or NULL */
  const float *bias2, *bn1_a, *bn1_b;
  const float *bias3, *bn2_a, *bn2_b;
  float slope;
  void* out;
  int32_t nbatch;                        /* 0: x holds N images */
} slu_ctx_block_h8_desc;
int slu_ctx_block_h8_supported(int Cin, int C, int H, int W);
int slu_ctx_block_h8_fwd(const slu_ctx_block_h8_desc* desc, slu_stream_t stream);

/* Segmentation head + MC-dropout reduction in one pass on the h8 path (SalsaNext.py:213 + trainer.py:1143-1154):
 * x: h8 [T*B][G][HW][8], pass-major (image t*B + b = pass t of scan b), 8 G = input channels of the head (G in {2, 4, 8});
 * wpack = slu_pack_conv_weight_h8 of the head's [C][8 G][1][1] weight (C <= 32); bias [C] or NULL.  Outputs as slu_mc_reduce:
 * p_bar fp32 [B][C][HW], h_norm / mi_norm fp32 [B][HW], preds int64 [B][HW].  HW % 32 == 0. */
int slu_head_mc_h8(const void* x, int T, int B, int G, int HW, const void* wpack, const float* bias, int C, float eps, float* p_bar,
                   float* h_norm, float* mi_norm, int64_t* preds, slu_stream_t stream);

/* ---- Dirichlet head (the reference's default loss path, configs/SemanticKitti_default.yaml:10) ---------------
 * alpha = 1 + softplus(scale / T) * softmax(shape) + eps   (probability_helper.py:89-105; trainer.py:533-535 splits the C+1
 *   output channels into shape = outputs[:, :C] and scale = outputs[:, C:C+1], hence the batch strides in elements)
 * alpha0 = sum_c alpha + eps, p_hat = alpha / alpha0        (trainer.py:537-538)
 * entropy   = -sum_c p_hat log(p_hat + eps)                 (get_predictive_entropy :116-121; divide by ln C for _norm :148-153)
 * aleatoric = -sum_c p_hat (digamma(alpha+1) - digamma(alpha0+1))   (get_aleatoric_uncertainty :124-130); epistemic = entropy - aleatoric
 * preds = argmax_c alpha.  Every output pointer may be NULL.  C <= 32. */
int slu_dirichlet_head(const float* shape_logits, long long shape_batch_stride, const float* scale_logits, long long scale_batch_stride,
                       int B, int C, int HW, float temperature, float eps, float* alpha, float* p_hat, float* entropy, float* aleatoric,
                       int64_t* preds, slu_stream_t stream);
/* the same uncertainty measures from a given alpha [B, C, H, W] */
int slu_dirichlet_uncertainty(const float* alpha, int B, int C, int HW, float eps, float* p_hat, float* entropy, float* aleatoric,
                              int64_t* preds, slu_stream_t stream);

/* ---- AUROC of error detection (metrics/auroc.py:36-78) -----------------------------------------------------------
 * slu_auroc_scores: per pixel, probabilities by mode (0 alpha: a / (sum a + eps); 1 logits: softmax; 2 probs: clamp >= 0, renormalise,
 *   auroc.py:36-45), prediction = argmax, uncertainty score by score_kind (0 entropy, 1 entropy_norm, 2 mi, 3 mi_norm, 4 1-maxprob;
 *   mi / mi_norm are the Dirichlet mutual information for mode alpha and fall through to the plain entropy otherwise, :47-63) or
 *   score_override [B,H,W] verbatim; flags[pix] = 0 correct / 1 error / 2 label == ignore_index (has_ignore).  preds [B,C,H,W], C <= 32.
 * slu_auroc_compute: AUROC of `n` samples (score, is_error in {0,1}) exactly as :65-78 (sort by score descending, trapezoid over the
 *   ROC) = sum over negatives of #positives ranked before it / (P N); out3 = {auroc (NaN if P or N is 0), P, N}; optionally the
 *   samples in sorted order (for ROC curves).  The order among equal scores is arbitrary (as numpy's argsort in the reference). */
int slu_auroc_scores(const float* preds, const int64_t* labels, const float* score_override, int B, int C, int HW, int mode, int score_kind,
                     int has_ignore, int64_t ignore_index, float eps, float* scores, uint8_t* flags, slu_stream_t stream);
size_t slu_auroc_workspace_bytes(long long n);
int slu_auroc_compute(const float* scores, const uint8_t* is_error, long long n, void* workspace, size_t workspace_bytes, double* out3,
                      float* sorted_scores, uint8_t* sorted_is_error, slu_stream_t stream);

/* ---- AURC / E-AURC of selective prediction (metrics/aurc.py:7-45, :60-120) ----------------------------------------
 * slu_aurc_samples: per pixel, prediction = first argmax of probs [B,C,H,W] as given (no renormalisation), C <= 32; conf = the max
 *   probability (use_max_prob_confidence), else 1 - clamp(ent_mc, 0, 1) when ent_mc [B,H,W] is given, else
 *   1 - clamp(H / log C, 0, 1) with H = -sum max(p, 1e-12) log max(p, 1e-12); flags[pix] = 0 correct / 1 error / 2 label == ignore_index.
 * slu_aurc_compute: `n` samples (conf, is_error in {0,1}) sorted ascending by conf, stable (equal confidences keep their sample order;
 *   -0.0 == +0.0).  A curve point sits at the first element of every group of equal confidences among positions 0..n-2 (s_1 < ... < s_m):
 *   R_0 = E/n, R_k = (E - e_{s_k}) / (n-1-s_k), cov_k = (n-1-s_k)/n, AURC = trapezoid over the points with weights (s_k - s_{k-1})/n plus
 *   the tail R_m (n-2-s_m)/n, AURC_opt = (1/n) sum_{j<=E} j / (n-E+j).  out6 = {AURC, EAURC, AURC_opt, E, m, s_m} (s_m = -1 when m = 0);
 *   recalls[j] = e_{m_j - 1} / max(E, 1), m_j = max(1, int(n ks[j] / 100)), ks a HOST array of nks <= 16 percentages; optionally the
 *   curve points 0..m (curve_cov / curve_risk, fp64, room for n entries, both or neither) and the samples in sorted order.  Every sum is
 *   fp64 in a fixed order: the result is the same bits run to run.  n < 2^31. */
int slu_aurc_samples(const float* probs, const int64_t* labels, const float* ent_mc, int B, int C, int HW, int64_t ignore_index,
                     int use_max_prob_confidence, float* conf, uint8_t* flags, slu_stream_t stream);
size_t slu_aurc_workspace_bytes(long long n);
int slu_aurc_compute(const float* confids, const uint8_t* is_error, long long n, void* workspace, size_t workspace_bytes,
                     const double* ks, int nks, double* out6, double* recalls, double* curve_cov, double* curve_risk,
                     float* sorted_confids, uint8_t* sorted_is_error, slu_stream_t stream);

/* ---- accuracy vs uncertainty bins (models/evaluator.py:640-749 UncertaintyAccuracyAggregator) ---------------------
 * slu_ua_samples: u_out = clamp(uncertainty, 0, 1); flags = 1 label == pred / 0 otherwise / 2 label in ignore_ids (:659-673).
 * slu_binned_counts: count[b] += #samples in bin b, n_correct[b] += #correct ones, bins as np.histogram(u, bins=edges) (:733-739):
 *   [e_b, e_b+1), the last one closed, values outside [e_0, e_K] dropped; edges float32 [n_bins + 1] on the device, n_bins <= 256;
 *   count / n_correct int64 [n_bins], accumulated (zero them first). */
int slu_ua_samples(const int64_t* labels, const int64_t* preds, const float* uncertainty, long long n, const int64_t* ignore_ids, int n_ignore,
                   float* u_out, uint8_t* flags, slu_stream_t stream);
int slu_binned_counts(const float* u, const uint8_t* correct, long long n, const float* edges, int n_bins, int64_t* count, int64_t* n_correct,
                      slu_stream_t stream);

/* ---- ECE sample buffers (metrics/ece.py:55-111,115-140 ECEAggregator with max_samples / binning='adaptive') ----------
 * slu_ece_samples: per pixel conf = clamp(max_c p_c, 0, 1) with p by mode (0 alpha: a / (sum a + eps); 1 logits: softmax; 2 probs:
 *   clamp >= 0, / max(sum, eps); ece.py:55-64) and flags = 1 argmax == label / 0 otherwise / 2 label == ignore_index (has_ignore)
 *   (:75-84).  preds [B,C,HW], C <= 32; conf f32 [B,HW], flags u8 [B,HW].
 * slu_binned_stats: slu_binned_counts plus sum_u[b] += sum of u over bin b (f64): the three np.histogram calls of :136-140. */
int slu_ece_samples(const float* preds, const int64_t* labels, int B, int C, int HW, int mode, int has_ignore, int64_t ignore_index, float eps,
                    float* conf, uint8_t* flags, slu_stream_t stream);
int slu_binned_stats(const float* u, const uint8_t* correct, long long n, const float* edges, int n_bins, int64_t* count, int64_t* n_correct,
                     double* sum_u, slu_stream_t stream);

/* ---- per-class sample lists (models/evaluator.py:211-232 UncertaintyPerClassAggregator.update) --------------------
 * out_values = [values[labels == 0] ..., values[labels == 1] ..., ...] in scan order inside each class (what the reference's boolean
 * masks on host copies return), counts int64 [C] = samples per class; labels outside [0, C) are dropped.  out_values holds n floats;
 * C <= 32, n < 2^32. */
size_t slu_group_by_class_workspace_bytes(long long n);
int slu_group_by_class(const int64_t* labels, const float* values, long long n, int C, float* out_values, int64_t* counts, void* workspace,
                       size_t workspace_bytes, slu_stream_t stream);

/* ---- temperature scaling (models/temp_scaling.py:26-33,78,88-104 the cache; :142-154,158-170 the objective; DESIGN "Temperature
 * scaling on the device") ---------------------------------------------------------------------------------------------------------
 * slu_calib_rows: the calibration cache of one batch.  out [B,C,HW] fp32 of `kind` 0 logits / 1 probs / 2 log-probs; per pixel
 *     kind 0: m = max_c x_c, e_c = exp(x_c - m), p_c = e_c / sum_c e_c (the softmax form, sum in class order), row_c = logf(max(p_c, 1e-12f))
 *     kind 1: row_c = logf(max(x_c, 1e-12f))              kind 2: p_c = exp(x_c), row_c = logf(max(p_c, 1e-12f))
 *   p_c is an fp32 value, but e_c, their sum and the quotient are evaluated in fp64 and rounded once (log p near 0 magnifies every
 *   ulp of p), and so are exp and logf: a row is the correctly rounded logarithm of the correctly rounded probability.
 *   The pixels with label != ignore_index (every pixel when !has_ignore) are appended in (b, h, w) order -- what the reference's
 *   boolean mask returns -- at row count[0]: rows [cap, C] fp32 row-major, row_labels [cap] int64, then count[0] += their number
 *   (count: DEVICE int64, zero it before the first batch).  A row at or past `cap` is dropped, never written: count[0] > cap afterwards
 *   tells.  Plain launches (valid pixels per 256-pixel block, their scan by one workgroup, the scatter; rows leave through LDS in
 *   256-byte segments); no workgroup waits on another.  C <= 32 (SLU_EUNSUPPORTED above), B HW < 2^31.
 * slu_temp_nll: the objective of the fit and its derivative for the rows i = idx[j], j < M (idx DEVICE int64; NULL: i = j < N, M ignored).
 *   With x = rows[i], y = row_labels[i]:
 *     T = max(expf(log_T[0]), 1e-3f), an fp32 value (the exponential correctly rounded),  s_c = x_c / T,  m = max_c s_c,
 *     S = sum_c exp(s_c - m) in class order,  p_c = exp(s_c - m) / S
 *     loss = m + log(S) - s_y
 *     g    = (x_y - sum_c p_c x_c) / T = d loss / d log_T, evaluated as sum_c p_c (x_y - x_c) / T;   g = 0 where expf(log_T[0]) < 1e-3f
 *            (the sub-gradient of clamp_min)
 *   Everything after T is fp64 on the fp32 rows: an fp32 row is about as far from the exact value as the reference's own fp32
 *   evaluation, and the sum over the rows of either can cancel to a tenth of that (DESIGN).
 *   loss_sum[0] = sum loss, g_sum[0] = sum g (fp64: per-thread, then the wave's butterfly, the workgroup's four waves in order, one
 *   partial per workgroup, and one workgroup that adds the partials in index order: no floating-point atomics, the same bits run to
 *   run); bad[0] = rows with y outside [0, C) or i outside [0, N): they contribute nothing.  log_T is read on the DEVICE.  All three
 *   outputs are overwritten.  C <= 32. */
size_t slu_calib_rows_workspace_bytes(int B, int HW);
int slu_calib_rows(const float* out, int kind, const int64_t* labels, int B, int C, int HW, int has_ignore, int64_t ignore_index, float* rows,
                   int64_t* row_labels, long long cap, int64_t* count, void* workspace, size_t workspace_bytes, slu_stream_t stream);
size_t slu_temp_nll_workspace_bytes(long long n);
int slu_temp_nll(const float* rows, const int64_t* row_labels, long long N, int C, const int64_t* idx, long long M, const float* log_T,
                 double* loss_sum, double* g_sum, int64_t* bad, void* workspace, size_t workspace_bytes, slu_stream_t stream);

/* ---- Tversky loss (models/losses.py:74-128, the 'Tversky' loss branch trainer.py:497-503) -----------------------
 * valid = 0 <= y < C and (no ignore or y != ignore_index); p by model_act (0 logits: softmax, 1 probs, 2 log_probs: exp);
 * per class over valid pixels S = sum p, TP = sum p [y = c], N = #[y = c];  tversky = (TP + s) / (TP + alpha (S - TP) + beta (N - TP) + s);
 * loss = mean (reduction 0) / sum (1) / per class (2) of 1 - tversky; 0 when no pixel is valid.
 * fwd: sums double [3][C] (S | TP | N, zeroed inside), coef float [2][C] (backward coefficients), loss float [1] or [C], any_valid [1].
 * bwd: grad_x [B,C,H,W] = d loss / d x through the activation; grad_out = upstream gradient (DEVICE, [1] or [C], NULL = 1). */
int slu_tversky_fwd(const float* x, const int64_t* labels, int B, int C, int HW, int model_act, int has_ignore, int64_t ignore_index, float alpha,
                    float beta, float smooth, int reduction, double* sums, float* coef, float* loss, float* any_valid, slu_stream_t stream);
int slu_tversky_bwd(const float* x, const int64_t* labels, int B, int C, int HW, int model_act, int has_ignore, int64_t ignore_index, float alpha,
                    float beta, const float* coef, const float* grad_out, int grad_out_per_class, float* grad_x, slu_stream_t stream);

/* ---- per-pixel Dirichlet losses (losses/dirichlet_losses.py:73-221,317-385, losses/regularizers.py:291-389) -----
 * loss = sum over valid pixels (label != ignore_index, 0 <= label < C) of v(alpha[:, pixel], label) / #valid, with
 *   kind 0 NLLDirichletCategorical: -(log(a_y + eps) - log(a0 + eps))          kind 1 DigammaDirichletCE: psi(a0) - psi(a_y)
 *   kind 2 BrierDirichlet: sum_i E[p_i^2] - 2 p_y + 1 (param = s_ref, < 0: alpha0)   kind 3 DirichletMSELoss (Sensoy eq. 5)
 *   kind 4 KL_offClasses_to_uniform (with_conf_weighting = False): KL(Dir(alpha~) || Dir(1)), true class replaced by 1.
 * fwd: sum (double[1]) and count (int64[1]) are zeroed and accumulated; the caller divides (0 valid pixels: loss 0).
 * bwd: grad_alpha [B,C,H,W] = gscale[0] * d v / d alpha at valid pixels, 0 elsewhere; gscale = upstream gradient / count (DEVICE). */
int slu_dirichlet_loss_fwd(const float* alpha, const int64_t* labels, int B, int C, int HW, int kind, float param, float eps, int has_ignore,
                           int64_t ignore_index, double* sum, int64_t* count, slu_stream_t stream);
int slu_dirichlet_loss_bwd(const float* alpha, const int64_t* labels, int B, int C, int HW, int kind, float param, float eps, int has_ignore,
                           int64_t ignore_index, const float* gscale, float* grad_alpha, slu_stream_t stream);

/* The same pass with a parameter vector (HOST floats) and the two gated regularisers of the Dirichlet path:
 *   kind 5 ComplementKLUniform (losses/dirichlet_losses.py:228-314): w(p_y) * KL(p_off / (1 - p_y) || U); params = {gamma, tau, sigma,
 *          s_target (< 0: no evidence gate), normalize (0/1), detach_uncert (0/1)}; mean over the valid pixels; 0 when C <= 2.
 *   kind 6 WrongLowEvidence (losses/regularizers.py:218-289): gate * relu(ln a0 - ln(C + s_low + eps))^2 with gate = [argmax != y] *
 *          sigmoid((p_max - p_y - margin) / k) (k = 0: hard margin; margin <= 0: no margin gate); params = {s_low, margin, k};
 *          the mean runs over sum(gate): fwd writes sums2 = {sum of values, sum of gates} and the caller divides by max(sums2[1], 1).
 * kinds 0-4 take params = {param} (or none).  bwd: gscale = upstream gradient / the forward's denominator (DEVICE). */
int slu_dirichlet_loss_fwd_ex(const float* alpha, const int64_t* labels, int B, int C, int HW, int kind, const float* params, int nparams, float eps,
                              int has_ignore, int64_t ignore_index, double* sums2, int64_t* count, slu_stream_t stream);
int slu_dirichlet_loss_bwd_ex(const float* alpha, const int64_t* labels, int B, int C, int HW, int kind, const float* params, int nparams, float eps,
                              int has_ignore, int64_t ignore_index, const float* gscale, float* grad_alpha, slu_stream_t stream);

/* ---- spherical projection of a point cloud into the range image (dataset/utils.py:61-67,288-349) ------------------
 * pc: float64 [N][C] (x, y, z, then any channels: intensity, label ...; the reference's dataloader concatenates to float64,
 * dataloader_semantic_KITTI.py:49).  Rows / columns by numpy.digitize on the reversed linspace bins (theta range = data min / max
 * when use_data_theta_range, else [theta_min, theta_max]; phi in [-pi, pi]); per pixel the NEAREST point survives (the reference
 * writes in descending range order); img float32 [H][W][C], zeros where no point fell; theta_range_out double[2] or NULL. */
size_t slu_spherical_projection_workspace_bytes(int N, int H, int W);
int slu_spherical_projection(const double* pc, int N, int C, int H, int W, int use_data_theta_range, double theta_min, double theta_max,
                             void* workspace, size_t workspace_bytes, float* img, double* theta_range_out, slu_stream_t stream);
/* The same with the remaining options of the reference function and the dataloaders' flip augmentation:
 *   bins_h: explicit row bins, float64 [H] on the device, strictly monotone (bins_increasing 0 / 1), rows = numpy.digitize(theta, bins_h) - 1
 *           (dataset/utils.py:326-327,334; NULL: the reversed linspace of the theta range);
 *   keep_farthest: sort_largest_first=True of the reference -- points are then written in ASCENDING range order, so the farthest
 *           point of a pixel survives (:301-304);
 *   flip: write the image with reversed columns and negated y (dataloader_semantic_KITTI.py:72-74). */
int slu_spherical_projection_ex(const double* pc, int N, int C, int H, int W, int use_data_theta_range, double theta_min, double theta_max,
                                const double* bins_h, int bins_increasing, int keep_farthest, int flip, void* workspace, size_t workspace_bytes,
                                float* img, double* theta_range_out, slu_stream_t stream);

/* ---- the two ends of the dataloader's __getitem__ around the projection (dataloader_semantic_KITTI.py:31-99) --------
 * slu_kitti_decode: xyzi float32 [N][4] (the .bin file), label uint32 [N] (the .label file; low 16 bits = semantic id), lut int32
 *   [lut_size] = dataset/definitions.py id_map (-1 where the dict has no key) -> pc float64 [N][5] = (x, y, z, intensity, class);
 *   rotate != 0: xyz @ Rz with the given cosine / sine (rotate_z, dataset/utils.py:4-18).  bad_count int32[1] (zero it first) counts
 *   labels without a LUT entry (the reference raises KeyError).
 * slu_range_image_split: projected image float32 [H][W][C >= 5] (x, y, z, intensity, class) and optionally its normals [H][W][3] ->
 *   range [H][W] = |xyz|, reflectivity [H][W], xyz [3][H][W], normals_chw [3][H][W], labels int64 [H][W] (:83-99). */
int slu_kitti_decode(const float* xyzi, const uint32_t* label, int N, const int32_t* lut, int lut_size, int rotate, double cos_a, double sin_a,
                     double* pc, int32_t* bad_count, slu_stream_t stream);
/* SemanticKitti(resize=True) (dataloader_semantic_KITTI.py:61-62): cv2.resize(img, (OW, OH), interpolation=cv2.INTER_NEAREST) of the projected
 * [H][W][C] image -- source index min(floor(dst * src_size / dst_size), src_size - 1) per axis, OpenCV's definition (cv2 is absent from the
 * build image: unpinned like the normals); flip != 0: the dataloader's flip augmentation applied after it (:71-73). */
int slu_resize_nearest_hwc(const float* img, int H, int W, int C, float* out, int OH, int OW, int flip, slu_stream_t stream);
int slu_range_image_split(const float* img, const float* normals, int H, int W, int C, float* range, float* refl, float* xyz, float* normals_chw,
                          int64_t* labels, slu_stream_t stream);

/* ---- the other four dataloaders around the same projection (dataset/dataloader_semantic_{STF,THAB,CUDAL,WADS}.py) ------------------
 * slu_point_decode: slu_kitti_decode with every step optional.  records float32 [N][stride], stride 4 or 5 (STF reads 5-float records and
 *   uses the first 4, dataloader_semantic_STF.py:37); intensity_div > 0: intensity / intensity_div as a float32 division (:38), 0: none;
 *   mask_labels: label & 0xFFFF (KITTI / CUDAL / WADS) or the raw uint32 word (STF :43); lut NULL: the class is the label itself;
 *   remap_from >= 0: a class equal to it becomes remap_to, after the lut (STF remap_adverse_label, :55-56); clip != 0: valid[i] uint8 [N] = the
 *   float32 norm of np.linalg.norm(xyzi[:, 0:3], axis=-1) is >= clip_min (STF :49-54: taken BEFORE the rotation) -- the cloud keeps all N
 *   rows in file order, slu_spherical_projection_valid skips the rows whose flag is 0; rotate / cos_a / sin_a / pc / bad_count as in
 *   slu_kitti_decode.
 * slu_spherical_projection_valid: slu_spherical_projection_ex (nearest point, linspace rows) over the points with valid[i] != 0 only: the
 *   others take no part in the data theta range and win no pixel; empty_count int32[1] or NULL: += 1 when the data theta range is asked
 *   for and no point is valid (numpy's theta.min() raises there, dataset/utils.py:323). */
int slu_point_decode(const float* records, int stride, const uint32_t* label, int N, float intensity_div, int mask_labels, const int32_t* lut,
                     int lut_size, int remap_from, int remap_to, int clip, float clip_min, int rotate, double cos_a, double sin_a, double* pc,
                     uint8_t* valid, int32_t* bad_count, slu_stream_t stream);
int slu_spherical_projection_valid(const double* pc, const uint8_t* valid, int N, int C, int H, int W, int use_data_theta_range, double theta_min,
                                   double theta_max, int flip, void* workspace, size_t workspace_bytes, float* img, int32_t* empty_count,
                                   slu_stream_t stream);
/* slu_organised_scan: SemanticTHAB.__getitem__ up to the image (dataloader_semantic_THAB.py:35-59): records float32 [H*W][4] (16-byte
 *   aligned) and label uint32 [H*W] of an organised scan -> img float32 [H][W][5] = (x, y, z, intensity, lut[label & 0xFFFF]).  In the
 *   loader's order and precision: float64 image, flip (columns reversed, y negated, :52-55), np.roll by `shift` columns (any integer;
 *   rotate_equirectangular_image, dataset/utils.py:21-28), xyz @ Rz in float64 (:59), one rounding to float32.  range float32 [H][W] or
 *   NULL: the float64 norm of the float64 xyz rounded to float32, which is what the loader returns (:67,77). */
int slu_organised_scan(const float* records, const uint32_t* label, int H, int W, const int32_t* lut, int lut_size, int flip, long long shift,
                       int rotate, double cos_a, double sin_a, float* img, float* range, int32_t* bad_count, slu_stream_t stream);
/* slu_nonempty_rows: img[~np.all(np.linalg.norm(img, axis=-1) == 0, axis=1)] as a table (dataloader_semantic_WADS.py:125).  rows int32
 *   [2 H + 1]: rows[0] = H' = number of rows with a non-zero pixel, rows[1 .. H'] = their indices in ascending order (rows[H + 1 ..] scratch).
 * slu_resize_nearest_rows_hwc: slu_resize_nearest_hwc of the H' kept rows (:126-127): source row rows[1 + min(floor(dst * H' / OH), H' - 1)],
 *   H' read on the device; flip as there.  H' = 0 (cv2.resize raises): *no_row_count += 1 and the output is zeros. */
int slu_nonempty_rows(const float* img, int H, int W, int C, int32_t* rows, slu_stream_t stream);
int slu_resize_nearest_rows_hwc(const float* img, int H, int W, int C, const int32_t* rows, float* out, int OH, int OW, int flip,
                                int32_t* no_row_count, slu_stream_t stream);
/* slu_channel_max: key uint32[1] = the maximum of img[..., channel] over an [H][W][C] float32 image in an order-preserving integer form.
 * slu_range_image_split_ex: slu_range_image_split with range_in float32 [H][W] or NULL (given: copied instead of |xyz|, the THAB range) and
 *   refl_max_key (slu_channel_max of channel 3) or NULL (given: reflectivity / max(maximum, 1.0f) as a float32 division,
 *   dataloader_semantic_CUDAL.py:107). */
int slu_channel_max(const float* img, int H, int W, int C, int channel, uint32_t* key, slu_stream_t stream);
int slu_range_image_split_ex(const float* img, const float* normals, int H, int W, int C, const float* range_in, const uint32_t* refl_max_key,
                             float* range, float* refl, float* xyz, float* normals_chw, int64_t* labels, slu_stream_t stream);

/* ---- surface normals of the projected image (dataset/utils.py:30-58 build_normal_xyz; inference_ouster.py:70) ------
 * xyz: fp32 [H][W][channels >= 3] (x, y, z first); normals: fp32 [H][W][3] = -(d xyz/d col x d xyz/d row) / (|.| + 1e-10) with the 3x3
 * Scharr derivatives of OpenCV (cv2.Scharr(..., scale = 1 / norm_factor), BORDER_REFLECT_101). */
int slu_build_normals(const float* xyz, int H, int W, int channels, float norm_factor, float* normals, slu_stream_t stream);

/* ---- training path of the ResNet-FPN models (SURVEY 8(a) row a3 backward, 8(b) Autograd row; models/semanticFCN.py:266-354,
 * baselines/Reichert/semanticFCN_opt.py:366-455; trainer.py:783-786 calls loss.backward() on them): per-pixel / data-movement kernels of
 * the autograd nodes in semanticlidarunc_amd/fpn_autograd.py.  Dense fp32 NCHW tensors, device pointers.
 * slu_pointwise_{fwd,bwd}: op 0 = LeakyReLU(slope >= 0; 0 = nn.ReLU), 1 = tanh (AttentionModule, semanticFCN.py:32), 2 = ELU(alpha 1) + 1
 *   (decoder_semantic + 1, :352).  The backward takes the forward's OUTPUT y: dx = dy * f'(x(y)).
 * slu_maxpool3s2_bwd: nn.MaxPool2d(3, 2, 1) (stem, :149); the gradient goes to the FIRST maximum of a window in row-major order, as ATen does.
 * slu_nearest_down_bwd: backward of F.interpolate(mode='nearest', scale_factor=1/factor) (:283-285): dx [N][C][H][W] from dy [N][C][H/f][W/f].
 * slu_replace_tail_{fwd,bwd}: out = cat(x[:, :C-m], meta) (:309-313); dx (zero in the replaced channels) and / or dmeta may be NULL.
 * slu_row_softmax_mul_bwd: out = value * softmax_W(score) (:35-38); dscore [N][1][H][W] and / or dvalue may be NULL.  W <= 4096.
 * slu_depth_to_space_bwd: dx [N][Cout r r][H][W] from the channel slice [c_off, c_off + Cout) of dy [N][Ctot][H r][W r] (slu_depth_to_space).
 * slu_bilinear_upsample_bwd: backward of slu_bilinear_upsample (align_corners = False); dx [N][C][H][W] from dy [N][C][H s][W s].
 * slu_groupnorm_bwd: x, dy [N][C][HW]; mean / rstd [N groups] from slu_groupnorm_fwd; relu != 0: the forward applied ReLU and y is its output;
 *   dgamma / dbeta: float64 [C], ADDED to (zero them first), may be NULL.
 * slu_spatial_softmax_gate_bwd: backward of slu_spatial_softmax_gate with its stats [N][2]; workspace: float [N][HW]. */
int slu_pointwise_fwd(const float* x, float* y, size_t n, int op, float slope, slu_stream_t stream);
int slu_pointwise_bwd(const float* dy, const float* y, float* dx, size_t n, int op, float slope, slu_stream_t stream);
int slu_maxpool3s2_bwd(const float* x, const float* dy, float* dx, int N, int C, int H, int W, slu_stream_t stream);
int slu_nearest_down_bwd(const float* dy, float* dx, int N, int C, int H, int W, int factor, slu_stream_t stream);
int slu_replace_tail_fwd(const float* x, const float* meta, float* out, int N, int C, int m, int H, int W, slu_stream_t stream);
int slu_replace_tail_bwd(const float* dout, float* dx, float* dmeta, int N, int C, int m, int H, int W, slu_stream_t stream);
int slu_row_softmax_mul_bwd(const float* score, const float* value, const float* dout, float* dscore, float* dvalue, int N, int C, int H, int W,
                            slu_stream_t stream);
int slu_depth_to_space_bwd(const float* dy, float* dx, int N, int Cout, int H, int W, int r, int c_off, int Ctot, slu_stream_t stream);
int slu_bilinear_upsample_bwd(const float* dy, float* dx, int N, int C, int H, int W, int scale, slu_stream_t stream);
int slu_groupnorm_bwd(const float* x, const float* y, const float* dy, const float* gamma, const float* mean, const float* rstd, float* dx,
                      double* dgamma, double* dbeta, int N, int C, int HW, int groups, int relu, slu_stream_t stream);
int slu_spatial_softmax_gate_bwd(const float* x, const float* score, const float* stats, const float* dout, float* dx, float* dscore,
                                 float* workspace, int N, int C, int HW, slu_stream_t stream);

/* ---- all Dropout2d multipliers of one MC-dropout evaluation in one launch (SalsaNext.py:98,106,145,149,168; utils/mc_dropout.py:13-34) ----
 * A site is one nn.Dropout2d application: an [N][C] table of multipliers, 0 with probability p, else 1 / (1 - p); inactive sites give 1.
 * The draws are Philox4x32-10(key = seed, counter = offset + g / 4)[g % 4] for the g-th element of the call (sites in table order, `begin` =
 * first g of the site), i.e. a pure function of torch's generator state: the host reads (seed, offset) from the CUDA generator and advances
 * the offset by ceil(total draws / 4).  An output is an [N][C] table buf[begin ...] = product over its <= 3 sites:
 *   site_a[n][off_a + c] * site_b[n][off_b + c'] * site_c[n][off_c + c'],  c' = shuffled ? c / 4 : c  (stored channel c of a tensor read
 *   through PixelShuffle(2) feeds shuffled channel c / 4: UpBlock's dropout1 / dropout2 act on the shuffled tensor, SalsaNext.py:141-149);
 * a site index of -1 drops the factor.  shuffled == 2: the same values, written in the stored order of slu_h8_src.shuffle -- position
 * 8 (4 go + sub) + k holds the multiplier of channel c = 32 go + 4 k + sub (C a multiple of 32).
 * `sites`, `outs`: DEVICE arrays; outs sorted by `begin`; total = sum of N * C over the outputs. */
typedef struct slu_dropout_site {
  long long begin;
  int C, active;
  float p;
  int reserved;
} slu_dropout_site;
typedef struct slu_dropout_out {
  long long begin;
  int C, site_a, off_a, site_b, off_b, site_c, off_c, shuffled;
} slu_dropout_out;
int slu_dropout_draw(const slu_dropout_site* sites, int nsites, const slu_dropout_out* outs, int nout, int N, unsigned long long seed,
                     unsigned long long offset, float* buf, long long total, slu_stream_t stream);

/* ---- EfficientNetV2 blocks of the semanticFCN_opt encoder (baselines/Reichert/semanticFCN_opt.py:170-180,238-247,396-404;
 * the block structure is torchvision's efficientnet_v2_{s,m,l}: FusedMBConv / MBConv with depthwise 3x3, squeeze-excitation, SiLU) -----------
 * slu_dwconv3x3_fwd: depthwise 3x3, padding 1, stride 1 or 2, with the eval BatchNorm folded into w [C][9] / bias [C]; act 0 none, 3 SiLU.
 *   x [N][C][H][W] -> y [N][C][ceil(H/stride)][ceil(W/stride)].
 * slu_global_avgpool: mean over H W -> out [N][C] (SqueezeExcitation.avgpool).
 * slu_se_gate: scale [N][C] = sigmoid(w2 [C][S] . SiLU(w1 [S][C] . avg + b1) + b2)  (fc1 / fc2 of SqueezeExcitation are 1x1 convs on a 1x1 map);
 *   the scale reaches the block's projection conv as a per-(sample, channel) input multiplier (slu_conv_src.scale).
 * slu_dwconv3x3_wgrad (training, trainer.py:783-786 backward through the MBConv blocks): dw [C][9] = sum over (n, y, x) of dy[n][c][y][x] *
 *   x[n][c][y + i - 1][x + j - 1] for the stride-1 depthwise conv (a stride-2 one is run as stride 1 + sub-sampling in training); the data
 *   gradient is slu_dwconv3x3_fwd on dy with the nine taps reversed. */
int slu_dwconv3x3_wgrad(const float* x, const float* dy, float* dw, int N, int C, int H, int W, slu_stream_t stream);
int slu_dwconv3x3_fwd(const float* x, const float* w, const float* bias, float* y, int N, int C, int H, int W, int stride, int act, slu_stream_t stream);
int slu_global_avgpool(const float* x, float* out, int N, int C, int HW, slu_stream_t stream);
int slu_se_gate(const float* avg, const float* w1, const float* b1, const float* w2, const float* b2, float* scale, int N, int C, int S,
                slu_stream_t stream);

/* ---- What the encoder unit kernels below share (ShuffleNetV2 tail, SqueezeNet Fire and ceil pool, RegNetY sampling) -------------------------
 * slu_cat2: the input of a unit, the channel concatenation  src0[:, coff0 : coff0 + c0]  (+)  src1[:, :c1]  of dense NCHW fp32 tensors with
 * ct0 / ct1 stored channels at one H x W (src1 NULL, c1 = 0: one source); C = c0 + c1.  It is how a stage reads x[:, :-m] (+) meta_k, or half
 * of a tensor, in place.  c0 >= 1, 0 <= coff0, coff0 + c0 <= ct0, and with src1 1 <= c1 <= ct1: anything else is SLU_EINVAL.  The output of an
 * entry point that takes one must not overlap either stored tensor (SLU_EINVAL).
 * Packed weights: the A operand of v_mfma_f32_32x32x2_f32 as the kernels load it.  The image of W [R][K] (or [R][K][taps]) with K-chunk kc is
 * [ceil(R / 32)][taps][ceil(K / kc) * kc / 2][64] floats: lane l of (32-row block m, tap t, K-step k2) holds W[32 m + (l & 31)][2 k2 + (l >> 5)][t],
 * 0 outside the matrix.  slu_shuffle_tail_pack: W = wpw [Co][C], kc = 32.  slu_fire_pack: the images of wsq [S][Cin] (kc = 32), w1 [E1][S]
 * (kc = 16) and w3 [E3][S][9] (kc = 16, taps = 9), one after the other. */
typedef struct slu_cat2 {
  const float* src0;
  const float* src1;
  int32_t ct0, coff0, c0;
  int32_t ct1, c1;
} slu_cat2;                /* 40 bytes */

/* ---- ShuffleNetV2 unit tail (models/semanticFCN.py:181-190 and baselines/Reichert/semanticFCN_opt.py:227-236 build torchvision's
 * shufflenet_v2_x{0_5,1_0,1_5,2_0}; the unit is torchvision's InvertedResidual) ---------------------------------------------------------
 * slu_shuffle_tail_fwd: depthwise 3x3 (pad 1, stride 1 or 2) -> pointwise 1x1 -> ReLU with both eval BatchNorms folded in, stored through the
 * unit's concat + channel_shuffle(., 2), and optionally the copy of the pass-through half, in one launch:
 *
 *   y[n,j]               = relu( bpw[j] + sum_c wpw[j,c] * ( bdw[c] + sum_{a,b} wdw[c,3a+b] * src[n,c, s*oy-1+a, s*ox-1+b] ) )       j < Co
 *   out[n, 2j + parity]  = y[n,j]
 *   out[n, 2j]           = pass[n,j]       when pass != NULL (parity must then be 1)
 *
 * src is the slu_cat2 `in` at H x W, C = c0 + c1 channels.  out is [N][2 Co][Ho][Wo], Ho = ceil(H / stride), Wo likewise; the channels of the other
 * parity are left untouched when pass is NULL.  pass is [N][pass_ct][Ho][Wo] and its first Co channels are copied.  The depthwise result stays
 * on chip.  The pointwise product is exact fp32 (v_mfma_f32_32x32x2_f32) whatever the conv precision of the surrounding model; no atomics, so
 * results are bit-identical run to run.  wpack = slu_shuffle_tail_pack of wpw [Co][C] (slu_shuffle_tail_packed_floats(Co, C) floats; 0 =
 * unsupported).  Co <= 512, stride 1 / 2, N <= 65535, H W < 2^31; anything else is SLU_EUNSUPPORTED.  out must not overlap `in` or pass
 * (SLU_EINVAL). */
typedef struct slu_shuffle_tail_desc {   /* HOST struct */
  slu_cat2 in;
  int32_t N, H, W, stride;
  int32_t Co, parity;
  int32_t pass_ct;
  const float* wdw;      /* [C][9]  */
  const float* bdw;      /* [C]     */
  const float* wpack;
  const float* bpw;      /* [Co]    */
  const float* pass;
  float* out;
} slu_shuffle_tail_desc;
size_t slu_shuffle_tail_packed_floats(int co, int c);
int slu_shuffle_tail_pack(const float* w, int co, int c, float* out, slu_stream_t stream);
int slu_shuffle_tail_fwd(const slu_shuffle_tail_desc* d, slu_stream_t stream);

/* ---- SqueezeNet Fire module (models/semanticFCN.py:121-123,155-169 and baselines/Reichert/semanticFCN_opt.py:167-169,201-215 build torchvision's
 * squeezenet1_0; the unit is torchvision's Fire, and the network has no BatchNorm) -----------------------------------------------------------
 * slu_fire_fwd: squeeze 1x1 -> ReLU -> {expand 1x1, expand 3x3 / pad 1} -> ReLU -> concat in one launch:
 *
 *   s[n,k]        = relu( bsq[k] + sum_c wsq[k,c] * src[n,c] )                                       k < S
 *   out[n,j]      = relu( b1[j] + sum_k w1[j,k] * s[n,k] )                                           j < E1
 *   out[n,E1 + j] = relu( b3[j] + sum_{k,a,b} w3[j,k,a,b] * s[n,k, y-1+a, x-1+b] )                   j < E3
 *
 * src is the slu_cat2 `in` at H x W, Cin = c0 + c1 channels.  out is [N][E1 + E3][H][W].  The squeeze map lives in LDS with a one-pixel halo around a
 * 4 x 32 output tile and never goes to global memory; outside the image it is 0 (the padding of the 3x3 -- not relu(bsq), not the squeeze of a
 * clamped input), inside the image but outside the tile it is computed from the real input.  Every product is exact fp32
 * (v_mfma_f32_32x32x2_f32) whatever the conv precision of the surrounding model; no atomics, so results are bit-identical run to run.
 * wpack = slu_fire_pack of wsq [S][Cin], w1 [E1][S], w3 [E3][S][3][3] (slu_fire_packed_floats(Cin, S, E1, E3) floats, zero-filled outside the
 * matrices; 0 = unsupported).  Any Cin >= 1, 1 <= S <= 64, 1 <= E1, E3 <= 256, N <= 65535, H W < 2^31; anything else is SLU_EUNSUPPORTED.
 * slu_maxpool3s2_ceil_fwd: nn.MaxPool2d(3, 2, padding=0, ceil_mode=True) of the slu_cat2 `in` at H x W -> y [N][c0 + c1][Ho][Wo],
 * Ho = ceil((H - 3) / 2) + 1, Wo likewise; windows start at (2 oy, 2 ox) and are clipped at the far edge; H, W >= 3 (SLU_EINVAL below).  Not
 * slu_maxpool3s2_fwd (padding 1): for even H the output size is the same and the windows are shifted by one. */
typedef struct slu_fire_desc {   /* HOST struct */
  slu_cat2 in;
  int32_t N, H, W;
  int32_t S, E1, E3;
  int32_t reserved;
  const float* wpack;
  const float* bsq;      /* [S]  */
  const float* b1;       /* [E1] */
  const float* b3;       /* [E3] */
  float* out;
} slu_fire_desc;
size_t slu_fire_packed_floats(int cin, int s, int e1, int e3);
int slu_fire_pack(const float* wsq, const float* w1, const float* w3, int cin, int s, int e1, int e3, float* out, slu_stream_t stream);
int slu_fire_fwd(const slu_fire_desc* d, slu_stream_t stream);
int slu_maxpool3s2_ceil_fwd(const slu_cat2* in, float* y, int N, int H, int W, slu_stream_t stream);

/* ---- RegNetY block (models/semanticFCN.py:97-108,171-179 and baselines/Reichert/semanticFCN_opt.py:143-154 build torchvision's
 * regnet_y_{400mf,800mf,1_6gf,3_2gf}; the unit is torchvision's ResBottleneckBlock with a ReLU SqueezeExcitation) ---------------------------
 * slu_regnet_gconv_fwd: f.b -- grouped 3x3 conv, pad 1, stride 1 or 2, gw = 8 / 16 / 24 channels per group, with the eval BatchNorm folded
 * into the weights and bias, + ReLU, and the partial sums of the spatial mean of what it stores:
 *
 *   y[n, g gw + o, oy, ox] = relu( bias[g gw + o] + sum_{c < gw, a, b} w[g gw + o, c, a, b] * x[n, g gw + c, s oy - 1 + a, s ox - 1 + b] )
 *   psum[n, c, t]          = sum of y[n, c] over the pixels of output tile t            t < T = slu_regnet_gconv_tiles(H, W, stride)
 *
 * x is channels [coff, coff + C) of a dense NCHW fp32 tensor with ct stored channels at H x W; y is [N][C][Ho][Wo], Ho = ceil(H / stride), Wo
 * likewise; a stride-2 launch reads only the rows and columns it needs.  wg holds the weights as [C / gw][gw (c)][9 (tap)][gw (o)]: the
 * 9 gw weights that one input channel of a group feeds are consecutive.  Exact fp32 (fmaf chains) whatever the conv precision of the
 * surrounding model; no atomics: a tile's sum is reduced inside its workgroup in a fixed order, so y and psum are bit-identical run to run.
 * C a multiple of gw, N <= 65535, H W < 2^31; any other gw is SLU_EUNSUPPORTED.
 * slu_regnet_se_gate: mean[n, c] = inv_count * sum_t psum[n, c, t] (tile order), gate[n, c] = sigmoid(b2[c] + sum_s w2[c, s] *
 * relu(b1[s] + sum_c' w1[s, c'] * mean[n, c'])) -- fc1 [S][C], ReLU, fc2 [C][S], sigmoid of torchvision's SqueezeExcitation as RegNet builds
 * it (slu_se_gate is the SiLU form of EfficientNet).  psum [N][C][T]; T = 1 and inv_count = 1 take a plain [N][C] mean.  mean (optional,
 * [N][C]) receives the means.  Any S >= 1 and C >= 1 with (C + S) * 4 <= 64 KiB.  The gate reaches f.c as slu_conv_src.scale.
 * slu_regnet_sample2: y [N][c0 + c1][ceil(H / 2)][ceil(W / 2)] = in[:, :, ::2, ::2] of the slu_cat2 `in` at H x W -- what the 1x1 / stride-2
 * projection of a stage's first block reads, with the meta channels in place. */
int slu_regnet_gconv_tiles(int H, int W, int stride);
int slu_regnet_gconv_fwd(const float* x, int ct, int coff, const float* wg, const float* bias, float* y, float* psum, int N, int C, int gw, int H, int W,
                         int stride, slu_stream_t stream);
int slu_regnet_se_gate(const float* psum, int T, float inv_count, const float* w1, const float* b1, const float* w2, const float* b2, float* gate,
                       float* mean, int N, int C, int S, slu_stream_t stream);
int slu_regnet_sample2(const slu_cat2* in, float* y, int N, int H, int W, slu_stream_t stream);

/* ---- EfficientNetV2 MBConv middle (models/semanticFCN.py:124-135,192-201 builds torchvision's efficientnet_v2_{s,m,l}; the unit is torchvision's
 * MBConv: depthwise 3x3 + BatchNorm + SiLU, then a SqueezeExcitation with SiLU between its two layers) -----------------------------------------
 * slu_dwconv3x3_se_fwd: depthwise 3x3 conv, pad 1, stride 1 or 2, with the eval BatchNorm folded into the weights and bias, + SiLU, and the
 * partial sums of the spatial mean of what it stores:
 *
 *   y[n, c, oy, ox] = silu( bias[c] + sum_{a, b} w[c, 3 a + b] * x[n, c, s oy - 1 + a, s ox - 1 + b] )
 *   psum[n, c, t]   = sum of y[n, c] over the rows of output tile t                       t < T = slu_dwconv3x3_se_tiles(H, W, stride)
 *
 * x is a dense NCHW fp32 tensor at H x W, w [C][9], bias [C]; y is [N][C][Ho][Wo], Ho = ceil(H / stride), Wo likewise; psum is [N][C][T].  A tile
 * is a run of whole output rows (about 2048 outputs: an 8 x 256 plane is one tile), reduced inside its workgroup in a fixed order: no atomics,
 * so y and psum are bit-identical run to run.  y equals slu_dwconv3x3_fwd(act = SiLU) bit for bit.  16-byte loads where W % 4 == 0 and x is
 * 16-byte aligned, 16-byte stores where Wo % 4 == 0 and y is; any other width takes a scalar route.  N, C <= 65535, H W < 2^31, W up to about
 * 5000 (three input rows must fit the kernel's LDS): anything else is SLU_EUNSUPPORTED, and slu_dwconv3x3_se_tiles returns 0 for it.
 * slu_se_gate_psum: mean[n, c] = inv_count * sum_t psum[n, c, t] (tile order), scale[n, c] = sigmoid(b2[c] + sum_s w2[c, s] *
 * silu(b1[s] + sum_c' w1[s, c'] * mean[n, c'])) -- slu_se_gate reading the tile sums instead of a pooled vector.  fc1 [S][C], fc2 [C][S], both
 * biases required; T = 1 and inv_count = 1 take a plain [N][C] mean.  C <= 1536 and S <= 96 as slu_se_gate; anything else is SLU_EINVAL.  The
 * scale reaches the projection conv as slu_conv_src.scale. */
int slu_dwconv3x3_se_tiles(int H, int W, int stride);
int slu_dwconv3x3_se_fwd(const float* x, const float* w, const float* bias, float* y, float* psum, int N, int C, int H, int W, int stride,
                         slu_stream_t stream);
int slu_se_gate_psum(const float* psum, int T, float inv_count, const float* w1, const float* b1, const float* w2, const float* b2, float* scale,
                     int N, int C, int S, slu_stream_t stream);

/* ---- CENet ResNet-34 decoder (baselines/CENet/CENet_ResNet34.py:165-184) ------------------------------------------------------------------
 * Both use F.interpolate(mode = 'bilinear', align_corners = True): source coordinate = destination * (in - 1) / (out - 1), and 0 where
 * out == 1 or in == 1; the taps are found from the integer ratio exactly, so in == out returns the input bit for bit.
 * slu_bilinear_ac_cat: 1 .. 3 sources [N][C_k][h_k][w_k], each interpolated to H x W and written into channels [c_off_k, c_off_k + C_k) of the
 * dense [N][C_tot][H][W] buffer `out` in ONE launch (the three interpolations of :165-167 and their part of the torch.cat of :170); channels
 * outside the slices are left as they are.  `srcs` is a HOST array.  Slices that overlap or leave C_tot are SLU_EINVAL.  16-byte stores where
 * W % 4 == 0 and out is 16-byte aligned, scalar ones otherwise.  N * sum C_k <= 65535, H <= 1048560, sizes below 2^22 with
 * (out - 1) * (in - 1) < 2^31 per axis: anything else is SLU_EUNSUPPORTED.
 * slu_bilinear_ac_softmax: y [N][C][H][W] = softmax over C of the interpolation of the logits x [N][C][h][w] to H x W (h == H and w == W: plain
 * softmax); 1 <= C <= 32 (SLU_EINVAL above), N, H <= 65535.  The model's aux heads run their 1x1 conv on the low-resolution map and
 * interpolate the logits here: a 1x1 conv commutes with the interpolation because the four weights sum to 1, so the result equals the
 * reference's order (interpolate, conv, softmax) up to rounding, not bit for bit. */
typedef struct slu_bilinear_src {   /* HOST struct, 24 bytes */
  const float* ptr;   /* [N][C][h][w] */
  int32_t C, h, w;
  int32_t c_off;      /* first channel of `out` this source is written to */
} slu_bilinear_src;
int slu_bilinear_ac_cat(const slu_bilinear_src* srcs, int nsrc, float* out, int N, int C_tot, int H, int W, slu_stream_t stream);
int slu_bilinear_ac_softmax(const float* x, float* y, int N, int C, int h, int w, int H, int W, slu_stream_t stream);

/* ---- FIDNet ResNet34_point (baselines/FIDNet/ResNet.py:451-593, 145-170) ---------------------------------------------------------------------
 * slu_point_mlp: a chain of 1 .. 4 per-pixel 1x1 convs, each with bias and LeakyReLU, in ONE launch (the point-MLP stem of :469-502, 563-576 with
 * eval BatchNorm folded into the convs):
 *
 *   y = act( W_L . ... act( W_1 . x + b_1 ) ... + b_L )    per pixel;  act(v) = v > 0 ? v : slope * v, on the last layer only where act_last != 0
 *
 * x [N][C0][HW] -> out [N][widths[L - 1]][HW], HW the flattened pixel count of an image (there is no spatial structure).  `widths` is a HOST array
 * of the L layer widths; bias holds b_1 .. b_L one after the other (sum of the widths floats).  wpack holds, one after the other, the Packed-weights
 * images (above) of W_l [widths[l]][K_l] with K-chunk 16, each written by one slu_point_mlp_pack(w, cout, cin, out) call:
 * (cout / 32) * ceil(cin / 16) * 8 * 64 floats.  The intermediate maps stay in LDS as the next layer's B operand; the input and the last
 * layer's output are the only activations that touch global memory.  Every product is exact fp32 (v_mfma_f32_32x32x2_f32, a k-ordered fmaf
 * chain) whatever the conv precision of the surrounding model; no atomics, so results are bit-identical run to run.
 * 1 <= C0 <= 32, every width a multiple of 32 and at most 512, N <= 65535, HW < 2^31 - 1: anything else is SLU_EUNSUPPORTED (more than 4 layers:
 * SLU_EINVAL).
 * slu_bilinear_ac_sum: out [N][C][H][W] = sum over k of the align_corners = True interpolation of src_k [N][C][h_k][w_k] to H x W, 1 .. 3 sources
 * of the same C (c_off must be 0), the terms added in source order; the coordinates and the limits are slu_bilinear_ac_cat's, and one source at
 * the output size returns the input bit for bit.  `srcs` is a HOST array. */
int slu_point_mlp_pack(const float* w, int cout, int cin, float* out, slu_stream_t stream);
int slu_point_mlp(const float* x, const float* wpack, const float* bias, const int* widths, int nlayers, int N, int C0, long long HW, float slope,
                  int act_last, float* out, slu_stream_t stream);
int slu_bilinear_ac_sum(const slu_bilinear_src* srcs, int nsrc, float* out, int N, int C, int H, int W, slu_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SLU_H_ */
