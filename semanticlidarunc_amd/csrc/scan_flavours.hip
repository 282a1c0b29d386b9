// What the dataloaders of the other four datasets do around the projection that SemanticKitti's does not (src/dataset/
// dataloader_semantic_{STF,THAB,CUDAL,WADS}.py of the reference); the projection itself, the normals and the plain split are in projection.hip.
//   decode    STF: 5-float records, intensity /= 255 (float32 division), raw uint32 labels, optional 20 -> 0 remap, points with a float32
//             |xyz| below 1.8 removed BEFORE the rotation and the data theta range (dataloader_semantic_STF.py:37-56)
//   assembly  THAB: the file already is an organised H x W scan: id_map, flip, column roll, yaw in float64 (dataloader_semantic_THAB.py:35-59)
//   rows      WADS: image rows without any return are deleted before the nearest resize (dataloader_semantic_WADS.py:125-127)
//   maximum   CUDAL: reflectivity / max(image maximum, 1) (dataloader_semantic_CUDAL.py:107)
// No fused multiply-add where numpy rounds twice: contraction is off in every kernel that squares, sums or rotates.
#include "slu_common.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------------
// general point decode
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void point_decode_kernel(const float* __restrict__ rec, int stride, const unsigned* __restrict__ label, int N,
                                                           float intensity_div, unsigned label_mask, const int* __restrict__ lut, int lut_size,
                                                           int remap_from, int remap_to, int clip, float clip_min, int rotate, double ca, double sa,
                                                           double* __restrict__ pc, unsigned char* __restrict__ valid, int* __restrict__ bad) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const float* p = rec + (size_t)i * stride;
  const float xf = p[0], yf = p[1], zf = p[2];
  float w = p[3];
  if (intensity_div != 0.0f) w = w / intensity_div;      // xyzi[:, 3] /= 255. on a float32 array: a division, rounded once
  if (clip) {
    // np.linalg.norm(float32 [N, 3], axis=-1): the squares and their sum in float32, x^2 + y^2 first, then the square root; a NaN norm
    // fails `>= clip_min` like numpy's comparison and the point goes
    const float nrm = sqrtf((xf * xf + yf * yf) + zf * zf);
    valid[i] = nrm >= clip_min ? 1 : 0;
  }
  double x = (double)xf, y = (double)yf, z = (double)zf;
  if (rotate) {                           // [x y z] @ [[c, -s, 0], [s, c, 0], [0, 0, 1]] as in kitti_decode_kernel
    const double xr = (x * ca + y * sa) + z * 0.0;
    const double yr = (x * -sa + y * ca) + z * 0.0;
    x = xr;
    y = yr;
  }
  const unsigned sem = label[i] & label_mask;
  double cls;
  if (lut) {
    int c = sem < (unsigned)lut_size ? lut[sem] : -1;
    if (c < 0) {                          // the reference's dict lookup raises KeyError: counted here, raised by the host
      atomicAdd(bad, 1);
      c = 0;
    }
    if (c == remap_from) c = remap_to;
    cls = (double)c;
  } else {
    cls = (remap_from >= 0 && sem == (unsigned)remap_from) ? (double)remap_to : (double)sem;       // uint32 -> float64 is exact
  }
  double* o = pc + (size_t)i * 5;
  o[0] = x; o[1] = y; o[2] = z; o[3] = (double)w; o[4] = cls;
}

// ---------------------------------------------------------------------------------------------------------------------
// organised-scan assembly
// ---------------------------------------------------------------------------------------------------------------------
// out[row][col] = rotate(flip(in))[row][(col - shift) mod W]: np.roll(image, shift, axis=1) moves column c to c + shift
__global__ __launch_bounds__(256) void organised_scan_kernel(const float* __restrict__ rec, const unsigned* __restrict__ label, int H, int W,
                                                             const int* __restrict__ lut, int lut_size, int flip, int shift, int rotate, double ca,
                                                             double sa, float* __restrict__ img, float* __restrict__ range, int* __restrict__ bad) {
#pragma clang fp contract(off)
  const int px = blockIdx.x * blockDim.x + threadIdx.x;
  if (px >= H * W) return;
  const int row = px / W, col = px - row * W;
  int src = col - shift;                  // shift in [0, W)
  if (src < 0) src += W;
  if (flip) src = W - 1 - src;
  const size_t idx = (size_t)row * W + src;
  const float4 p = reinterpret_cast<const float4*>(rec)[idx];
  double x = (double)p.x, y = (double)p.y, z = (double)p.z;
  if (flip) y = -y;
  if (rotate) {
    const double xr = (x * ca + y * sa) + z * 0.0;
    const double yr = (x * -sa + y * ca) + z * 0.0;
    x = xr;
    y = yr;
  }
  const unsigned sem = label[idx] & 0xFFFFu;
  int cls = sem < (unsigned)lut_size ? lut[sem] : -1;
  if (cls < 0) {
    atomicAdd(bad, 1);
    cls = 0;
  }
  float* o = img + (size_t)px * 5;
  o[0] = (float)x; o[1] = (float)y; o[2] = (float)z; o[3] = p.w; o[4] = (float)cls;
  // the loader's range image is the float64 norm of the float64 image, rounded to float32 afterwards (dataloader_semantic_THAB.py:67,77)
  if (range) range[px] = (float)sqrt((x * x + y * y) + z * z);
}

// ---------------------------------------------------------------------------------------------------------------------
// rows without a return, and the nearest resize through the table of the others
// ---------------------------------------------------------------------------------------------------------------------
// rows[0] = kept-row count H', rows[1 .. H] = source row of kept row k (the first H' entries), rows[H + 1 .. 2H] = per-row flags
__global__ __launch_bounds__(256) void row_flag_kernel(const float* __restrict__ img, int W, int C, int* __restrict__ flags) {
#pragma clang fp contract(off)
  const float* r = img + (size_t)blockIdx.x * W * C;
  int any = 0;
  // np.linalg.norm(row pixel) == 0: the float32 sum of squares is 0 exactly when every square is (an underflowing square counts as 0)
  for (size_t e = threadIdx.x; e < (size_t)W * C; e += blockDim.x) {
    const float v = r[e];
    any |= (v * v != 0.0f) ? 1 : 0;
  }
  any = __syncthreads_or(any);
  if (threadIdx.x == 0) flags[blockIdx.x] = any ? 1 : 0;
}

__global__ __launch_bounds__(256) void row_scan_kernel(int H, int* __restrict__ rows) {
  __shared__ int part[256];
  const int* flags = rows + 1 + H;
  int* table = rows + 1;
  const int chunk = (H + 255) / 256;
  const int lo = threadIdx.x * chunk < H ? threadIdx.x * chunk : H;
  const int hi = lo + chunk < H ? lo + chunk : H;
  int n = 0;
  for (int r = lo; r < hi; ++r) n += flags[r];
  part[threadIdx.x] = n;
  __syncthreads();
  if (threadIdx.x == 0) {                 // exclusive scan of 256 partial counts
    int run = 0;
    for (int t = 0; t < 256; ++t) {
      const int v = part[t];
      part[t] = run;
      run += v;
    }
    rows[0] = run;
  }
  __syncthreads();
  int at = part[threadIdx.x];             // at <= lo: a kept row never moves down, so table[at] with at < H stays in bounds
  for (int r = lo; r < hi; ++r)
    if (flags[r]) table[at++] = r;
}

__global__ __launch_bounds__(256) void resize_rows_kernel(const float* __restrict__ img, int H, int W, int C, const int* __restrict__ rows,
                                                          float* __restrict__ out, int OH, int OW, double fx, int flip, int* __restrict__ bad) {
  const int Hk = rows[0];
  const size_t total = (size_t)OH * OW * C;
  if (Hk <= 0 || Hk > H) {                // no row left: cv2.resize of the reference raises; counted for the host, zeros written
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(bad, 1);
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) out[e] = 0.0f;
    return;
  }
  const double fy = (double)Hk / (double)OH;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(e % C);
    const size_t px = e / C;
    int ox = (int)(px % OW);
    const int oy = (int)(px / OW);
    if (flip) ox = OW - 1 - ox;
    int sy = (int)floor((double)oy * fy), sx = (int)floor((double)ox * fx);
    sy = sy < Hk - 1 ? sy : Hk - 1;
    sx = sx < W - 1 ? sx : W - 1;
    int srow = rows[1 + sy];
    srow = srow < 0 ? 0 : (srow < H ? srow : H - 1);
    float v = img[((size_t)srow * W + sx) * C + c];
    if (flip && c == 1) v = -v;
    out[e] = v;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// channel maximum and the split that divides by it
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned orderable32(float v) {                    // monotone map float -> uint32; 0 lies below every value
  const unsigned u = __float_as_uint(v);
  return (u >> 31) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float from_orderable32(unsigned k) {
  return __uint_as_float((k >> 31) ? (k & 0x7FFFFFFFu) : ~k);
}

__global__ __launch_bounds__(256) void channel_max_kernel(const float* __restrict__ img, int HW, int C, int channel, unsigned* __restrict__ key) {
  unsigned hi = 0u;
  for (size_t px = (size_t)blockIdx.x * blockDim.x + threadIdx.x; px < (size_t)HW; px += (size_t)gridDim.x * blockDim.x) {
    const unsigned k = orderable32(img[px * C + channel]);
    hi = k > hi ? k : hi;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned h2 = __shfl_xor(hi, o, 64);
    hi = h2 > hi ? h2 : hi;
  }
  if ((threadIdx.x & 63) == 0) atomicMax(key, hi);
}

__global__ __launch_bounds__(256) void range_image_split_ex_kernel(const float* __restrict__ img, const float* __restrict__ normals, int HW, int C,
                                                                   const float* __restrict__ range_in, const unsigned* __restrict__ refl_max_key,
                                                                   float* __restrict__ range, float* __restrict__ refl, float* __restrict__ xyz,
                                                                   float* __restrict__ normals_chw, int64_t* __restrict__ labels) {
#pragma clang fp contract(off)
  const int px = blockIdx.x * blockDim.x + threadIdx.x;
  if (px >= HW) return;
  const float* p = img + (size_t)px * C;
  const float x = p[0], y = p[1], z = p[2];
  range[px] = range_in ? range_in[px] : sqrtf((x * x + y * y) + z * z);
  float r = p[3];
  if (refl_max_key) {                     // img[..., 3] / np.maximum(img[..., 3].max(), 1.0): float32 maximum, float32 division
    const float m = from_orderable32(refl_max_key[0]);
    r = r / (m > 1.0f ? m : 1.0f);
  }
  refl[px] = r;
  xyz[px] = x; xyz[HW + px] = y; xyz[2 * (size_t)HW + px] = z;
  labels[px] = (int64_t)p[4];
  if (normals) {
    normals_chw[px] = normals[(size_t)px * 3];
    normals_chw[HW + px] = normals[(size_t)px * 3 + 1];
    normals_chw[2 * (size_t)HW + px] = normals[(size_t)px * 3 + 2];
  }
}

}  // namespace

extern "C" int slu_point_decode(const float* records, int stride, const uint32_t* label, int N, float intensity_div, int mask_labels, const int32_t* lut,
                                int lut_size, int remap_from, int remap_to, int clip, float clip_min, int rotate, double cos_a, double sin_a, double* pc,
                                uint8_t* valid, int32_t* bad_count, slu_stream_t stream) {
  if (!records || !label || !pc || !bad_count || N <= 0 || (stride != 4 && stride != 5) || (lut && lut_size <= 0) || (clip && !valid) ||
      !(intensity_div >= 0.0f))
    return SLU_EINVAL;
  hipLaunchKernelGGL(point_decode_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, slu_stream(stream), records, stride, label, N, intensity_div,
                     mask_labels ? 0xFFFFu : 0xFFFFFFFFu, lut, lut_size, remap_from, remap_to, clip ? 1 : 0, clip_min, rotate ? 1 : 0, cos_a, sin_a, pc, valid,
                     bad_count);
  SLU_CHECK_LAUNCH();
}

extern "C" int slu_organised_scan(const float* records, const uint32_t* label, int H, int W, const int32_t* lut, int lut_size, int flip, long long shift,
                                  int rotate, double cos_a, double sin_a, float* img, float* range, int32_t* bad_count, slu_stream_t stream) {
  if (!records || !label || !lut || !img || !bad_count || H <= 0 || W <= 0 || lut_size <= 0 || (long long)H * W > 0x7ffffffe || ((uintptr_t)records & 15))
    return SLU_EINVAL;
  const int s = (int)(((shift % W) + W) % W);
  const int HW = H * W;
  hipLaunchKernelGGL(organised_scan_kernel, dim3((unsigned)((HW + 255) / 256)), dim3(256), 0, slu_stream(stream), records, label, H, W, lut, lut_size,
                     flip ? 1 : 0, s, rotate ? 1 : 0, cos_a, sin_a, img, range, bad_count);
  SLU_CHECK_LAUNCH();
}

extern "C" int slu_nonempty_rows(const float* img, int H, int W, int C, int32_t* rows, slu_stream_t stream) {
  if (!img || !rows || H <= 0 || W <= 0 || C <= 0) return SLU_EINVAL;
  hipStream_t st = slu_stream(stream);
  hipLaunchKernelGGL(row_flag_kernel, dim3((unsigned)H), dim3(256), 0, st, img, W, C, rows + 1 + H);
  hipLaunchKernelGGL(row_scan_kernel, dim3(1), dim3(256), 0, st, H, rows);
  SLU_CHECK_LAUNCH();
}

extern "C" int slu_resize_nearest_rows_hwc(const float* img, int H, int W, int C, const int32_t* rows, float* out, int OH, int OW, int flip,
                                           int32_t* no_row_count, slu_stream_t stream) {
  if (!img || !rows || !out || !no_row_count || H <= 0 || W <= 0 || C <= 0 || OH <= 0 || OW <= 0 || (flip && C < 2)) return SLU_EINVAL;
  const size_t total = (size_t)OH * OW * C;
  hipLaunchKernelGGL(resize_rows_kernel, dim3(slu_grid_1d(total, 65535)), dim3(256), 0, slu_stream(stream), img, H, W, C, rows, out, OH, OW,
                     (double)W / (double)OW, flip ? 1 : 0, no_row_count);
  SLU_CHECK_LAUNCH();
}

extern "C" int slu_channel_max(const float* img, int H, int W, int C, int channel, uint32_t* key, slu_stream_t stream) {
  if (!img || !key || H <= 0 || W <= 0 || C <= 0 || channel < 0 || channel >= C || (long long)H * W > 0x7ffffffe) return SLU_EINVAL;
  hipStream_t st = slu_stream(stream);
  if (hipMemsetAsync(key, 0, sizeof(uint32_t), st) != hipSuccess) return SLU_ELAUNCH;
  const int HW = H * W;
  hipLaunchKernelGGL(channel_max_kernel, dim3(slu_grid_1d((size_t)HW, 256)), dim3(256), 0, st, img, HW, C, channel, key);
  SLU_CHECK_LAUNCH();
}

extern "C" int slu_range_image_split_ex(const float* img, const float* normals, int H, int W, int C, const float* range_in, const uint32_t* refl_max_key,
                                        float* range, float* refl, float* xyz, float* normals_chw, int64_t* labels, slu_stream_t stream) {
  if (!img || !range || !refl || !xyz || !labels || H <= 0 || W <= 0 || C < 5 || (normals && !normals_chw) || (long long)H * W > 0x7ffffffe) return SLU_EINVAL;
  const int HW = H * W;
  hipLaunchKernelGGL(range_image_split_ex_kernel, dim3((unsigned)((HW + 255) / 256)), dim3(256), 0, slu_stream(stream), img, normals, HW, C, range_in,
                     refl_max_key, range, refl, xyz, normals_chw, labels);
  SLU_CHECK_LAUNCH();
}
