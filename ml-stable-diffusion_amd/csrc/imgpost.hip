// Image post-processing between the VAE decoder and the safety checker, on the device (pipeline.py:286-320 of the reference does it in
// numpy, PIL and transformers' CLIPImageProcessor on the host; Decoder.swift:40-68, SafetyChecker.swift:55-99):
//   image_rgb8_kernel   decoder output fp32 NCHW in [-1, 1] -> 8-bit RGB (B, H, W, 3), numpy_to_pil's arithmetic bit for bit
//   clip_input_kernel   8-bit RGB -> the checker's clip_input (B, 3, S, S) fp16: Pillow's 8-bit bicubic resize (two separable passes,
//                       the intermediate image rounded to uint8), centre crop, rescale, normalise - every step exact integer or
//                       IEEE-rounded fp32 arithmetic, so the result equals the host route bit for bit
// Both are small, latency-bound launches (28 x B workgroups at S = 224): what they buy is the host work and the upload they
// replace, not a fraction of any roof.
#include <algorithm>
#include <cmath>

#include "kernels.h"

namespace sd {

// Pillow's bicubic filter (a = -0.5) and coefficient precomputation (Resample.c precompute_coeffs + normalize_coeffs_8bpc), in double
// like Pillow: no contraction, C truncation.  Zeros behind the n taps of a row.
#pragma clang fp contract(off)
static double bicubic_filter(double t) {
  const double a = -0.5;
  if (t < 0.0) t = -t;
  if (t < 1.0) return ((a + 2.0) * t - (a + 3.0)) * t * t + 1;
  if (t < 2.0) return (((t - 5) * t + 8) * t - 4) * a;
  return 0.0;
}

int resample_ksize(int in_size, int out_size) {
  const double scale = (double)in_size / (double)out_size, fs = std::max(scale, 1.0);
  return (int)std::ceil(2.0 * fs) * 2 + 1;
}

void resample_coeffs(int in_size, int out_size, int32_t* bounds, int32_t* coeffs) {
  const double scale = (double)in_size / (double)out_size, fs = std::max(scale, 1.0), support = 2.0 * fs;
  const int ksize = resample_ksize(in_size, out_size);
  std::vector<double> w(ksize);
  for (int xx = 0; xx < out_size; ++xx) {
    const double center = (xx + 0.5) * scale;
    const int xmin = std::max((int)(center - support + 0.5), 0);
    const int n = std::min((int)(center + support + 0.5), in_size) - xmin;
    double ww = 0.0;
    for (int x = 0; x < n; ++x) {
      w[x] = bicubic_filter((x + xmin - center + 0.5) / fs);
      ww += w[x];
    }
    bounds[2 * xx] = xmin;
    bounds[2 * xx + 1] = n;
    int32_t* k = coeffs + (size_t)xx * ksize;
    for (int x = 0; x < ksize; ++x) {
      if (x >= n) {
        k[x] = 0;
        continue;
      }
      const double v = ww != 0.0 ? w[x] / ww : w[x];
      k[x] = v < 0 ? (int)(v * (double)(1 << kResampleBits) - 0.5) : (int)(v * (double)(1 << kResampleBits) + 0.5);
    }
  }
}

namespace {

// clamp(x / 2 + 0.5, 0, 1) * 255, rounded half to even: (np.clip(image / 2 + 0.5, 0, 1) * 255).round().  x * 0.5f is exact, so the
// compiler's fma for the first line changes nothing; the multiply by 255 has nothing to contract into.  +-inf -> 255 / 0.
__device__ __forceinline__ unsigned quantise_u8(float x) {
  const float v = fminf(fmaxf(x * 0.5f + 0.5f, 0.0f), 1.0f);
  return (unsigned)rintf(v * 255.0f);
}

// image (B, 3, H, W) fp32 -> rgb8 (B, H, W, 3).  VEC (H * W % 4 == 0, both pointers 16-byte aligned): a lane takes four consecutive
// pixels - one 16-byte load per colour plane, twelve output bytes as three dword stores.  Else one pixel per lane, byte stores: the
// form for image sizes whose planes do not start on 16-byte boundaries.  Grid-stride: any grid is in bounds.
template <bool VEC>
__global__ __launch_bounds__(256) void image_rgb8_kernel(const float* __restrict__ image, uint8_t* __restrict__ rgb8, int B, int HW) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  if (VEC) {
    const size_t g4 = (size_t)HW / 4, n = (size_t)B * g4;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
      const size_t b = i / g4, g = i - b * g4;
      const floatx4* src = reinterpret_cast<const floatx4*>(image + b * 3 * HW) + g;
      const floatx4 r = src[0], gr = src[g4], bl = src[2 * g4];
      unsigned q[12];
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        q[3 * p] = quantise_u8(r[p]);
        q[3 * p + 1] = quantise_u8(gr[p]);
        q[3 * p + 2] = quantise_u8(bl[p]);
      }
      unsigned* dst = reinterpret_cast<unsigned*>(rgb8 + (b * HW + g * 4) * 3);
#pragma unroll
      for (int d = 0; d < 3; ++d) dst[d] = q[4 * d] | (q[4 * d + 1] << 8) | (q[4 * d + 2] << 16) | (q[4 * d + 3] << 24);
    }
  } else {
    const size_t n = (size_t)B * HW;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
      const size_t b = i / HW, p = i - b * HW;
      for (int c = 0; c < 3; ++c) rgb8[i * 3 + c] = (uint8_t)quantise_u8(image[(b * 3 + c) * HW + p]);
    }
  }
}

constexpr int kTileRows = 8;   // output rows of the crop window per workgroup

// One workgroup per (tile of kTileRows output rows of the crop window, image).  Only the crop window is computed: every output sample
// of a separable resize depends on its own taps alone, so this equals resize-then-crop.
//   phase 1  the horizontal pass over the source rows [r_lo, r_lo + nrows) that the tile's vertical taps read, for the S columns of
//            the crop window, into LDS as uint8 [nrows][S][3]; the (u / 255 - mean) / std table of the 3 x 256 possible samples
//   barrier
//   phase 2  the vertical pass out of LDS, the table lookup, two columns per lane packed into one dword store
// Taps: every loop runs to the axis' ksize over zero-padded coefficients, with the source index clamped into the image (rows: into
// the staged rows), so control flow is uniform.  uint8 x 23-bit signed coefficient is a 24-bit multiply; the sums are exact in int32.
__global__ __launch_bounds__(256) void clip_input_kernel(const uint8_t* __restrict__ rgb8, half_t* __restrict__ out, ClipInputDesc d) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  half_t* norm = reinterpret_cast<half_t*>(lds);              // [3][256]
  unsigned char* rows = lds + 3 * 256 * sizeof(half_t);        // [nrows][S][3]
  const int tid = threadIdx.x, S = d.S, b = blockIdx.y;
  const int y0 = blockIdx.x * kTileRows, y1 = min(y0 + kTileRows, S);
  const int r_lo = d.vbounds[2 * (d.top + y0)];
  const int nrows = min(d.vbounds[2 * (d.top + y1 - 1)] + d.ksv, d.H) - r_lo;
  const uint8_t* src = rgb8 + (size_t)b * d.H * d.W * 3;

  for (int i = tid; i < 3 * 256; i += 256) {
    const int c = i >> 8;
    norm[i] = (half_t)__fdiv_rn(__fdiv_rn((float)(i & 255), 255.0f) - d.mean[c], d.std[c]);
  }
  for (int i = tid; i < nrows * S; i += 256) {
    const int r = i / S, x = i - r * S;
    const int xmin = d.hbounds[2 * (d.left + x)];
    const int32_t* k = d.hcoeffs + (size_t)(d.left + x) * d.ksh;
    const uint8_t* line = src + (size_t)(r_lo + r) * d.W * 3;
    int s0 = 1 << (kResampleBits - 1), s1 = s0, s2 = s0;
    for (int j = 0; j < d.ksh; ++j) {
      const uint8_t* p = line + min(xmin + j, d.W - 1) * 3;
      const int kj = k[j];
      s0 += __mul24((int)p[0], kj);
      s1 += __mul24((int)p[1], kj);
      s2 += __mul24((int)p[2], kj);
    }
    unsigned char* q = rows + (size_t)i * 3;
    q[0] = (unsigned char)min(max(s0 >> kResampleBits, 0), 255);
    q[1] = (unsigned char)min(max(s1 >> kResampleBits, 0), 255);
    q[2] = (unsigned char)min(max(s2 >> kResampleBits, 0), 255);
  }
  __syncthreads();

  const int S2 = S / 2, per_c = (y1 - y0) * S2;
  for (int i = tid; i < 3 * per_c; i += 256) {
    const int c = i / per_c, rem = i - c * per_c, yy = rem / S2, x = (rem - yy * S2) * 2;
    const int y = y0 + yy;
    const int ymin = d.vbounds[2 * (d.top + y)] - r_lo;
    const int32_t* k = d.vcoeffs + (size_t)(d.top + y) * d.ksv;
    int s0 = 1 << (kResampleBits - 1), s1 = s0;
    for (int j = 0; j < d.ksv; ++j) {
      const unsigned char* p = rows + ((size_t)min(ymin + j, nrows - 1) * S + x) * 3 + c;
      const int kj = k[j];
      s0 += __mul24((int)p[0], kj);
      s1 += __mul24((int)p[3], kj);
    }
    const int u0 = min(max(s0 >> kResampleBits, 0), 255), u1 = min(max(s1 >> kResampleBits, 0), 255);
    half2v v;
    v[0] = norm[c * 256 + u0];
    v[1] = norm[c * 256 + u1];
    *reinterpret_cast<half2v*>(out + (((size_t)b * 3 + c) * S + y) * S + x) = v;
  }
}

inline int grid_for(size_t n) { return (int)std::min<size_t>((n + 255) / 256, 2048); }

}  // namespace

void launch_image_rgb8(const float* image, uint8_t* rgb8, int B, int H, int W, hipStream_t s) {
  SD_REQUIRE(B >= 1 && H >= 1 && W >= 1 && (size_t)H * W <= (size_t)INT32_MAX / 3, kInvalidArgument, "image_rgb8: %d images of %dx%d", B, H, W);
  const int HW = H * W;
  const bool vec = HW % 4 == 0 && (reinterpret_cast<uintptr_t>(image) | reinterpret_cast<uintptr_t>(rgb8)) % 16 == 0;
  if (vec)
    hipLaunchKernelGGL(image_rgb8_kernel<true>, dim3(grid_for((size_t)B * HW / 4)), dim3(256), 0, s, image, rgb8, B, HW);
  else
    hipLaunchKernelGGL(image_rgb8_kernel<false>, dim3(grid_for((size_t)B * HW)), dim3(256), 0, s, image, rgb8, B, HW);
  SD_HIP(hipGetLastError());
}

ClipInputPlan plan_clip_input(int H, int W, int rh, int rw, int S) {
  SD_REQUIRE(H >= 1 && W >= 1 && rh >= 1 && rw >= 1 && S >= 1, kInvalidArgument, "clip_input: %dx%d -> %dx%d -> %d", H, W, rh, rw, S);
  SD_REQUIRE(rh >= S && rw >= S, kInvalidArgument, "clip_input: the resized image %dx%d is smaller than the %dx%d crop (transformers would zero-pad)",
             rh, rw, S, S);
  SD_REQUIRE(S % 2 == 0, kUnsupported, "clip_input: odd crop size %d (the kernel stores two columns per dword)", S);
  ClipInputPlan p;
  p.H = H, p.W = W, p.rh = rh, p.rw = rw, p.S = S;
  p.ksh = resample_ksize(W, rw);
  p.ksv = resample_ksize(H, rh);
  p.hbounds.resize((size_t)rw * 2), p.hcoeffs.resize((size_t)rw * p.ksh);
  p.vbounds.resize((size_t)rh * 2), p.vcoeffs.resize((size_t)rh * p.ksv);
  resample_coeffs(W, rw, p.hbounds.data(), p.hcoeffs.data());
  resample_coeffs(H, rh, p.vbounds.data(), p.vcoeffs.data());
  for (const std::vector<int32_t>* t : {&p.hcoeffs, &p.vcoeffs})
    for (int32_t k : *t) SD_REQUIRE(k > -(1 << 23) && k < (1 << 23), kInternal, "clip_input: coefficient %d does not fit 24 bits", k);
  // the rows a tile stages, as the kernel computes them
  const int top = (rh - S) / 2;
  int nrows = 0;
  for (int y0 = 0; y0 < S; y0 += kTileRows) {
    const int y1 = std::min(y0 + kTileRows, S);
    nrows = std::max(nrows, std::min(p.vbounds[2 * (top + y1 - 1)] + p.ksv, H) - p.vbounds[2 * (top + y0)]);
  }
  p.lds_bytes = 3 * 256 * sizeof(half_t) + (size_t)nrows * S * 3;
  SD_REQUIRE(p.lds_bytes <= 64 * 1024, kUnsupported, "clip_input: %dx%d -> %dx%d stages %d rows of %d pixels (%zu bytes of LDS, 64 KB are planned for)",
             H, W, rh, rw, nrows, S, p.lds_bytes);
  return p;
}

void launch_clip_input(const uint8_t* rgb8, half_t* out, int B, const ClipInputDesc& d, size_t lds_bytes, hipStream_t s) {
  SD_REQUIRE(B >= 1 && B <= 65535, kInvalidArgument, "clip_input: batch %d", B);
  hipLaunchKernelGGL(clip_input_kernel, dim3(cdiv(d.S, kTileRows), B), dim3(256), lds_bytes, s, rgb8, out, d);
  SD_HIP(hipGetLastError());
}

}  // namespace sd
