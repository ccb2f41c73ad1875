// CLIP vision tower + concept head of the safety checker: the kernels that neither the UNet path nor the text tower has.
//
// Math (reference): diffusers' StableDiffusionSafetyChecker - transformers' CLIPVisionModel (ViT-L/14), visual_projection and the
// concept head - as the reference converts it (python_coreml_stable_diffusion/torch2coreml.py:1119-1309, the vectorised head at
// :1177-1209) and calls it on every generated image (pipeline.py:286-311; SafetyChecker.swift).  The GEMMs (patch embedding as a
// 1x1 GEMM over gathered patch rows, q|k|v, out_proj, fc1, fc2), the LayerNorms, the MLP activation and visual_projection run on
// igemm.hip / norm.hip / clip.hip / misc.hip; this file holds
//   vit_attention_kernel   non-causal flash-style attention, head dim 64, any S >= 1, on MFMA
//   vit_patch_rows_kernel  (B, 3, I, I) NCHW -> one row of 3 p p (zero-padded to a multiple of 64) values per patch
//   vit_tokens_kernel      class token + position embeddings
//   safety_head_kernel     cosine similarities, thresholds, the special-care adjustment, the per-image verdict (all fp32)
#include "kernels.h"

namespace sd {
namespace {

// ---------------------------------------------------------------------------------------------------------------------------
// Attention.  qkv rows are [q | k | v] of width 3 D (D = heads * 64), the stacked projection's output as it is; out rows have width D.
// One workgroup = (batch, head, 64 queries); its four waves own 16 queries each.  Keys stream through LDS in tiles of 64:
//   Ks [key][d]  as loaded                   -> A operand of S^T = K Q^T   (v_mfma_f32_16x16x32_f16: 16 keys x 16 queries, k = d)
//   Vt [d][key]  transposed while stored     -> A operand of O^T = V^T P^T (16 d x 16 queries, k = key)
// Both products put the QUERY on the lane (column lane & 15), so a lane's score registers, its running max / sum and its output
// registers all belong to one query: the softmax needs two cross-lane steps (over the four lane groups), none for the rescale.
// A score block leaves the MFMA with keys 4 g + r (g = lane >> 4, r = register) of its 16 keys in lane group g; two blocks side by
// side are exactly the eight k-elements lane group g feeds the next MFMA with, provided the V^T fragment is read in that same key
// order: element j of group g = key 4 g + j (j < 4), 16 + 4 g + (j - 4) (j >= 4) of a 32-key step - two 8-byte LDS reads.
// Ragged S: rows past S are loaded as zeros (K, V, Q alike: never whatever the neighbouring buffer holds), keys past S get the finite
// score -1e30 and the probability 0 (a select, not an exponential), queries past S are computed on zeros and not stored.
constexpr int VIT_TQ = 64, VIT_TK = 64;
constexpr int VIT_LD = 72;   // LDS row stride in halves: 144 B, 16-B aligned, rows 36 banks apart

__global__ __launch_bounds__(256) void vit_attention_kernel(const half_t* __restrict__ qkv, half_t* __restrict__ out, int S, int heads,
                                                            float scale_log2e) {
  __shared__ __attribute__((aligned(16))) half_t Ks[VIT_TK * VIT_LD];
  __shared__ __attribute__((aligned(16))) half_t Vt[64 * VIT_LD];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int h = blockIdx.y, b = blockIdx.z;
  const int D = heads * 64;
  const size_t ld = (size_t)3 * D;
  const half_t* base = qkv + (size_t)b * S * ld + h * 64;
  const int q = blockIdx.x * VIT_TQ + wave * 16 + c;   // this lane's query

  half8 qf[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    qf[ks] = (half8)(half_t)0;
    if (q < S) qf[ks] = *reinterpret_cast<const half8*>(base + (size_t)q * ld + 32 * ks + 8 * g);
  }
  floatx4 o[4];
#pragma unroll
  for (int db = 0; db < 4; ++db) o[db] = (floatx4)0.f;
  float m = -1e30f, l = 0.f;   // running max (log2 domain) of the query, this lane's share of its running sum

  const int ntiles = (S + VIT_TK - 1) / VIT_TK;
  for (int kt = 0; kt < ntiles; ++kt) {
    const int k0 = kt * VIT_TK;
    __syncthreads();   // the previous tile has been read
#pragma unroll
    for (int i = t; i < VIT_TK * 8; i += 256) {   // K: 8 threads per key row, 128 contiguous bytes
      const int key = i >> 3, ch = (i & 7) * 8;
      half8 v = (half8)(half_t)0;
      if (k0 + key < S) v = *reinterpret_cast<const half8*>(base + (size_t)(k0 + key) * ld + D + ch);
      *reinterpret_cast<half8*>(Ks + key * VIT_LD + ch) = v;
    }
#pragma unroll
    for (int i = t; i < VIT_TK * 8; i += 256) {   // V: a wave stores 64 consecutive keys of one d row (no bank conflict)
      const int key = i & 63, ch = (i >> 6) * 8;
      half8 v = (half8)(half_t)0;
      if (k0 + key < S) v = *reinterpret_cast<const half8*>(base + (size_t)(k0 + key) * ld + 2 * D + ch);
#pragma unroll
      for (int e = 0; e < 8; ++e) Vt[(ch + e) * VIT_LD + key] = v[e];
    }
    __syncthreads();

    // s[kb][r]: key k0 + 16 kb + 4 g + r against query c
    floatx4 s[4];
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
      s[kb] = (floatx4)0.f;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const half8 a = *reinterpret_cast<const half8*>(Ks + (16 * kb + c) * VIT_LD + 32 * ks + 8 * g);
        s[kb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, qf[ks], s[kb], 0, 0, 0);
      }
    }
    float mx = m;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool valid = k0 + 16 * kb + 4 * g + r < S;
        s[kb][r] = valid ? s[kb][r] * scale_log2e : -1e30f;
        mx = fmaxf(mx, s[kb][r]);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));   // key k0 is valid in every tile: mx is a real score from the first tile on
    const float alpha = exp2f(m - mx);    // first tile: exp2(-1e30 - mx) = 0 exactly, on l = 0 and o = 0
    m = mx;
    l *= alpha;
#pragma unroll
    for (int db = 0; db < 4; ++db) o[db] *= alpha;
    half4 p[4];
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool valid = k0 + 16 * kb + 4 * g + r < S;
        const float e = valid ? exp2f(s[kb][r] - mx) : 0.f;
        l += e;
        p[kb][r] = (half_t)e;
      }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      half8 pb;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        pb[j] = p[2 * ks][j];
        pb[4 + j] = p[2 * ks + 1][j];
      }
#pragma unroll
      for (int db = 0; db < 4; ++db) {
        const half_t* row = Vt + (16 * db + c) * VIT_LD + 32 * ks + 4 * g;
        const half4 lo = *reinterpret_cast<const half4*>(row), hi = *reinterpret_cast<const half4*>(row + 16);
        half8 a;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          a[j] = lo[j];
          a[4 + j] = hi[j];
        }
        o[db] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, pb, o[db], 0, 0, 0);
      }
    }
  }
  l += __shfl_xor(l, 16);
  l += __shfl_xor(l, 32);
  if (q < S) {
    const float inv = 1.0f / l;   // l >= 1: the key that holds the maximum contributes exp2(0)
    half_t* dst = out + ((size_t)b * S + q) * D + h * 64 + 4 * g;
#pragma unroll
    for (int db = 0; db < 4; ++db) {   // o[db][r] = O[query c][d = 16 db + 4 g + r]
      half4 v;
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = (half_t)(o[db][r] * inv);
      *reinterpret_cast<half4*>(dst + 16 * db) = v;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Patch embedding front: rows[b * G * G + gy * G + gx][c * p * p + py * p + px] = img[b][c][gy * p + py][gx * p + px], the order of
// the flattened (D, 3, p, p) conv weight; columns [3 p p, Kp) are zero (the weight is padded the same way).  One block per patch.
__global__ void vit_patch_rows_kernel(const half_t* __restrict__ img, half_t* __restrict__ rows, int I, int p, int G, int Kp) {
  const int patch = blockIdx.x;                 // b * G * G + gy * G + gx
  const int b = patch / (G * G), gy = (patch / G) % G, gx = patch % G;
  const int pp = p * p;
  for (int k = threadIdx.x; k < Kp; k += blockDim.x) {
    half_t v = (half_t)0;
    if (k < 3 * pp) {
      const int ch = k / pp, py = (k % pp) / p, px = k % p;
      v = img[(((size_t)b * 3 + ch) * I + gy * p + py) * I + gx * p + px];
    }
    rows[(size_t)patch * Kp + k] = v;
  }
}

// x[b][0] = class_embedding + pos[0];  x[b][1 + j] = patch[b][j] + pos[1 + j]   (CLIPVisionEmbeddings.forward).  One block per token.
__global__ void vit_tokens_kernel(const half_t* __restrict__ patch, const half_t* __restrict__ cls, const half_t* __restrict__ pos,
                                  half_t* __restrict__ x, int S, int D) {
  const int row = blockIdx.x, b = row / S, tkn = row % S;
  const half_t* src = tkn == 0 ? cls : patch + ((size_t)b * (S - 1) + tkn - 1) * D;
  const half_t* pe = pos + (size_t)tkn * D;
  for (int c = threadIdx.x * 8; c < D; c += blockDim.x * 8) {
    const half8 a = *reinterpret_cast<const half8*>(src + c), e = *reinterpret_cast<const half8*>(pe + c);
    half8 y;
#pragma unroll
    for (int i = 0; i < 8; ++i) y[i] = (half_t)((float)a[i] + (float)e[i]);
    *reinterpret_cast<half8*>(x + (size_t)row * D + c) = y;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// The concept head, one workgroup per image, fp32 throughout.  With cos(a, b) = <a, b> / (|a| |b|):
//   special[i] = cos(image, special_embeds[i]) - special_w[i] + adjustment;   lift = 0.01 if any special[i] > 0 else 0
//   concept[i] = cos(image, concept_embeds[i]) - concept_w[i] + lift;         has_nsfw = any concept[i] > 0
// Every dot product is one wave's strided sum followed by a butterfly: a fixed order, so two runs agree bit for bit.
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ float cosine(const float* __restrict__ a, float inv_na, const float* __restrict__ e, int P, int lane) {
  float dot = 0.f, nn = 0.f;
  for (int k = lane; k < P; k += 64) {
    const float v = e[k];
    dot += a[k] * v;
    nn += v * v;
  }
  dot = wave_sum(dot);
  nn = wave_sum(nn);
  return dot * inv_na * (1.0f / sqrtf(nn));
}
__global__ __launch_bounds__(256) void safety_head_kernel(const float* __restrict__ image, const float* __restrict__ concept_e,
                                                          const float* __restrict__ special_e, const float* __restrict__ concept_w,
                                                          const float* __restrict__ special_w, const float* __restrict__ adjustment,
                                                          int P, int n_concepts, int n_special, float* __restrict__ has_nsfw,
                                                          float* __restrict__ scores) {
  __shared__ int special_hit, concept_hit;
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* a = image + (size_t)b * P;
  if (threadIdx.x == 0) special_hit = 0, concept_hit = 0;
  float na = 0.f;
  for (int k = lane; k < P; k += 64) na += a[k] * a[k];
  const float inv_na = 1.0f / sqrtf(wave_sum(na));   // every wave computes the same value in the same order
  const float adj = adjustment[0];
  __syncthreads();
  for (int i = wave; i < n_special; i += 4) {
    const float sc = cosine(a, inv_na, special_e + (size_t)i * P, P, lane) - special_w[i] + adj;
    if (lane == 0 && sc > 0.f) special_hit = 1;
  }
  __syncthreads();
  const float lift = special_hit ? 0.01f : 0.f;
  for (int i = wave; i < n_concepts; i += 4) {
    const float sc = cosine(a, inv_na, concept_e + (size_t)i * P, P, lane) - concept_w[i] + lift;
    if (lane == 0) {
      scores[(size_t)b * n_concepts + i] = sc;
      if (sc > 0.f) concept_hit = 1;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) has_nsfw[b] = concept_hit ? 1.f : 0.f;
}

}  // namespace

bool vit_attention_ok(int d) { return d == 64; }

void launch_vit_attention(const half_t* qkv, half_t* out, int B, int S, int heads, int d, hipStream_t s) {
  SD_REQUIRE(vit_attention_ok(d), kUnsupported, "vit_attention: head dim %d (the kernel is built for 64)", d);
  SD_REQUIRE(B >= 1 && S >= 1 && heads >= 1 && heads <= 65535 && B <= 65535, kInvalidArgument, "vit_attention: B=%d S=%d heads=%d", B, S,
             heads);
  const float scale_log2e = 1.4426950408889634f / sqrtf((float)d);
  hipLaunchKernelGGL(vit_attention_kernel, dim3(cdiv(S, VIT_TQ), heads, B), dim3(256), 0, s, qkv, out, S, heads, scale_log2e);
  SD_HIP(hipGetLastError());
}

void launch_vit_patch_rows(const half_t* img, half_t* rows, int B, int I, int p, int Kp, hipStream_t s) {
  SD_REQUIRE(p >= 1 && I >= p && I % p == 0 && Kp >= 3 * p * p, kInvalidArgument, "vit_patch_rows: image %d patch %d row %d", I, p, Kp);
  const int G = I / p;
  hipLaunchKernelGGL(vit_patch_rows_kernel, dim3(B * G * G), dim3(256), 0, s, img, rows, I, p, G, Kp);
  SD_HIP(hipGetLastError());
}

void launch_vit_tokens(const half_t* patch, const half_t* cls, const half_t* pos, half_t* x, int B, int S, int D, hipStream_t s) {
  SD_REQUIRE(D % 8 == 0 && S >= 2, kUnsupported, "vit_tokens: hidden size %d, %d tokens", D, S);
  hipLaunchKernelGGL(vit_tokens_kernel, dim3(B * S), dim3(128), 0, s, patch, cls, pos, x, S, D);
  SD_HIP(hipGetLastError());
}

void launch_safety_head(const float* image_embeds, const float* concept_embeds, const float* special_embeds, const float* concept_w,
                        const float* special_w, const float* adjustment, int B, int P, int n_concepts, int n_special, float* has_nsfw,
                        float* concept_scores, hipStream_t s) {
  SD_REQUIRE(B >= 1 && P >= 1 && n_concepts >= 1 && n_special >= 0, kInvalidArgument, "safety_head: B=%d P=%d concepts=%d special=%d", B, P,
             n_concepts, n_special);
  hipLaunchKernelGGL(safety_head_kernel, dim3(B), dim3(256), 0, s, image_embeds, concept_embeds, special_embeds, concept_w, special_w,
                     adjustment, P, n_concepts, n_special, has_nsfw, concept_scores);
  SD_HIP(hipGetLastError());
}

}  // namespace sd
