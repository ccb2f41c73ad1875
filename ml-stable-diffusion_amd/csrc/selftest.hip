// Hardware self-check: verifies on the running GPU the two lane-layout facts every kernel in
// this library is built on (cdna_hip_programming.md section 3):
//   bit 0  v_mfma_f32_32x32x16_f16 operand/accumulator lane mapping
//          A: lane l holds A[i=l&31][k=8*(l>>5)+e], B: B[k=8*(l>>5)+e][j=l&31],
//          D: lane l reg r holds D[i=(r&3)+8*(r>>2)+4*(l>>5)][j=l&31]
//   bit 1  the DPP butterfly (quad_perm xor1, xor2, row_half_mirror, row_mirror) + the
//          v_permlane16_swap xor-16 step used for the ORIGINAL-attention row reductions
//   bit 2  the v_permlane32_swap xor-32 exchange of the SPLIT_EINSUM softmax
//   bit 3  v_mfma_i32_32x32x32_i8 (the W8A8 weight stream, wstream.hip): 16 int8 per lane and operand,
//          A: lane l holds A[i=l&31][k=16*(l>>5)+e], B: B[k=16*(l>>5)+e][j=l&31], e = 0..15 (byte e of the four registers),
//          D as above.  Checked with A = identity against an asymmetric B (D must be B: the k of every (lane, byte) is
//          then read off directly) and with asymmetric data on both sides
//   bit 4  v_mfma_i32_16x16x64_i8 (the W8A8 small-M GEMM, smgemm_i8.hip): 16 int8 per lane and operand,
//          A: lane l holds A[i=l&15][k=16*(l>>4)+e], B: B[k=16*(l>>4)+e][j=l&15], e = 0..15 (byte e of the four registers),
//          D: lane l reg r holds D[i=4*(l>>4)+r][j=l&15] (the 16x16 map of every dtype).  Checked like bit 3: A = the 16 x 64
//          selector A[i][k] = (k == 16 q + i) for each quarter q of K against an asymmetric B (D must be rows 16 q .. of B), then
//          asymmetric data on both sides
// Asymmetric integer data so a transposed or permuted mapping cannot pass by accident.
#include "kernels.h"

namespace sd {
namespace {

__global__ void mfma_probe(const half_t* __restrict__ A, const half_t* __restrict__ B, float* __restrict__ D) {
  const int l = threadIdx.x;
  half8 a, b;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int k = 8 * (l >> 5) + e;
    a[e] = A[(l & 31) * 16 + k];     // A[32][16] row-major
    b[e] = B[k * 32 + (l & 31)];     // B[16][32] row-major
  }
  floatx16 c;
#pragma unroll
  for (int r = 0; r < 16; ++r) c[r] = 0.f;
  c = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int i = (r & 3) + 8 * (r >> 2) + 4 * (l >> 5), j = l & 31;
    D[i * 32 + j] = c[r];
  }
}

typedef int intx4 __attribute__((ext_vector_type(4)));
typedef int intx16 __attribute__((ext_vector_type(16)));

__global__ void mfma_i8_probe(const int8_t* __restrict__ A, const int8_t* __restrict__ B, int* __restrict__ D) {
  const int l = threadIdx.x;
  intx4 a = {0, 0, 0, 0}, b = {0, 0, 0, 0};
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int k = 16 * (l >> 5) + e;
    a[e >> 2] |= (int)((unsigned)(unsigned char)A[(l & 31) * 32 + k] << (8 * (e & 3)));   // A[32][32] row-major
    b[e >> 2] |= (int)((unsigned)(unsigned char)B[k * 32 + (l & 31)] << (8 * (e & 3)));   // B[32][32] row-major
  }
  intx16 c;
#pragma unroll
  for (int r = 0; r < 16; ++r) c[r] = 0;
  c = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b, c, 0, 0, 0);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int i = (r & 3) + 8 * (r >> 2) + 4 * (l >> 5), j = l & 31;
    D[i * 32 + j] = c[r];
  }
}

__global__ void mfma_i8_16_probe(const int8_t* __restrict__ A, const int8_t* __restrict__ B, int* __restrict__ D) {
  const int l = threadIdx.x;
  intx4 a = {0, 0, 0, 0}, b = {0, 0, 0, 0};
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int k = 16 * (l >> 4) + e;
    a[e >> 2] |= (int)((unsigned)(unsigned char)A[(l & 15) * 64 + k] << (8 * (e & 3)));   // A[16][64] row-major
    b[e >> 2] |= (int)((unsigned)(unsigned char)B[k * 16 + (l & 15)] << (8 * (e & 3)));   // B[64][16] row-major
  }
  intx4 c = {0, 0, 0, 0};
  c = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, c, 0, 0, 0);
#pragma unroll
  for (int r = 0; r < 4; ++r) D[(4 * (l >> 4) + r) * 16 + (l & 15)] = c[r];
}

template <int CTRL>
__device__ __forceinline__ float dpp_mov(float x) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xF, 0xF, true));
}

__device__ __forceinline__ void swap16(float v, float& x, float& y) {
  const unsigned u = __float_as_uint(v);
  const auto r = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  const unsigned r0 = r[0], r1 = r[1];   // scalars first: bit-casting the vector-element lvalue reads lane 0 twice
  x = __uint_as_float(r0);
  y = __uint_as_float(r1);
}
__device__ __forceinline__ void swap32(float v, float& x, float& y) {
  const unsigned u = __float_as_uint(v);
  const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  const unsigned r0 = r[0], r1 = r[1];   // scalars first: bit-casting the vector-element lvalue reads lane 0 twice
  x = __uint_as_float(r0);
  y = __uint_as_float(r1);
}

// out_x32[l] = in[l] - 2 * in[l ^ 32] would be wrong under any other pairing; the swap returns
// {low-half value, high-half value} in every lane, so own/partner are picked by (l >> 5)
__global__ void dpp_probe(const float* __restrict__ in, float* __restrict__ out_max, float* __restrict__ out_sum,
                          float* __restrict__ out_x32) {
  const int l = threadIdx.x;
  float v = in[l];
  float x, y;
  float m = v;
  m = fmaxf(m, dpp_mov<0xB1>(m));
  m = fmaxf(m, dpp_mov<0x4E>(m));
  m = fmaxf(m, dpp_mov<0x141>(m));
  m = fmaxf(m, dpp_mov<0x140>(m));
  swap16(m, x, y);
  m = fmaxf(x, y);
  float s = v;
  s += dpp_mov<0xB1>(s);
  s += dpp_mov<0x4E>(s);
  s += dpp_mov<0x141>(s);
  s += dpp_mov<0x140>(s);
  swap16(s, x, y);
  s = x + y;
  out_max[l] = m;
  out_sum[l] = s;
  swap32(v, x, y);
  out_x32[l] = x - 2.f * y;      // every lane: in[l & 31] - 2 * in[(l & 31) + 32]
}

}  // namespace

int selftest_mfma() {
  int result = 0;
  half_t hA[32 * 16], hB[16 * 32];
  float ref[32 * 32], got[32 * 32];
  for (int i = 0; i < 32; ++i)
    for (int k = 0; k < 16; ++k) hA[i * 16 + k] = (half_t)(float)((i * 3 + k * 7) % 11 - 5);
  for (int k = 0; k < 16; ++k)
    for (int j = 0; j < 32; ++j) hB[k * 32 + j] = (half_t)(float)((k * 5 + j * 2) % 13 - 6);
  for (int i = 0; i < 32; ++i)
    for (int j = 0; j < 32; ++j) {
      float s = 0.f;
      for (int k = 0; k < 16; ++k) s += (float)hA[i * 16 + k] * (float)hB[k * 32 + j];
      ref[i * 32 + j] = s;
    }
  half_t *dA, *dB;
  float *dD, *dIn, *dMax, *dSum, *dX32;
  SD_HIP(hipMalloc(&dA, sizeof(hA)));
  SD_HIP(hipMalloc(&dB, sizeof(hB)));
  SD_HIP(hipMalloc(&dD, sizeof(got)));
  SD_HIP(hipMalloc(&dIn, 64 * 4));
  SD_HIP(hipMalloc(&dMax, 64 * 4));
  SD_HIP(hipMalloc(&dSum, 64 * 4));
  SD_HIP(hipMalloc(&dX32, 64 * 4));
  SD_HIP(hipMemcpy(dA, hA, sizeof(hA), hipMemcpyHostToDevice));
  SD_HIP(hipMemcpy(dB, hB, sizeof(hB), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(mfma_probe, dim3(1), dim3(64), 0, 0, dA, dB, dD);
  SD_HIP(hipDeviceSynchronize());
  SD_HIP(hipMemcpy(got, dD, sizeof(got), hipMemcpyDeviceToHost));
  int bad = 0;
  for (int i = 0; i < 32 * 32; ++i)
    if (got[i] != ref[i]) {
      if (bad < 8) fprintf(stderr, "[sd selftest] mfma D[%d][%d] = %g, expected %g\n", i / 32, i % 32, got[i], ref[i]);
      ++bad;
    }
  if (bad) result |= 1;

  float hin[64], hmax[64], hsum[64], hx32[64];
  for (int l = 0; l < 64; ++l) hin[l] = (float)((l * 37) % 101) - 50.f;
  SD_HIP(hipMemcpy(dIn, hin, sizeof(hin), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(dpp_probe, dim3(1), dim3(64), 0, 0, dIn, dMax, dSum, dX32);
  SD_HIP(hipDeviceSynchronize());
  SD_HIP(hipMemcpy(hmax, dMax, sizeof(hmax), hipMemcpyDeviceToHost));
  SD_HIP(hipMemcpy(hsum, dSum, sizeof(hsum), hipMemcpyDeviceToHost));
  SD_HIP(hipMemcpy(hx32, dX32, sizeof(hx32), hipMemcpyDeviceToHost));
  bad = 0;
  for (int hf = 0; hf < 2; ++hf) {
    float m = -1e30f, s = 0.f;
    for (int l = 0; l < 32; ++l) {
      m = fmaxf(m, hin[hf * 32 + l]);
      s += hin[hf * 32 + l];
    }
    for (int l = 0; l < 32; ++l)
      if (hmax[hf * 32 + l] != m || hsum[hf * 32 + l] != s) {
        if (bad < 8)
          fprintf(stderr, "[sd selftest] dpp lane %d: max %g (want %g) sum %g (want %g)\n", hf * 32 + l,
                  hmax[hf * 32 + l], m, hsum[hf * 32 + l], s);
        ++bad;
      }
  }
  if (bad) result |= 2;
  bad = 0;
  for (int l = 0; l < 64; ++l) {
    const float want = hin[l & 31] - 2.f * hin[(l & 31) + 32];
    if (hx32[l] != want) {
      if (bad < 8) fprintf(stderr, "[sd selftest] permlane32_swap lane %d: %g (want %g)\n", l, hx32[l], want);
      ++bad;
    }
  }
  if (bad) result |= 4;
  {   // bit 3: the int8 form, A = identity first, then asymmetric data on both sides
    int8_t hA8[32 * 32], hB8[32 * 32], *dA8, *dB8;
    int ref8[32 * 32], got8[32 * 32], *dD8;
    SD_HIP(hipMalloc(&dA8, sizeof(hA8)));
    SD_HIP(hipMalloc(&dB8, sizeof(hB8)));
    SD_HIP(hipMalloc(&dD8, sizeof(got8)));
    for (int k = 0; k < 32; ++k)
      for (int j = 0; j < 32; ++j) hB8[k * 32 + j] = (int8_t)((k * 37 + j * 11) % 255 - 127);   // -127 .. 127, no row or column alike
    bad = 0;
    for (int pass = 0; pass < 2; ++pass) {
      for (int i = 0; i < 32; ++i)
        for (int k = 0; k < 32; ++k) hA8[i * 32 + k] = pass == 0 ? (int8_t)(i == k) : (int8_t)((i * 29 + k * 53) % 255 - 127);
      for (int i = 0; i < 32; ++i)
        for (int j = 0; j < 32; ++j) {
          int sum = 0;
          for (int k = 0; k < 32; ++k) sum += (int)hA8[i * 32 + k] * (int)hB8[k * 32 + j];
          ref8[i * 32 + j] = sum;
        }
      SD_HIP(hipMemcpy(dA8, hA8, sizeof(hA8), hipMemcpyHostToDevice));
      SD_HIP(hipMemcpy(dB8, hB8, sizeof(hB8), hipMemcpyHostToDevice));
      hipLaunchKernelGGL(mfma_i8_probe, dim3(1), dim3(64), 0, 0, dA8, dB8, dD8);
      SD_HIP(hipDeviceSynchronize());
      SD_HIP(hipMemcpy(got8, dD8, sizeof(got8), hipMemcpyDeviceToHost));
      for (int i = 0; i < 32 * 32; ++i)
        if (got8[i] != ref8[i]) {
          if (bad < 8) fprintf(stderr, "[sd selftest] mfma i8 (pass %d) D[%d][%d] = %d, expected %d\n", pass, i / 32, i % 32, got8[i], ref8[i]);
          ++bad;
        }
    }
    if (bad) result |= 8;
    (void)hipFree(dA8);
    (void)hipFree(dB8);
    (void)hipFree(dD8);
  }
  {   // bit 4: the 16x16x64 int8 form - a selector of each quarter of K first (passes 0-3), then asymmetric data on both sides
    int8_t hA8[16 * 64], hB8[64 * 16], *dA8, *dB8;
    int ref8[16 * 16], got8[16 * 16], *dD8;
    SD_HIP(hipMalloc(&dA8, sizeof(hA8)));
    SD_HIP(hipMalloc(&dB8, sizeof(hB8)));
    SD_HIP(hipMalloc(&dD8, sizeof(got8)));
    for (int k = 0; k < 64; ++k)
      for (int j = 0; j < 16; ++j) hB8[k * 16 + j] = (int8_t)((k * 37 + j * 11) % 255 - 127);   // -127 .. 127, no row or column alike
    bad = 0;
    for (int pass = 0; pass < 5; ++pass) {
      for (int i = 0; i < 16; ++i)
        for (int k = 0; k < 64; ++k) hA8[i * 64 + k] = pass < 4 ? (int8_t)(k == 16 * pass + i) : (int8_t)((i * 29 + k * 53) % 255 - 127);
      for (int i = 0; i < 16; ++i)
        for (int j = 0; j < 16; ++j) {
          int sum = 0;
          for (int k = 0; k < 64; ++k) sum += (int)hA8[i * 64 + k] * (int)hB8[k * 16 + j];
          ref8[i * 16 + j] = sum;
        }
      SD_HIP(hipMemcpy(dA8, hA8, sizeof(hA8), hipMemcpyHostToDevice));
      SD_HIP(hipMemcpy(dB8, hB8, sizeof(hB8), hipMemcpyHostToDevice));
      hipLaunchKernelGGL(mfma_i8_16_probe, dim3(1), dim3(64), 0, 0, dA8, dB8, dD8);
      SD_HIP(hipDeviceSynchronize());
      SD_HIP(hipMemcpy(got8, dD8, sizeof(got8), hipMemcpyDeviceToHost));
      for (int i = 0; i < 16 * 16; ++i)
        if (got8[i] != ref8[i]) {
          if (bad < 8) fprintf(stderr, "[sd selftest] mfma i8 16x16x64 (pass %d) D[%d][%d] = %d, expected %d\n", pass, i / 16, i % 16, got8[i], ref8[i]);
          ++bad;
        }
    }
    if (bad) result |= 16;
    (void)hipFree(dA8);
    (void)hipFree(dB8);
    (void)hipFree(dD8);
  }
  (void)hipFree(dA);
  (void)hipFree(dB);
  (void)hipFree(dD);
  (void)hipFree(dIn);
  (void)hipFree(dMax);
  (void)hipFree(dSum);
  (void)hipFree(dX32);
  return result;
}

}  // namespace sd
