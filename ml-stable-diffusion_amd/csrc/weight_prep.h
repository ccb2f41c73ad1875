// Host-side weight layout rules, stated once: the UNet builder (unet.cpp) and the operator entry points (capi_ops.cpp) both
// call these, so an operator test checks the layout the step runs.  Plain host C++: no HIP call, no allocation.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "kernels.h"

namespace sd {

// GEGLU (ff.net.0.proj, unet.py:613-617): destination row of output row o of an n-row [values | gates] matrix.  Value and gate
// channels interleave in blocks of 32, so the GEMM epilogue multiplies them in registers (the device-side twin of this rule is
// conv_generic_kernel's, conv_small.hip).
inline int geglu_row(int o, int n) {
  const int half_n = n / 2;
  const bool gate = o >= half_n;
  const int j = gate ? o - half_n : o;
  return (j / 32) * 64 + (gate ? 32 : 0) + (j % 32);
}

// [Cout][Cin][k][k] (or Linear [Cout][Cin], k = 1) -> [Cout][k][k][Cin]; geglu: rows move through geglu_row
template <typename S, typename D>
void retile_ohwi(const S* src, int cout, int cin, int k, bool geglu, D* dst) {
  const int kk = k * k;
  for (int o = 0; o < cout; ++o) {
    const int dst_o = geglu ? geglu_row(o, cout) : o;
    for (int c = 0; c < cin; ++c)
      for (int t = 0; t < kk; ++t) dst[((size_t)dst_o * kk + t) * cin + c] = (D)src[((size_t)o * cin + c) * kk + t];
  }
}

// The upsampler conv as four 2x2 phase convs (conv3x3_halo_sp.hip, plan tile 21).  Nearest-x2 followed by a 3x3 / pad-1 conv equals,
// for output phase (a, b) = (Y & 1, X & 1), a 2x2 conv over the low-res image whose tap (dy, dx) sits at low-res offset
// (a + dy - 1, b + dx - 1) and carries the sum of the 3x3 weights that land on that low-res pixel:
//   rows:  a = 0: dy 0 <- ky {0}, dy 1 <- ky {1, 2};   a = 1: dy 0 <- ky {0, 1}, dy 1 <- ky {2};   columns alike with b, dx, kx.
// src [Cout][Cin][3][3] (the checkpoint's order) -> dst [4 phases p = 2a + b][Cout][4 taps t = 2dy + dx][Cin] fp16: a (phase, n) row
// is K' = 4 Cin contiguous, tap-major then channel.  Each folded weight is the sum of its 1, 2 or 4 source values, added in fp32 in
// the order (ky, kx) ascending and rounded to fp16 ONCE.  A sum outside the fp16 range is refused.
inline size_t subpixel_fold_halves(int cout, int cin) { return (size_t)16 * cout * cin; }
inline int subpixel_first(int phase_bit, int d) { return phase_bit == 0 ? d : 2 * d; }             // first source tap of fold position d
inline int subpixel_count(int phase_bit, int d) { return (phase_bit == 0) == (d == 0) ? 1 : 2; }   // how many source taps it sums
template <typename S>
void subpixel_fold(const S* src, int cout, int cin, half_t* dst) {
  SD_REQUIRE(src && dst && cout > 0 && cin > 0, kInvalidArgument, "subpixel_fold: Cout %d Cin %d", cout, cin);
  for (int p = 0; p < 4; ++p) {
    const int a = p >> 1, b = p & 1;
    for (int o = 0; o < cout; ++o)
      for (int t = 0; t < 4; ++t) {
        const int dy = t >> 1, dx = t & 1;
        const int ky0 = subpixel_first(a, dy), nky = subpixel_count(a, dy), kx0 = subpixel_first(b, dx), nkx = subpixel_count(b, dx);
        half_t* row = dst + (((size_t)p * cout + o) * 4 + t) * cin;
        for (int c = 0; c < cin; ++c) {
          const S* w9 = src + ((size_t)o * cin + c) * 9;
          float s = 0.f;
          for (int ky = ky0; ky < ky0 + nky; ++ky)
            for (int kx = kx0; kx < kx0 + nkx; ++kx) s += (float)w9[ky * 3 + kx];
          SD_REQUIRE(std::fabs(s) <= 65504.0f, kInvalidArgument, "subpixel_fold: the folded weight of output %d input %d phase %d tap %d is %g, outside fp16",
                     o, c, p, t, (double)s);   // (a NaN fails the comparison too)
          row[c] = (half_t)s;
        }
      }
  }
}

// LayerNorm folded into the projection behind it, one projection w [cout][cin] (+ bias or NULL):
//   y = LN(x) . W^T + b  ==  rstd*(x . (W*gamma)^T) - rstd*mean*colsum(W*gamma) + (b + W.beta)
// Writes rows row0 + o (geglu: geglu_row(o, cout)) of w_out [..][cin], colsum and bias_out.  gamma == beta == NULL: the weights
// are copied unchanged and the bias passes through.  colsum sums what the MFMA actually multiplies: the fp16-rounded values.
template <typename W>
void fold_layernorm_rows(const W* w, const float* bias, const float* gamma, const float* beta, int cout, int cin, int row0,
                         bool geglu, half_t* w_out, float* colsum, float* bias_out) {
  for (int o = 0; o < cout; ++o) {
    const int dst = geglu ? geglu_row(o, cout) : row0 + o;
    double cs = 0.0, bb = bias ? (double)bias[o] : 0.0;
    for (int c = 0; c < cin; ++c) {
      const float wv = (float)w[(size_t)o * cin + c];
      const half_t h = gamma ? (half_t)(wv * gamma[c]) : (half_t)w[(size_t)o * cin + c];
      w_out[(size_t)dst * cin + c] = h;
      cs += (double)(float)h;
      if (beta) bb += (double)wv * (double)beta[c];
    }
    colsum[dst] = (float)cs;
    bias_out[dst] = (float)bb;
  }
}

// One lane's share of a palettized weight stream (wstream.hip plan tile 14, smgemm.hip plan tile 15; decoded by pal_decode.h): a
// little-endian bit stream of nbits-wide fields (field f at bits [f * nbits, (f + 1) * nbits)), padded to whole 16-byte words.
// Word q of every lane of a wave lies together - [q][lane][16 B] - so each load instruction of a kernel is one coalesced 1-KB wave load.
struct PalLaneWriter {
  int nbits;
  std::vector<uint8_t> bytes;   // the lane's words (+ room for the last window's spill)
  uint64_t window = 0;          // bits not yet stored, little-endian; fewer than 8 of them between fields
  int held = 0;
  size_t at = 0;
  PalLaneWriter(int nbits_, int words) : nbits(nbits_), bytes((size_t)words * 16 + 8, (uint8_t)0) {}
  void put(uint64_t index) {
    window |= index << held;
    held += nbits;
    while (held >= 8) {
      bytes[at++] = (uint8_t)window;
      window >>= 8;
      held -= 8;
    }
  }
  // the lane's words into its wave's block of the stream (words x 64 lanes x 16 B), and a fresh lane
  void flush(uint8_t* wave_block, int lane) {
    if (held) bytes[at++] = (uint8_t)window;
    for (size_t q = 0; (q + 1) * 16 + 8 <= bytes.size(); ++q)
      std::copy(bytes.begin() + q * 16, bytes.begin() + (q + 1) * 16, wave_block + (q * 64 + lane) * 16);
    std::fill(bytes.begin(), bytes.end(), (uint8_t)0);
    window = 0;
    held = 0;
    at = 0;
  }
};

// The palettized weight stream of wstream.hip (plan tile 14).  A lane of the (strip, slice) wave owns NF = 2 * taps fragments of 8
// weights - fragment j, element e: output row strip * 32 + (lane & 31), input channel slice * 32 + (j & 1) * 16 + (lane >> 5) * 8 + e,
// tap j >> 1 (the order of wstream_retile_kernel).  Its NF * 8 palette indices, in that order, are the lane's stream; the wave's block
// lies at [strip][slice].
inline int wstream_pal_words(int taps, int nbits) { return (2 * taps * 8 * nbits + 127) / 128; }
inline size_t wstream_pal_bytes(int N, int Ctot, int ksize, int nbits) {
  return (size_t)(N / 32) * (Ctot / 32) * wstream_pal_words(ksize * ksize, nbits) * 64 * 16;
}
// indices [N][Ctot][k][k] (the checkpoint's order) -> the stream; dst holds wstream_pal_bytes(...) bytes
inline void wstream_pal_pack(const uint8_t* indices, int N, int Ctot, int ksize, int nbits, uint8_t* dst) {
  const int taps = ksize * ksize, nslices = Ctot / 32, Q = wstream_pal_words(taps, nbits), nf = 2 * taps;
  PalLaneWriter w(nbits, Q);
  for (int strip = 0; strip < N / 32; ++strip)
    for (int slice = 0; slice < nslices; ++slice)
      for (int lane = 0; lane < 64; ++lane) {
        const int n = strip * 32 + (lane & 31);
        for (int j = 0; j < nf; ++j) {
          const uint8_t* src = indices + ((size_t)n * Ctot + slice * 32 + (j & 1) * 16 + (lane >> 5) * 8) * taps + (j >> 1);
          for (int e = 0; e < 8; ++e) w.put(src[(size_t)e * taps]);
        }
        w.flush(dst + ((size_t)strip * nslices + slice) * Q * 1024, lane);
      }
}

// W8A8 (plan tile 17, wstream.hip's int8 source; the reference's quantize_cumulative_config, activation_quantization.py:141-203:
// symmetric, per-output-channel weights, per-tensor activations - parity with coremltools' quantizer unpinned).
// The weight quantizer, w [N][per_row] fp32 (a conv's (Cout, Ctot, k, k) row by row): s_w[n] = absmax_n / 127 (an all-zero row: 1),
// q = clip(rint(w / s_w[n]), -127, 127) - fp32 division, round to nearest even (the default rounding mode; nearbyintf raises no
// inexact flag).  Every element must be finite (kInvalidArgument).  Returns the squared error sum (w - q * s_w)^2 in float64.
inline double w8a8_quantize_weight(const float* w, int N, size_t per_row, int8_t* q, float* scale) {
  double err = 0.0;
  for (int n = 0; n < N; ++n) {
    const float* row = w + (size_t)n * per_row;
    float amax = 0.f;
    for (size_t i = 0; i < per_row; ++i) {
      SD_REQUIRE(std::isfinite(row[i]), kInvalidArgument, "w8a8 quantizer: row %d element %zu is not finite", n, i);
      amax = std::max(amax, std::fabs(row[i]));
    }
    const float s = amax > 0.f ? amax / 127.0f : 1.0f;
    scale[n] = s;
    for (size_t i = 0; i < per_row; ++i) {
      const float r = std::min(std::max(std::nearbyintf(row[i] / s), -127.0f), 127.0f);
      q[(size_t)n * per_row + i] = (int8_t)r;
      const double dlt = (double)row[i] - (double)r * (double)s;
      err += dlt * dlt;
    }
  }
  return err;
}
// The int8 weight stream of wstream.hip: [N / 32][Ctot / 32][taps][64 lanes][16 B].  Lane l of the (strip, slice) wave holds, for tap
// t, the 16 weights of output row strip * 32 + (l & 31), input channels slice * 32 + (l >> 5) * 16 + (0 .. 15): one operand of
// v_mfma_i32_32x32x32_i8, loaded as one coalesced 1-KB wave load.  q [N][Ctot][k][k] (the checkpoint's order); dst holds N * Ctot * k * k bytes.
inline size_t wstream_i8_bytes(int N, int Ctot, int ksize) { return (size_t)N * Ctot * ksize * ksize; }
inline void wstream_i8_pack(const int8_t* q, int N, int Ctot, int ksize, int8_t* dst) {
  const int taps = ksize * ksize, nslices = Ctot / 32;
  for (int strip = 0; strip < N / 32; ++strip)
    for (int slice = 0; slice < nslices; ++slice)
      for (int t = 0; t < taps; ++t)
        for (int lane = 0; lane < 64; ++lane) {
          const int8_t* src = q + ((size_t)(strip * 32 + (lane & 31)) * Ctot + slice * 32 + (lane >> 5) * 16) * taps + t;
          int8_t* out = dst + ((((size_t)strip * nslices + slice) * taps + t) * 64 + lane) * 16;
          for (int e = 0; e < 16; ++e) out[e] = src[(size_t)e * taps];
        }
}
// The int8 weights of conv3x3_halo_i8.hip (plan tile 18): [N][k * k][Ctot], the fp16 halo kernel's K order (retile_ohwi) at one byte
// per weight - a (n, tap, 64-channel chunk) row is 64 contiguous bytes, what one DMA lane quartet fetches.  q [N][Ctot][k][k] (the
// checkpoint's order); dst holds N * Ctot * k * k bytes.
inline void halo_i8_pack(const int8_t* q, int N, int Ctot, int ksize, int8_t* dst) { retile_ohwi(q, N, Ctot, ksize, false, dst); }
// The int8 weights of smgemm_i8.hip and smgemm_q8.hip (plan tiles 19 and 24): [N][K], the checkpoint's own order of a 1x1 conv / Linear - wave w of a tile
// fetches rows 16 w .. 16 w + 15 of a K64 stage as one 1-KB LDS-DMA piece, 16 rows x 64 contiguous bytes, and the swizzle of its LDS
// image is applied on the source address.  The layout is stated here once: the function is a copy.  N % 16 == 0, K % 64 == 0.
inline size_t smgemm_i8_bytes(int N, int K) { return (size_t)N * K; }
inline void smgemm_i8_pack(const int8_t* q, int N, int K, int8_t* dst) { std::copy(q, q + smgemm_i8_bytes(N, K), dst); }
// The int8 weights of smgeglu_i8.hip (plan tile 20), q [N2][K] of ff.net.0.proj in the checkpoint's row order (rows 0 .. N2 / 2 - 1 the
// values, the rest the gates), N2 % 32 == 0, K % 64 == 0: [N2 / 16 strips][16 rows][K] - strip 2 U + v holds the checkpoint rows
// v * N2 / 2 + 16 U + (0 .. 15), the 16 value (v = 0) or gate (v = 1) rows of the output's 16-column unit U: the strip order of
// smgeglu_pal_pack at one byte per weight, rows whole.  A tile of 80 output columns reads the ten consecutive strips 10 n_tile ..
// 10 n_tile + 9, each stage 64 contiguous bytes of every row.  Bytes: N2 * K.
inline size_t smgeglu_i8_bytes(int N2, int K) { return (size_t)N2 * K; }
inline void smgeglu_i8_pack(const int8_t* q, int N2, int K, int8_t* dst) {
  for (int strip = 0; strip < N2 / 16; ++strip)
    for (int i = 0; i < 16; ++i) {
      const int o = (strip & 1) * (N2 / 2) + 16 * (strip >> 1) + i;   // checkpoint row
      std::copy(q + (size_t)o * K, q + (size_t)(o + 1) * K, dst + ((size_t)strip * 16 + i) * K);
    }
}
// The int8 weights of smqkv_i8.hip (plan tile 22), q [3C][K] = the stacked [Wq | Wk | Wv] of a self-attention, each in the checkpoint's
// row order, 3C % 16 == 0, K % 64 == 0: [3C / 16 strips][16 rows][K] - strip t holds the stacked rows 16 t .. 16 t + 15, every row
// whole.  A tile of 160 output columns stages the ten consecutive strips 10 n_tile .. 10 n_tile + 9, each stage 64 contiguous bytes of
// every row; with C % 160 == 0 a tile's strips belong to one of the three matrices.  The layout is stated here once: the function is a
// copy.  Bytes: 3C * K.
inline size_t smqkv_i8_bytes(int N3, int K) { return (size_t)N3 * K; }
inline void smqkv_i8_pack(const int8_t* q, int N3, int K, int8_t* dst) { std::copy(q, q + smqkv_i8_bytes(N3, K), dst); }
// What an upload of a W8A8 conv starts from (sd_op_conv2d_w8a8 / _halo, sd_op_gemm_w8a8, Net::conv), checked in the order the header lists: act_absmax, finite
// positive scales, no value of -128 (the symmetric scheme has none); the packed stream, cs[n] = fp32(s_a * s_w[n]) with s_a = act_absmax / 127, and inv_s = fp32(1 / s_a).
struct W8A8HostCopy {
  std::vector<int8_t> stream;
  std::vector<float> cs;
  float inv_s = 0.f;
};
inline bool w8a8_absmax_ok(float act_absmax) { return std::isfinite(act_absmax) && act_absmax > 0.f; }
inline W8A8HostCopy w8a8_host_copy(const char* what, const int8_t* q, const float* w_scale, float act_absmax, int N, int Ctot, int ksize,
                                   WeightSource kind = WeightSource::I8Wstream) {   // one of the six int8 kinds
  SD_REQUIRE(w8a8_absmax_ok(act_absmax), kInvalidArgument, "%s: act_absmax = %g, not a positive finite number", what, (double)act_absmax);
  const size_t n_el = wstream_i8_bytes(N, Ctot, ksize);
  W8A8HostCopy h;
  const float s_a = act_absmax / 127.0f;
  h.inv_s = 1.0f / s_a;
  SD_REQUIRE(std::isfinite(h.inv_s) && h.inv_s > 0.f, kInvalidArgument, "%s: act_absmax = %g has no finite inverse scale", what, (double)act_absmax);
  SD_REQUIRE(kind != WeightSource::I8Geglu || N % 64 == 0, kInvalidArgument, "%s: %d GEGLU rows do not interleave in blocks of 32", what, N);
  h.cs.resize(N);
  for (int n = 0; n < N; ++n) {
    SD_REQUIRE(std::isfinite(w_scale[n]) && w_scale[n] > 0.f, kInvalidArgument, "%s: w_scale[%d] = %g, not a positive finite number", what, n, (double)w_scale[n]);
    h.cs[kind == WeightSource::I8Geglu ? geglu_row(n, N) : n] = s_a * w_scale[n];   // (GEGLU: where the interleaved bias of row n lies)
  }
  for (size_t i = 0; i < n_el; ++i) SD_REQUIRE(q[i] != -128, kInvalidArgument, "%s: weight value -128 at element %zu, the symmetric range is [-127, 127]", what, i);
  h.stream.resize(n_el);
  if (kind == WeightSource::I8Halo) halo_i8_pack(q, N, Ctot, ksize, h.stream.data());
  else if (kind == WeightSource::I8Gemm || kind == WeightSource::I8GemmQ) smgemm_i8_pack(q, N, Ctot, h.stream.data());   // (ksize 1; tile 24 reads tile 19's layout)
  else if (kind == WeightSource::I8Geglu) smgeglu_i8_pack(q, N, Ctot, h.stream.data());
  else if (kind == WeightSource::I8Qkv) smqkv_i8_pack(q, N, Ctot, h.stream.data());     // (ksize 1; N = 3C stacked rows)
  else wstream_i8_pack(q, N, Ctot, ksize, h.stream.data());
  return h;
}

// The palettized weight stream of smgemm.hip (plan tile 15), indices [N][K] (a 1x1 conv / Linear), N % 16 == 0, K % 64 == 0.  The wave
// of 16-column strip n / 16 consumes K in stages of 64; lane l = 16 g + r16 multiplies, in stage s and sub-step kk (0, 1), the eight
// weights W[16 strip + r16][64 s + 32 kk + 8 g + e], e = 0..7: 16 indices per lane per stage.  Stages are cut into GROUPS of
// kSmPalGroup = 8 (the last group is padded with zero fields that no MFMA consumes); a lane's 128 indices of a group, in the order
// (s, kk, e), are its stream: exactly nbits words.  The wave's block lies at [strip][group].
constexpr int kSmPalGroup = 8;
inline int smgemm_pal_groups(int K) { return (K / 64 + kSmPalGroup - 1) / kSmPalGroup; }
inline size_t smgemm_pal_bytes(int N, int K, int nbits) { return (size_t)(N / 16) * smgemm_pal_groups(K) * nbits * 64 * 16; }
// dst holds smgemm_pal_bytes(...) bytes
inline void smgemm_pal_pack(const uint8_t* indices, int N, int K, int nbits, uint8_t* dst) {
  const int groups = smgemm_pal_groups(K), nk = K / 64;
  PalLaneWriter w(nbits, nbits);
  for (int strip = 0; strip < N / 16; ++strip)
    for (int grp = 0; grp < groups; ++grp)
      for (int lane = 0; lane < 64; ++lane) {
        const uint8_t* row = indices + (size_t)(strip * 16 + (lane & 15)) * K + (lane >> 4) * 8;
        for (int f = 0; f < kSmPalGroup * 16; ++f) {
          const int s = grp * kSmPalGroup + (f >> 4), kk = (f >> 3) & 1, e = f & 7;
          w.put(s < nk ? row[s * 64 + kk * 32 + e] : 0);
        }
        w.flush(dst + ((size_t)strip * groups + grp) * nbits * 1024, lane);
      }
}

// The palettized weight stream of smgeglu.hip (plan tile 16), indices [N2][K] of ff.net.0.proj in the checkpoint's row order (rows
// 0 .. N2 / 2 - 1 the values, the rest the gates), N2 % 32 == 0, K % 64 == 0.  The stream is smgemm_pal_pack's - strips of 16 rows,
// groups of 8 stages, nbits words of [64 lanes][16 B] per strip and group, lane 16 g + r16 holding row r16's indices of columns
// 64 s + 32 kk + 8 g + e in the order (s, kk, e) - over 16-row strips in the order the kernel's tile stages them: strip 2 U + v holds
// the checkpoint rows v * N2 / 2 + 16 U + (0 .. 15) - the 16 value (v = 0) or gate (v = 1) rows of the output's 16-column unit U
// (geglu_row puts them at rows 64 (U / 2) + 16 (U % 2) + 32 v of the fp16 upload).  A tile of 80 output columns reads the ten
// consecutive strips 10 n_tile .. 10 n_tile + 9, one per wave.  Bytes: smgemm_pal_bytes(N2, K, nbits).
inline void smgeglu_pal_pack(const uint8_t* indices, int N2, int K, int nbits, uint8_t* dst) {
  std::vector<uint8_t> rows((size_t)N2 * K);
  for (int strip = 0; strip < N2 / 16; ++strip)
    for (int i = 0; i < 16; ++i) {
      const int o = (strip & 1) * (N2 / 2) + 16 * (strip >> 1) + i;   // checkpoint row
      // the same row through the upload's interleave: where the fp16 kernel reads it
      SD_REQUIRE(geglu_row(o, N2) == 64 * (strip >> 2) + 16 * ((strip >> 1) & 1) + 32 * (strip & 1) + i, kInternal, "GEGLU strip order");
      std::copy(indices + (size_t)o * K, indices + (size_t)(o + 1) * K, rows.begin() + ((size_t)strip * 16 + i) * K);
    }
  smgemm_pal_pack(rows.data(), N2, K, nbits, dst);
}

// The palettized index stream of the 3x3 halo conv (conv3x3_halo_pal.hip, plan tile 25), indices [N][Ctot][3][3] (the
// checkpoint's order), Ctot % 64 == 0.  A compact bit stream without padding bits; the only padding is rows up to a multiple of 64,
// which carry index 0 (their outputs are never stored).  Bytes: ceil(N / 64) * 64 * 9 * Ctot * nbits / 8.
//   * per (64-row n-tile, 64-channel chunk, tap) one BLOCK of nbits * 128 dwords = 512 * nbits bytes; blocks in the order n-tile, chunk,
//     tap - the order a workgroup walks them, so its DMA offset advances by the constant 512 * nbits bytes per tap step;
//   * inside a block, dword j of stream (wk, lane), wk = 0, 1 the K half, lane = 0 .. 63, at dword index (j * 2 + wk) * 64 + lane;
//   * a stream is the lane's 32 indices of that step as little-endian nbits-wide fields (field f at bits [f * nbits, (f + 1) * nbits)
//     of its nbits dwords), in the order the fp16 kernel's read_step reads its fragments: field (2 s + j) * 8 + e, s, j = 0, 1,
//     e = 0 .. 7, is row 64 n_tile + 32 j + (lane & 31), channel 64 chunk + (2 (2 wk + s) + (lane >> 5)) * 8 + e.  The two
//     pixel-half waves of a K half read the same stream.
inline size_t halo_pal_bytes(int N, int Ctot, int nbits) { return (size_t)((N + 63) / 64) * 64 * 9 * Ctot * nbits / 8; }
// dst holds halo_pal_bytes(...) bytes
inline void halo_pal_pack(const uint8_t* indices, int N, int Ctot, int nbits, uint8_t* dst) {
  const int n_tiles = (N + 63) / 64, nch = Ctot / 64;
  const size_t block = (size_t)512 * nbits;
  for (int nt = 0; nt < n_tiles; ++nt)
    for (int ch = 0; ch < nch; ++ch)
      for (int tap = 0; tap < 9; ++tap) {
        uint8_t* blk = dst + (((size_t)nt * nch + ch) * 9 + tap) * block;
        for (int wk = 0; wk < 2; ++wk)
          for (int lane = 0; lane < 64; ++lane) {
            uint32_t words[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};   // nbits dwords (+ one for the last field's shift)
            for (int f = 0; f < 32; ++f) {
              const int s = f >> 4, j = (f >> 3) & 1, e = f & 7;
              const int n = nt * 64 + j * 32 + (lane & 31), c = ch * 64 + (2 * (2 * wk + s) + (lane >> 5)) * 8 + e;
              const uint64_t idx = n < N ? indices[((size_t)n * Ctot + c) * 9 + tap] : 0;
              const int bit = f * nbits, dw = bit >> 5, sh = bit & 31;
              const uint64_t v = idx << sh;
              words[dw] |= (uint32_t)v;
              words[dw + 1] |= (uint32_t)(v >> 32);
            }
            for (int j = 0; j < nbits; ++j) {
              uint8_t* o = blk + ((size_t)(j * 2 + wk) * 64 + lane) * 4;
              for (int b = 0; b < 4; ++b) o[b] = (uint8_t)(words[j] >> (8 * b));   // little-endian dwords
            }
          }
      }
}

// What every upload of a palettized tensor starts from (the operator entry points of capi_ops.cpp, Net::conv): indices inside the
// palette, the packed stream of the layout - wstream.hip's, smgemm.hip's, smgeglu.hip's (the latter two: indices [N][Ctot], ksize 1) or the halo conv's (ksize 3)
// - and the LUT zero-padded to the kPalLutHalves entries the kernels copy.  The caller has checked the shape against the layout and owns the device memory.
inline void palette_check_indices(const char* what, const uint8_t* indices, size_t n, int nbits) {
  for (size_t i = 0; i < n; ++i)
    SD_REQUIRE(indices[i] < (1u << nbits), kInvalidArgument, "%s: index %u at element %zu, the palette has %d entries", what,
               (unsigned)indices[i], i, 1 << nbits);
}
struct PaletteHostCopy {
  std::vector<uint8_t> stream;
  std::vector<half_t> lut;
};
inline PaletteHostCopy palette_host_copy(const char* what, const half_t* lut, int nbits, const uint8_t* indices, int N, int Ctot, int ksize,
                                         WeightSource kind) {   // one of the four palettized kinds
  palette_check_indices(what, indices, (size_t)N * Ctot * ksize * ksize, nbits);
  PaletteHostCopy h;
  h.stream.resize(kind == WeightSource::PalWstream ? wstream_pal_bytes(N, Ctot, ksize, nbits)
                  : kind == WeightSource::PalHalo  ? halo_pal_bytes(N, Ctot, nbits)
                                                   : smgemm_pal_bytes(N, Ctot, nbits));
  if (kind == WeightSource::PalHalo) halo_pal_pack(indices, N, Ctot, nbits, h.stream.data());
  else if (kind == WeightSource::PalGemm) smgemm_pal_pack(indices, N, Ctot, nbits, h.stream.data());
  else if (kind == WeightSource::PalGeglu) smgeglu_pal_pack(indices, N, Ctot, nbits, h.stream.data());
  else wstream_pal_pack(indices, N, Ctot, ksize, nbits, h.stream.data());
  h.lut.assign(kPalLutHalves, (half_t)0);
  std::copy(lut, lut + (1 << nbits), h.lut.begin());
  return h;
}

// The one upload of a compressed weight source, per host-copy type: host copy -> device stream + LUT / scales -> the descriptor's
// source (ConvDesc::cw).  `up(host, n)` returns a device copy of n elements from memory the caller owns (a handle's arena, an operator
// entry point's scratch); *bytes, when asked for, gets what went up.
template <class Up>
CompressedWeights upload_palettized(Up&& up, WeightSource kind, const char* what, const half_t* lut, int nbits, const uint8_t* indices, int N,
                                    int Ctot, int ksize, size_t* bytes = nullptr) {
  const PaletteHostCopy h = palette_host_copy(what, lut, nbits, indices, N, Ctot, ksize, kind);
  CompressedWeights c;
  c.kind = kind;
  c.stream = up(h.stream.data(), h.stream.size());
  c.lut = up(h.lut.data(), h.lut.size());
  c.bits = nbits;
  if (bytes) *bytes = h.stream.size() + h.lut.size() * sizeof(half_t);
  return c;
}
template <class Up>
CompressedWeights upload_w8a8(Up&& up, WeightSource kind, const char* what, const int8_t* q, const float* w_scale, float act_absmax, int N, int Ctot,
                              int ksize, size_t* bytes = nullptr) {
  const W8A8HostCopy h = w8a8_host_copy(what, q, w_scale, act_absmax, N, Ctot, ksize, kind);
  CompressedWeights c;
  c.kind = kind;
  c.stream = up(h.stream.data(), h.stream.size());
  c.scale = up(h.cs.data(), h.cs.size());
  c.inv_s = h.inv_s;
  if (bytes) *bytes = h.stream.size() + h.cs.size() * sizeof(float);
  return c;
}

}  // namespace sd
