// The K-split 3x3 / stride-1 halo convolution (plan tile 7) of the implicit-GEMM family: conv3x3_halo_ks_kernel, its LDS-size
// rules and its launcher.  Arguments, shared device helpers and epilogue: igemm_device.h.
#include "igemm_device.h"
#include "halo_ring.h"

namespace sd {

namespace {

// ---------------------------------------------------------------------------------------------
// 3x3 / stride 1 convolution with an LDS-resident input HALO tile (resnet convs, unet.py:435-456).
// The im2col kernel above re-fetches the activation tile once per tap (9x); its K step moves
// 32 KB into LDS for 2 MFLOP, and the measured LDS fill rate (~40 GB/s per CU, tools/prof_conv.py) -
// not the MFMA pipe - bounds it.  Here a workgroup owns an 8x16-pixel output tile: per 64-channel
// chunk it stages the 10x18 halo ONCE (23 KB, reused by all nine taps) plus one 16-KB weight tile
// per tap -> 167 KB instead of 288 KB per nine K steps.  The tap is a shift of the fragment's LDS
// row.  The next chunk's halo streams in as one 1-KB DMA piece per wave per tap.
// (Round 2's first halo kernel - one wave per 32x64 sub-tile, fragments read and waited for before the MFMAs, plan tiles
// 5 / 6 - lost to the K-split kernel below on every shape of every model and was removed in round 4; its ablation is
// profiles/r02_ablate_halo.txt.)  Halo geometry, piece schedule and counted waits: halo_ring.h.
// ---------------------------------------------------------------------------------------------
// Software-pipelined, K-split variant of the halo kernel (plan tile 7).  Measured on the kernel above
// (round 2's ablation builds of that kernel, profiles/r02_ablate_halo.txt): ONE workgroup alone on a CU needs 23 us for its 45 tap
// steps and every phase of a step is exposed - fragment reads 9-11 us, MFMAs 5 us, DMA issue 3 us, barriers and
// launch 6.5 us - because a wave reads its fragments, waits for them and only then issues its MFMAs; overlap
// exists only between two co-resident workgroups.  Here
//   * the four waves are 2 (pixel halves) x 2 (K halves: 32 of the chunk's 64 channels each), so a wave owns a
//     64-pixel x 64-channel accumulator tile: 8 ds_read_b128 per 8 MFMAs instead of 12 (every weight byte in LDS
//     is read by two waves instead of four), the K halves are summed through LDS once, in the epilogue;
//   * the fragments are double-buffered in registers: the reads of tap step s+1 and the DMA of step s+D are
//     issued between the MFMAs of step s (one barrier per step, placed where every wave has drained its reads of
//     step s, so the DMA may refill that ring stage at once: D-1 steps of lead);
//   * the LDS swizzle is keyed on the halo COLUMN ((hx >> 1) & 7) instead of the linear halo row: the 16 lanes of a
//     ds_read_b128 group then cover 16 consecutive columns under every tap shift - conflict-free (the row-keyed
//     swizzle of the kernel above measures 40 % bank-conflict cycles, profiles/r02_sq_counters.json);
//   * the DMA is buffer_load ... lds with a loop-invariant per-lane offset and a scalar running offset, the final chunk
//     of the K range is a separate instantiation (no DMA past the end), and nothing in a tap step is conditional: one
//     basic block per nine steps, so the interleaving above is what the scheduler emits.
// ---------------------------------------------------------------------------------------------

// GNL (round 5): GroupNorm(+SiLU) of the INPUT applied in the halo loader (ResnetBlock2D norm1 -> SiLU -> conv1
// and norm2 -> SiLU -> conv2, unet.py:472-481): x0 is the UN-normalised tensor, its producer left (sum, sumsq) partials
// (gnf_partial / gnf_entries); every workgroup folds the ones of its sample into a per-channel (mean, scale, shift) table in LDS
// (the GNF prologue of gemm_pipe_body) and every wave transforms the halo pieces IT fetched, in place, once they have landed -
// each halo element once per workgroup, not once per tap: read back its own 16 bytes, (x - mean) * scale + shift in packed
// fp16, SiLU in fp32, write back.  Pixels outside the image keep the zeros of the range-checked DMA (the conv pads the
// NORMALISED tensor).  The pieces of the next chunk go out two in step 0, one in steps 1-4 and are transformed in steps 3-7
// (landed: the counted wait of step t covers everything issued in steps <= t - (D - 1)); step 8 reads the halo as before.
// The GroupNorm launch and the round trip of the normalised tensor through HBM are gone.  D <= 4.
template <int D, int DBG = 0, bool GNL = false>
__global__ __launch_bounds__(256, halo_lds_bytes(64, D) <= 80 * 1024 ? 2 : 1) void conv3x3_halo_ks_kernel(IgemmArgs a) {
  constexpr int BN = 64, BM = 128, WR = 2, ROWB = BK * 2;   // ROWB: bytes per LDS row
  static_assert(halo_ks_wait_count<D, WR, GNL>(1) <= 63 && (D - 1) * WR <= 63, "vmcnt range");
  static_assert(halo_lds_bytes(64, D) >= 32 * 1024 + BM * (BN + 8) * 2 + BN * 4, "epilogue buffers fit the K-loop buffers");
  static_assert(!GNL || (D <= 4 && DBG == 0), "GroupNorm in the loader: rings of <= 4 stages");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const Xh = smem;                                          // [2][HALO_LDS_ROWS][BK] halves
  char* const Ws = smem + 2 * HALO_LDS_ROWS * ROWB;               // [D][BN][BK]
  // [BN] bias + timestep-embedding row, written in the epilogue only.  GNL: behind the epilogue's staging buffers (the K-loop
  // buffers are free by then) - its place behind the ring holds the GroupNorm table [Ctot] mean | scale | shift (halves), so the
  // 320-channel convs of the 64x64 level still fit two workgroups per CU (81 792 B with the 4-stage ring)
  float* sconst = GNL ? reinterpret_cast<float*>(smem + 32 * 1024 + BM * (BN + 8) * 2) : reinterpret_cast<float*>(Ws + D * BN * ROWB);
  half_t* const gn_tab = reinterpret_cast<half_t*>(Ws + D * BN * ROWB);
  float* const gn_stat = reinterpret_cast<float*>(Xh + HALO_LDS_ROWS * ROWB);   // [64] mean | [64] rstd: prologue only (halo buffer 1 is idle until step 0)

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wk = wave & 1;
  const int H = a.Ho, W = a.Wo;                 // output (= upsampled input) image; nearest-x2 is folded into the halo gather
  const int ush = a.up >> 1;

  const int n_tiles = (a.N + BN - 1) / BN;
  const int m_tiles = a.B * a.tiles_y * a.tiles_x;
  const int nwg = m_tiles * n_tiles;
  HALO_PLACE_WG                                 // -> bn_idx, mt
  const int b = mt / (a.tiles_y * a.tiles_x);
  const int trem = mt - b * (a.tiles_y * a.tiles_x);
  const int ty = trem / a.tiles_x, tx = trem - ty * a.tiles_x;
  const int y0 = ty * 8, x0 = tx * 16;
  const int n_blk = bn_idx * BN;

  const int nch = a.Ctot / BK;
  const int split = blockIdx.y;
  const int ch_begin = split * a.nk_per_split;
  int ch_end = ch_begin + a.nk_per_split;
  if (ch_end > nch) ch_end = nch;

  // DMA through buffer_load_dwordx4 ... lds: the per-lane part of an address is a loop-invariant 32-bit VGPR offset, the
  // part that advances per tap / chunk is the scalar soffset, so a DMA instruction costs NO vector ALU work inside the
  // tap loop (the 64-bit global_load_lds form needs ~6 VALU per piece; measured in round 2, profiles/r02_ablate_halo.txt: DMA issue was
  // the largest exposed cost of the loop, 4.4 of 16.8 us).  Rows outside the image read as zeros through the buffer
  // range check (offset >= num_records -> 0); weight rows past N are clamped to row N-1 (their outputs are not stored).
  constexpr unsigned kOob = 0x80000000u;
  const __amdgpu_buffer_rsrc_t rs_w =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<half_t*>(a.w), 0, (int)((size_t)a.N * a.K * 2), 0x00020000);
  const size_t xpix = (size_t)a.B * a.Hi * a.Wi;
  unsigned hoff0[HALO_PPW], hoff1[HALO_PPW];            // byte offset of this lane's 16 bytes of halo piece j at channel 0
  // piece of slot j.  The 24th slot (wave 3, j = 5) has no piece of its own: plain kernel - it fetches piece 22 a second time
  // (same bytes); GNL - it must not touch another wave's piece (that wave transforms it in place), so it re-fetches the wave's
  // OWN previous piece, and that piece is transformed once, behind the later of its two fetches (slot 5 instead of slot 4)
  auto piece_of = [&](int j) { return (wave + 4 * j < HALO_PIECES) ? wave + 4 * j : (GNL ? wave + 4 * (j - 1) : HALO_PIECES - 1); };
#pragma unroll
  for (int j = 0; j < HALO_PPW; ++j) {
    const int p = piece_of(j);
    const int hr = 8 * p + (lane >> 3);
    const int hy = hr / HALO_W, hx = hr - hy * HALO_W;
    const int iy = y0 - 1 + hy, ix = x0 - 1 + hx;
    const bool ok = (hr < HALO_ROWS) && iy >= 0 && iy < H && ix >= 0 && ix < W;
    const unsigned pix = (unsigned)((b * a.Hi + (iy >> ush)) * a.Wi + (ix >> ush));   // unet.py:498-500 nearest upsample
    const unsigned sw = (unsigned)(((lane & 7) ^ ((hx >> 1) & 7)) * 16);   // column-keyed swizzle
    hoff0[j] = ok ? pix * (unsigned)a.C0 * 2u + sw : kOob;
    hoff1[j] = ok ? pix * (unsigned)a.C1 * 2u + sw : kOob;
  }
  const int pchunk = tid & 7, lrow = tid >> 3;
  const int wchunk = pchunk ^ ((lrow >> 1) & 7);
  unsigned woff[WR];
#pragma unroll
  for (int i = 0; i < WR; ++i) {
    int n = n_blk + lrow + 32 * i;
    if (n > a.N - 1) n = a.N - 1;
    woff[i] = (unsigned)n * (unsigned)a.K * 2u + (unsigned)wchunk * 16u;
  }

  // the halo of one channel chunk: HALO_SRC (halo_ring.h), single source with GNL
  auto issue_x_piece = [&](int j, const __amdgpu_buffer_rsrc_t& rs, unsigned off, int soff, int xstage) {
    if constexpr ((DBG & 8) != 0) return;
    char* dst = Xh + xstage * (HALO_LDS_ROWS * ROWB) + piece_of(j) * 1024;
    dma16_to_lds(rs, dst, off, soff);
  };
  // GNL: GroupNorm(+SiLU) of slot j of this wave, in place, in halo buffer `xstage` holding channel chunk `ch`.  Only called
  // once the piece has landed (this wave's own DMA: no other wave touches these 16 bytes before the next barrier).
  // Branch-free on purpose (selects, no exec-masked store): a tap step stays ONE basic block, so the MFMA / read / DMA interleaving
  // of the loop body is still what the scheduler emits.
  auto gn_transform = [&](int j, int xstage, int ch) {
    if constexpr (GNL) {
      char* pp = Xh + xstage * (HALO_LDS_ROWS * ROWB) + piece_of(j) * 1024 + lane * 16;
      const half8 raw = *reinterpret_cast<const half8*>(pp);
      half8 v = raw;
      // the lane's channel group is the swizzled 16-B slot it fetched: bits 4-6 of its source offset (pixel offsets are multiples
      // of 128 B); a lane outside the image (kOob) reads some row of the table and stores nothing
      const int k0 = ch * BK + (int)((hoff0[j] >> 4) & 7u) * 8;
      const half8 gm = *reinterpret_cast<const half8*>(gn_tab + k0);
      const half8 gs = *reinterpret_cast<const half8*>(gn_tab + a.Ctot + k0);
      const half8 gh = *reinterpret_cast<const half8*>(gn_tab + 2 * a.Ctot + k0);
      v = __builtin_elementwise_fma(v - gm, gs, gh);   // rounding relative to |x - mean| (gemm_pipe_body GNF)
#pragma unroll
      for (int e = 0; e < 8; ++e) {                    // SiLU in fp32 (unet.py:474, :480: every GroupNorm in front of a 3x3 conv has one)
        const float f = (float)v[e];
        v[e] = (half_t)(f * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * f)));
      }
      // what goes back: the raw bytes for a pixel outside the image (the DMA's zeros: the conv pads the NORMALISED tensor) and for
      // wave 3's slot 4, whose piece slot 5 fetches a second time and transforms (a second landing after a transform here would
      // put raw data back; transforming twice would be wrong; writing raw over raw is harmless)
      const bool keep_raw = hoff0[j] == kOob || (j == HALO_PPW - 2 && wave + 4 * (HALO_PPW - 1) >= HALO_PIECES);
      half8 o;
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = keep_raw ? raw[e] : v[e];
      *reinterpret_cast<half8*>(pp) = o;
    }
  };
  const int total_steps = (ch_end - ch_begin) * 9;
  int iw_koff = ch_begin * BK * 2, iw_tap = 0, iw_step = 0;   // issue cursor of the weight ring (koff in bytes)
  auto issue_next_w = [&]() {
    if constexpr ((DBG & 4) != 0) return;
    char* ws = Ws + ((unsigned)iw_step % D) * (BN * ROWB) + wave * 1024;
#pragma unroll
    for (int i = 0; i < WR; ++i)
      dma16_to_lds(rs_w, ws + i * 4096, woff[i], iw_koff);
    ++iw_step;
    iw_koff += a.Ctot * 2;                                // next tap, same chunk
    if (++iw_tap == 9) {
      iw_tap = 0;
      iw_koff += (BK - 9 * a.Ctot) * 2;                   // tap 0 of the next chunk
    }
  };

  floatx16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int frow = lane & 31, hi = lane >> 5;
  // fragment byte offsets: this wave reads the 16-B chunks kc = 2 * (2 * wk + s) + hi, s = 0, 1 of every row
  int hrb[2];                                             // halo row of this lane's pixel (tap (0,0)), in bytes
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int ml = (wm * 2 + i) * 32 + frow;
    hrb[i] = ((ml >> 4) * HALO_W + (ml & 15)) * ROWB;
  }
  const int hx0 = frow & 15;
  int xsw[3][2], wsw[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int kc = 2 * (2 * wk + s) + hi;
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) xsw[kx][s] = (kc ^ (((hx0 + kx) >> 1) & 7)) * 16;
    wsw[s] = frow * ROWB + (kc ^ ((frow >> 1) & 7)) * 16;
  }

  float const_b = 0.f, const_t = 0.f;
  if (!a.slab && tid < BN && n_blk + tid < a.N) {
    if (a.bias) const_b = a.bias[n_blk + tid];
    if (a.temb) const_t = a.temb[(size_t)b * a.temb_stride + n_blk + tid];
  }

  auto read_step = [&](half8 (&xf)[2][2], half8 (&wf)[2][2], const char* xs, const char* ws, int tap) {
    const int ky = tap / 3, kx = tap - ky * 3;
    const int toffb = (ky * HALO_W + kx) * ROWB;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        if constexpr ((DBG & 2) != 0) asm volatile("" : "=v"(xf[s][i]));
        else xf[s][i] = *reinterpret_cast<const half8*>(xs + hrb[i] + toffb + xsw[kx][s]);
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        if constexpr ((DBG & 2) != 0) asm volatile("" : "=v"(wf[s][j]));
        else wf[s][j] = *reinterpret_cast<const half8*>(ws + j * 32 * ROWB + wsw[s]);
      }
    }
  };
  auto mfma_step = [&](half8 (&xf)[2][2], half8 (&wf)[2][2]) {
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          if constexpr ((DBG & 1) != 0) asm volatile("" ::"v"(wf[s][j]), "v"(xf[s][i]));
          else acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[s][j], xf[s][i], acc[i][j], 0, 0, 0);
        }
  };

  half8 xfA[2][2], wfA[2][2], xfB[2][2], wfB[2][2];
  if (ch_begin < ch_end) {
    // GNL prologue, part 1 (oldest VMEM ops of the wave, before the first DMA; inside this branch, so that no path reaches the
    // join behind it with these loads outstanding - the compiler would drain vmcnt(0), ring and all, there): this sample's partial
    // statistics - eight lanes per group, 16 entries (8 float4) each, entries <= 128; entries past the count are allocated but
    // stale, so they are loaded unconditionally (no branch, no early wait) and masked - and gamma / beta of the channels whose
    // table rows this thread writes
    floatx4 gnl_v[GNL ? 8 : 1];
    float gnl_g[GNL ? 8 : 1], gnl_b[GNL ? 8 : 1];
    if constexpr (GNL) {
      const int g = tid >> 3, j = tid & 7;
      const floatx4* src = reinterpret_cast<const floatx4*>(a.gnf_partial + (((size_t)b * a.gnf_G + (g < a.gnf_G ? g : 0)) * kGnMaxSlabs + j * 16) * 2);
#pragma unroll
      for (int k = 0; k < 8; ++k) gnl_v[k] = src[k];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int k = min(tid + 256 * i, a.Ctot - 1);
        gnl_g[i] = a.gnf_gamma[k];
        gnl_b[i] = a.gnf_beta[k];
      }
    }
    HALO_SRC(GNL, rs0, off0, soff0, ch_begin)
#pragma unroll
    for (int j = 0; j < HALO_PPW; ++j) issue_x_piece(j, rs0, off0[j], soff0, 0);
#pragma unroll
    for (int p = 0; p < D; ++p) {
      asm volatile("" ::: "memory");                      // keep the DMA issue order: the counted wait below relies on it
      if (p < total_steps) issue_next_w();
    }
    if constexpr (GNL) {
      // part 2: fold (fixed order), statistics -> LDS, per-channel table -> LDS; the barrier below publishes it
      float s = 0.f, q = 0.f;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int e0 = (tid & 7) * 16 + 2 * k;            // first of the two entries of this float4
        const bool l0 = e0 < a.gnf_entries, l1 = e0 + 1 < a.gnf_entries;
        s += (l0 ? gnl_v[k][0] : 0.f) + (l1 ? gnl_v[k][2] : 0.f);
        q += (l0 ? gnl_v[k][1] : 0.f) + (l1 ? gnl_v[k][3] : 0.f);
      }
#pragma unroll
      for (int o = 1; o < 8; o <<= 1) {
        s += __shfl_xor(s, o);
        q += __shfl_xor(q, o);
      }
      const int cpg = a.Ctot / a.gnf_G;
      if ((tid & 7) == 0 && (tid >> 3) < a.gnf_G) {
        const float inv_n = 1.0f / ((float)cpg * (float)(a.Hi * a.Wi));
        const float mean = s * inv_n;
        gn_stat[tid >> 3] = mean;
        gn_stat[64 + (tid >> 3)] = rsqrtf(fmaxf(q * inv_n - mean * mean, 0.f) + a.gnf_eps);
      }
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int k = tid + 256 * i;
        if (k < a.Ctot) {
          const int g = k / cpg;
          const float sc = gnl_g[i] * gn_stat[64 + g];
          const half_t mh = (half_t)gn_stat[g];
          gn_tab[k] = mh;
          gn_tab[a.Ctot + k] = (half_t)sc;
          gn_tab[2 * a.Ctot + k] = (half_t)(gnl_b[i] - (gn_stat[g] - (float)mh) * sc);
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    if (total_steps >= D) wait_vmcnt_barrier<(D - 1) * WR>();   // the first halo and weight tile 0 have landed (GNL: and the table is visible)
    else wait_vmcnt_barrier<0>();
    if constexpr (GNL) {   // the first chunk's halo: every wave normalises the pieces it fetched, then all of them meet
#pragma unroll
      for (int j = 0; j < HALO_PPW; ++j) gn_transform(j, 0, ch_begin);
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    }
    read_step(xfA, wfA, Xh, Ws, 0);
  }
  int st = 0;
  // One chunk = nine tap steps.  PAR = parity of the chunk's first step (which register set holds its fragments); LAST = the
  // final chunk of this workgroup's K range: no next halo, no weight tiles past the end, the waits count what is left.
  auto chunk = [&](auto par, auto last, int ch) {
    constexpr int PAR = decltype(par)::value;
    constexpr bool LAST = decltype(last)::value;
    const int xst = (ch - ch_begin) & 1;
    const bool first_chunk = ch == ch_begin;
    HALO_SRC(GNL, rsn, offn, soffn, (LAST ? ch : ch + 1))
#pragma unroll
    for (int tap = 0; tap < 9; ++tap, ++st) {
      auto body = [&](half8 (&cx)[2][2], half8 (&cw)[2][2], half8 (&nx)[2][2], half8 (&nw)[2][2]) {
        if (LAST && tap == 8) {                           // the final step: nothing left to fetch
          mfma_step(cx, cw);
          return;
        }
        // this wave's fragment reads of step st are in registers: after the barrier NO wave reads ring stage st % D any more
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        // weight tile st+1 (at tap 8: and the next halo) has landed
        if constexpr (LAST) halo_ks_wait_last<D, WR>(tap);
        else if (D > 4 && first_chunk) {
          // fewer halo pieces behind the weight tiles than in steady state: count the tiles only - but at tap 8 the next
          // chunk's halo (last piece issued at tap 5, two steps = 2 * WR weight pieces ago) must have landed as well
          if (tap == 8) wait_vmcnt_barrier<((D - 2) * WR < 2 * WR ? (D - 2) * WR : 2 * WR)>();
          else wait_vmcnt_barrier<(D - 2) * WR>();
        }
        else halo_ks_wait<D, WR, GNL>(tap);
        const int tapn = tap == 8 ? 0 : tap + 1;
        const char* xs = Xh + (tap == 8 ? xst ^ 1 : xst) * (HALO_LDS_ROWS * ROWB);
        const char* ws = Ws + ((unsigned)(st + 1) % D) * (BN * ROWB);
        read_step(nx, nw, xs, ws, tapn);                  // fragments of step st+1 -> the other register set
        const bool w_live = !LAST || tap + D < 9;
        if (w_live) issue_next_w();                       // weight tile st+D -> stage st % D
        if constexpr (GNL) {
          if (!LAST) {
            if (tap == 0) {
              issue_x_piece(0, rsn, offn[0], soffn, xst ^ 1);
              issue_x_piece(1, rsn, offn[1], soffn, xst ^ 1);
            } else if (tap <= 4) {
              issue_x_piece(tap + 1, rsn, offn[tap + 1 < HALO_PPW ? tap + 1 : 0], soffn, xst ^ 1);
            }
            // pieces issued in steps <= tap - 3 have landed behind the wait above (D <= 4): normalise them in place
            if (tap == 3) {
              gn_transform(0, xst ^ 1, ch + 1);
              gn_transform(1, xst ^ 1, ch + 1);
            } else if (tap >= 4 && tap <= 7) {
              gn_transform(tap - 2, xst ^ 1, ch + 1);
            }
          }
        } else {
          const bool x_live = !LAST && tap < HALO_PPW;
          if (x_live) issue_x_piece(tap, rsn, offn[tap < HALO_PPW ? tap : 0], soffn, xst ^ 1);
        }
        mfma_step(cx, cw);
        // issue order: an MFMA, then two of the next step's reads ... the DMA pieces behind the later MFMAs
        if constexpr (DBG == 0) {
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
          }
#pragma unroll
          for (int g = 0; g < 3; ++g) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x010, 1, 0);
          }
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        }
      };
      if (((tap + PAR) & 1) == 0) body(xfA, wfA, xfB, wfB);
      else body(xfB, wfB, xfA, wfA);
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  HALO_WALK_CHUNKS(chunk, ch_begin, ch_end)
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __syncthreads();                                        // every wave is out of the K loop: LDS is free

  // ---- epilogue: halo_epilogue.inc, the statement tiles 21 and 25 include as well ----
#define HALO_OUT_PIXEL(y, x) (b * H + y) * W + x
#define HALO_GN_STATS true
#include "halo_epilogue.inc"
#undef HALO_OUT_PIXEL
#undef HALO_GN_STATS
}

// 2 weight stages: two workgroups per CU.  GNL: halo_gnl_lds_bytes (conv_plan.h)
template <int D, int DBG = 0, bool GNL = false>
void launch_halo_ks_d(const IgemmArgs& a, hipStream_t s) {
  const size_t lds = GNL ? halo_gnl_lds_bytes(D, a.Ctot) : halo_lds_bytes(64, D);
  static_assert(halo_lds_bytes(64, D) <= kLdsBudget, "LDS");
  auto k = conv3x3_halo_ks_kernel<D, DBG, GNL>;
  static DynLdsOnce once;
  once.set(k, GNL ? kLdsBudget : lds);   // GNL: the table grows with Ctot - allow the full LDS once
  dim3 grid(a.B * a.tiles_x * a.tiles_y * cdiv(a.N, 64), a.splitk);
  hipLaunchKernelGGL(k, grid, dim3(256), lds, s, a);
}

// stages: the ring depth the plan resolved (GroupNorm in the loader: 3 / 4 only, the table must fit - decode_plan)
void launch_halo_ks_ring(const IgemmArgs& a, int stages, hipStream_t s) {
  if (a.debug >= 32) {   // ablation builds of the 4-stage kernel: debug = 32 + DBG bits
    switch (a.debug - 32) {
      case 1: launch_halo_ks_d<4, 1>(a, s); return;
      case 2: launch_halo_ks_d<4, 2>(a, s); return;
      case 3: launch_halo_ks_d<4, 3>(a, s); return;
      case 4: launch_halo_ks_d<4, 4>(a, s); return;
      case 8: launch_halo_ks_d<4, 8>(a, s); return;
      case 12: launch_halo_ks_d<4, 12>(a, s); return;
      case 13: launch_halo_ks_d<4, 13>(a, s); return;
      case 14: launch_halo_ks_d<4, 14>(a, s); return;
      case 15: launch_halo_ks_d<4, 15>(a, s); return;
      default: break;
    }
  }
  const bool gnl = a.gnf_partial != nullptr;
  switch (stages) {
    case 2: if (!gnl) return launch_halo_ks_d<2>(a, s); break;
    case 3: return gnl ? launch_halo_ks_d<3, 0, true>(a, s) : launch_halo_ks_d<3>(a, s);
    case 4: return gnl ? launch_halo_ks_d<4, 0, true>(a, s) : launch_halo_ks_d<4>(a, s);
    case 6: if (!gnl) return launch_halo_ks_d<6>(a, s); break;
    case 8: if (!gnl) return launch_halo_ks_d<8>(a, s); break;
    default: break;
  }
  SD_REQUIRE(false, kInternal, "halo conv: no kernel with a ring of %d stages (GroupNorm loader %d)", stages, gnl ? 1 : 0);
}

}  // namespace

// GroupNorm(+SiLU) of the input applied in the loader of the 3x3 halo kernel (ConvDesc::gnf_* on a ksize-3 conv): shapes it takes
bool conv_gn_loader_ok(const ConvDesc& d) {
  const int c1 = d.x1 ? d.C1 : 0;
  const int ctot = d.C0 + c1;
  return d.ksize == 3 && d.stride == 1 && d.up == 1 && halo_ks_ok(d) && !d.ln_colsum && !d.out_t && d.out_mode == kOutHalf && !d.debug &&
         d.gnf_groups >= 1 && d.gnf_groups <= 32 && ctot % d.gnf_groups == 0 && ctot <= 2048 && d.Hi == d.Ho && d.Wi == d.Wo &&
         halo_gnl_lds_bytes(3, ctot) <= kLdsBudget;
}

// plan tile 7.  Returns the GroupNorm partial entries per (sample, group) the epilogue wrote (setup_gn_stats).
int launch_halo_ks(const ConvDesc& d, const ConvPlan& p, float* partial, hipStream_t s) {
  IgemmArgs a = planned_args(d, p, partial);
  set_tile_order(a, p.bm, p.bn, true);
  const int gn_entries = setup_gn_stats(d, a, 0);
  a.nk_total = a.Ctot / BK;   // the kernel walks 64-channel chunks
  launch_halo_ks_ring(a, p.stages, s);
  return gn_entries;
}

}  // namespace sd
