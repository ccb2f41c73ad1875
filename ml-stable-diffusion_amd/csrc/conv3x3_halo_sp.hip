// Sub-pixel form of the upsampler conv (plan tile 21): nearest-x2 upsample followed by a 3x3 / pad-1 conv, run as FOUR 2x2 convs on
// the low-res image, one per output phase (a, b) = (Y & 1, X & 1) - conv3x3_halo_sp_kernel, its tap-step schedule and its launcher.
//   phase a = 0 reads low-res rows i-1 (w[0]) and i (w[1] + w[2]);  a = 1 reads rows i (w[0] + w[1]) and i+1 (w[2]);  columns alike with b;
//   zero padding of the upsampled image is zero padding of the low-res image.
// 16 tap products per low-res pixel instead of the 36 plan tile 7 spends on it (it multiplies every low-res pixel up to four times
// per tap row and column): 4/9 of the MFMAs.  The weights are folded on the host, once per handle (weight_prep.h subpixel_fold:
// [4 phases][N][4 taps][Ctot], a (phase, n) row K' = 4 Ctot contiguous, tap-major then channel).
// The geometry is tile 7's (conv3x3_halo.hip) on the LOW-RES image: 8x16 pixels per workgroup, the 10x18 halo of a 64-channel chunk
// staged once per chunk by LDS-DMA under the column-keyed swizzle, 2 x 2 waves (pixel halves x K halves), fragments double-buffered in
// registers, one barrier per tap step, split-K slabs over chunks (blockIdx.y), a separate final-chunk instantiation, nothing
// conditional inside a tap step.  What differs:
//   * the halo is the low-res image itself (no x2 in the gather), single source;
//   * the phase is one more factor of the m-tile index;
//   * a chunk runs the FOUR tap steps (ky, kx) in {a, a+1} x {b, b+1}: the LDS row shifts tile 7 uses for those taps, so its bank
//     argument carries over unchanged;
//   * output pixel (i, j) of the tile goes to (2 i + a, 2 j + b) of the 2H x 2W image; a pixel's 64 channels are one 128-B segment.
// The epilogue is the statement tile 7 runs (halo_epilogue.inc, included by both) with that output pixel and without the GroupNorm
// statistics; the workgroup placement is halo_ring.h's.
#include "igemm_device.h"
#include "halo_ring.h"

namespace sd {

namespace {

// ---- the four-step schedule ----
// Per chunk a wave issues its HALO_PPW = 6 halo pieces of the NEXT chunk and, per step, the WR = 2 weight pieces of step s + D:
// 14 DMAs per four steps (tile 7: 24 per nine).  The other halo buffer is free from the barrier of step 0 and is first read behind
// the wait of step 3, so the pieces go out as early as they can: three in step 0, three in step 1, IN FRONT of the step's weight pieces.
constexpr int SP_TAPS = 4;
constexpr int sp_mod4(int t) { return ((t % SP_TAPS) + SP_TAPS) % SP_TAPS; }
constexpr int sp_x_issued(int tap) { return sp_mod4(tap) < 2 ? HALO_PPW / 2 : 0; }
static_assert(2 * (HALO_PPW / 2) == HALO_PPW, "the halo pieces of a wave go out in two equal steps");

// VMEM ops a wave has issued after the weight tile of step s+1 when it waits in step s (tap `tap`).  That tile went out in step
// s+1-D, BEHIND the halo pieces of its own step (which are therefore waited for too); after it, in order, steps s+2-D .. s-1, each
// [halo pieces of the step][WR weight pieces].  At tap 3 the next chunk's halo is read right behind the wait: its last piece went out
// in step 1, followed by that step's weight pieces and all of step 2.
// (The first chunk sees the same counts: the prologue issues whole weight tiles only in the places of taps 2 and 3, which carry no halo pieces.)
template <int D, int WR>
constexpr int sp_wait_count(int tap) {
  int n = 0;
  for (int i = 2; i <= D - 1; ++i) n += WR + sp_x_issued(tap - D + i);
  const int halo = 2 * WR + sp_x_issued(2);
  if (tap == SP_TAPS - 1 && n > halo) n = halo;
  return n;
}
// ... in the final chunk of a workgroup's K range: no halo pieces, weight tiles only while they exist (tap + D < 4); the steps in front
// of the chunk (u < 0: taps 2 and 3 of the previous chunk, or the prologue) issued one whole weight tile and nothing else
template <int D, int WR>
constexpr int sp_wait_count_last(int tap) {
  int n = 0;
  for (int u = tap - D + 2; u <= tap - 1; ++u) n += (u < 0 || u + D < SP_TAPS) ? WR : 0;
  return n;
}
template <int D, int WR>
constexpr bool sp_counts_ok() {
  for (int t = 0; t < SP_TAPS; ++t) {
    if (sp_wait_count<D, WR>(t) > 63 || sp_wait_count<D, WR>(t) < 1) return false;   // counted, and never a full drain inside the loop
    if (sp_wait_count_last<D, WR>(t) > 63) return false;
  }
  return true;
}

struct HaloSpArgs {
  IgemmArgs a;       // Hi x Wi: the low-res image (the halo); Ho x Wo = 2 Hi x 2 Wi; K = 4 Ctot; tiles_x / tiles_y over the low-res image
  int phase_outer;   // 1: the phase is the slowest factor of the m-tile index, 0: the fastest (the four phases of a tile are neighbours)
};

template <int D>
__global__ __launch_bounds__(256, halo_lds_bytes(64, D) <= 80 * 1024 ? 2 : 1) void conv3x3_halo_sp_kernel(HaloSpArgs ha) {
  const IgemmArgs& a = ha.a;
  constexpr int BN = 64, BM = 128, WR = 2, ROWB = BK * 2;   // ROWB: bytes per LDS row
  static_assert(D >= 3 && D <= SP_TAPS, "rings of 3 or 4 stages: a weight tile goes out at most one chunk ahead");
  static_assert(sp_counts_ok<D, WR>() && (D - 1) * WR <= 63, "vmcnt range");
  static_assert(halo_lds_bytes(64, D) >= 32 * 1024 + BM * (BN + 8) * 2 + BN * 4, "epilogue buffers fit the K-loop buffers");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const Xh = smem;                                          // [2][HALO_LDS_ROWS][BK] halves
  char* const Ws = smem + 2 * HALO_LDS_ROWS * ROWB;               // [D][BN][BK]
  float* const sconst = reinterpret_cast<float*>(Ws + D * BN * ROWB);   // [BN] bias + timestep-embedding row, written in the epilogue only

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wk = wave & 1;
  const int H = a.Hi, W = a.Wi;                 // the low-res image: halo and tile grid
  const int Ho = a.Ho, Wo = a.Wo;

  const int n_tiles = (a.N + BN - 1) / BN;
  const int sp_tiles = a.B * a.tiles_y * a.tiles_x;
  const int m_tiles = 4 * sp_tiles;
  const int nwg = m_tiles * n_tiles;
  HALO_PLACE_WG                                 // -> bn_idx, mt
  const int phase = ha.phase_outer ? mt / sp_tiles : mt & 3;
  const int st_idx = ha.phase_outer ? mt - phase * sp_tiles : mt >> 2;
  const int pa = phase >> 1, pb = phase & 1;    // output rows Y = 2 i + pa, columns X = 2 j + pb
  const int b = st_idx / (a.tiles_y * a.tiles_x);
  const int trem = st_idx - b * (a.tiles_y * a.tiles_x);
  const int ty = trem / a.tiles_x, tx = trem - ty * a.tiles_x;
  const int y0 = ty * 8, x0 = tx * 16;
  const int n_blk = bn_idx * BN;

  const int nch = a.Ctot / BK;
  const int split = blockIdx.y;
  const int ch_begin = split * a.nk_per_split;
  int ch_end = ch_begin + a.nk_per_split;
  if (ch_end > nch) ch_end = nch;

  // DMA through buffer_load_dwordx4 ... lds as in tile 7: loop-invariant per-lane offsets, scalar running offsets; rows outside the
  // image read as zeros through the buffer range check, weight rows past N are clamped to row N-1 of the phase (not stored)
  constexpr unsigned kOob = 0x80000000u;
  const __amdgpu_buffer_rsrc_t rs_w =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<half_t*>(a.w), 0, (int)((size_t)4 * a.N * a.K * 2), 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_x =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<half_t*>(a.x0), 0, (int)((size_t)a.B * H * W * a.C0 * 2), 0x00020000);
  unsigned hoff[HALO_PPW];                              // byte offset of this lane's 16 bytes of halo piece j at channel 0
  // piece of slot j; the 24th slot (wave 3, j = 5) fetches piece 22 a second time (same bytes)
  auto piece_of = [&](int j) { return (wave + 4 * j < HALO_PIECES) ? wave + 4 * j : HALO_PIECES - 1; };
#pragma unroll
  for (int j = 0; j < HALO_PPW; ++j) {
    const int p = piece_of(j);
    const int hr = 8 * p + (lane >> 3);
    const int hy = hr / HALO_W, hx = hr - hy * HALO_W;
    const int iy = y0 - 1 + hy, ix = x0 - 1 + hx;
    const bool ok = (hr < HALO_ROWS) && iy >= 0 && iy < H && ix >= 0 && ix < W;
    const unsigned pix = (unsigned)((b * H + iy) * W + ix);
    const unsigned sw = (unsigned)(((lane & 7) ^ ((hx >> 1) & 7)) * 16);   // column-keyed swizzle
    hoff[j] = ok ? pix * (unsigned)a.C0 * 2u + sw : kOob;
  }
  const int pchunk = tid & 7, lrow = tid >> 3;
  const int wchunk = pchunk ^ ((lrow >> 1) & 7);
  unsigned woff[WR];
#pragma unroll
  for (int i = 0; i < WR; ++i) {
    int n = n_blk + lrow + 32 * i;
    if (n > a.N - 1) n = a.N - 1;
    woff[i] = (unsigned)(phase * a.N + n) * (unsigned)a.K * 2u + (unsigned)wchunk * 16u;
  }
  auto issue_x_piece = [&](int j, int ch, int xstage) {
    char* dst = Xh + xstage * (HALO_LDS_ROWS * ROWB) + piece_of(j) * 1024;
    dma16_to_lds(rs_x, dst, hoff[j], ch * BK * 2);
  };
  int iw_koff = ch_begin * BK * 2, iw_tap = 0, iw_step = 0;   // issue cursor of the weight ring (koff in bytes)
  auto issue_next_w = [&]() {
    char* ws = Ws + ((unsigned)iw_step % D) * (BN * ROWB) + wave * 1024;
#pragma unroll
    for (int i = 0; i < WR; ++i)
      dma16_to_lds(rs_w, ws + i * 4096, woff[i], iw_koff);
    ++iw_step;
    iw_koff += a.Ctot * 2;                                // next tap, same chunk
    if (++iw_tap == SP_TAPS) {
      iw_tap = 0;
      iw_koff += (BK - SP_TAPS * a.Ctot) * 2;             // tap 0 of the next chunk
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
  int hrb[2];                                             // halo row of this lane's pixel (halo position (0,0)), in bytes
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int ml = (wm * 2 + i) * 32 + frow;
    hrb[i] = ((ml >> 4) * HALO_W + (ml & 15)) * ROWB;
  }
  const int hx0 = frow & 15;
  int xsw[2][2], wsw[2];                                  // xsw[dx]: the swizzle under the column shift kx = pb + dx
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int kc = 2 * (2 * wk + s) + hi;
#pragma unroll
    for (int dx = 0; dx < 2; ++dx) xsw[dx][s] = (kc ^ (((hx0 + pb + dx) >> 1) & 7)) * 16;
    wsw[s] = frow * ROWB + (kc ^ ((frow >> 1) & 7)) * 16;
  }
  int toffb[SP_TAPS];                                     // LDS row shift of tap t = 2 dy + dx: halo position (pa + dy, pb + dx); workgroup-uniform
#pragma unroll
  for (int t = 0; t < SP_TAPS; ++t) toffb[t] = ((pa + (t >> 1)) * HALO_W + pb + (t & 1)) * ROWB;

  float const_b = 0.f, const_t = 0.f;
  if (!a.slab && tid < BN && n_blk + tid < a.N) {
    if (a.bias) const_b = a.bias[n_blk + tid];
    if (a.temb) const_t = a.temb[(size_t)b * a.temb_stride + n_blk + tid];
  }

  auto read_step = [&](half8 (&xf)[2][2], half8 (&wf)[2][2], const char* xs, const char* ws, int tap) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
#pragma unroll
      for (int i = 0; i < 2; ++i) xf[s][i] = *reinterpret_cast<const half8*>(xs + hrb[i] + toffb[tap] + xsw[tap & 1][s]);
#pragma unroll
      for (int j = 0; j < 2; ++j) wf[s][j] = *reinterpret_cast<const half8*>(ws + j * 32 * ROWB + wsw[s]);
    }
  };
  auto mfma_step = [&](half8 (&xf)[2][2], half8 (&wf)[2][2]) {
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[s][j], xf[s][i], acc[i][j], 0, 0, 0);
  };

  half8 xfA[2][2], wfA[2][2], xfB[2][2], wfB[2][2];
  if (ch_begin < ch_end) {
#pragma unroll
    for (int j = 0; j < HALO_PPW; ++j) issue_x_piece(j, ch_begin, 0);
#pragma unroll
    for (int p = 0; p < D; ++p) {                         // (a K range holds >= SP_TAPS >= D steps)
      asm volatile("" ::: "memory");                      // keep the DMA issue order: the counted waits rely on it
      issue_next_w();
    }
    wait_vmcnt_barrier<(D - 1) * WR>();                   // the first halo and weight tile 0 have landed
    read_step(xfA, wfA, Xh, Ws, 0);
  }
  int st = 0;
  // One chunk = four tap steps, an even number: the fragments of a chunk's first step are always in register set A.  LAST = the final
  // chunk of this workgroup's K range: no next halo, no weight tiles past the end, the waits count what is left.
  auto chunk = [&](auto last, int ch) {
    constexpr bool LAST = decltype(last)::value;
    const int xst = (ch - ch_begin) & 1;
    auto step = [&](auto tap_c, half8 (&cx)[2][2], half8 (&cw)[2][2], half8 (&nx)[2][2], half8 (&nw)[2][2]) {
      constexpr int tap = decltype(tap_c)::value;
      if constexpr (LAST && tap == SP_TAPS - 1) {         // the final step: nothing left to fetch
        mfma_step(cx, cw);
      } else {
        // this wave's fragment reads of step st are in registers: after the barrier NO wave reads ring stage st % D any more
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        // weight tile st+1 (at tap 3: and the next halo) has landed
        wait_vmcnt_barrier<LAST ? sp_wait_count_last<D, WR>(tap) : sp_wait_count<D, WR>(tap)>();
        constexpr int tapn = tap == SP_TAPS - 1 ? 0 : tap + 1;
        const char* xs = Xh + (tap == SP_TAPS - 1 ? xst ^ 1 : xst) * (HALO_LDS_ROWS * ROWB);
        const char* ws = Ws + ((unsigned)(st + 1) % D) * (BN * ROWB);
        read_step(nx, nw, xs, ws, tapn);                  // fragments of step st+1 -> the other register set
        constexpr int nx_pieces = LAST ? 0 : sp_x_issued(tap);
        constexpr bool w_live = !LAST || tap + D < SP_TAPS;
#pragma unroll
        for (int j = 0; j < nx_pieces; ++j) issue_x_piece(tap * (HALO_PPW / 2) + j, ch + 1, xst ^ 1);   // the next chunk's halo
        asm volatile("" ::: "memory");                    // halo pieces in front of the weight pieces: the counts above
        if constexpr (w_live) issue_next_w();             // weight tile st+D -> stage st % D
        mfma_step(cx, cw);
        // issue order: an MFMA, then two of the next step's reads ... the DMA pieces behind the later MFMAs
        constexpr int nv = nx_pieces + (w_live ? WR : 0);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
        }
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        if constexpr (nv >= 1) __builtin_amdgcn_sched_group_barrier(0x010, nv >= 4 ? 2 : 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        if constexpr (nv >= 2) __builtin_amdgcn_sched_group_barrier(0x010, nv >= 5 ? 2 : 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        if constexpr (nv >= 3) __builtin_amdgcn_sched_group_barrier(0x010, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      }
      ++st;
      __builtin_amdgcn_sched_barrier(0);
    };
    step(std::integral_constant<int, 0>{}, xfA, wfA, xfB, wfB);
    step(std::integral_constant<int, 1>{}, xfB, wfB, xfA, wfA);
    step(std::integral_constant<int, 2>{}, xfA, wfA, xfB, wfB);
    step(std::integral_constant<int, 3>{}, xfB, wfB, xfA, wfA);
  };
  if (ch_begin < ch_end) {
    int ch = ch_begin;
    for (; ch + 1 < ch_end; ++ch) chunk(std::false_type{}, ch);
    chunk(std::true_type{}, ch);
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __syncthreads();                                        // every wave is out of the K loop: LDS is free

  // ---- epilogue: tile 7's (halo_epilogue.inc); the output pixel is (2 y + pa, 2 x + pb) of the 2H x 2W image, no GroupNorm statistics ----
#define HALO_OUT_PIXEL(y, x) (b * Ho + 2 * y + pa) * Wo + 2 * x + pb
#define HALO_GN_STATS false
#include "halo_epilogue.inc"
#undef HALO_OUT_PIXEL
#undef HALO_GN_STATS
}

template <int D>
void launch_halo_sp_d(const HaloSpArgs& ha, hipStream_t s) {
  constexpr size_t lds = halo_lds_bytes(64, D);
  static_assert(lds <= 80 * 1024, "two workgroups per CU");
  auto k = conv3x3_halo_sp_kernel<D>;
  static DynLdsOnce once;
  once.set(k, lds);
  const IgemmArgs& a = ha.a;
  dim3 grid(4 * a.B * a.tiles_x * a.tiles_y * cdiv(a.N, 64), a.splitk);
  hipLaunchKernelGGL(k, grid, dim3(256), lds, s, ha);
}

}  // namespace

// plan tile 21.  d is the upsampler's descriptor (ksize 3, up 2, subpix) whose d.w is the folded matrix of subpixel_fold.  The
// epilogue leaves no GroupNorm statistics (returns 0: a GroupNorm behind it runs its own pass).
int launch_halo_sp(const ConvDesc& d, const ConvPlan& p, float* partial, hipStream_t s) {
  SD_REQUIRE(d.subpix && halo_sp_refusal(d) == nullptr && d.w && p.kernel == ConvKernel::HaloSubpix, kInvalidArgument,
             "plan tile 21 (conv3x3_halo_sp.hip): %s", halo_sp_refusal(d) ? halo_sp_refusal(d) : "not a sub-pixel plan");
  HaloSpArgs ha;
  ha.a = planned_args(d, p, partial);
  IgemmArgs& a = ha.a;
  a.K = SP_TAPS * a.Ctot;                                 // a (phase, n) row of the folded matrix
  a.tiles_x = cdiv(d.Wi, 16);                             // the tile grid lies on the low-res image
  a.tiles_y = cdiv(d.Hi, 8);
  a.nk_total = a.Ctot / BK;                               // the kernel walks 64-channel chunks
  a.nk_per_split = cdiv(a.nk_total, p.splitk);
  // tile order as tile 7 chooses it, over the 4 x (low-res tiles) m-tiles and a phase's quarter of the weights
  a.n_fast = choose_tile_order(2.0 * a.B * a.Hi * a.Wi * a.Ctot, 2.0 * a.N * a.K, 4.0 * a.B * a.tiles_x * a.tiles_y, (double)cdiv(a.N, 64), true);
  static const int phase_outer = tune_env_int("SD_SUBPIX_PHASE_OUTER", 0);   // A/B: the phase order in the grid
  ha.phase_outer = phase_outer != 0;
  switch (p.stages) {
    case 3: launch_halo_sp_d<3>(ha, s); break;
    case 4: launch_halo_sp_d<4>(ha, s); break;
    default: SD_REQUIRE(false, kInternal, "sub-pixel halo conv: no kernel with a ring of %d stages", p.stages);
  }
  return 0;
}

}  // namespace sd
