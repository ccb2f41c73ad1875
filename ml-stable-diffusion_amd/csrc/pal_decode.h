// Palette indices -> MFMA weight fragments, as the kernels that read palettized weights do it (wstream.hip plan tile 14, smgemm.hip
// plan tile 15; the streams are weight_prep.h's).  A lane owns a little-endian bit stream of NBITS-wide fields in 16-byte words it
// holds in registers; field f lies at bits [f * NBITS, (f + 1) * NBITS).  Fragment `frag` of the stream is its fields 8 frag .. 8 frag + 7.
#pragma once
#include <type_traits>

#include "sd_common.h"

namespace sd {

// One fragment: every index is one 2-byte LDS read of the LUT (`lutp`: kPalLutHalves entries in LDS), placed in the low or high half
// of a fragment register; a field that straddles a dword is one funnel shift (it ends inside the stream's words).  `frag` must be a
// constant where the call is inlined - a constexpr, or the variable of an unrolled loop - so that every field position is one: the
// code then has no variable shift.
template <int NBITS, int Q>
__device__ __forceinline__ half8 pal_decode(const uintx4 (&wq)[Q], int frag, const unsigned short* lutp) {
  constexpr unsigned MASK = (1u << NBITS) - 1u;
  uintx4 pk = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int bit = (frag * 8 + e) * NBITS, dw = bit >> 5, sh = bit & 31;
    const unsigned lo = wq[dw >> 2][dw & 3];
    unsigned idx;
    if (sh + NBITS <= 32) {
      idx = (lo >> sh) & MASK;
    } else {
      const int dn = dw + 1;
      idx = __builtin_amdgcn_alignbit(wq[dn >> 2][dn & 3], lo, sh) & MASK;
    }
    const unsigned v = lutp[idx];
    pk[e >> 1] = (e & 1) ? (pk[e >> 1] | (v << 16)) : v;
  }
  return __builtin_bit_cast(half8, pk);
}

// f(std::integral_constant<int, NBITS>{}) for the index width of a descriptor (palette_bits_ok)
template <typename F>
void pal_dispatch_bits(int nbits, const char* what, F&& f) {
  switch (nbits) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 6: f(std::integral_constant<int, 6>{}); break;
    case 8: f(std::integral_constant<int, 8>{}); break;
    default: fail(kInternal, "%s: no kernel for %d-bit indices", what, nbits);
  }
}

}  // namespace sd
