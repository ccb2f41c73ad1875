// Stand-alone host check of the sub-pixel weight fold (csrc/weight_prep.h subpixel_fold, plan tile 21): built with the address and
// undefined-behaviour sanitizers by tests/test_subpixel.py and run on the CPU.  No GPU call is made; nothing here is loaded into Python.
//   hipcc --offload-arch=gfx950 -x hip -O1 -g -Xarch_host -fsanitize=address,undefined \
//         -I ml-stable-diffusion_amd/csrc tools/subpixel_host_check.cpp -o subpixel_host_check && ./subpixel_host_check
#include <cmath>
#include <cstdarg>
#include <cstring>

#include "weight_prep.h"

namespace sd {
void fail(int code, const char* fmt, ...) {   // (the library's own lives in weights.cpp)
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  throw Error(code, buf);
}
}  // namespace sd

// The fold against the identity it stands for, on one low-res pixel neighbourhood: for every phase the four folded taps applied to
// the 3x3 low-res patch equal the nine source taps applied to the upsampled patch.  Weights are multiples of 2^-6, so every sum is exact.
template <typename S>
static int check_shape(int cout, int cin) {
  const size_t n = (size_t)cout * cin * 9;
  std::vector<S> w(n);
  unsigned s = 2463534242u + (unsigned)(cout * 131 + cin * 7);
  for (size_t i = 0; i < n; ++i) {
    s = s * 1664525u + 1013904223u;
    w[i] = (S)((float)((int)(s >> 25) - 64) / 64.0f);   // multiples of 2^-6 in [-1, 1)
  }
  std::vector<sd::half_t> f(sd::subpixel_fold_halves(cout, cin));
  if (f.size() != (size_t)16 * cout * cin) return 1;
  sd::subpixel_fold(w.data(), cout, cin, f.data());
  for (int p = 0; p < 4; ++p) {
    const int a = p >> 1, b = p & 1;
    for (int o = 0; o < cout; ++o)
      for (int c = 0; c < cin; ++c) {
        // source tap (ky, kx) of output (2i + a, 2j + b) reads upsampled (2i + a + ky - 1, 2j + b + kx - 1) = low-res offset
        // floor((a + ky - 1) / 2), floor((b + kx - 1) / 2) in {-1, 0, 1}; collect per low-res offset
        float want[3][3] = {};
        for (int ky = 0; ky < 3; ++ky)
          for (int kx = 0; kx < 3; ++kx) {
            const int ry = (a + ky - 1 + 2) / 2 - 1, rx = (b + kx - 1 + 2) / 2 - 1;
            want[ry + 1][rx + 1] += (float)w[((size_t)o * cin + c) * 9 + ky * 3 + kx];
          }
        float got[3][3] = {};
        for (int t = 0; t < 4; ++t) got[a + (t >> 1)][b + (t & 1)] = (float)f[(((size_t)p * cout + o) * 4 + t) * cin + c];
        for (int y = 0; y < 3; ++y)
          for (int x = 0; x < 3; ++x)
            if (want[y][x] != got[y][x]) return 2;
      }
  }
  return 0;
}

int main() {
  const int shapes[][2] = {{4, 64}, {72, 192}, {64, 128}};
  for (const auto& sh : shapes) {
    int rc = check_shape<float>(sh[0], sh[1]);
    if (!rc) rc = check_shape<sd::half_t>(sh[0], sh[1]) ? 10 : 0;
    if (rc) {
      std::printf("subpixel host check FAILED (%d) at Cout=%d Cin=%d\n", rc, sh[0], sh[1]);
      return 1;
    }
  }
  // refusals: an empty shape, a NULL pointer, a sum outside fp16, a NaN
  int refused = 0;
  std::vector<float> w(2 * 64 * 9, 1.0f);
  std::vector<sd::half_t> f(sd::subpixel_fold_halves(2, 64));
  try { sd::subpixel_fold(w.data(), 0, 64, f.data()); } catch (const sd::Error&) { ++refused; }
  try { sd::subpixel_fold<float>(nullptr, 2, 64, f.data()); } catch (const sd::Error&) { ++refused; }
  w[9 + 4] = w[9 + 5] = 40000.0f;   // (ky 1, kx 1) + (ky 1, kx 2) meet in phase (0, 0) / (1, 0), tap dx = 1
  try { sd::subpixel_fold(w.data(), 2, 64, f.data()); } catch (const sd::Error&) { ++refused; }
  w[9 + 4] = w[9 + 5] = 1.0f;
  w[3] = std::nanf("");
  try { sd::subpixel_fold(w.data(), 2, 64, f.data()); } catch (const sd::Error&) { ++refused; }
  w[3] = 1.0f;
  sd::subpixel_fold(w.data(), 2, 64, f.data());   // and the same buffer folds once the values are in range
  if (refused != 4 || (float)f[0] != 1.0f) {
    std::printf("subpixel host check FAILED: %d of 4 refusals\n", refused);
    return 1;
  }
  std::printf("subpixel host check OK\n");
  return 0;
}
