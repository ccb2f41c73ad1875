// Stand-alone host check of the W8A8 quantizer and packer (csrc/weight_prep.h): built with the address and undefined-behaviour
// sanitizers by tests/test_w8a8.py and run on the CPU.  No GPU call is made; nothing here is loaded into Python.
//   hipcc --offload-arch=gfx950 -x hip -O1 -g -Xarch_host -fsanitize=address,undefined \
//         -I ml-stable-diffusion_amd/csrc tools/w8a8_host_check.cpp -o w8a8_host_check && ./w8a8_host_check
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

static int check_shape(int N, int Ctot, int k) {
  const size_t per_row = (size_t)Ctot * k * k, n = (size_t)N * per_row;
  std::vector<float> w(n);
  unsigned s = 12345u + (unsigned)(N * 131 + Ctot * 7 + k);
  for (size_t i = 0; i < n; ++i) {
    s = s * 1664525u + 1013904223u;
    w[i] = ((float)(s >> 8) / 8388608.0f - 1.0f) * (1.0f + (float)(i % 7));
  }
  std::fill(w.begin(), w.begin() + per_row, 0.0f);   // an all-zero row
  w[per_row] = -65504.0f;                             // a row whose absmax is negative and as large as fp16 goes
  std::vector<int8_t> q(n), stream(sd::wstream_i8_bytes(N, Ctot, k), (int8_t)-128);
  std::vector<float> scale(N);
  const double err = sd::w8a8_quantize_weight(w.data(), N, per_row, q.data(), scale.data());
  if (!(err >= 0.0) || scale[0] != 1.0f || q[per_row] != -127) return 1;
  for (size_t i = 0; i < n; ++i)
    if (q[i] == -128) return 2;
  sd::wstream_i8_pack(q.data(), N, Ctot, k, stream.data());
  // every element lands exactly once: the multiset of values is kept and the first lane's first byte is q[0][0][tap 0]
  long sum_q = 0, sum_s = 0;
  for (size_t i = 0; i < n; ++i) sum_q += q[i], sum_s += stream[i];
  if (sum_q != sum_s || stream[0] != q[0]) return 3;
  const sd::W8A8HostCopy h = sd::w8a8_host_copy("check", q.data(), scale.data(), 3.5f, N, Ctot, k);
  if (h.stream != stream || h.cs.size() != (size_t)N || !(h.inv_s > 0.f)) return 4;
  return 0;
}

int main() {
  const int shapes[][3] = {{32, 64, 3}, {64, 192, 3}, {32, 64, 1}};
  for (const auto& sh : shapes) {
    const int rc = check_shape(sh[0], sh[1], sh[2]);
    if (rc) {
      std::printf("w8a8 host check FAILED (%d) at N=%d Ctot=%d k=%d\n", rc, sh[0], sh[1], sh[2]);
      return 1;
    }
  }
  // refusals: a non-finite weight, a -128 value, a range that is no positive number
  int refused = 0;
  {
    std::vector<float> w(64, 1.0f), sc(2);
    std::vector<int8_t> q(64);
    w[5] = NAN;
    try { sd::w8a8_quantize_weight(w.data(), 2, 32, q.data(), sc.data()); } catch (const sd::Error&) { ++refused; }
    std::vector<int8_t> q2(32 * 32, (int8_t)1);
    std::vector<float> s2(32, 0.5f);
    q2[7] = -128;
    try { sd::w8a8_host_copy("check", q2.data(), s2.data(), 1.0f, 32, 32, 1); } catch (const sd::Error&) { ++refused; }
    q2[7] = 0;
    try { sd::w8a8_host_copy("check", q2.data(), s2.data(), 0.0f, 32, 32, 1); } catch (const sd::Error&) { ++refused; }
  }
  if (refused != 3) {
    std::printf("w8a8 host check FAILED: %d of 3 refusals\n", refused);
    return 1;
  }
  std::printf("w8a8 host check OK\n");
  return 0;
}
