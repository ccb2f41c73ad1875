// Shared by the extern "C" translation units (capi.cpp, capi_ops.cpp): exceptions never cross the ABI, and the operator-level
// entry points allocate from a scoped device scratch.
#pragma once
#include <algorithm>
#include <cstdio>
#include <exception>

#include "unet.h"
#include "vae.h"

namespace sd {
extern thread_local std::string g_last_error;
// what a Scratch (below) found when it checked its guards on the way out of the call that guarded() is running
inline thread_local std::string g_guard_report;

template <typename F>
int guarded(F&& f) {
  g_guard_report.clear();
  try {
    f();
    if (!g_guard_report.empty()) {   // a Scratch of f found a guard byte changed (capi_util.h: its destructor cannot throw)
      g_last_error = g_guard_report;
      return kInternal;
    }
    g_last_error.clear();
    return kOk;
  } catch (const Error& e) {
    g_last_error = e.what();
    return e.code;
  } catch (const std::bad_alloc&) {
    g_last_error = "out of host memory";
    return kInternal;
  } catch (const std::exception& e) {
    g_last_error = e.what();
    return kInternal;
  }
}

inline void require_device() {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0)
    fail(kHipError, "no HIP device visible (%s): libsdmi355 has no CPU fallback", hipGetErrorString(e));
}

// Scoped device scratch of the operator-level entry points: the ONE allocator of their device buffers, and the harness contract.
//
// A handle gives a tensor a 256-byte aligned address (Arena::alloc), zero bytes up to the next 256-byte boundary behind it, and then the
// next tensor of the arena; its workspaces are reused dirty.  An entry point gets the stricter version of that: every buffer is
//   [ front guard: kOpFrontGuard bytes of 0xff ][ n elements ][ back guard: >= kOpGuard elements of 0xff ]
// in one allocation, the data 256-byte aligned, the poison (fp16 / fp32 NaN patterns) starting AT element n.  Each request names its kind:
//   dev(n, host)   an input: the host data copied in
//   out(n)         an output or a workspace: the elements start as 0xff too - a skipped element reads back as NaN, a slab or partial
//                  that is read without having been written poisons what is computed from it
//   zeroed(n)      zero-filled: only where the kernel's contract with a handle says zero; the call site says why
// The fills are complete before the call returns (they run on the null stream, which the scratch's non-blocking stream does not wait
// for).  When the scratch goes out of scope it waits for its stream and checks every guard byte of every buffer, front and back, inputs
// and weights included.  A destructor cannot throw: it leaves its finding in g_guard_report, and guarded() - which every entry point
// runs in - turns that into kInternal.  Fills and checks sit outside timed()'s event pair.

constexpr size_t kOpGuard = 4096;        // elements behind every buffer, at least
constexpr size_t kOpFrontGuard = 256;    // bytes in front of every buffer (a multiple of Arena::alloc's alignment)

struct Scratch {
  struct Buf {
    char* base;
    size_t n, elem, back;   // elements, bytes per element, bytes of the back guard
    const char* what;
  };
  const char* entry;        // the entry point's name, for the report
  std::vector<Buf> bufs;
  std::vector<void*> raws;
  hipStream_t stream = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  const int unwinding = std::uncaught_exceptions();
  explicit Scratch(const char* entry_point) : entry(entry_point) {
    require_device();
    device_zero_chunk();   // the conv launches only read it
    SD_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    SD_HIP(hipEventCreate(&e0));
    SD_HIP(hipEventCreate(&e1));
  }
  Scratch(const Scratch&) = delete;
  Scratch& operator=(const Scratch&) = delete;
  ~Scratch() {
    const bool ran = !stream || hipStreamSynchronize(stream) == hipSuccess;
    // (an exception on its way out already carries the call's error: nothing to add to it)
    if (ran && std::uncaught_exceptions() == unwinding && g_guard_report.empty()) check_guards();
    for (const Buf& b : bufs) (void)hipFree(b.base);
    for (void* p : raws) (void)hipFree(p);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (stream) (void)hipStreamDestroy(stream);
  }

  template <typename T>
  T* dev(size_t n, const T* host, const char* what = "input") {
    SD_REQUIRE(host, kInternal, "%s: %s has no host source (an output or workspace is out(), a zero-filled buffer zeroed())", entry, what);
    return reinterpret_cast<T*>(alloc(n, sizeof(T), kOpGuard, what, host, 0));
  }
  // fill: the byte the ELEMENTS start as where 0xff is a value the kernel may write (the guards are 0xff always)
  template <typename T>
  T* out(size_t n, const char* what, size_t guard = kOpGuard, int fill = 0xff) {
    return reinterpret_cast<T*>(alloc(n, sizeof(T), std::max(guard, kOpGuard), what, nullptr, fill));
  }
  template <typename T>
  T* zeroed(size_t n, const char* what) {
    return reinterpret_cast<T*>(alloc(n, sizeof(T), kOpGuard, what, nullptr, 0));
  }
  // unguarded: the cache-flush buffer of SD_BENCH_COLD, which no kernel of the library is handed
  void* raw(size_t bytes) {
    void* p = nullptr;
    SD_HIP(hipMalloc(&p, bytes));
    raws.push_back(p);
    return p;
  }

 private:
  char* alloc(size_t n, size_t elem, size_t guard, const char* what, const void* host, int fill) {
    const size_t bytes = n * elem, back = guard * elem;
    void* p = nullptr;
    SD_HIP(hipMalloc(&p, kOpFrontGuard + bytes + back));
    char* base = reinterpret_cast<char*>(p);
    bufs.push_back(Buf{base, n, elem, back, what});
    char* data = base + kOpFrontGuard;
    SD_HIP(hipMemset(base, 0xff, kOpFrontGuard));
    SD_HIP(hipMemset(data + bytes, 0xff, back));
    if (host && bytes) SD_HIP(hipMemcpy(data, host, bytes, hipMemcpyHostToDevice));
    if (!host && bytes) SD_HIP(hipMemset(data, fill, bytes));
    SD_HIP(hipStreamSynchronize(nullptr));
    return data;
  }
  // the first changed guard byte into g_guard_report: entry point, buffer, side, offset.  Never throws.
  void check_guards() noexcept {
    char text[512] = "";
    try {
      std::vector<uint8_t> g;
      for (size_t i = 0; i < bufs.size() && !text[0]; ++i) {
        const Buf& b = bufs[i];
        g.resize(kOpFrontGuard + b.back);
        if (hipMemcpy(g.data(), b.base, kOpFrontGuard, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(g.data() + kOpFrontGuard, b.base + kOpFrontGuard + b.n * b.elem, b.back, hipMemcpyDeviceToHost) != hipSuccess) {
          snprintf(text, sizeof(text), "%s: the guards of buffer %zu (%s, %zu elements of %zu bytes) could not be read back after the launches",
                   entry, i, b.what, b.n, b.elem);
          break;
        }
        size_t k = kOpFrontGuard;   // front guard: nearest the data first, offset 1 = the byte in front of the first element
        while (k > 0 && g[k - 1] == 0xff) --k;
        if (k > 0) {
          changed(text, sizeof(text), i, "front guard", kOpFrontGuard - k + 1, "in front of the first element", g[k - 1]);
          break;
        }
        for (k = 0; k < b.back && g[kOpFrontGuard + k] == 0xff;) ++k;   // back guard: offset 0 = the byte behind the last element
        if (k < b.back) changed(text, sizeof(text), i, "back guard", k, "behind the last element", g[kOpFrontGuard + k]);
      }
      if (text[0]) g_guard_report = text;
    } catch (...) {   // out of host memory: the call still must not pass as checked
      try {
        g_guard_report = "the operator harness could not check its guards (out of host memory)";
      } catch (...) {
      }
    }
  }
  void changed(char* text, size_t size, size_t i, const char* side, size_t offset, const char* where, int value) const noexcept {
    const Buf& b = bufs[i];
    snprintf(text, size, "%s: the %s of buffer %zu (%s, %zu elements of %zu bytes) was written: byte %zu %s holds 0x%02x, not 0xff", entry, side,
             i, b.what, b.n, b.elem, offset, where, value);
  }

 public:
  template <typename F>
  void timed(int iters, float* ms, F&& launch) {
    if (iters < 1) iters = 1;
    static const bool poison = tune_env_set("SD_POISON_LDS");   // debug: NaN patterns into every CU's LDS in front of the launches
    if (poison) {   // (the result the caller reads is the last launch's)
      launch();     // sets kernel attributes
      launch_lds_poison(stream);
      launch();
      SD_HIP(hipStreamSynchronize(stream));
      if (ms) *ms = 0.f;
      return;
    }
    launch();   // warm (also sets kernel attributes)
    SD_HIP(hipStreamSynchronize(stream));
    // SD_BENCH_COLD=1: every timed launch starts with cold caches like a kernel inside the UNet step does (its
    // weights were last touched 1.7 GB of traffic ago): a 512-MiB fill between launches evicts the L2s and the
    // 256-MiB Infinity Cache; each launch gets its own event pair.  Default: back-to-back launches, operands warm.
    static const bool cold = tune_env_set("SD_BENCH_COLD");
    if (cold) {
      const size_t flush_bytes = (size_t)512 << 20;
      void* flush = raw(flush_bytes);
      float total = 0.f;
      for (int i = 0; i < iters; ++i) {
        SD_HIP(hipMemsetAsync(flush, i & 0xff, flush_bytes, stream));
        SD_HIP(hipEventRecord(e0, stream));
        launch();
        SD_HIP(hipEventRecord(e1, stream));
        SD_HIP(hipEventSynchronize(e1));
        float t = 0.f;
        SD_HIP(hipEventElapsedTime(&t, e0, e1));
        total += t;
      }
      if (ms) *ms = total / (float)iters;
      return;
    }
    SD_HIP(hipEventRecord(e0, stream));
    for (int i = 0; i < iters; ++i) launch();
    SD_HIP(hipEventRecord(e1, stream));
    SD_HIP(hipEventSynchronize(e1));
    float t = 0.f;
    SD_HIP(hipEventElapsedTime(&t, e0, e1));
    if (ms) *ms = t / (float)iters;
  }
};

}  // namespace sd
