// Shared by the extern "C" translation units (capi.cpp, capi_ops.cpp): exceptions never cross the ABI, and the operator-level
// entry points allocate from a scoped device scratch.
#pragma once
#include <algorithm>

#include "unet.h"
#include "vae.h"

namespace sd {
extern thread_local std::string g_last_error;

template <typename F>
int guarded(F&& f) {
  try {
    f();
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

// scoped device scratch for the operator-level entry points
struct Scratch {
  std::vector<void*> ptrs;
  hipStream_t stream = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  Scratch() {
    require_device();
    device_zero_chunk();   // the conv launches only read it
    SD_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    SD_HIP(hipEventCreate(&e0));
    SD_HIP(hipEventCreate(&e1));
  }
  ~Scratch() {
    if (stream) (void)hipStreamSynchronize(stream);
    for (void* p : ptrs) (void)hipFree(p);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (stream) (void)hipStreamDestroy(stream);
  }
  template <typename T>
  T* dev(size_t n, const T* host = nullptr) {
    void* p = nullptr;
    SD_HIP(hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T)));
    ptrs.push_back(p);
    if (host)
      SD_HIP(hipMemcpy(p, host, n * sizeof(T), hipMemcpyHostToDevice));
    else
      SD_HIP(hipMemset(p, 0, std::max<size_t>(n, 1) * sizeof(T)));
    return reinterpret_cast<T*>(p);
  }
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
      void* flush = dev<char>(flush_bytes);
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
