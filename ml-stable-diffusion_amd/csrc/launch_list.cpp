#include "launch_list.h"

#include <algorithm>

namespace sd {

hipStream_t open_device(int device) {
  int ndev = 0;
  const hipError_t e = hipGetDeviceCount(&ndev);
  SD_REQUIRE(e == hipSuccess && ndev > 0, kHipError, "no HIP device visible (%s): libsdmi355 has no CPU fallback", hipGetErrorString(e));
  SD_REQUIRE(device >= 0 && device < ndev, kInvalidArgument, "device %d out of range (%d visible)", device, ndev);
  SD_HIP(hipSetDevice(device));
  hipStream_t stream = nullptr;
  SD_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
  device_zero_chunk();   // the conv / GEMM launches only read it
  return stream;
}

hipGraphExec_t capture_graph(hipStream_t stream, const std::function<void()>& body) {
  SD_HIP(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
  hipGraph_t g = nullptr;
  try {
    body();
  } catch (...) {
    (void)hipStreamEndCapture(stream, &g);
    if (g) (void)hipGraphDestroy(g);
    throw;
  }
  SD_HIP(hipStreamEndCapture(stream, &g));
  hipGraphExec_t exec = nullptr;
  const hipError_t e = hipGraphInstantiate(&exec, g, nullptr, nullptr, 0);
  (void)hipGraphDestroy(g);
  SD_REQUIRE(e == hipSuccess, kHipError, "hipGraphInstantiate failed: %s", hipGetErrorString(e));
  return exec;
}

void LaunchList::close() {
  if (!graph && !stream) return;
  (void)hipSetDevice(device);
  if (graph) (void)hipGraphExecDestroy(graph);
  if (stream) {
    (void)hipStreamSynchronize(stream);
    (void)hipStreamDestroy(stream);
  }
  graph = nullptr;
  stream = nullptr;
}

half_t* LaunchList::upload_rows(const WeightStore& ws, const std::vector<std::string>& names, int rows_each, int cols, int cols_padded) {
  const size_t ldw = cols_padded ? cols_padded : cols;
  std::vector<half_t> host(names.size() * rows_each * ldw, (half_t)0);
  for (size_t i = 0; i < names.size(); ++i) {
    const HostTensor& t = ws.get(names[i]);
    SD_REQUIRE(t.numel() == (size_t)rows_each * cols, kInvalidArgument, "%s has %zu elements, expected %d x %d", names[i].c_str(),
               t.numel(), rows_each, cols);
    for (int r = 0; r < rows_each; ++r) {
      const float* src = t.data.data() + (size_t)r * cols;
      half_t* dst = host.data() + (i * rows_each + r) * ldw;
      for (int c = 0; c < cols; ++c) dst[c] = (half_t)src[c];
    }
  }
  half_t* d = arena.alloc_n<half_t>(host.size());
  SD_HIP(hipMemcpy(d, host.data(), host.size() * sizeof(half_t), hipMemcpyHostToDevice));
  return d;
}

float* LaunchList::upload_vec(const WeightStore& ws, const std::vector<std::string>& names, size_t n_each) {
  std::vector<float> host;
  for (const auto& n : names) {
    const HostTensor& t = ws.get(n);
    SD_REQUIRE(t.numel() == n_each, kInvalidArgument, "%s has %zu elements, expected %zu", n.c_str(), t.numel(), n_each);
    host.insert(host.end(), t.data.begin(), t.data.end());
  }
  float* d = arena.alloc_n<float>(host.size());
  SD_HIP(hipMemcpy(d, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
  return d;
}

void LaunchList::gemm(const half_t* x, const half_t* w, const float* bias, const half_t* res, half_t* out, int M, int N, int K,
                      const char* what) {
  ConvDesc d;
  d.x0 = x;
  d.C0 = K;
  d.w = w;
  d.bias = bias;
  d.res = res;
  d.out = out;
  d.B = 1;
  d.Hi = 1;
  d.Wi = M;
  d.Ho = 1;
  d.Wo = M;
  d.N = N;
  SD_REQUIRE(conv_fast_path_ok(d), kUnsupported, "%s GEMM %d x %d not MFMA-tileable", what, N, K);
  ws_need = std::max(ws_need, conv_workspace_bytes(d));
  push([this, d](hipStream_t s) { launch_conv(d, ws_conv, s); });
}

void LaunchList::seal() {
  if (ws_need > 0) {
    ws_conv.partial = reinterpret_cast<float*>(arena.alloc(ws_need));
    ws_conv.partial_bytes = ws_need;
  }
  SD_HIP(hipStreamSynchronize(stream));
}

void LaunchList::launch(bool use_graph, hipEvent_t before) {
  auto run = [this] {
    for (auto& op : ops) op(stream);
  };
  if (use_graph && !graph) {
    run();   // eager first: kernel attributes, code objects
    SD_HIP(hipStreamSynchronize(stream));
    graph = capture_graph(stream, run);
  }
  if (before) SD_HIP(hipEventRecord(before, stream));
  if (use_graph)
    SD_HIP(hipGraphLaunch(graph, stream));
  else
    run();
}

}  // namespace sd
