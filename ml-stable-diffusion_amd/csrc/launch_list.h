// What a model handle owns that is not model-specific: its device and stream, the arena, the launch list, the conv / GEMM
// workspace and the captured graph - and the three things every handle does the same way: open a device, capture a graph,
// upload checkpoint rows.  The text encoder and the safety checker are LaunchLists; the UNet / ControlNet and VAE handles hold one
// in their common base (net.h: `ops` is their main list, `graph` one captured forward) and walk it through Net::run_ops_on.
#pragma once
#include <functional>

#include "kernels.h"
#include "weights.h"

namespace sd {

// One entry of a handle's launch list: the launch closure plus what the per-op profile reports about it.
struct Op {
  std::function<void(hipStream_t)> fn;
  std::string label;   // "<kind> <shape> <checkpoint name>"
  double flop = 0;     // algorithmic FLOP (2 per MAC) of MFMA ops, 0 for bandwidth ops
  Op() = default;
  template <class F, class = std::enable_if_t<!std::is_same<std::decay_t<F>, Op>::value>>
  Op(F&& f) : fn(std::forward<F>(f)) {}
  void operator()(hipStream_t s) const { fn(s); }
};

// Makes `device` current and returns a new non-blocking stream on it: kHipError without a GPU (there is no CPU fallback),
// kInvalidArgument for an index out of range.  Also allocates the conv kernels' zero chunk, so that it is never first
// allocated under graph capture.
hipStream_t open_device(int device);

// Stream capture that cannot leave the stream in capture mode: an op that throws between Begin and End (SD_HIP /
// SD_REQUIRE inside a launch) ends and discards the capture before the error travels on.
hipGraphExec_t capture_graph(hipStream_t stream, const std::function<void()>& body);

struct LaunchList {
  int device = 0;
  hipStream_t stream = nullptr;
  hipGraphExec_t graph = nullptr;
  Arena arena;
  std::vector<Op> ops;
  ConvWorkspace ws_conv;
  size_t ws_need = 0;

  LaunchList() = default;
  LaunchList(const LaunchList&) = delete;
  ~LaunchList() { close(); }
  void open(int dev) {
    device = dev;
    stream = open_device(dev);
  }
  void close();   // the graph, then the stream (drained first); the arena goes with the object
  // fp16 rows of the named matrices (rows_each x cols checkpoint values each) stacked along the rows, stored with
  // `cols_padded` (>= cols, zeros behind) halves per row
  half_t* upload_rows(const WeightStore& ws, const std::vector<std::string>& names, int rows_each, int cols, int cols_padded = 0);
  // fp32 copies of the named tensors (n_each elements each), one behind the other
  float* upload_vec(const WeightStore& ws, const std::vector<std::string>& names, size_t n_each);
  // out[M][N] = x[M][K] . w[N][K]^T + bias (+ res): the UNet's 1x1 implicit-GEMM path over M ragged rows; `what` names the
  // handle in the error text
  void gemm(const half_t* x, const half_t* w, const float* bias, const half_t* res, half_t* out, int M, int N, int K, const char* what);
  template <class F>
  void push(F&& fn) {
    ops.emplace_back(std::forward<F>(fn));
  }
  void seal();                    // end of construction: the workspace the GEMMs asked for, uploads complete
  // The whole list on `stream`: eagerly, or as one graph replay (the first call runs it eagerly once - kernel attributes, code
  // objects - and captures it).  `before`: an event recorded in front of the pass that counts (the replay, not the capture).
  void launch(bool use_graph, hipEvent_t before = nullptr);
};

}  // namespace sd
