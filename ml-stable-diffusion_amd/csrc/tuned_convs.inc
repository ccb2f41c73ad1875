// Plan table: {kind, ksize, stride, up, Ctot, N, M, tile, staging, splitk}  (kind: conv_plan.cpp choose_plan; staging:
// conv_plan.cpp decode_plan).  Measured IN SEQUENCE on MI355X by tools/tune_plans.py (per-op HIP events of the eager SD2.1-base
// CFG-batch-2 step, caches as cold as in the step): entries beat the previous plan by more than 3 %.
// other BASELINE configs (tools/gpu_r2_q.sh): shapes that SD2.1-base does not have
// round 3: the software-pipelined 1x1 GEMM kernel (gemm_pipe_kernel, first with its 3-stage ring), accepted END TO END by
// tools/tune_e2e.py on the SD2.1-base CFG-batch-2 step (5.886 -> 5.751 ms on the tuning box, profiles/r03_tune_e2e_pipe.log);
// listed first: the first matching row wins
// round 5: the weight-streaming kernel of wstream.hip (tile 9; its code names the waves per workgroup) on the 8x8 level
{0, 3, 1, 1, 1280, 1280, 128, 9, 0, 1},
{0, 3, 1, 1, 2560, 1280, 128, 9, 0, 1},
// round 9: the merged transformer tail [Wp W2 | Wp] [g | h2] (K = 5120 + 1280, two sources) keeps the plan of the 5120 -> 1280 GEMM it
// replaces with a fifth split: 20 K steps per split as measured there, four splits on g and one on h2 (the source boundary is a
// split boundary); accepted with the merge itself by the step A/B of profiles/r09_tail_merge_step_ab.txt; ten other plans (4 / 10
// splits, the other tiles, a 3-stage ring) all lost to these end to end (tools/tune_e2e.py, same file)
{0, 1, 1, 1, 6400, 1280, 512, 1, 3, 5},
{0, 1, 1, 1, 6400, 1280, 128, 3, 3, 5},
{0, 1, 1, 1, 6400, 1280, 1152, 2, 6, 2},  // SDXL-base 96x96: the merged tail on the plan of the 5120 -> 1280 GEMM it replaces (tools/tune_e2e.py, 15.188 -> 15.182 ms; five other plans lost)
{0, 1, 1, 1, 5120, 1280, 512, 1, 3, 4},  // r6 re-tune on the final library (tools/tune_e2e.py, 4.397 -> 4.377 ms with the 640 -> 640 conv row below; was 2, 6, 2)
{3, 1, 1, 1, 320, 960, 8192, 1, 8, 1},  // r4: 2-stage pipelined ring accepted end to end (tools/tune_e2e.py, 4.761 -> 4.698 ms; was tile 3 staging 6)
{0, 1, 1, 1, 1280, 320, 8192, 3, 6, 1},
{3, 1, 1, 1, 640, 1920, 2048, 4, 8, 1},  // r4: 2-stage pipelined ring accepted end to end (tools/tune_e2e.py, 4.761 -> 4.698 ms; was tile 3 staging 6)
{0, 1, 1, 1, 640, 320, 8192, 3, 6, 1},
{0, 1, 1, 1, 960, 320, 8192, 3, 6, 1},
{0, 1, 1, 1, 1280, 1280, 1152, 3, 6, 1},  // SDXL-base 96x96, r3 end to end (17.60 -> 17.22 ms)
{2, 1, 1, 1, 1280, 10240, 1152, 1, 8, 1},  // SDXL-base 96x96: 2-stage pipelined ring, end to end 18.24 -> 17.82 ms (profiles/r03_exp_pipe_d2.txt)
{2, 1, 1, 1, 640, 5120, 4608, 1, 8, 1},  // SDXL-base 96x96: 2-stage pipelined ring, end to end 17.65 -> 17.59 ms
{2, 1, 1, 1, 768, 6144, 4608, 1, 8, 1},  // SDXL-refiner 96x96: 2-stage pipelined ring, end to end 14.694 -> 14.552 ms (tools/tune_e2e.py, r4)
{2, 1, 1, 1, 1536, 12288, 1152, 1, 8, 1},  // SDXL-refiner 96x96: 2-stage pipelined ring, end to end 14.552 -> 14.435 ms
{0, 1, 1, 1, 5120, 1280, 1152, 2, 6, 2},  // SDXL-base 96x96, r3 end to end
{1, 1, 1, 1, 1280, 1280, 1152, 3, 6, 1},  // SDXL-base 96x96, r3 end to end
{0, 1, 1, 1, 640, 640, 4608, 2, 6, 1},  // SDXL-base 96x96, r3 end to end
{0, 1, 1, 1, 2560, 640, 4608, 4, 6, 1},  // SDXL-base 96x96, r3 end to end
{0, 1, 1, 1, 2560, 1280, 1152, 2, 6, 1},  // SDXL-base 96x96, r3 end to end
{0, 3, 1, 1, 640, 640, 2048, 7, 4, 1},  // r6 re-tune end to end (six-stage weight ring; was staging 3, the r3 conv re-tune)
{0, 1, 1, 1, 768, 768, 4608, 2, 6, 1},  // SDXL-refiner 96x96, r3 end to end (17.65 -> 16.56 ms)
{0, 1, 1, 1, 3072, 768, 4608, 2, 6, 1},  // SDXL-refiner 96x96, r3 end to end
{0, 1, 1, 1, 1536, 1536, 1152, 3, 6, 1},  // SDXL-refiner 96x96, r3 end to end
{0, 1, 1, 1, 6144, 1536, 1152, 3, 6, 1},  // SDXL-refiner 96x96, r3 end to end
{3, 1, 1, 1, 768, 2304, 4608, 4, 0, 1},  // SDXL-refiner 96x96, r3 end to end (15.79 -> 15.61 ms)
{3, 1, 1, 1, 1536, 4608, 1152, 4, 0, 1},  // SDXL-refiner 96x96, r3 end to end
{3, 1, 1, 1, 1280, 3840, 1152, 1, 8, 1},  // SDXL-base 96x96: 2-stage pipelined ring, end to end 17.82 -> 17.65 ms
{3, 1, 1, 1, 640, 1920, 4608, 4, 0, 1},  // SDXL-base 96x96: accepted end to end (tools/gpu_r2_w.sh, 18.30 -> 16.89 ms per step)
{0, 1, 1, 1, 1920, 640, 4608, 4, 2, 1},  // SDXL-base 96x96: accepted end to end (tools/gpu_r2_w.sh, 18.30 -> 16.89 ms per step)
{0, 3, 2, 1, 320, 320, 4608, 4, 3, 1},  // SDXL-base 96x96: accepted end to end (tools/gpu_r2_w.sh, 18.30 -> 16.89 ms per step)
{0, 3, 2, 1, 640, 640, 1152, 3, 2, 4},  // SDXL-base 96x96: accepted end to end (tools/gpu_r2_w.sh, 18.30 -> 16.89 ms per step)
{0, 1, 1, 1, 1920, 1280, 1152, 2, 3, 1},  // SDXL-base 96x96: accepted end to end (tools/gpu_r2_w.sh, 18.30 -> 16.89 ms per step)
{0, 3, 1, 1, 1280, 1280, 1152, 7, 4, 1},  // SDXL-base 96x96: accepted end to end
{0, 3, 1, 1, 640, 640, 4608, 7, 2, 1},  // SDXL-base 96x96: accepted end to end
{0, 3, 1, 1, 320, 320, 18432, 7, 3, 1},  // SDXL-base 96x96: accepted end to end
{0, 3, 1, 1, 2560, 1280, 1152, 7, 4, 1},  // SDXL-base 96x96: accepted end to end
{0, 3, 1, 1, 640, 320, 18432, 7, 3, 1},  // SDXL-base 96x96: accepted end to end
{0, 3, 1, 2, 640, 640, 18432, 7, 2, 1},  // SDXL-base 96x96: accepted end to end
{0, 3, 1, 1, 1920, 640, 4608, 7, 3, 1},  // SDXL-base 96x96: accepted end to end
{0, 3, 1, 2, 1280, 1280, 4608, 7, 3, 1},  // SDXL-base 96x96: accepted end to end
{0, 3, 1, 1, 960, 320, 18432, 7, 3, 1},  // SDXL-base 96x96: accepted end to end
{0, 3, 1, 1, 1280, 640, 4608, 7, 2, 1},  // SDXL-base 96x96: accepted end to end
{0, 3, 1, 1, 960, 640, 4608, 7, 2, 1},  // SDXL-base 96x96: accepted end to end
{0, 3, 1, 1, 1920, 1280, 1152, 7, 4, 1},  // SDXL-base 96x96: accepted end to end
// K-split halo kernel on the 8x8 level, the upsample convs and refined ring depths: accepted END TO END (graph replay of the step)
{0, 3, 1, 1, 1280, 1280, 128, 7, 4, 5},  // accepted end to end (tools/tune_e2e.py)
{0, 3, 1, 1, 1280, 1280, 512, 7, 4, 3},  // accepted end to end (tools/tune_e2e.py)
{0, 3, 1, 1, 2560, 1280, 128, 7, 4, 5},  // accepted end to end (tools/tune_e2e.py)
{0, 3, 1, 2, 1280, 1280, 2048, 7, 3, 1},  // accepted end to end (tools/tune_e2e.py)
{0, 3, 1, 1, 2560, 1280, 512, 7, 4, 3},  // accepted end to end (tools/tune_e2e.py)
{0, 3, 1, 2, 640, 640, 8192, 7, 3, 1},  // accepted end to end (tools/tune_e2e.py)
{0, 3, 1, 1, 1920, 1280, 512, 7, 4, 3},  // accepted end to end (tools/tune_e2e.py)
{0, 3, 1, 2, 1280, 1280, 512, 7, 4, 3},  // accepted end to end (tools/tune_e2e.py)
// round-2 K-split software-pipelined halo kernel (tile 7), measured in sequence (tools/gpu_r2_j.sh)
{0, 3, 1, 1, 320, 320, 8192, 7, 3, 1},  // 242.4 -> 184.1 us per step (in sequence)
{0, 3, 1, 1, 640, 320, 8192, 7, 3, 1},  // 120.4 -> 79.9 us per step (in sequence)
{0, 3, 1, 1, 960, 320, 8192, 7, 3, 1},  // 90.6 -> 54.5 us per step (in sequence)
{0, 3, 1, 1, 1920, 640, 2048, 7, 3, 3},  // 90.5 -> 54.7 us per step (in sequence)
{0, 3, 1, 1, 1280, 640, 2048, 7, 3, 3},  // 66.9 -> 43.4 us per step (in sequence)
{0, 3, 1, 1, 960, 640, 2048, 7, 3, 3},  // 51.7 -> 36.8 us per step (in sequence)
{0, 3, 1, 1, 320, 640, 2048, 7, 3, 1},  // 33.2 -> 25.2 us per step (in sequence)
{0, 3, 1, 1, 640, 1280, 512, 7, 3, 4},  // 29.0 -> 24.4 us per step (in sequence)
// in-sequence entries of the first round-2 sweep that still stand
{0, 1, 1, 1, 1280, 1280, 512, 3, 3, 1},  // 437.7 -> 263.0 us per step (in sequence)
{0, 1, 1, 1, 640, 640, 2048, 3, 2, 1},  // 303.2 -> 242.8 us per step (in sequence)
{0, 1, 1, 1, 320, 320, 8192, 3, 8, 1},  // r4: 2-stage pipelined ring accepted end to end (tools/tune_e2e.py, 4.761 -> 4.698 ms; was tile 3 staging 2)
{2, 1, 1, 1, 640, 5120, 2048, 4, 0, 1},  // 239.0 -> 163.6 us per step (in sequence)
{2, 1, 1, 1, 320, 2560, 8192, 1, 8, 1},  // r4: 2-stage pipelined ring accepted end to end (tools/tune_e2e.py, 4.761 -> 4.698 ms; was tile 4 staging 0)
{2, 1, 1, 1, 1280, 10240, 512, 4, 0, 1},  // 170.3 -> 163.4 us per step (in sequence)
{0, 1, 1, 1, 2560, 640, 2048, 3, 3, 1},  // 147.5 -> 126.6 us per step (in sequence)
{3, 1, 1, 1, 1280, 3840, 512, 4, 2, 1},  // 116.5 -> 91.0 us per step (in sequence)
{1, 1, 1, 1, 1280, 1280, 512, 3, 3, 1},  // 106.8 -> 72.8 us per step (in sequence)
{1, 1, 1, 1, 640, 640, 2048, 4, 2, 1},  // 102.2 -> 63.6 us per step (in sequence)
{1, 1, 1, 1, 320, 320, 8192, 3, 0, 1},  // 101.6 -> 61.6 us per step (in sequence)
{0, 1, 1, 1, 2560, 1280, 128, 3, 3, 4},  // 72.0 -> 42.1 us per step (in sequence)
{0, 1, 1, 1, 1280, 1280, 128, 3, 3, 4},  // 56.8 -> 50.2 us per step (in sequence)
{0, 1, 1, 1, 2560, 1280, 512, 3, 3, 1},  // 50.2 -> 37.7 us per step (in sequence)
{0, 1, 1, 1, 1920, 640, 2048, 3, 3, 1},  // 31.4 -> 20.6 us per step (in sequence)
{0, 1, 1, 1, 1920, 1280, 512, 3, 3, 1},  // 28.7 -> 15.8 us per step (in sequence)
{0, 3, 2, 1, 1280, 1280, 128, 4, 3, 8},  // 28.3 -> 23.3 us per step (in sequence)
{0, 3, 2, 1, 320, 320, 2048, 3, 2, 4},  // 27.8 -> 19.9 us per step (in sequence)
{0, 1, 1, 1, 5120, 1280, 128, 3, 3, 4},  // 25.1 -> 17.0 us per step (in sequence)
{2, 1, 1, 1, 1280, 10240, 128, 4, 3, 1},  // 25.0 -> 18.3 us per step (in sequence)
{0, 1, 1, 1, 1280, 640, 2048, 3, 3, 1},  // 23.2 -> 16.0 us per step (in sequence)
{3, 1, 1, 1, 1280, 3840, 128, 3, 3, 1},  // 21.8 -> 14.6 us per step (in sequence)
{0, 3, 2, 1, 640, 640, 512, 4, 3, 4},  // 21.7 -> 20.7 us per step (in sequence)
{1, 1, 1, 1, 1280, 1280, 128, 3, 3, 1},  // 21.4 -> 14.4 us per step (in sequence)
{0, 1, 1, 1, 960, 640, 2048, 3, 3, 1},  // 19.2 -> 13.8 us per step (in sequence)
{0, 1, 1, 1, 640, 1280, 512, 3, 3, 1},  // 13.6 -> 9.6 us per step (in sequence)
{0, 1, 1, 1, 320, 640, 2048, 3, 2, 1},  // 10.6 -> 9.4 us per step (in sequence)
// round-1 entries (stand-alone microbenchmarks) that the in-sequence sweep did not improve on
