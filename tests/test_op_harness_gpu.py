"""The operator harness can fail.  Every sd_op_* entry point allocates its device buffers from one guarded allocator
(csrc/capi_util.h Scratch): 0xff guards in front of and behind every buffer, outputs and workspaces poisoned, every guard checked
after the last launch.  sd_op_harness_selftest drives an element-wise kernel (float32(src)) with one deliberate off-by-one per mode,
made by the entry point's own pointer arithmetic inside its own allocations - nothing here can touch memory the call does not own.
The operator suite relies on exactly these six behaviours to turn each of its ragged-shape cases into a bounds test."""
import numpy as np
import pytest

from python_hip_stable_diffusion import _lib

pytestmark = pytest.mark.gpu

N = 1003                                   # odd, four workgroups of 256
SRC = (np.arange(N, dtype=np.float32) % 97 - 48.0).astype(np.float16) / 8      # exact in fp16, no NaN, first value non-zero
SD_OK, SD_ERR_INTERNAL = 0, -5


def run(mode):
    return _lib.harness_selftest(mode, SRC)


def test_clean_launch_passes():
    status, text, dst = run(0)
    assert status == SD_OK and np.array_equal(dst, SRC.astype(np.float32)), (status, text)


def test_write_behind_an_output_is_caught():
    status, text, _ = run(1)
    assert status == SD_ERR_INTERNAL and "harness_selftest" in text and "dst" in text and "back guard" in text and "byte 0 " in text, (status, text)


def test_write_in_front_of_an_output_is_caught():
    status, text, _ = run(2)
    assert status == SD_ERR_INTERNAL and "harness_selftest" in text and "dst" in text and "front guard" in text and "byte 1 " in text, (status, text)


def test_write_into_the_guard_of_an_input_is_caught():
    status, text, _ = run(3)
    assert status == SD_ERR_INTERNAL and "harness_selftest" in text and "src" in text and "back guard" in text, (status, text)


def test_skipped_output_element_reads_back_nan():
    status, text, dst = run(4)
    assert status == SD_OK and np.isnan(dst[-1]) and np.array_equal(dst[:-1], SRC[:-1].astype(np.float32)), (status, text, dst[-3:])


def test_read_behind_an_input_poisons_the_dependent_output():
    status, text, dst = run(5)
    assert status == SD_OK and np.isnan(dst[-1]) and np.array_equal(dst[:-1], SRC[1:].astype(np.float32)), (status, text, dst[-3:])
