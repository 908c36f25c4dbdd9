"""Host check of the index-arithmetic temporal shift the GPU shift matrix compares the kernels with (tests/test_shift_matrix_gpu.py):
it equals the oracle's restatement of TemporalShift.shift (STH/ops/temporal_shift.py:28-46) over the whole grid, and the reference's own
output (G3) at shift_div = 8."""
import numpy as np
import pytest
import torch

from oracle import ref_model as O
from tests.helpers import golden, rnd
from tests.test_shift_matrix_gpu import MOVE_C, MOVE_T, shift_by_index


@pytest.mark.parametrize("div", [1, 2, 3, 4, 8, 16])
def test_index_shift_equals_the_oracle(div):
    for t in MOVE_T:
        for c in MOVE_C:
            x = rnd((2 * t, c, 3, 1), 50 + t + c)
            assert torch.equal(shift_by_index(x, t, div), O.temporal_shift(x, t, div)), (div, t, c)


def test_index_shift_equals_the_reference_golden():
    g = golden("g3_temporal_shift")
    xa = torch.arange(2 * 8 * 16 * 3 * 3, dtype=torch.float32).view(16, 16, 3, 3)
    assert np.array_equal(shift_by_index(xa, 8, 8).numpy(), g["out_arange"])
    assert np.array_equal(shift_by_index(rnd((12, 64, 2, 2), 31), 4, 8).numpy(), g["out_rand"])
