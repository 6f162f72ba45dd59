"""The uniform replay draw as a plain-integer oracle, checked on its own.

Probe `probe` of step-epoch `epoch` takes the first two philox words of the
PER draw's own stream, x = (w0 << 32) | w1, and lands on slot
floor(x * n / 2^64) of the n occupied rows.  The product is exact in Python
integers; the kernel takes the high half of a 64 x 64-bit multiply.  The
oracle is `uniform_batch` of tests/_oracles.py, which the GPU tests
(test_gpu_uniform_replay.py) use too.
"""

import numpy as np
import pytest

from _oracles import philox4x32_10, uniform_batch


DRAWS = 10 ** 4


@pytest.mark.parametrize("n", [1, 2 ** 24 + 1, 10 ** 8])
def test_every_index_is_below_n(n):
    idx = uniform_batch(21, 1, DRAWS, n)
    assert idx.min() >= 0 and idx.max() < n
    if n == 1:
        assert (idx == 0).all()
    else:
        # spread over the range, not stuck in one corner of it
        assert idx.min() < n // 100 and idx.max() > n - n // 100
        assert len(np.unique(idx)) > DRAWS * 0.99


def test_reaches_slots_a_float32_product_cannot():
    """float32 values from 2^26 up are multiples of 8, so a float32 u * n
    lands only on every eighth slot of the top third of a 1e8-row replay."""
    n = 10 ** 8
    idx = uniform_batch(21, 1, DRAWS, n)
    top = idx[idx >= 2 ** 26]
    assert len(top) > DRAWS // 4
    f32 = np.float32(top).astype(np.int64)
    assert (f32 % 8 == 0).all()             # what float32 can hold up there
    assert (top % 8 != 0).any()
    assert len(np.unique(top % 8)) == 8     # every residue, in fact


def test_stream_is_the_per_draws():
    """Same key and counters as the PER probe (seed, ctr_hi = epoch, ctr_lo =
    probe); epochs and probes give different draws."""
    n = 700
    a = uniform_batch(21, 1, 64, n)
    assert not np.array_equal(a, uniform_batch(21, 2, 64, n))
    assert not np.array_equal(a, uniform_batch(22, 1, 64, n))
    w = philox4x32_10(21, 1, 5)
    assert a[5] == (((w[0] << 32) | w[1]) * n) >> 64
    # close to uniform: 64 x 100 draws over 7 bins of 100 slots
    idx = np.concatenate([uniform_batch(21, e, 64, n) for e in range(1, 101)])
    hist = np.bincount(idx // 100, minlength=7)
    assert hist.min() > 0.85 * len(idx) / 7 and hist.max() < 1.15 * len(idx) / 7
