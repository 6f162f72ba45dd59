"""C51 projection at the edges of the support: rows that clamp at either
end, Tz exactly on an atom, and supports where float32
(v_max - v_min) / delta rounds ABOVE K-1 (K=28 and K=55 on [-300, 0] and
[-100, 50]) — there an uncapped ceil(b) indexes one bin past the row."""

import numpy as np
import pytest
import torch

import _oracles as orc
from d4pg_amd.algo.projection import categorical_projection

GAMMA_N = 0.99 ** 5
SUPPORTS = [(-300.0, 0.0), (-100.0, 50.0)]


def test_top_bin_overflow_supports_exist():
    """The premise: float32 b at Tz = v_max exceeds K-1 for these K."""
    f = np.float32
    for v_min, v_max in SUPPORTS:
        for K, over in [(28, True), (55, True), (51, False), (64, False),
                        (2, False)]:
            delta = f(f(v_max - v_min) / f(K - 1))
            b = f(f(f(v_max) - f(v_min)) / delta)
            assert (b > K - 1) == over, (v_min, v_max, K, b)


@pytest.mark.parametrize("v_min,v_max", SUPPORTS)
@pytest.mark.parametrize("K", [2, 28, 51, 55, 64])
def test_projection_edges_match_float64_oracle(K, v_min, v_max):
    B = 64
    rng = np.random.default_rng(K)
    p = rng.random((B, K)).astype(np.float32)
    p /= p.sum(axis=1, keepdims=True)
    r, d = orc.edge_rows(B, K, v_min, v_max, seed=K)
    m = categorical_projection(torch.from_numpy(p), torch.from_numpy(r),
                               torch.from_numpy(d), v_min, v_max,
                               GAMMA_N).numpy()
    want = orc.project64(p, r, d, v_min, v_max, GAMMA_N)
    np.testing.assert_allclose(m, want, atol=5e-6)
    assert np.abs(m.sum(axis=1) - 1.0).max() <= 1e-5
    assert np.abs(want.sum(axis=1) - 1.0).max() <= 1e-5
    # the clamped / on-atom rows are deltas on the expected bin
    js = [0, 1, K // 2, K - 1]
    for i in range(B):
        c = i % orc.N_CATEGORIES
        hit = {0: K - 1, 1: K - 1, 2: 0, 4: 0, 5: K - 1}.get(c)
        if c == 3:
            hit = js[(i // orc.N_CATEGORIES) % 4]
        if hit is not None:
            assert m[i, hit] == pytest.approx(1.0, abs=5e-6), (i, c)
