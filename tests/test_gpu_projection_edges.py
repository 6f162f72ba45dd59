"""GPU C51 projection at the support edges, on all three engine paths,
against the float64 oracle (tests/_oracles.project64).

The replay holds 512 transitions whose (reward, done) category is
`index % 8` (see _oracles.edge_rows): rows that clamp at either end, rows
with Tz exactly on an atom, and K in {28, 55} where float32
(v_max - v_min) / delta rounds above K-1, so that before the top-bin cap
every clamped atom added its mass one float past the LDS row.
"""

import numpy as np
import pytest
import torch

import _engine_kit as kit
import _oracles as orc

pytestmark = pytest.mark.gpu

O, A, H = 5, 2, 128
N = 512
V_MIN, V_MAX = -300.0, 0.0
GAMMA_N = 0.99 ** 5
SEED = 3

# (K, B, atol on m): persistent megakernel / row-block / per-layer MFMA path
CASES = [(K, B, atol) for K in (28, 55, 64)
         for B, atol in ((64, 5e-5), (300, 1e-4), (640, 1e-4))]


def _expected_draw(B, seed=SEED):
    """Uniform priorities (all leaves 1.0) => the draw is known on the CPU."""
    st, _ = orc.build_trees(np.ones(N), N)
    return np.array([orc.descend(st, N, orc.probe_mass(seed, 1, i, st[1]), N)
                     for i in range(B)])


@pytest.mark.parametrize("K,B,atol", CASES)
def test_projection_edges_gpu(K, B, atol):
    shape = kit.Shape(B, H, O, A, K)
    eng = kit.engine(shape, kit.modules(shape, seed=K), capacity=N, seed=SEED)
    assert bool(eng.info().get("persistent", False)) == (B <= 256)
    rng = np.random.default_rng(K)
    r, d = orc.edge_rows(N, K, V_MIN, V_MAX, seed=K)
    eng.ingest(torch.from_numpy(rng.standard_normal((N, O)).astype("f")),
               torch.from_numpy(rng.uniform(-1, 1, (N, A)).astype("f")),
               torch.from_numpy(r),
               torch.from_numpy(rng.standard_normal((N, O)).astype("f")),
               torch.from_numpy(d))
    eng.step(1)

    idx = eng.read("bidx").numpy()
    assert np.array_equal(idx, _expected_draw(B))
    assert set(idx % orc.N_CATEGORIES) == set(range(orc.N_CATEGORIES))
    br, bd = eng.read("br").numpy(), eng.read("bd").numpy()
    assert np.array_equal(br, r[idx]) and np.array_equal(bd, d[idx])

    p_t = eng.read("p_t").numpy()
    m = eng.read("m_proj").numpy()
    q = eng.read("q").numpy().astype(np.float64)
    want = orc.project64(p_t, br, bd, V_MIN, V_MAX, GAMMA_N)
    err = np.abs(m - want).max()
    rowsum = np.abs(m.sum(axis=1, dtype=np.float64) - 1.0).max()
    print(f"K={K} B={B}: max|m - m64|={err:.3g} max|rowsum-1|={rowsum:.3g}")
    np.testing.assert_allclose(m, want, atol=atol)
    # p_t rows are a float32 softmax: their own sum is 1 to a few ulp, and
    # the projection only redistributes it
    assert rowsum <= 1e-5
    np.testing.assert_allclose(eng.read("pri").numpy(),
                               (want * q).sum(axis=1) + 1e-6, atol=1e-5)
    np.testing.assert_allclose(eng.read("dlog").numpy(), (q - want) / B,
                               atol=5e-6)
    # clamped rows are deltas on the end bins
    top = np.isin(idx % orc.N_CATEGORIES, (0, 1, 5))
    bot = np.isin(idx % orc.N_CATEGORIES, (2, 4))
    np.testing.assert_allclose(m[top, K - 1], 1.0, atol=1e-5)
    np.testing.assert_allclose(m[bot, 0], 1.0, atol=1e-5)
