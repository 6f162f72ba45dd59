"""CPU unit tests of the shared numpy oracles (tests/_oracles.py) that the
GPU exact-sampling and projection tests lean on."""

import numpy as np
import pytest

import _oracles as orc

# Known-answer vectors of philox4x32-10 published with Random123
# (kat_vectors: counter[4], key[2] -> output[4]).
PHILOX_KAT = [
    ((0x00000000, 0x00000000, 0x00000000, 0x00000000),
     (0x00000000, 0x00000000),
     (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff),
     (0xffffffff, 0xffffffff),
     (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344),
     (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("ctr,key,out", PHILOX_KAT)
def test_philox_known_answers(ctr, key, out):
    assert orc.philox4x32_10_raw(ctr, key) == out


def test_philox_engine_word_order():
    """seed -> key, ctr_lo -> words 0,1, ctr_hi -> words 2,3."""
    ctr, key, out = PHILOX_KAT[2]
    seed = key[0] | (key[1] << 32)
    lo = ctr[0] | (ctr[1] << 32)
    hi = ctr[2] | (ctr[3] << 32)
    assert orc.philox4x32_10(seed, hi, lo) == out


def test_u01_float32_rounding():
    assert orc.u01(0).dtype == np.float32
    assert orc.u01(0) == np.float32(2.3283064e-10)
    # 2^32 - 1 rounds to 2^32 in float32; +1 is absorbed; * 2^-32 -> 1
    assert orc.u01(0xFFFFFFFF) == np.float32(1.0)
    # 2^24 + 1 is not representable: the cast rounds to even BEFORE the +1
    assert orc.u01((1 << 24) + 1) == np.float32(
        (np.float32(1 << 24) + np.float32(1.0)) * np.float32(2.3283064e-10))
    for x in (1, 12345, 0x7FFFFFFF, 0x80000001, 0xDEADBEEF):
        v = orc.u01(x)
        assert 0.0 < v <= 1.0
        assert abs(float(v) - (x + 1) / 2.0 ** 32) <= 2.0 ** -24


@pytest.mark.parametrize("tree_cap,size", [(8, 8), (16, 11), (512, 300),
                                           (1024, 700)])
def test_build_trees_and_descend(tree_cap, size):
    rng = np.random.default_rng(tree_cap + size)
    leaves = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), size))
    st, mt = orc.build_trees(leaves, tree_cap)
    n = np.arange(1, tree_cap)
    assert np.array_equal(st[n], st[2 * n] + st[2 * n + 1])
    assert np.array_equal(mt[n], np.minimum(mt[2 * n], mt[2 * n + 1]))
    assert st[1] == pytest.approx(leaves.sum(), rel=1e-12)
    assert mt[1] == leaves.min()
    assert (st[tree_cap + size:] == 0).all()
    assert np.isinf(mt[tree_cap + size:]).all()

    cum = np.cumsum(leaves)
    # strictly interior points, well away (>= 1e-9 relative) from every
    # cumulative boundary, where summation order cannot change the leaf
    mass = rng.uniform(0, st[1], 400)
    gap = np.abs(mass[:, None] - cum[None, :]).min(axis=1)
    mass = mass[gap > 1e-9 * st[1]]
    assert len(mass) > 300
    want = np.searchsorted(cum, mass)
    got = [orc.descend(st, tree_cap, m, size) for m in mass]
    assert np.array_equal(got, want)
    # the range-top guard
    assert orc.descend(st, tree_cap, st[1] * (1 + 1e-12), size) == size - 1


def test_descend_boundary_goes_left():
    st, _ = orc.build_trees([1.0, 2.0, 4.0, 8.0], 4)
    assert orc.descend(st, 4, 1.0, 4) == 0       # mass == left: stay left
    assert orc.descend(st, 4, np.nextafter(1.0, 2.0), 4) == 1
    assert orc.descend(st, 4, 3.0, 4) == 1
    assert orc.descend(st, 4, 7.0, 4) == 2
    assert orc.descend(st, 4, 15.0, 4) == 3


def test_ring_oracle_matches_cpu_per_buffer():
    """Across a wrapping sequence of batched adds the ring agrees with the
    CPU prioritized buffer fed the same rows one by one."""
    from d4pg_amd.replay.per import PrioritizedReplayBuffer
    cap, tree_cap, O, A = 37, 64, 5, 2
    alpha = 0.6
    ring = orc.RingOracle(cap, tree_cap)
    buf = PrioritizedReplayBuffer(cap, alpha)
    rng = np.random.default_rng(0)
    seen_wrap = False
    for call, T in enumerate([20, 17, 1, 30, 80]):
        s = rng.standard_normal((T, O)).astype("f")
        a = rng.uniform(-1, 1, (T, A)).astype("f")
        r = rng.uniform(-30, 0, T).astype("f")
        s2 = rng.standard_normal((T, O)).astype("f")
        d = (rng.random(T) < 0.3).astype("f")
        # a different new-row priority per call, as after training
        buf._max_priority = 1.0 + call
        ring.add(s, a, r, s2, d, leaf=(1.0 + call) ** alpha)
        for t in range(T):
            buf.add(s[t], a[t], r[t], s2[t], d[t])
        st = buf._store
        assert (ring.size, ring.pos) == (st.size, st.pos)
        seen_wrap |= ring.size == cap and ring.pos != 0
        got = ring.occupied()
        want = (st.states, st.actions, st.rewards, st.next_states, st.dones)
        for g, w in zip(got, want):
            assert np.array_equal(g, w[:st.size])
        sum_t, min_t = ring.trees()
        assert np.array_equal(sum_t, buf._it_sum.tree)
        assert np.array_equal(min_t, buf._it_min.tree)
    assert seen_wrap and ring.pos == (20 + 17 + 1 + 30 + 80) % cap
    # T = 80 > 2 * capacity: every slot holds the last row mapped to it
    assert np.array_equal(ring.rows["r"][(148 - 37 + np.arange(37)) % cap],
                          r[-37:])


def test_n01_moments_and_edges():
    """Over 10^4 consecutive counters: mean within 0.05 of 0 (5 sigma of the
    estimator, sigma = 0.01) and std within 0.05 of 1 (7 sigma, 0.007)."""
    x = np.array([orc.n01(*orc.roll_noise_words(5, 1, 0, i)[:2])
                  for i in range(10000)])
    assert abs(x.mean()) < 0.05
    assert abs(x.std() - 1.0) < 0.05
    # u1 = 2^-32 (word 0) stays finite; u2 = 1 (word 2^32-1) is cos(2 pi)
    top = np.sqrt(-2.0 * np.log(float(orc.u01(0))))
    assert orc.n01(0, 0xFFFFFFFF) == pytest.approx(top, rel=1e-12)
    assert 6.6 < top < 6.7


def test_roll_streams_are_distinct_and_in_range():
    seed = 9
    th, td = zip(*[orc.roll_reset_state(seed, 1, i) for i in range(256)])
    th, td = np.array(th), np.array(td)
    assert th.dtype == np.float32 and td.dtype == np.float32
    assert np.abs(th).max() <= np.pi and np.abs(td).max() <= 1.0
    assert len(np.unique(th)) == 256 and len(np.unique(td)) == 256
    # the counter packs (episode, tick + 2); tick 0 never collides with the
    # reset counter (| 1), and episodes do not alias ticks
    w = orc.roll_noise_words
    assert w(seed, 1, 0, 3) != w(seed, 2, 0, 3)
    assert w(seed, 1, 0, 3) != w(seed, 1, 1, 3)
    assert w(seed, 1, 0, 3) != w(seed, 1, 0, 4)
    assert w(seed, 1, 0, 3) == orc.philox4x32_10(seed ^ 0x2F01E,
                                                 (1 << 20) | 2, 3)
    th2, _ = orc.roll_reset_state(seed, 2, 0)
    assert th2 != th[0]


def test_is_weights_formula():
    leaves = np.array([0.5, 2.0, 1.0, 4.0, 0.25])
    st, mt = orc.build_trees(leaves, 8)
    # schedule: start, middle, saturated
    assert orc.per_beta(0.4, 10, 0) == np.float32(0.4)
    assert float(orc.per_beta(0.4, 10, 5)) == pytest.approx(0.7, rel=1e-6)
    assert orc.per_beta(0.4, 10, 50) == np.float32(1.0)
    for t in (0, 5, 50):
        beta = float(orc.per_beta(0.4, 10, t))
        w = orc.is_weights(st, mt, np.arange(5), 5, 0.4, 10, t)
        np.testing.assert_allclose(w, (leaves / leaves.min()) ** -beta,
                                   rtol=1e-12)
        assert w.max() == pytest.approx(1.0, abs=1e-12)
