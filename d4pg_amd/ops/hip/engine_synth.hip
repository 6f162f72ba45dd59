// Device rollout of the synthetic-spec envs, for any (obs, act): M vectorized
// SyntheticEnv instances (s' = tanh(s.W + a.U + sigma.N(0,1)), r = -mean(s'^2)
// + 0.1.mean(a^2), fixed horizon), exploration noise and the n-step fold,
// writing rows straight into the on-HBM replay.  Used by
// Engine::synth_rollout_*.  Host twin and parity oracle: VectorSynthetic +
// VecNStep (d4pg_amd/envs/vector.py).
//
// Episodes are synchronized (all M envs end at the horizon), as for Pendulum,
// so the emit pattern is static and k_roll_tick's ring fold carries over with
// general strides.  Per tick: the policy chain obs -> act, k_syn_act (noise,
// clip, ring write), the mixing GEMM z = [obs ‖ act_env] . [W; U] through the
// engine's own forward kernels, then k_syn_tick (process noise, tanh, reward,
// fold and emit).  The episode prologue and epilogue, the exploration noise,
// the leaf write and the table of philox keys are engine_rollcore.hip's.

namespace d4pg {

struct SynRollArgs : RollCore {
    int O, A;
    float act_high, proc_sigma;
    // env state: the core's obs [M][O] IS the env state; act_env [M][A] =
    // clipped noisy action * act_high, z [M][O] mixing GEMM output
    float *act_env, *z;
    // n-step rings: s_ring [n][M][O], a_ring [n][M][A], r_ring [n][M]
    float *s_ring, *a_ring, *r_ring;
};

// Reset draw of dim k of env i at episode ep: 0.1 * N(0,1)
// (SyntheticEnv._reset), shared with the evaluation reset (engine_eval.hip).
__device__ inline float syn_reset_draw(uint64_t seed, long long ep, int i,
                                       int k) {
    Philox4 r = philox4(seed ^ 0xD011Eull, ((uint64_t)ep << 20) | 1u,
                        ((uint64_t)k << 32) | (uint64_t)i);
    return 0.1f * n01(r.v[0], r.v[1]);
}

// SyntheticEnv._step of env i by one wave, after the mixing GEMM left z:
// s' = tanh(z + sigma * N(0,1)) into the env's obs row (and into s2_row, the
// replay's next-state row, when non-null), then r = -mean(s'^2) +
// 0.1 * mean(act_env^2) by two wave sums, returned on every lane.  Lanes
// stride over the dims, so every O-wide row access is coalesced.  The one
// copy of the dynamics: the training tick below and the evaluation tick call
// it, each with its own seed.
__device__ inline float syn_env_step(const float* z, float* obs, float* s2_row,
                                     const float* act_env, int O, int A,
                                     float proc_sigma, uint64_t seed,
                                     long long ep, int tick, int i, int lane) {
    float ss = 0.0f;
    for (int k = lane; k < O; k += 64) {
        float zz = z[k];
        if (proc_sigma != 0.0f) {
            Philox4 r = philox4(seed ^ 0x51A7Eull,
                                ((uint64_t)ep << 20) | (uint64_t)(tick + 2),
                                ((uint64_t)k << 32) | (uint64_t)i);
            zz += proc_sigma * n01(r.v[0], r.v[1]);
        }
        const float s2 = tanhf(zz);
        obs[k] = s2;
        if (s2_row) s2_row[k] = s2;
        ss += s2 * s2;
    }
    float sa = 0.0f;
    for (int k = lane; k < A; k += 64) {
        const float u = act_env[k];
        sa += u * u;
    }
    for (int s = 32; s > 0; s >>= 1) {
        ss += __shfl_xor(ss, s, 64);
        sa += __shfl_xor(sa, s, 64);
    }
    return -ss / (float)O + 0.1f * sa / (float)A;
}

// reset all M envs: state 0.1 * N(0,1) per dim (SyntheticEnv._reset), OU
// state to mu
__global__ void k_syn_reset(SynRollArgs a) {
    const long long ep = a.ep_state[0];
    const int O = a.O;
    const long stride = (long)gridDim.x * blockDim.x;
    const long t0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
    for (long e = t0; e < (long)a.M * O; e += stride) {
        const int i = (int)(e / O), k = (int)(e % O);
        a.obs[e] = syn_reset_draw(a.seed, ep, i, k);
    }
    for (long e = t0; e < (long)a.M * a.A; e += stride) a.ou_x[e] = a.ou_mu;
}

// after the policy forward: exploration noise -> clip -> the NORMALIZED
// action into the ring, the scaled one to the env; s_t into the ring before
// the env steps
__global__ void k_syn_act(SynRollArgs a, int tick, int slot) {
    const long long ep = a.ep_state[0];
    const int M = a.M, O = a.O, A = a.A;
    const long stride = (long)gridDim.x * blockDim.x;
    const long t0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
    for (long e = t0; e < (long)M * A; e += stride) {
        const int i = (int)(e / A), k = (int)(e % A);
        const float u = roll_explore(
            a, ep, tick, ((uint64_t)k << 32) | (uint64_t)i, a.act[e],
            a.ou_x + e);
        a.a_ring[(long)slot * M * A + e] = u;
        a.act_env[e] = u * a.act_high;
    }
    for (long e = t0; e < (long)M * O; e += stride)
        a.s_ring[(long)slot * M * O + e] = a.obs[e];
}

// one synchronized tick after the mixing GEMM: one wave per env, lanes
// striding over the dims (k = lane, lane + 64, ...) so every O-wide row
// access is coalesced.  Process noise -> tanh -> reward (two wave sums) ->
// ring write -> (optional) matured-transition emit into the replay.
// slot/emit_k/done are per-tick constants baked into the episode graph.
__global__ __launch_bounds__(256)
void k_syn_tick(SynRollArgs a, int tick, int slot, int emit_k, int done) {
    const int lane = threadIdx.x & 63;
    const int wpb = blockDim.x >> 6;
    const long long ep = a.ep_state[0], base = a.ep_state[1];
    const double pa = emit_k >= 0 ? roll_leaf_value(a) : 0.0;
    const int M = a.M, O = a.O, A = a.A, n = a.n;
    const int start = (slot + 1) % n;           // oldest ring entry
    for (int i = blockIdx.x * wpb + (threadIdx.x >> 6); i < M;
         i += gridDim.x * wpb) {
        const long dst = emit_k >= 0
            ? (long)((base + (long long)emit_k * M + i) % a.capacity) : 0;

        const float r = syn_env_step(
            a.z + (long)i * O, a.obs + (long)i * O,
            emit_k >= 0 ? a.rs2 + dst * O : nullptr, a.act_env + (long)i * A,
            O, A, a.proc_sigma, a.seed, ep, tick, i, lane);
        if (lane == 0) a.r_ring[(long)slot * M + i] = r;

        // --- matured n-step emit (VecNStep parity): transition
        // (s_{t-n+1}, a_{t-n+1}, sum gamma^k r, s_{t+1}, done); the ring's
        // newest entry is this tick's r, still in a register ---
        if (emit_k >= 0) {
            const float* s0 = a.s_ring + ((long)start * M + i) * O;
            const float* a0 = a.a_ring + ((long)start * M + i) * A;
            for (int k = lane; k < O; k += 64) a.rs[dst * O + k] = s0[k];
            for (int k = lane; k < A; k += 64) a.ra[dst * A + k] = a0[k];
            if (lane == 0) {
                float R = 0.0f, gk = 1.0f;
                for (int k = 0; k < n - 1; ++k) {
                    R += gk * a.r_ring[(long)((start + k) % n) * M + i];
                    gk *= a.gamma;
                }
                R += gk * r;
                a.rr[dst] = R;
                a.rd[dst] = (float)done;
                roll_write_leaf(a, dst, pa);
            }
        }
    }
}

}  // namespace d4pg
