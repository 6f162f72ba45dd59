// Device rollout kernels: M vectorized Pendulum envs, exploration noise and the
// n-step fold, writing transitions straight into the on-HBM replay.  Used by
// Engine::rollout_* (GPU actor ranks); the policy forward between ticks is
// k_fwd below 512 envs and k_mfma_fwd from 512 up.  The episode prologue and
// epilogue, the noise and the leaf write are engine_rollcore.hip's.

namespace d4pg {

// ===========================================================================
// GPU-resident actor rollout: M vectorized Pendulum envs + exploration
// noise (K11) + n-step fold (K15) entirely on device, transitions written
// straight into the on-HBM replay ring.  Re-expresses the reference's
// per-env-step actor loop (main.py:142-152 + random_process.py:4-45) and
// the host twins VectorPendulum / VecNStep (d4pg_amd/envs/vector.py), which
// serve as the parity oracles.
//
// Per tick: [fwd chain obs->act over M rows] then ONE k_roll_tick kernel
// (noise + dynamics + ring write + n-step emit).  Tree leaves are written
// at emit; internal nodes are rebuilt ONCE per episode by the full
// per-level sweep (k_tree_build_level — ~2M f64 nodes, bandwidth-cheap),
// which beats per-tick path repair by orders of magnitude.  The whole
// episode is one hipGraph; per-episode variability (philox epoch, replay
// base position) lives in device memory so graph replays stay fresh.
// ===========================================================================

__device__ inline float d4pg_angle_norm(float x) {
    const float PI = 3.14159265358979323846f;
    float y = fmodf(x + PI, 2.0f * PI);
    if (y < 0.0f) y += 2.0f * PI;
    return y - PI;
}

// Reset draw of env i at episode ep (Pendulum-v1 reset distribution: th
// uniform in [-pi, pi], thdot in [-1, 1]); the training reset and the
// evaluation reset (engine_eval.hip) both call it with their own seed.
__device__ inline void pendulum_reset_draw(uint64_t seed, long long ep, int i,
                                           float& th, float& td) {
    Philox4 r = philox4(seed ^ 0xD011Eull, ((uint64_t)ep << 20) | 1u,
                        (uint64_t)i);
    th = (2.0f * u01(r.v[0]) - 1.0f) * 3.14159265358979f;
    td = 2.0f * u01(r.v[1]) - 1.0f;
}

// One env step (VectorPendulum.step parity) under the clipped normalized
// action u_n: advances (th, td) in place and returns the reward -cost.  The
// one copy of the dynamics; the training tick below and the evaluation tick
// call it.
__device__ inline float pendulum_step(float u_n, float& th, float& td) {
    const float max_torque = 2.0f, max_speed = 8.0f, dt = 0.05f, g = 10.0f;
    float u = u_n * max_torque;
    float an = d4pg_angle_norm(th);
    float cost = an * an + 0.1f * td * td + 0.001f * u * u;
    float newtd = td + (1.5f * g * sinf(th) + 3.0f * u) * dt;
    newtd = fminf(fmaxf(newtd, -max_speed), max_speed);
    th = th + newtd * dt;
    td = newtd;
    return -cost;
}

struct RollArgs : RollCore {
    int O, A;
    float *th, *thdot;                 // env state [M]
    // n-step rings [n][M][*]
    float *s_ring, *a_ring, *r_ring;
};

// reset all M envs (uniform th in [-pi,pi], thdot in [-1,1] — Pendulum-v1
// reset distribution) + OU state to mu, and emit the first observation
__global__ void k_roll_reset(RollArgs a) {
    long long ep = a.ep_state[0];
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < a.M;
         i += gridDim.x * blockDim.x) {
        float th, td;
        pendulum_reset_draw(a.seed, ep, i, th, td);
        a.th[i] = th;
        a.thdot[i] = td;
        a.obs[i * 3 + 0] = cosf(th);
        a.obs[i * 3 + 1] = sinf(th);
        a.obs[i * 3 + 2] = td;
        for (int k = 0; k < a.A; ++k) a.ou_x[i * a.A + k] = a.ou_mu;
    }
}

// one synchronized tick for all M envs: noise -> clip -> dynamics ->
// n-step ring write -> (optional) matured-transition emit into the replay.
// slot/emit_k/done are per-tick constants baked into the episode graph.
__global__ void k_roll_tick(RollArgs a, int tick, int slot, int emit_k,
                            int done) {
    long long ep = a.ep_state[0];
    long long base = a.ep_state[1];
    double pa = roll_leaf_value(a);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < a.M;
         i += gridDim.x * blockDim.x) {
        float u_n = roll_explore(a, ep, tick, (uint64_t)i, a.act[i * a.A],
                                 a.ou_x + i * a.A);

        // --- n-step ring: store s_t, a_t BEFORE stepping ---
        a.s_ring[(slot * a.M + i) * 3 + 0] = a.obs[i * 3 + 0];
        a.s_ring[(slot * a.M + i) * 3 + 1] = a.obs[i * 3 + 1];
        a.s_ring[(slot * a.M + i) * 3 + 2] = a.obs[i * 3 + 2];
        a.a_ring[slot * a.M + i] = u_n;

        // --- Pendulum dynamics (VectorPendulum.step parity) ---
        float th = a.th[i], td = a.thdot[i];
        const float r = pendulum_step(u_n, th, td);
        a.th[i] = th;
        a.thdot[i] = td;
        a.r_ring[slot * a.M + i] = r;
        float o0 = cosf(th), o1 = sinf(th), o2 = td;
        a.obs[i * 3 + 0] = o0;
        a.obs[i * 3 + 1] = o1;
        a.obs[i * 3 + 2] = o2;

        // --- matured n-step emit (VecNStep parity): transition
        // (s_{t-n+1}, a_{t-n+1}, sum gamma^k r, s_{t+1}, done) ---
        if (emit_k >= 0) {
            int start = (slot + 1) % a.n;       // oldest ring entry
            float R = 0.0f, gk = 1.0f;
            for (int k = 0; k < a.n; ++k) {
                R += gk * a.r_ring[((start + k) % a.n) * a.M + i];
                gk *= a.gamma;
            }
            long dst = (base + (long)emit_k * a.M + i) % a.capacity;
            a.rs[dst * 3 + 0] = a.s_ring[(start * a.M + i) * 3 + 0];
            a.rs[dst * 3 + 1] = a.s_ring[(start * a.M + i) * 3 + 1];
            a.rs[dst * 3 + 2] = a.s_ring[(start * a.M + i) * 3 + 2];
            a.ra[dst] = a.a_ring[start * a.M + i];
            a.rr[dst] = R;
            a.rs2[dst * 3 + 0] = o0;
            a.rs2[dst * 3 + 1] = o1;
            a.rs2[dst * 3 + 2] = o2;
            a.rd[dst] = (float)done;
            roll_write_leaf(a, dst, pa);
        }
    }
}

}  // namespace d4pg
