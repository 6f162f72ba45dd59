// Device goal-reaching rollout with hindsight relabelling: M vectorized
// GoalReach envs (a point in [-1,1]^D moved by a velocity action, sparse
// reward), exploration noise, the n-step fold and the "future"-strategy HER
// relabel, writing rows straight into the on-HBM replay.  Used by
// Engine::goal_rollout_*; the policy forward between ticks is the same
// chain the Pendulum rollout uses.  Host twins and parity oracles:
// VectorGoalReach (d4pg_amd/envs/vector.py) and vector_add_experience
// (d4pg_amd/her.py), which calls the scalar add_experience once per env.
//
// Unlike the Pendulum rollout, episodes end per env (on success), so the
// number of rows an episode produces is data-dependent, and the relabel needs
// the whole episode.  Ticks therefore only record (ep_pos, ep_act); after the
// last tick the episode is counted per env (k_goal_count), the counts are
// scanned over envs (k_goal_scan) and every env writes its rows densely at
// its own offset (k_goal_emit) — no atomics, so placement is deterministic
// and a graph replay equals the uncaptured launches bitwise.  Everything
// data-dependent (lengths, counts, offsets, totals) lives in device memory,
// so the whole episode is still one hipGraph.

namespace d4pg {

// ep_state words past the core's [0..2]: [3] successes, [4] env steps (sum
// of lengths); [5..7] rows, successes and env steps summed over the episodes
// of one run call
struct GoalRollArgs : RollCore {
    int D;
    float speed, tol, her_ratio;
    // env state: pos/goal [M][D]; the core's obs is [M][2D] = pos ‖ goal
    float *pos, *goal;
    int *alive, *len, *succ;           // [M]
    // episode buffers: ep_pos [horizon+1][M][D], ep_act [horizon][M][D]
    float *ep_pos, *ep_act;
    // rows per env and their exclusive scan [M]
    int* count;
    long long* offset;
};

// sparse reward of GoalReachEnv.compute_reward: 0 within tol, else -1
__device__ inline float goal_reward(const float* p, const float* g, int D,
                                    float tol) {
    float d2 = 0.0f;
    for (int k = 0; k < D; ++k) {
        float d = p[k] - g[k];
        d2 += d * d;
    }
    return sqrtf(d2) <= tol ? 0.0f : -1.0f;
}

// The env step, in one copy for the training tick below and the evaluation
// tick (engine_eval.hip): GoalReachEnv._step's move and clip of one dim under
// the clipped action u, and the success test on the stored position, which
// is the test the emit's rewards use.
__device__ inline float goal_move(float p, float speed, float u) {
    p = p + speed * u;
    return fminf(fmaxf(p, -1.0f), 1.0f);
}

__device__ inline bool goal_reached(const float* p, const float* g, int D,
                                    float tol) {
    return goal_reward(p, g, D, tol) == 0.0f;
}

// Reset draw of dim k of env i at episode ep: pos and goal uniform in
// [-1, 1], shared with the evaluation reset.
__device__ inline void goal_reset_draw(uint64_t seed, long long ep, int i,
                                       int k, float& p, float& g) {
    Philox4 r = philox4(seed ^ 0xD011Eull, ((uint64_t)ep << 20) | 1u,
                        ((uint64_t)k << 32) | (uint64_t)i);
    p = 2.0f * u01(r.v[0]) - 1.0f;
    g = 2.0f * u01(r.v[1]) - 1.0f;
}

// HER draw of step t of env i (T = the env's episode length, t < T): whether
// the step gets a hindsight row and, if so, the future index in [t, T) whose
// achieved position becomes the goal.  u01 is in (0,1], so a ratio of 1
// always hits and a ratio of 0 never does.
__device__ inline bool goal_her_draw(const GoalRollArgs& a, long long ep,
                                     int t, int i, int T, int& fut) {
    if (!(a.her_ratio > 0.0f)) return false;
    Philox4 w = philox4(a.seed ^ 0x4E12Eull,
                        ((uint64_t)ep << 20) | (uint64_t)t, (uint64_t)i);
    fut = t + (int)(w.v[1] % (uint32_t)(T - t));
    return u01(w.v[0]) <= a.her_ratio;
}

// reset all M envs: pos and goal uniform in [-1,1]^D, OU state to mu, and
// the first observation.  No success check here, as on the host.
__global__ void k_goal_reset(GoalRollArgs a) {
    long long ep = a.ep_state[0];
    const int D = a.D;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < a.M;
         i += gridDim.x * blockDim.x) {
        for (int k = 0; k < D; ++k) {
            float p, g;
            goal_reset_draw(a.seed, ep, i, k, p, g);
            a.pos[i * D + k] = p;
            a.goal[i * D + k] = g;
            a.obs[i * 2 * D + k] = p;
            a.obs[i * 2 * D + D + k] = g;
            a.ep_pos[(long)i * D + k] = p;
            a.ou_x[i * D + k] = a.ou_mu;
        }
        a.alive[i] = 1;
        a.len[i] = 0;
        a.succ[i] = 0;
    }
}

// one synchronized tick: envs that already succeeded do nothing; the others
// take noise -> clip -> move -> record, and stop on success
__global__ void k_goal_tick(GoalRollArgs a, int tick) {
    long long ep = a.ep_state[0];
    const int D = a.D, M = a.M;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < M;
         i += gridDim.x * blockDim.x) {
        if (!a.alive[i]) continue;
        for (int k = 0; k < D; ++k) {
            const float u = roll_explore(
                a, ep, tick, ((uint64_t)k << 32) | (uint64_t)i,
                a.act[i * D + k], a.ou_x + i * D + k);
            a.ep_act[((long)tick * M + i) * D + k] = u;

            // --- GoalReachEnv._step ---
            const float p = goal_move(a.pos[i * D + k], a.speed, u);
            a.pos[i * D + k] = p;
            a.obs[i * 2 * D + k] = p;
            a.ep_pos[((long)(tick + 1) * M + i) * D + k] = p;
        }
        a.len[i] = tick + 1;
        // the same test the emit's rewards use, on the stored position
        if (goal_reached(a.pos + i * D, a.goal + i * D, D, a.tol)) {
            a.succ[i] = 1;
            a.alive[i] = 0;
        }
    }
}

// rows env i will write: the folded real rows plus one per HER hit
__global__ void k_goal_count(GoalRollArgs a) {
    long long ep = a.ep_state[0];
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < a.M;
         i += gridDim.x * blockDim.x) {
        int T = a.len[i];
        int c = T - a.n + 1 > 0 ? T - a.n + 1 : 0;
        for (int t = 0; t < T; ++t) {
            int fut;
            c += goal_her_draw(a, ep, t, i, T, fut) ? 1 : 0;
        }
        a.count[i] = c;
    }
}

// exclusive scan of count[] over the M envs into offset[], one workgroup.
// Thread t sums a contiguous run of envs, the 1024 run sums are scanned by
// wave 0 (16 per lane, then a shuffle scan over the 64 lanes), and every
// thread walks its run again.  The episode's totals (rows, successes, env
// steps) go to the per-episode words; the integer adds are order-free.
#define GOAL_SCAN_THREADS 1024
__global__ __launch_bounds__(GOAL_SCAN_THREADS)
void k_goal_scan(GoalRollArgs a) {
    __shared__ long long run_sum[GOAL_SCAN_THREADS];
    __shared__ int acc[2];
    const int tid = threadIdx.x, M = a.M;
    const int per = (M + GOAL_SCAN_THREADS - 1) / GOAL_SCAN_THREADS;
    const int lo = tid * per < M ? tid * per : M;
    const int hi = lo + per < M ? lo + per : M;
    if (tid < 2) acc[tid] = 0;
    __syncthreads();
    long long s = 0;
    int steps = 0, succ = 0;
    for (int i = lo; i < hi; ++i) {
        s += a.count[i];
        steps += a.len[i];
        succ += a.succ[i];
    }
    run_sum[tid] = s;
    if (steps) atomicAdd(&acc[0], steps);
    if (succ) atomicAdd(&acc[1], succ);
    __syncthreads();
    if (tid < 64) {
        const int q0 = tid * (GOAL_SCAN_THREADS / 64);
        long long v = 0;
        for (int q = 0; q < GOAL_SCAN_THREADS / 64; ++q) {
            long long x = run_sum[q0 + q];
            run_sum[q0 + q] = v;
            v += x;
        }
        const long long own = v;
        for (int d = 1; d < 64; d <<= 1) {
            long long y = __shfl_up(v, d, 64);
            if (tid >= d) v += y;
        }
        const long long before = v - own;
        for (int q = 0; q < GOAL_SCAN_THREADS / 64; ++q)
            run_sum[q0 + q] += before;
        if (tid == 63) {
            a.ep_state[2] = v;
            a.ep_state[3] = acc[1];
            a.ep_state[4] = acc[0];
        }
    }
    __syncthreads();
    long long run = run_sum[tid];
    for (int i = lo; i < hi; ++i) {
        a.offset[i] = run;
        run += a.count[i];
    }
}

// one wave per env, lanes over the env's steps: real (n-step folded) rows by
// ascending t, then the HER rows by ascending t, at (base + offset[i] + j) %
// capacity — the order add_experience writes them.  HER-row positions come
// from a ballot of the hit lanes; horizons past 64 loop in chunks of 64.
__global__ __launch_bounds__(256)
void k_goal_emit(GoalRollArgs a) {
    const int lane = threadIdx.x & 63;
    const int wpb = blockDim.x >> 6;
    const long long ep = a.ep_state[0], base = a.ep_state[1];
    const double pa = roll_leaf_value(a);
    const int D = a.D, M = a.M, O = 2 * a.D;
    for (int i = blockIdx.x * wpb + (threadIdx.x >> 6); i < M;
         i += gridDim.x * wpb) {
        const int T = a.len[i];
        const int succ = a.succ[i];
        const long long row0 = base + a.offset[i];
        const int n_real = T - a.n + 1 > 0 ? T - a.n + 1 : 0;
        const float* g = a.goal + (long)i * D;

        // --- real rows: (pos_{t-n+1}‖g, a_{t-n+1}, sum gamma^k r,
        // pos_{t+1}‖g, done); done only where the env's last step succeeded
        // (the step limit is not a terminal here, as in her.py) ---
        for (int j = lane; j < n_real; j += 64) {
            const int t = j + a.n - 1;
            float R = 0.0f, gk = 1.0f;
            for (int k = 0; k < a.n; ++k) {
                R += gk * goal_reward(
                    a.ep_pos + ((long)(j + k + 1) * M + i) * D, g, D, a.tol);
                gk *= a.gamma;
            }
            const long dst = (long)((row0 + j) % a.capacity);
            const float* p0 = a.ep_pos + ((long)j * M + i) * D;
            const float* p1 = a.ep_pos + ((long)(t + 1) * M + i) * D;
            const float* ac = a.ep_act + ((long)j * M + i) * D;
            for (int k = 0; k < D; ++k) {
                a.rs[dst * O + k] = p0[k];
                a.rs[dst * O + D + k] = g[k];
                a.ra[dst * D + k] = ac[k];
                a.rs2[dst * O + k] = p1[k];
                a.rs2[dst * O + D + k] = g[k];
            }
            a.rr[dst] = R;
            a.rd[dst] = (t == T - 1 && succ) ? 1.0f : 0.0f;
            roll_write_leaf(a, dst, pa);
        }

        // --- HER rows (one-step): (pos_t‖g', a_t, r', pos_{t+1}‖g',
        // r' == 0) with g' = pos_{fut+1} ---
        int hits_before = 0;
        for (int c = 0; c < T; c += 64) {
            const int t = c + lane;
            int fut = 0;
            const bool hit = t < T && goal_her_draw(a, ep, t, i, T, fut);
            const unsigned long long m = __ballot(hit);
            if (hit) {
                const int j = n_real + hits_before
                              + __popcll(m & ((1ull << lane) - 1ull));
                const long dst = (long)((row0 + j) % a.capacity);
                const float* p0 = a.ep_pos + ((long)t * M + i) * D;
                const float* p1 = a.ep_pos + ((long)(t + 1) * M + i) * D;
                const float* ng = a.ep_pos + ((long)(fut + 1) * M + i) * D;
                const float* ac = a.ep_act + ((long)t * M + i) * D;
                const float r = goal_reward(p1, ng, D, a.tol);
                for (int k = 0; k < D; ++k) {
                    a.rs[dst * O + k] = p0[k];
                    a.rs[dst * O + D + k] = ng[k];
                    a.ra[dst * D + k] = ac[k];
                    a.rs2[dst * O + k] = p1[k];
                    a.rs2[dst * O + D + k] = ng[k];
                }
                a.rr[dst] = r;
                a.rd[dst] = r == 0.0f ? 1.0f : 0.0f;
                roll_write_leaf(a, dst, pa);
            }
            hits_before += __popcll(m);
        }
    }
}

// episode epilogue: advance the replay counters by the device-side total
__global__ void k_goal_end(GoalRollArgs a) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        const long long total = a.ep_state[2];
        roll_advance(a, total);
        a.ep_state[5] += total;
        a.ep_state[6] += a.ep_state[3];
        a.ep_state[7] += a.ep_state[4];
    }
}

}  // namespace d4pg
