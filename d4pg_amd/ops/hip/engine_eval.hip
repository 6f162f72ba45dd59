// Device greedy evaluation: E vectorized envs of the kind the allocated
// rollout producer models, driven by the policy chain with no exploration
// noise (action = clip(tanh head, -1, 1)), accumulating the undiscounted
// episode return per env.  Used by Engine::eval_*.  Host twin and parity
// oracle: vector_evaluate (d4pg_amd/envs/vector.py).
//
// An evaluation episode has no side effects on anything training reads: it
// writes no replay row and no tree leaf, leaves the Counters alone and keeps
// all of its state (env state, obs, act, returns, lengths, result words and
// its own philox epoch) in a pool of its own.  The env steps themselves are
// the rollouts' own (pendulum_step, goal_move / goal_reached, syn_env_step),
// as are the reset draws, so the dynamics exist once.
//
// Random streams: the rollout's key table (engine_rollcore.hip) with the
// evaluation's own seed and epoch word.  Per tick: the policy chain obs ->
// act, then one tick kernel (for the synthetic envs k_eval_syn_act, the
// mixing GEMM and k_eval_syn_tick).  After the last tick k_eval_reduce folds
// the per-env results into eight result words, in a fixed order and with no
// atomics, so a graph replay equals the uncaptured launches bitwise.

namespace d4pg {

// Result words (8 bytes each), summed over the episodes of one eval_run
// call: [0] sum of returns (double), [1] min and [2] max return (double),
// [3] successes, [4] env steps, [5] env episodes counted, [6] philox epoch
// of the last episode, [7] episodes.  Word [8] is the epoch itself.
#define EVAL_WORDS 8
#define EVAL_EPOCH 8

struct EvalArgs {
    int E, horizon, fixed_starts;
    uint64_t seed;
    float *obs, *act;                  // [E][obs], [E][act]
    double* ret;                       // [E]
    int *len, *succ;                   // [E]
    long long* words;
    // Pendulum: env state [E]
    float *th, *thdot;
    // GoalReach: pos / goal [E][D], alive [E]
    int D;
    float speed, tol;
    float *pos, *goal;
    int* alive;
    // synthetic: act_env [E][A], z [E][O]
    int O, A;
    float act_high, proc_sigma;
    float *act_env, *z;
};

// episode prologue: the epoch advances once per episode unless the starts
// are fixed (common random numbers across calls)
__global__ void k_eval_begin(EvalArgs a) {
    if (threadIdx.x == 0 && blockIdx.x == 0 && !a.fixed_starts)
        a.words[EVAL_EPOCH] += 1;
}

__device__ inline void eval_clear(const EvalArgs& a, int i) {
    a.ret[i] = 0.0;
    a.len[i] = 0;
    a.succ[i] = 0;
}

__device__ inline float eval_clip(float u) {
    return fminf(fmaxf(u, -1.0f), 1.0f);
}

// ---------------------------------------------------------------- Pendulum
__global__ void k_eval_pend_reset(EvalArgs a) {
    const long long ep = a.words[EVAL_EPOCH];
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < a.E;
         i += gridDim.x * blockDim.x) {
        float th, td;
        pendulum_reset_draw(a.seed, ep, i, th, td);
        a.th[i] = th;
        a.thdot[i] = td;
        a.obs[i * 3 + 0] = cosf(th);
        a.obs[i * 3 + 1] = sinf(th);
        a.obs[i * 3 + 2] = td;
        eval_clear(a, i);
    }
}

__global__ void k_eval_pend_tick(EvalArgs a, int tick) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < a.E;
         i += gridDim.x * blockDim.x) {
        float th = a.th[i], td = a.thdot[i];
        const float r = pendulum_step(eval_clip(a.act[i]), th, td);
        a.th[i] = th;
        a.thdot[i] = td;
        a.obs[i * 3 + 0] = cosf(th);
        a.obs[i * 3 + 1] = sinf(th);
        a.obs[i * 3 + 2] = td;
        a.ret[i] += (double)r;
        a.len[i] = tick + 1;
    }
}

// --------------------------------------------------------------- GoalReach
__global__ void k_eval_goal_reset(EvalArgs a) {
    const long long ep = a.words[EVAL_EPOCH];
    const int D = a.D;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < a.E;
         i += gridDim.x * blockDim.x) {
        for (int k = 0; k < D; ++k) {
            float p, g;
            goal_reset_draw(a.seed, ep, i, k, p, g);
            a.pos[i * D + k] = p;
            a.goal[i * D + k] = g;
            a.obs[i * 2 * D + k] = p;
            a.obs[i * 2 * D + D + k] = g;
        }
        a.alive[i] = 1;
        eval_clear(a, i);
    }
}

// envs that already succeeded do nothing, as in k_goal_tick; the others
// move, take the sparse reward of the new position and stop on success
__global__ void k_eval_goal_tick(EvalArgs a, int tick) {
    const int D = a.D;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < a.E;
         i += gridDim.x * blockDim.x) {
        if (!a.alive[i]) continue;
        for (int k = 0; k < D; ++k) {
            const float p = goal_move(a.pos[i * D + k], a.speed,
                                      eval_clip(a.act[i * D + k]));
            a.pos[i * D + k] = p;
            a.obs[i * 2 * D + k] = p;
        }
        a.len[i] = tick + 1;
        a.ret[i] += (double)goal_reward(a.pos + i * D, a.goal + i * D, D,
                                        a.tol);
        if (goal_reached(a.pos + i * D, a.goal + i * D, D, a.tol)) {
            a.succ[i] = 1;
            a.alive[i] = 0;
        }
    }
}

// --------------------------------------------------------------- synthetic
__global__ void k_eval_syn_reset(EvalArgs a) {
    const long long ep = a.words[EVAL_EPOCH];
    const int O = a.O;
    const long stride = (long)gridDim.x * blockDim.x;
    const long t0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
    for (long e = t0; e < (long)a.E * O; e += stride)
        a.obs[e] = syn_reset_draw(a.seed, ep, (int)(e / O), (int)(e % O));
    for (long e = t0; e < (long)a.E; e += stride) eval_clear(a, (int)e);
}

// after the policy forward: clip, and the scaled action to the env
__global__ void k_eval_syn_act(EvalArgs a) {
    const long stride = (long)gridDim.x * blockDim.x;
    const long t0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
    for (long e = t0; e < (long)a.E * a.A; e += stride)
        a.act_env[e] = eval_clip(a.act[e]) * a.act_high;
}

// after the mixing GEMM: one wave per env, as in k_syn_tick; the process
// noise stays on (it is part of the env)
__global__ __launch_bounds__(256)
void k_eval_syn_tick(EvalArgs a, int tick) {
    const int lane = threadIdx.x & 63;
    const int wpb = blockDim.x >> 6;
    const long long ep = a.words[EVAL_EPOCH];
    const int O = a.O, A = a.A;
    for (int i = blockIdx.x * wpb + (threadIdx.x >> 6); i < a.E;
         i += gridDim.x * wpb) {
        const float r = syn_env_step(
            a.z + (long)i * O, a.obs + (long)i * O, nullptr,
            a.act_env + (long)i * A, O, A, a.proc_sigma, a.seed, ep, tick, i,
            lane);
        if (lane == 0) {
            a.ret[i] += (double)r;
            a.len[i] = tick + 1;
        }
    }
}

// ------------------------------------------------------------------ reduce
// One workgroup: thread t folds envs t, t + 256, ... in ascending order, a
// fixed-order LDS tree folds the 256 partials, and thread 0 adds the episode
// to the call's result words.
#define EVAL_REDUCE_THREADS 256
__global__ __launch_bounds__(EVAL_REDUCE_THREADS)
void k_eval_reduce(EvalArgs a) {
    __shared__ double s_sum[EVAL_REDUCE_THREADS], s_min[EVAL_REDUCE_THREADS],
                      s_max[EVAL_REDUCE_THREADS];
    __shared__ long long s_succ[EVAL_REDUCE_THREADS],
                         s_steps[EVAL_REDUCE_THREADS];
    const int tid = threadIdx.x;
    double sum = 0.0, mn = HUGE_VAL, mx = -HUGE_VAL;
    long long succ = 0, steps = 0;
    for (int i = tid; i < a.E; i += EVAL_REDUCE_THREADS) {
        const double r = a.ret[i];
        sum += r;
        mn = fmin(mn, r);
        mx = fmax(mx, r);
        succ += a.succ[i];
        steps += a.len[i];
    }
    s_sum[tid] = sum; s_min[tid] = mn; s_max[tid] = mx;
    s_succ[tid] = succ; s_steps[tid] = steps;
    __syncthreads();
    for (int s = EVAL_REDUCE_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) {
            s_sum[tid] += s_sum[tid + s];
            s_min[tid] = fmin(s_min[tid], s_min[tid + s]);
            s_max[tid] = fmax(s_max[tid], s_max[tid + s]);
            s_succ[tid] += s_succ[tid + s];
            s_steps[tid] += s_steps[tid + s];
        }
        __syncthreads();
    }
    if (tid == 0) {
        long long* w = a.words;
        const bool first = w[5] == 0;
        const double psum = __longlong_as_double(w[0]);
        const double pmin = __longlong_as_double(w[1]);
        const double pmax = __longlong_as_double(w[2]);
        w[0] = __double_as_longlong(first ? s_sum[0] : psum + s_sum[0]);
        w[1] = __double_as_longlong(first ? s_min[0] : fmin(pmin, s_min[0]));
        w[2] = __double_as_longlong(first ? s_max[0] : fmax(pmax, s_max[0]));
        w[3] += s_succ[0];
        w[4] += s_steps[0];
        w[5] += a.E;
        w[6] = w[EVAL_EPOCH];
        w[7] += 1;
    }
}

}  // namespace d4pg
