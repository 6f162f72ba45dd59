// What the three device rollouts (engine_rollout.hip, engine_goal.hip,
// engine_synth.hip) share: the args every producer carries, the episode
// prologue and epilogue, the exploration noise and the PER leaf of a new row.
// The environments differ in their tick, count, scan and emit kernels; what
// is here is the same for all of them by construction, as engine_rowmath.hip
// arranges for the learner paths.
//
// Philox keys of the rollout streams (seed ^ constant; ctr_hi = (episode <<
// 20) | sub-stream, ctr_lo = (dim << 32) | env):
//   0xD011E  reset state          sub-stream 1          (all rollouts)
//   0x2F01E  exploration noise    sub-stream tick + 2   (roll_explore)
//   0x4E12E  HER draw             sub-stream t          (goal rollout)
//   0x51A7E  process noise        sub-stream tick + 2   (synth rollout)
// The greedy evaluation (engine_eval.hip) draws from the same table with its
// own seed, seed_eval = rollout seed ^ 0x5EEDE7A1 unless eval_alloc sets
// another, and its own epoch word in place of `episode`: reset states from
// seed_eval ^ 0xD011E sub-stream 1, the synth process noise from seed_eval ^
// 0x51A7E; it has no exploration and no HER draw.  With fixed starts the
// epoch stays at 1; otherwise it advances once per evaluation episode.

namespace d4pg {

// standard normal via Box-Muller on two philox lanes
__device__ inline float n01(uint32_t a, uint32_t b) {
    float u1 = u01(a), u2 = u01(b);
    u1 = fmaxf(u1, 1e-12f);
    return sqrtf(-2.0f * logf(u1)) *
           cosf(6.283185307179586f * u2);
}

// The producers' args structs derive from this and add their env's own
// fields, so kernel bodies read a.M whichever struct they take.
struct RollCore {
    int M, n, horizon;
    float gamma, eps, ou_theta, ou_sigma, ou_mu, ou_dt;
    int noise_kind;                    // 0 = gaussian, 1 = OU
    uint64_t seed;
    float per_alpha;
    // observation [M][obs], policy output [M][act], OU state [M][act]
    float *obs, *act, *ou_x;
    // per-episode device words: [0] philox epoch, [1] replay base pos,
    // [2] rows emitted; [3..7] are the goal rollout's (engine_goal.hip)
    long long* ep_state;
    // replay
    float *rs, *ra, *rr, *rs2, *rd;
    double *sum_tree, *min_tree;       // null: uniform replay
    long tree_cap, capacity;
    Counters* cnt;
};

// episode prologue: bump the philox epoch, latch the replay write base
__global__ void k_roll_begin(RollCore a) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        a.ep_state[0] += 1;
        a.ep_state[1] = a.cnt->pos;
    }
}

// advance the replay counters by the episode's emitted block
__device__ inline void roll_advance(const RollCore& a, long long emitted) {
    long long base = a.ep_state[1];
    a.cnt->pos = (base + emitted) % a.capacity;
    long long sz = a.cnt->size + emitted;
    a.cnt->size = sz > a.capacity ? a.capacity : sz;
}

// episode epilogue of the rollouts whose row count is static
__global__ void k_roll_end(RollCore a, long emitted) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        a.ep_state[2] = emitted;
        roll_advance(a, emitted);
    }
}

// Exploration noise (K11) on policy output u (tanh, in (-1,1)) and the clip
// to [-1, 1]: one philox stream per (env, dim, tick), ctr_lo = (dim << 32) |
// env.  *ou is the OU state of that (env, dim).  eps == 0 skips the Gaussian
// draw; the OU state advances whatever eps is (it is state, and eps only
// scales what is added).
__device__ inline float roll_explore_n01(const RollCore& a, long long ep,
                                         int tick, uint64_t ctr_lo) {
    Philox4 r = philox4(a.seed ^ 0x2F01Eull,
                        ((uint64_t)ep << 20) | (uint64_t)(tick + 2), ctr_lo);
    return n01(r.v[0], r.v[1]);
}

__device__ inline float roll_explore(const RollCore& a, long long ep, int tick,
                                     uint64_t ctr_lo, float u, float* ou) {
    if (a.noise_kind == 0 && a.eps != 0.0f) {
        u += a.eps * roll_explore_n01(a, ep, tick, ctr_lo);
    } else if (a.noise_kind == 1) {
        float x = *ou;
        x += a.ou_theta * (a.ou_mu - x) * a.ou_dt
             + a.ou_sigma * sqrtf(a.ou_dt) * roll_explore_n01(a, ep, tick,
                                                              ctr_lo);
        *ou = x;
        u += a.eps * x;
    }
    return fminf(fmaxf(u, -1.0f), 1.0f);
}

// PER leaf of a new row: max_priority^alpha in both trees.  A kernel reads
// the value once, before its row loop.
__device__ inline double roll_leaf_value(const RollCore& a) {
    return a.sum_tree
        ? per_leaf_value(a.cnt->max_priority, a.per_alpha) : 0.0;
}

__device__ inline void roll_write_leaf(const RollCore& a, long dst, double pa) {
    if (a.sum_tree) {
        a.sum_tree[a.tree_cap + dst] = pa;
        a.min_tree[a.tree_cap + dst] = pa;
    }
}

}  // namespace d4pg
