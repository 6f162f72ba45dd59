// Common types (layer geometry, config, device counters, the StepArgs block
// every train-step kernel takes), the philox RNG and the small device helpers
// every path shares.  Used by all other parts; the step's row and probe
// formulas follow in engine_rowmath.hip.
//
// Numerics: fp32 end-to-end, matching the reference's CPU fp32; per-thread
// dot products accumulate in ascending-k order so every path agrees with
// the eager torch oracle within fp32 tolerance.

#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <cmath>
#include <vector>
#include <stdexcept>

#define HIP_CHECK(cmd) do { \
    hipError_t e_ = (cmd); \
    if (e_ != hipSuccess) { \
        char buf[256]; \
        snprintf(buf, sizeof(buf), "HIP error %s at %s:%d", \
                 hipGetErrorString(e_), __FILE__, __LINE__); \
        throw std::runtime_error(buf); \
    } \
} while (0)

namespace d4pg {

// ---------------------------------------------------------------------------
// philox4x32-10 counter-based RNG (device)
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t mulhi32(uint32_t a, uint32_t b) {
    return (uint32_t)(((uint64_t)a * b) >> 32);
}

struct Philox4 { uint32_t v[4]; };

__device__ inline Philox4 philox4(uint64_t seed, uint64_t ctr_hi,
                                  uint64_t ctr_lo) {
    uint32_t c0 = (uint32_t)ctr_lo, c1 = (uint32_t)(ctr_lo >> 32);
    uint32_t c2 = (uint32_t)ctr_hi, c3 = (uint32_t)(ctr_hi >> 32);
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
    const uint32_t W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        uint32_t hi0 = mulhi32(M0, c0), lo0 = M0 * c0;
        uint32_t hi1 = mulhi32(M1, c2), lo1 = M1 * c2;
        uint32_t n0 = hi1 ^ c1 ^ k0, n1 = lo1;
        uint32_t n2 = hi0 ^ c3 ^ k1, n3 = lo0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += W0; k1 += W1;
    }
    return {c0, c1, c2, c3};
}

__device__ inline float u01(uint32_t x) {           // (0,1]
    return ((float)x + 1.0f) * 2.3283064e-10f;
}

// ---------------------------------------------------------------------------
// Engine state blocks
// ---------------------------------------------------------------------------

// One linear layer's geometry inside a parameter slab.
struct LayerDesc {
    int in1, in2, out;       // in2 > 0 => concat second input
    long w_off, b_off;       // offsets into the net's slab (floats)
};

enum Act { ACT_NONE = 0, ACT_RELU = 1, ACT_TANH = 2, ACT_SOFTMAX = 3 };

// The critic head: C51 probabilities on a fixed support (softmax head,
// projection, cross-entropy) or the values of K fixed quantiles (identity
// head, quantile-Huber loss; ARCHITECTURE.md, "Quantile critic").
enum Dist { DIST_CATEGORICAL = 0, DIST_QUANTILE = 1 };

struct EngineCfg {
    int obs, act, hidden, atoms, batch;
    long capacity;             // replay capacity (will be rounded to pow2 tree)
    float v_min, v_max, gamma_n, tau, lr_actor, lr_critic;
    float per_alpha, per_beta0, per_eps;
    long per_beta_iters;
    uint64_t seed;
    int is_weighting;          // apply IS weights to the CE loss
    int prioritized = 1;       // 0: uniform replay, no sum/min trees
    int true_td = 0;           // priority |E_m[z] - E_q[z]| for <m, q>
    int gemm_bf16 = 0;         // wide train step: bf16 MFMA operands (RNE),
                               // fp32 accumulate; batch > 512 only
    double max_grad_norm = 0;  // global-norm gradient clip, per net; 0: off
    int dist = DIST_CATEGORICAL;   // critic head (Dist)
    float kappa = 1.f;         // quantile head: Huber threshold, > 0
};

// device-side counters (one small block)
struct Counters {
    long long beta_t;          // PER beta schedule position (stateful)
    long long adam_t_actor;
    long long adam_t_critic;
    long long rng_epoch;       // bumped per step for fresh philox streams
    long long size;            // replay occupancy
    long long pos;             // replay ring position
    float max_priority;
    float loss_critic;         // per-step scalars (overwritten each step)
    float loss_actor;
};

// Gradient-clip statistics of the last step (written only when clipping is
// on; zero otherwise).  Derived state: not checkpointed, and deliberately not
// part of Counters, whose layout the staging counters and checkpoints share.
struct GradStats {
    double norm_actor, norm_critic;    // global L2 norm of the raw gradient
    float scale_actor, scale_critic;   // min(1, max_grad_norm / (norm + 1e-6))
};

// max fan-in a fwd workgroup stages (hidden(1024) + act margin)
#define FWD_XMAX 1032

__device__ inline float act_mask(int act, float h) {
    if (act == ACT_RELU) return h > 0.f ? 1.f : 0.f;
    if (act == ACT_TANH) return 1.f - h * h;
    return 1.f;
}

// Write-through store and L1-bypassing load for data one workgroup hands to
// another INSIDE a launch without a cache fence (the persistent kernel's quad
// and crew hand-offs, engine_persistent.hip): global_store_dword /
// global_load_dword ... sc1.  The store leaves no dirty line for a release
// fence to write back; the load is served by L2, never by a line this CU's
// L1 still holds from an earlier step.  The address_space(1) casts keep both
// `global_`: pointer parameters of __noinline__ functions are generic, and
// a flat_ load is not a valid hand-off load.
typedef __attribute__((address_space(1))) float gfloat;
__device__ __forceinline__ void st_wt(float* p, float v) {
    __hip_atomic_store((gfloat*)p, v, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ float ld_wt(const float* p) {
    return __hip_atomic_load((const gfloat*)p, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
}

// Layer pointer bundle for a net slab.
struct NetPtrs { const float *w1, *b1, *w2, *b2, *w3, *b3, *w4, *b4; };

__device__ inline NetPtrs net_ptrs(const float* slab, const LayerDesc* l) {
    return {slab + l[0].w_off, slab + l[0].b_off,
            slab + l[1].w_off, slab + l[1].b_off,
            slab + l[2].w_off, slab + l[2].b_off,
            slab + l[3].w_off, slab + l[3].b_off};
}

// Everything a train step reads or writes on the device: geometry and
// hyper-parameters (filled once by the Engine constructor) and the workspace
// pointers (carved by Engine::layout).  The one argument of k_step_persistent,
// k_critic_rowblock, k_policy_rowblock and k_per_sample; the wide path's
// per-layer launches read single fields.
struct StepArgs {
    int B, O, A, H, K;
    float v_min, v_max, gamma_n, per_eps, tau, lr_actor, lr_critic;
    float per_alpha, per_beta0, per_beta_iters;
    int is_weighting;
    int prioritized, true_td;
    uint64_t seed;
    long tree_cap;                   // 0 (and null trees) on uniform replay
    long n_actor, n_critic;
    LayerDesc al[4], cl[4];
    // params / grads / moments / targets
    float *p_actor, *p_actor_t, *p_critic, *p_critic_t;
    float *g_actor, *g_critic, *m_actor, *v_actor, *m_critic, *v_critic;
    // replay + trees
    float *rs, *ra, *rr, *rs2, *rd;
    double *sum_tree, *min_tree;
    // batch (bs is double-buffered on the persistent path: the policy-block
    // tail pre-samples the NEXT step's batch while this step's bs is still
    // read by the policy forward and the actor dW)
    float *bs, *bs_b, *ba, *br, *bs2, *bd, *bw, *pri;
    long *bidx;
    // activations / deltas workspace
    float *at_h1, *at_h2, *at_h3, *a2;              // actor_target path
    float *ct_h1, *ct_h2, *ct_h3, *p_t, *m_proj;    // critic_target path
    float *c_h1, *c_h2, *c_h3, *q, *dlog, *d3, *d2, *d1;   // critic + deltas
    float *pa_h1, *pa_h2, *pa_h3, *a_out;           // actor (policy) path
    float *pc_h1, *pc_h2, *pc_h3, *pq;              // critic(s, actor(s))
    // policy deltas (az1..3: at the actor's layers 1..3, both the row-block
    // and the wide path)
    float *pd3, *pd2, *pdh1, *adz, *az1, *az2, *az3;
    Counters* cnt;
    unsigned long long* gbar;        // persistent grid barrier state
    unsigned long long* tstamp;      // [64] per-phase s_memrealtime stamps
    float *da, *pda;                 // action-slice deltas (wide path)
    // gradient clipping (max_grad_norm > 0): per-chunk double sums of
    // squares of g_actor / g_critic (ceil(n / GN_CHUNK) each) and the
    // norm / scale block of the last step
    double max_grad_norm;
    double *gn_part_a, *gn_part_c;
    GradStats* gstat;
    // critic head (Dist) and the quantile head's Huber threshold; last, so
    // every other field keeps its offset.  v_min / v_max are unread under
    // DIST_QUANTILE
    int dist;
    float kappa;
};


}  // namespace d4pg
