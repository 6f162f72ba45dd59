// Per-layer VALU kernels: the tiled forward k_fwd (actor_forward and the
// rollout below 512 rows), the fused projection+CE and policy-gradient heads
// and the tanh backward of the wide path, and the fused Adam + soft-update
// shared by the row-block and wide paths.

namespace d4pg {

// A forward job: y = act(x1 [. x2] @ Wt + b), one launch per job.
struct FwdJob {
    const float* x1; const float* x2;
    const float* wt; const float* bias;
    float* y;
    int B, in1, in2, out, act;
    int nwg_b, nwg_o;        // tile grid: nwg_b row tiles x nwg_o col tiles
};

// ---- generic fused forward -------------------------------------------------
// Tile: TB rows x TO cols per workgroup; 256 threads; LDS-staged x and Wt
// chunks.  ACT_SOFTMAX requires out <= 64 and uses one wave per row.
#define TB 4
#define TO 64

__global__ void k_fwd(FwdJob j) {
    int bt = blockIdx.x / j.nwg_o;     // which row tile
    int ot = blockIdx.x % j.nwg_o;     // which col tile
    int b0 = bt * TB, o0 = ot * TO;
    int in_total = j.in1 + j.in2;

    // x rows staged ONCE (LDS broadcast reads after); weights read straight
    // from global — coalesced 256 B per wave per k, pipelined by the unroll
    // (the previous sync-staged-chunks version was latency-bound at ~20 us
    // per launch; this form measures ~3-5 us at B=64, H=256).
    __shared__ float xs[TB][FWD_XMAX];

    int tid = threadIdx.x;
    for (int t = tid; t < TB * in_total; t += 256) {
        int bb = t / in_total, kk = t % in_total;
        int gb = b0 + bb;
        float v = 0.f;
        if (gb < j.B)
            v = (kk < j.in1) ? j.x1[(long)gb * j.in1 + kk]
                             : j.x2[(long)gb * j.in2 + (kk - j.in1)];
        xs[bb][kk] = v;
    }
    __syncthreads();

    int tb = tid / TO;                 // 0..TB-1
    int to = tid % TO;                 // 0..TO-1
    int b = b0 + tb, o = o0 + to;

    float acc = 0.f;
    if (o < j.out) {
        const float* wcol = j.wt + o;
#pragma unroll 8
        for (int k = 0; k < in_total; ++k)
            acc += xs[tb][k] * wcol[(long)k * j.out];
    }

    if (b < j.B && o < j.out) {
        acc += j.bias[o];
        if (j.act == ACT_RELU) acc = fmaxf(acc, 0.f);
        else if (j.act == ACT_TANH) acc = tanhf(acc);
    }
    if (j.act == ACT_SOFTMAX) {
        // one wave handles one row (TO==64 lanes over out<=64 columns)
        bool valid = b < j.B && o < j.out;
        float sm = softmax_wave(acc, valid);
        if (valid) j.y[(long)b * j.out + o] = sm;
    } else if (b < j.B && o < j.out) {
        j.y[(long)b * j.out + o] = acc;
    }
}

// ---- fused C51 projection + CE grad + priorities (wide path) ----------------
// One wave per row over c51_project_row + ce_grad_row, the formulas the
// persistent p_project_ce and k_critic_rowblock run too; fusing the two saves
// a launch + the m round-trip.  QR: qr_target_row + qr_grad_row in their
// place (p_t holds theta', q theta, m_out T), as on the other two paths.
template <bool QR>
__global__ void k_project_ce(const float* __restrict__ p_t,
                             const float* __restrict__ r,
                             const float* __restrict__ d,
                             const float* __restrict__ q,
                             const float* __restrict__ w,
                             float* __restrict__ m_out,
                             float* __restrict__ dlogits,
                             float* __restrict__ pri, Counters* cnt,
                             int B, int K, float v_min, float v_max,
                             float gamma_n, float per_eps,
                             int is_weighting, int true_td, float kappa) {
    int lane = threadIdx.x & 63;
    int wrow = threadIdx.x / 64;
    int wpb = blockDim.x / 64;
    extern __shared__ float lm[];
    float* mrow = lm + wrow * 64;
    __shared__ float loss_red[8];
    float ce_acc = 0.f;
    // grid-stride over rows with a single per-wg loss atomic at the end:
    // one atomicAdd per ROW to the shared loss scalar serialized ~50 us
    // at B=4096 (4096 same-address RMWs)
    for (int row = blockIdx.x * wpb + wrow; row < B;
         row += gridDim.x * wpb) {
        float p = (lane < K) ? p_t[(long)row * K + lane] : 0.f;
        if (QR) {
            float t = qr_target_row(mrow, p, r[row], d[row], gamma_n, K,
                                    lane);
            float th = (lane < K) ? q[(long)row * K + lane] : 0.f;
            if (lane < K) m_out[(long)row * K + lane] = t;
            float scale = (is_weighting && w) ? w[row] : 1.f;
            QrRow g = qr_grad_row(mrow, th, scale, B, K, kappa, per_eps,
                                  lane);
            if (lane < K) dlogits[(long)row * K + lane] = g.dz;
            if (lane == 0) {
                pri[row] = g.pri;
                ce_acc += scale * g.loss / (float)B;
            }
            __builtin_amdgcn_wave_barrier();
            continue;
        }
        c51_project_row(mrow, p, r[row], d[row], v_min, v_max, gamma_n, K,
                        lane);
        float mv = (lane < K) ? mrow[lane] : 0.f;
        float qv = (lane < K) ? q[(long)row * K + lane] : 0.f;
        if (lane < K) m_out[(long)row * K + lane] = mv;
        float scale = (is_weighting && w) ? w[row] : 1.f;
        CeRow g = ce_grad_row(mv, qv, scale, B);
        if (lane < K) dlogits[(long)row * K + lane] = g.dz;
        float pr = ce_priority_row(mv, qv, g.dot,
                                   c51_atom(v_min, v_max, K, lane), true_td,
                                   per_eps);
        if (lane == 0) {
            pri[row] = pr;
            ce_acc += scale * g.ce / (float)B;
        }
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    if (lane == 0) loss_red[wrow] = ce_acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = 0.f;
        for (int wv = 0; wv < wpb; ++wv) s += loss_red[wv];
        atomicAdd(&cnt->loss_critic, s);
    }
}

// ---- policy gradient through the softmax head (K6 seed) ---------------------
// QR: the quantile head's constant gradient and mean (qr_policy_row).
template <bool QR>
__global__ void k_policy_grad(const float* __restrict__ q,
                              float* __restrict__ dlogits,
                              Counters* cnt,
                              int B, int K, float v_min, float v_max) {
    int lane = threadIdx.x & 63;
    int wrow = threadIdx.x / 64;
    int wpb = blockDim.x / 64;
    __shared__ float loss_red[8];
    float loss_acc = 0.f;
    float z = c51_atom(v_min, v_max, K, lane);
    // grid-stride rows + one per-wg loss atomic (see k_project_ce)
    for (int row = blockIdx.x * wpb + wrow; row < B;
         row += gridDim.x * wpb) {
        float qv = (lane < K) ? q[(long)row * K + lane] : 0.f;
        float e;
        float dz = QR ? qr_policy_row(qv, B, K, lane, e)
                      : policy_grad_row(qv, z, B, e);
        if (lane < K) dlogits[(long)row * K + lane] = dz;
        if (lane == 0) loss_acc += -e / (float)B;
    }
    __syncthreads();
    if (lane == 0) loss_red[wrow] = loss_acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = 0.f;
        for (int wv = 0; wv < wpb; ++wv) s += loss_red[wv];
        atomicAdd(&cnt->loss_actor, s);
    }
}

// tanh backward at the actor output: dz4 = da * (1 - a_out^2)
__global__ void k_tanh_bwd(const float* __restrict__ da,
                           const float* __restrict__ a_out,
                           float* __restrict__ dz, long n) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        float y = a_out[i];
        dz[i] = da[i] * (1.f - y * y);
    }
}

// ---- fused Adam + target soft-update in one pass (row-block, wide) ---------
// (the element update is written out here and in p_adam_lerp, see adam_bias)
// CLIP: the gradient enters as scale * g[i], rounded once into gi before the
// update reads it (an explicit multiply, never contracted into the update:
// at scale 1.0 the clip-on form is bitwise the plain one).  The slab g keeps
// the raw gradient.
template <bool CLIP>
__device__ __forceinline__ void adam_lerp_grid(
        float* __restrict__ p, const float* __restrict__ g,
        float* __restrict__ m, float* __restrict__ v,
        float* __restrict__ tgt, long n, float lr, float b1, float b2,
        float eps, float tau, const Counters* cnt, int is_actor,
        float scale) {
    AdamBias bc = adam_bias(b1, b2, is_actor ? cnt->adam_t_actor
                                             : cnt->adam_t_critic);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (long)gridDim.x * blockDim.x) {
        float gi = CLIP ? __fmul_rn(scale, g[i]) : g[i];
        float mi = b1 * m[i] + (1.f - b1) * gi;
        float vi = b2 * v[i] + (1.f - b2) * gi * gi;
        m[i] = mi; v[i] = vi;
        float pn = p[i] - lr * (mi / bc.bc1) / (sqrtf(vi / bc.bc2) + eps);
        p[i] = pn;
        tgt[i] += tau * (pn - tgt[i]);
    }
}

__global__ void k_adam_lerp(float* __restrict__ p, const float* __restrict__ g,
                            float* __restrict__ m, float* __restrict__ v,
                            float* __restrict__ tgt, long n, float lr,
                            float b1, float b2, float eps, float tau,
                            const Counters* cnt, int is_actor) {
    adam_lerp_grid<false>(p, g, m, v, tgt, n, lr, b1, b2, eps, tau, cnt,
                          is_actor, 1.f);
}

// The clip-on instantiation: the scale is read from the statistics block
// k_grad_finish wrote just before (device memory, because it changes per
// step under graph replay).
__global__ void k_adam_lerp_clip(float* __restrict__ p,
                                 const float* __restrict__ g,
                                 float* __restrict__ m, float* __restrict__ v,
                                 float* __restrict__ tgt, long n, float lr,
                                 float b1, float b2, float eps, float tau,
                                 const Counters* cnt, int is_actor,
                                 const GradStats* st) {
    adam_lerp_grid<true>(p, g, m, v, tgt, n, lr, b1, b2, eps, tau, cnt,
                         is_actor,
                         is_actor ? st->scale_actor : st->scale_critic);
}

// ---- global-norm gradient clipping (row-block, wide) -------------------------
// One workgroup per GN_CHUNK chunk of the slab, then a one-workgroup finish:
// the two helpers of engine_rowmath.hip the persistent kernel calls too.
__global__ void __launch_bounds__(256)
k_grad_norm(const float* __restrict__ g, long n, double* gn_part) {
    __shared__ double red[256];
    grad_sumsq_chunk(g, n, (int)blockIdx.x, gn_part, red);
}

__global__ void k_grad_finish(const double* gn_part, long n, double max_norm,
                              GradStats* st, int is_actor) {
    if (threadIdx.x == 0)
        grad_stats_write(st, is_actor,
                         grad_clip_finish(gn_part, n, max_norm));
}

}  // namespace d4pg
