// Row-block kernels: one wave owns one batch row through the whole forward /
// backward-dX chain, plus the batched dW launch k_bwd4.  Used by train steps
// at 256 < B <= 512, by every split step up to B = 512, and as the fallback
// when the persistent grid is not co-resident; 8 kernels per step, hipGraph-
// captured.

namespace d4pg {

// ===========================================================================
// Row-block megakernels (small-batch learner path)
// ===========================================================================
// Key observation: until the dW reduction, every quantity in the D4PG train
// step is per-batch-row: forwards, softmax, the C51 projection, CE/policy
// gradients and the whole backward-dX chain.  So ONE WAVE owns ONE row and
// runs the entire chain against L2-resident weights with zero barriers —
// the step then needs only 8 kernels (sample, critic-row-block, critic-dW,
// critic-Adam+lerp, policy-row-block, actor-dW, actor-Adam+lerp, PER
// write-back), which matters because at B=64 the step is bounded by the
// ~1.5-5 us per-kernel floor, not by FLOPs.

// per-wave LDS carve (floats): [xb XMAX][yb XMAX][h1 H][h2 H][h3 H]
// [aa 32][row0 64][row1 64][row2 64]
struct RowLds {
    float *xb, *yb, *h1, *h2, *h3, *aa, *r0, *r1, *r2;
};

__device__ inline RowLds rb_carve(float* base, int wid, int H) {
    long per = 2 * FWD_XMAX + 3 * H + 32 + 3 * 64;
    float* p = base + (long)wid * per;
    RowLds L;
    L.xb = p;               p += FWD_XMAX;
    L.yb = p;               p += FWD_XMAX;
    L.h1 = p;               p += H;
    L.h2 = p;               p += H;
    L.h3 = p;               p += H;
    L.aa = p;               p += 32;
    L.r0 = p;               p += 64;
    L.r1 = p;               p += 64;
    L.r2 = p;
    return L;
}

__host__ __device__ inline long rb_lds_bytes(int H) {
    return 4L * (2 * FWD_XMAX + 3 * H + 32 + 3 * 64) * 4;
}

// y[o] = act(sum_k xb[k] * Wt[k][o] + b[o]), lane-parallel over o.
__device__ inline void rb_fwd(const float* xb, float* yb, const float* wt,
                              const float* bias, int in_total, int out,
                              int act_kind, float* grow, int lane) {
    for (int oc = 0; oc < out; oc += 64) {
        int o = oc + lane;
        float acc = 0.f;
        if (o < out) {
            const float* wcol = wt + o;
#pragma unroll 16
            for (int k = 0; k < in_total; ++k)
                acc += xb[k] * wcol[(long)k * out];
            acc += bias[o];
            if (act_kind == ACT_RELU) acc = fmaxf(acc, 0.f);
            else if (act_kind == ACT_TANH) acc = tanhf(acc);
            yb[o] = acc;
            if (grow) grow[o] = acc;
        }
    }
}

// softmax head (out <= 64): q[o] = softmax(logits)[o]
__device__ inline void rb_fwd_softmax(const float* xb, float* qrow,
                                      const float* wt, const float* bias,
                                      int in_total, int out, float* grow,
                                      int lane) {
    float acc = -INFINITY;
    if (lane < out) {
        const float* wcol = wt + lane;
        float a = 0.f;
#pragma unroll 16
        for (int k = 0; k < in_total; ++k)
            a += xb[k] * wcol[(long)k * out];
        acc = a + bias[lane];
    }
    float q = softmax_wave(acc, lane < out);
    if (lane < out) {
        qrow[lane] = q;
        if (grow) grow[lane] = q;
    }
}

// The critic-family head (out <= 64) into qrow and the global row grow:
// softmax probabilities, or with QR the raw outputs (the quantile values).
template <bool QR>
__device__ inline void rb_fwd_head(const float* xb, float* qrow,
                                   const float* wt, const float* bias,
                                   int in_total, int out, float* grow,
                                   int lane) {
    if (QR) rb_fwd(xb, qrow, wt, bias, in_total, out, ACT_NONE, grow, lane);
    else rb_fwd_softmax(xb, qrow, wt, bias, in_total, out, grow, lane);
}

// dx[i] = (sum_o dz[o] * Wt[i][o]) * act'(hprev[i]), lane-parallel over i.
__device__ inline void rb_bwd_dx(const float* dzb, const float* wt,
                                 int in_lo, int in_hi, int in_total, int out,
                                 const float* hprev, int prev_act,
                                 float* dxb, float* grow, int lane) {
    for (int ic = in_lo; ic < in_hi; ic += 64) {
        int i = ic + lane;
        float acc = 0.f;
        if (i < in_hi) {
            const float* wrow = wt + (long)i * out;
#pragma unroll 16
            for (int o = 0; o < out; ++o)
                acc += dzb[o] * wrow[o];
            if (hprev)
                acc *= act_mask(prev_act, hprev[i - in_lo]);
            if (dxb) dxb[i - in_lo] = acc;
            if (grow) grow[i - in_lo] = acc;
        }
    }
}

// K2: target forwards + projection + critic forward + CE grad + priorities
// + backward-dX chain.  One wave per row, no barriers.  QR: the quantile
// head (identity heads, target samples for the projection, quantile-Huber
// for the CE row); the categorical instantiation carries no branch on it.
template <bool QR>
__global__ void __launch_bounds__(256)
k_critic_rowblock(StepArgs g) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int b = blockIdx.x * 4 + wid;
    if (b >= g.B) return;
    RowLds L = rb_carve(smem, wid, g.H);
    NetPtrs at = net_ptrs(g.p_actor_t, g.al);
    NetPtrs ct = net_ptrs(g.p_critic_t, g.cl);
    NetPtrs c = net_ptrs(g.p_critic, g.cl);
    int O = g.O, A = g.A, H = g.H, K = g.K;

    // ---- actor_target(s2) -> a2 ----
    for (int k = lane; k < O; k += 64) L.xb[k] = g.bs2[(long)b * O + k];
    rb_fwd(L.xb, L.yb, at.w1, at.b1, O, H, ACT_RELU, nullptr, lane);
    rb_fwd(L.yb, L.xb, at.w2, at.b2, H, H, ACT_NONE, nullptr, lane);
    rb_fwd(L.xb, L.yb, at.w3, at.b3, H, H, ACT_RELU, nullptr, lane);
    rb_fwd(L.yb, L.aa, at.w4, at.b4, H, A, ACT_TANH,
           g.a2 + (long)b * A, lane);

    // ---- critic_target(s2, a2) -> p_t ----
    for (int k = lane; k < O; k += 64) L.xb[k] = g.bs2[(long)b * O + k];
    rb_fwd(L.xb, L.yb, ct.w1, ct.b1, O, H, ACT_RELU, nullptr, lane);
    for (int k = lane; k < A; k += 64) L.yb[H + k] = L.aa[k];
    rb_fwd(L.yb, L.xb, ct.w2, ct.b2, H + A, H, ACT_RELU, nullptr, lane);
    rb_fwd(L.xb, L.yb, ct.w3, ct.b3, H, H, ACT_RELU, nullptr, lane);
    rb_fwd_head<QR>(L.yb, L.r0, ct.w4, ct.b4, H, K,
                    g.p_t + (long)b * K, lane);         // r0 = p_t row

    // ---- C51 projection of r0 -> r1 (m row); QR: target samples T ----
    if (QR)
        qr_target_row(L.r1, (lane < K) ? L.r0[lane] : 0.f, g.br[b], g.bd[b],
                      g.gamma_n, K, lane);
    else
        c51_project_row(L.r1, (lane < K) ? L.r0[lane] : 0.f, g.br[b],
                        g.bd[b], g.v_min, g.v_max, g.gamma_n, K, lane);
    if (lane < K) g.m_proj[(long)b * K + lane] = L.r1[lane];

    // ---- critic(s, a) -> q (saving h1..h3) ----
    for (int k = lane; k < O; k += 64) L.xb[k] = g.bs[(long)b * O + k];
    rb_fwd(L.xb, L.h1, c.w1, c.b1, O, H, ACT_RELU,
           g.c_h1 + (long)b * H, lane);
    for (int k = lane; k < H; k += 64) L.xb[k] = L.h1[k];
    for (int k = lane; k < A; k += 64) L.xb[H + k] = g.ba[(long)b * A + k];
    rb_fwd(L.xb, L.h2, c.w2, c.b2, H + A, H, ACT_RELU,
           g.c_h2 + (long)b * H, lane);
    rb_fwd(L.h2, L.h3, c.w3, c.b3, H, H, ACT_RELU,
           g.c_h3 + (long)b * H, lane);
    rb_fwd_head<QR>(L.h3, L.r0, c.w4, c.b4, H, K, g.q + (long)b * K, lane);

    // ---- CE grad + priority (r0 = q, r1 = m) ----
    if (QR) {
        float th = (lane < K) ? L.r0[lane] : 0.f;
        float scale = (g.is_weighting && g.bw) ? g.bw[b] : 1.f;
        QrRow r = qr_grad_row(L.r1, th, scale, g.B, K, g.kappa, g.per_eps,
                              lane);
        if (lane < K) {
            L.r2[lane] = r.dz;
            g.dlog[(long)b * K + lane] = r.dz;
        }
        if (lane == 0) {
            g.pri[b] = r.pri;
            atomicAdd(&g.cnt->loss_critic, scale * r.loss / (float)g.B);
        }
    } else {
        float qv = (lane < K) ? L.r0[lane] : 0.f;
        float mv = (lane < K) ? L.r1[lane] : 0.f;
        float scale = (g.is_weighting && g.bw) ? g.bw[b] : 1.f;
        CeRow r = ce_grad_row(mv, qv, scale, g.B);
        if (lane < K) {
            L.r2[lane] = r.dz;
            g.dlog[(long)b * K + lane] = r.dz;
        }
        float pri = ce_priority_row(mv, qv, r.dot,
                                    c51_atom(g.v_min, g.v_max, K, lane),
                                    g.true_td, g.per_eps);
        if (lane == 0) {
            g.pri[b] = pri;
            atomicAdd(&g.cnt->loss_critic, scale * r.ce / (float)g.B);
        }
    }

    // ---- backward-dX chain (r2 = dlogits) ----
    rb_bwd_dx(L.r2, c.w4, 0, H, H, K, L.h3, ACT_RELU, L.xb,
              g.d3 + (long)b * H, lane);                 // dz3
    rb_bwd_dx(L.xb, c.w3, 0, H, H, H, L.h2, ACT_RELU, L.yb,
              g.d2 + (long)b * H, lane);                 // dz2
    rb_bwd_dx(L.yb, c.w2, 0, H, H + A, H, L.h1, ACT_RELU, L.xb,
              g.d1 + (long)b * H, lane);                 // dz1 (h-part only)
}

// K5: actor forward + critic(s, actor(s)) + policy grad + dX chain down to
// the actor's per-layer dz's.  One wave per row.  QR as in k_critic_rowblock.
template <bool QR>
__global__ void __launch_bounds__(256)
k_policy_rowblock(StepArgs g) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int b = blockIdx.x * 4 + wid;
    if (b >= g.B) return;
    RowLds L = rb_carve(smem, wid, g.H);
    NetPtrs a = net_ptrs(g.p_actor, g.al);
    NetPtrs c = net_ptrs(g.p_critic, g.cl);
    int O = g.O, A = g.A, H = g.H, K = g.K;

    // ---- actor(s): save pa_h1..3 in h1..h3 ----
    for (int k = lane; k < O; k += 64) L.xb[k] = g.bs[(long)b * O + k];
    rb_fwd(L.xb, L.h1, a.w1, a.b1, O, H, ACT_RELU,
           g.pa_h1 + (long)b * H, lane);
    rb_fwd(L.h1, L.h2, a.w2, a.b2, H, H, ACT_NONE,
           g.pa_h2 + (long)b * H, lane);
    rb_fwd(L.h2, L.h3, a.w3, a.b3, H, H, ACT_RELU,
           g.pa_h3 + (long)b * H, lane);
    rb_fwd(L.h3, L.aa, a.w4, a.b4, H, A, ACT_TANH,
           g.a_out + (long)b * A, lane);

    // ---- critic(s, a_out): keep pc_h1..3 in xb/yb + globals ----
    for (int k = lane; k < O; k += 64) L.xb[k] = g.bs[(long)b * O + k];
    rb_fwd(L.xb, L.yb, c.w1, c.b1, O, H, ACT_RELU,
           g.pc_h1 + (long)b * H, lane);
    for (int k = lane; k < A; k += 64) L.yb[H + k] = L.aa[k];
    rb_fwd(L.yb, L.xb, c.w2, c.b2, H + A, H, ACT_RELU,
           g.pc_h2 + (long)b * H, lane);
    rb_fwd(L.xb, L.yb, c.w3, c.b3, H, H, ACT_RELU,
           g.pc_h3 + (long)b * H, lane);
    // yb holds pc_h3; xb holds pc_h2 — careful reuse below.
    rb_fwd_head<QR>(L.yb, L.r0, c.w4, c.b4, H, K, g.pq + (long)b * K, lane);

    // ---- policy head gradient: pd4 = -q (z - E[z]) / B ----
    {
        float qv = (lane < K) ? L.r0[lane] : 0.f;
        float e;
        float dz = QR ? qr_policy_row(qv, g.B, K, lane, e)
                      : policy_grad_row(qv,
                                        c51_atom(g.v_min, g.v_max, K, lane),
                                        g.B, e);
        if (lane < K) L.r2[lane] = dz;
        // the quantile form also publishes the head gradient in pd3, as the
        // persistent and wide paths do (the categorical row-block kernel
        // keeps it in LDS only, and stays as it was)
        if (QR && lane < K) g.pd3[(long)b * K + lane] = dz;
        if (lane == 0) atomicAdd(&g.cnt->loss_actor, -e / (float)g.B);
    }

    // ---- critic dX (no dW): r2 -> da -> actor dz chain ----
    // masks for the critic activations come from the global rows just
    // written (pc_h3/pc_h2); the actor's h1..h3 are still LDS-resident.
    const float* gpc_h3 = g.pc_h3 + (long)b * H;
    const float* gpc_h2 = g.pc_h2 + (long)b * H;
    // dz3' = (r2 @ W4c^T) * relu'(pc_h3)           -> xb
    rb_bwd_dx(L.r2, c.w4, 0, H, H, K, gpc_h3, ACT_RELU, L.xb, nullptr, lane);
    // dz2' = (xb @ W3c^T) * relu'(pc_h2)           -> yb
    rb_bwd_dx(L.xb, c.w3, 0, H, H, H, gpc_h2, ACT_RELU, L.yb, nullptr, lane);
    // da = action slice of (yb @ W2c^T)            -> r1[0..A)
    rb_bwd_dx(L.yb, c.w2, H, H + A, H + A, H, nullptr, ACT_NONE, L.r1,
              nullptr, lane);
    // adz = da * (1 - a_out^2)                     -> r1, stored
    if (lane < A) {
        float y = L.aa[lane];
        float v = L.r1[lane] * (1.f - y * y);
        L.r1[lane] = v;
        g.adz[(long)b * A + lane] = v;
    }
    // actor dz chain: az3 = (r1 @ W4a^T)*relu'(h3) -> xb
    rb_bwd_dx(L.r1, a.w4, 0, H, H, A, L.h3, ACT_RELU, L.xb,
              g.az3 + (long)b * H, lane);
    // az2 = (xb @ W3a^T) * 1 (h2 had no act)       -> yb
    rb_bwd_dx(L.xb, a.w3, 0, H, H, H, nullptr, ACT_NONE, L.yb,
              g.az2 + (long)b * H, lane);
    // az1 = (yb @ W2a^T) * relu'(h1)               -> xb
    rb_bwd_dx(L.yb, a.w2, 0, H, H, H, L.h1, ACT_RELU, L.xb,
              g.az1 + (long)b * H, lane);
}

// Weight-gradient job for one layer: given dz (grad wrt pre-activation,
// [B,out]):  dWt[i][o] = sum_b x[b][i] dz[b][o];  db[o] = sum_b dz[b][o]
// Four of these share one k_bwd4 launch, each owning a slice of its grid.
struct BwdJob {
    const float* dz;
    const float* x1; const float* x2;       // layer inputs (concat aware)
    float* dwt; float* dbias;
    int B, in1, in2, out;
    int wg0_dw, nwg_dw_i, nwg_dw_o;         // dW tile grid slice
};

// ---- batched dW + db (row-block path) ----------------------------------------
#define BWT 16          // dW tile: BWT_i x BWT_o, thread per (i,o)

// One dW tile [BWT i x BWT o]: x^T and dz slices staged per 64-row batch
// chunk, then pure-LDS MACs (one chunk at B=64).  Accumulation over b is
// ascending.  db folds in on the i0==0 tiles.
__device__ inline void bwd_one(const BwdJob& j, int wg) {
    int in_total = j.in1 + j.in2;
    int tid = threadIdx.x;
    int rel = wg - j.wg0_dw;
    int it = rel / j.nwg_dw_o, ot = rel % j.nwg_dw_o;
    int i0 = it * BWT, o0 = ot * BWT;
    __shared__ float xs[64][BWT + 1];            // [bchunk][i]
    __shared__ float zs[64][BWT + 1];            // [bchunk][o]
    int ti = tid / BWT, to = tid % BWT;          // thread -> (i, o)
    float acc = 0.f, accb = 0.f;
    for (int bc = 0; bc < j.B; bc += 64) {
        for (int t = tid; t < 64 * BWT; t += 256) {
            int bb = t / BWT, ii = t % BWT;
            int gb = bc + bb, gi = i0 + ii;
            float xv = 0.f;
            if (gb < j.B && gi < in_total)
                xv = (gi < j.in1) ? j.x1[(long)gb * j.in1 + gi]
                                  : j.x2[(long)gb * j.in2 + (gi - j.in1)];
            xs[bb][ii] = xv;
            int oo = ii, go = o0 + oo;
            zs[bb][oo] = (gb < j.B && go < j.out)
                ? j.dz[(long)gb * j.out + go] : 0.f;
        }
        __syncthreads();
#pragma unroll 16
        for (int bb = 0; bb < 64; ++bb) {
            acc += xs[bb][ti] * zs[bb][to];
            if (ti == 0) accb += zs[bb][to];
        }
        __syncthreads();
    }
    int gi = i0 + ti, go = o0 + to;
    if (gi < in_total && go < j.out)
        j.dwt[(long)gi * j.out + go] = acc;
    if (ti == 0 && go < j.out && i0 == 0)
        j.dbias[go] = accb;
}

// the four layers' weight gradients of one net in a single launch
__global__ void k_bwd4(BwdJob j0, BwdJob j1, BwdJob j2, BwdJob j3) {
    int wg = blockIdx.x;
    if (wg < j1.wg0_dw) { bwd_one(j0, wg); return; }
    if (wg < j2.wg0_dw) { bwd_one(j1, wg); return; }
    if (wg < j3.wg0_dw) { bwd_one(j2, wg); return; }
    bwd_one(j3, wg);
}

}  // namespace d4pg
