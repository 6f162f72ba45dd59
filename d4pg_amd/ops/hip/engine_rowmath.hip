// Row and probe formulas of the train step, one device implementation each:
// the wave-wide softmax, the C51 projection scatter, the CE and policy-head
// gradients and the row priority, their quantile-regression counterparts
// (target samples, quantile-Huber gradient, policy row), the PER descent / IS
// weight, the uniform draw, the sample+gather both share, the leaf write and
// level-synchronised path repair of the sum/min trees, the schedule-counter
// tick and Adam's bias-correction terms.  Used by all three paths
// (persistent, row-block, wide) and by the replay kernels, which is what keeps
// them bit-for-bit equal.  A "row" helper is called by one whole wave (64
// lanes, lane = atom); a "workgroup-wide" helper by every thread of the
// workgroup.  Helpers take plain values and pointers (the sample body, which
// touches twenty buffers, takes the StepArgs) and fix the operation order;
// callers own tiling, launch geometry and loss accumulation.

namespace d4pg {

// softmax over the valid lanes of a wave: lane's e / sum (0 on invalid lanes).
// (p_fwd keeps its own spelling of this, see the note there.)
__device__ __forceinline__ float softmax_wave(float v, bool valid) {
    float mx = valid ? v : -INFINITY;
    for (int s = 32; s > 0; s >>= 1) mx = fmaxf(mx, __shfl_xor(mx, s, 64));
    float e = valid ? __expf(v - mx) : 0.f;
    float sum = e;
    for (int s = 32; s > 0; s >>= 1) sum += __shfl_xor(sum, s, 64);
    return e / sum;
}

// ---- C51 -------------------------------------------------------------------
// Fractional bin position b of a clamped Tz and its two neighbour bins l < u.
// In float32 (v_max - v_min) / delta can round ABOVE K-1 (e.g. 27.000002 at
// K=28 on [-300, 0]); uncapped, ceil(b) = K indexes one float past the row.
// Capping b at K-1 leaves every in-range value bit-identical.  Equal-bin
// handling as in algo/projection.py (index-adjust so weights become (0,1)).
__device__ __forceinline__ float c51_bins(float tz, float v_min, float delta,
                                          int K, int& l, int& u) {
    float b = fminf((tz - v_min) / delta, (float)(K - 1));
    l = (int)floorf(b);
    u = (int)ceilf(b);
    if (l == u) { if (u > 0) l -= 1; else u += 1; }
    return b;
}

// atom `lane` of the support
__device__ __forceinline__ float c51_atom(float v_min, float v_max, int K,
                                          int lane) {
    float delta = (v_max - v_min) / (K - 1);
    return v_min + lane * delta;
}

// Project one row's target distribution (lane's p = p_t[row][lane]) through
// Tz = r + gamma_n (1 - d) z into the wave-private LDS row mrow[64]; on
// return mrow[0..K) holds the projected row m.
__device__ __forceinline__ void c51_project_row(float* mrow, float p, float r,
                                                float d, float v_min,
                                                float v_max, float gamma_n,
                                                int K, int lane) {
    mrow[lane] = 0.f;
    __builtin_amdgcn_wave_barrier();
    if (lane < K) {
        float delta = (v_max - v_min) / (K - 1);
        float z = v_min + lane * delta;
        float tz = r + gamma_n * (1.f - d) * z;
        tz = fminf(v_max, fmaxf(v_min, tz));
        int l, u;
        float b = c51_bins(tz, v_min, delta, K, l, u);
        atomicAdd(&mrow[l], p * ((float)u - b));
        atomicAdd(&mrow[u], p * (b - (float)l));
    }
    __builtin_amdgcn_wave_barrier();
}

// CE gradient of one row (mv, qv are 0 on lanes >= K): lane's dlogit, and
// wave-reduced on every lane dot = <m, q> (the priority before per_eps) and
// ce = -<m, log q> (the row's loss before scale / B).
struct CeRow { float dz, dot, ce; };

__device__ __forceinline__ CeRow ce_grad_row(float mv, float qv, float scale,
                                             int B) {
    float dot = mv * qv;
    float ce = -mv * __logf(qv + 1e-10f);
    for (int s = 32; s > 0; s >>= 1) {
        dot += __shfl_xor(dot, s, 64);
        ce += __shfl_xor(ce, s, 64);
    }
    return {scale * (qv - mv) / (float)B, dot, ce};
}

// The row's replay priority from ce_grad_row's inputs and its dot, on every
// lane: the reference's proxy <m, q> + eps, or with true_td the TD error of
// the expectations |E_m[z] - E_q[z]| + eps (z = lane's atom).  The two extra
// wave reductions run only under true_td (wave-uniform).
__device__ __forceinline__ float ce_priority_row(float mv, float qv,
                                                 float dot, float z,
                                                 int true_td, float per_eps) {
    if (!true_td) return dot + per_eps;
    float em = mv * z, eq = qv * z;
    for (int s = 32; s > 0; s >>= 1) {
        em += __shfl_xor(em, s, 64);
        eq += __shfl_xor(eq, s, 64);
    }
    return fabsf(em - eq) + per_eps;
}

// Policy-head gradient of one row through the softmax:
// L = -(1/B) sum_b sum_k q_k z_k  =>  dlogits_j = -q_j (z_j - E_q[z]) / B.
// e returns E_q[z], wave-reduced (the row's loss is -e / B).
__device__ __forceinline__ float policy_grad_row(float qv, float z, int B,
                                                 float& e) {
    e = qv * z;
    for (int s = 32; s > 0; s >>= 1) e += __shfl_xor(e, s, 64);
    return -qv * (z - e) / (float)B;
}

// ---- quantile regression (DIST_QUANTILE) -----------------------------------
// Lane i is quantile i, tau_i = (2i + 1) / (2K); the heads are the raw fc3
// outputs.  The weight |tau_i - 1{u < 0}| of a pair is tau_i for u >= 0 and
// 1 - tau_i below; both are formed as one integer ratio each, so each carries
// one rounding (1 - tau_i computed from a rounded tau_i would carry tau_i's
// absolute error, K times larger relative to 1 / 2K).  Every product and sum
// below is an explicit fmaf / __f*_rn, so the compiler's contraction choice
// cannot differ between the kernels that inline these helpers.

// Target samples of one row: lane's T = r + gamma_n (1 - d) theta' into the
// wave-private LDS row trow[64] (0 on lanes >= K); returns the lane's T.
__device__ __forceinline__ float qr_target_row(float* trow, float th_t,
                                               float r, float d,
                                               float gamma_n, int K,
                                               int lane) {
    float t = (lane < K)
        ? __fmaf_rn(__fmul_rn(gamma_n, 1.f - d), th_t, r) : 0.f;
    trow[lane] = t;
    __builtin_amdgcn_wave_barrier();
    return t;
}

// Quantile-Huber gradient of one row from trow (qr_target_row) and the lane's
// online quantile th (0 on lanes >= K).  Lane i walks j = 0 .. K-1 ascending:
//   u = T_j - theta_i,  w = |tau_i - 1{u < 0}|
//   gsum += w clip(u, -kappa, kappa),  lsum += w H(u)
// dz is the lane's head gradient scale / B * (-(gsum / kappa) / K); loss, on
// every lane, the row loss (1/K) sum_i sum_j rho_ij before scale / B; pri, on
// every lane, |mean_j T_j - mean_i theta_i| + per_eps.  The three wave sums
// share one butterfly.
struct QrRow { float dz, loss, pri; };

__device__ __forceinline__ QrRow qr_grad_row(const float* trow, float th,
                                             float scale, int B, int K,
                                             float kappa, float per_eps,
                                             int lane) {
    float k2 = (float)(2 * K);
    float w_pos = (float)(2 * lane + 1) / k2;             // tau_i
    float w_neg = (float)(2 * K - 2 * lane - 1) / k2;     // 1 - tau_i
    float hk = 0.5f * kappa;
    float gsum = 0.f, lsum = 0.f;
    for (int j = 0; j < K; ++j) {
        float u = __fsub_rn(trow[j], th);
        float au = fabsf(u);
        float w = (u < 0.f) ? w_neg : w_pos;
        float cl = fminf(fmaxf(u, -kappa), kappa);
        float h = (au <= kappa) ? __fmul_rn(__fmul_rn(0.5f, u), u)
                                : __fmul_rn(kappa, __fsub_rn(au, hk));
        gsum = __fmaf_rn(w, cl, gsum);
        lsum = __fmaf_rn(w, h, lsum);
    }
    bool valid = lane < K;
    float ls = valid ? lsum / kappa : 0.f;
    float ts = valid ? trow[lane] : 0.f;
    float qs = valid ? th : 0.f;
    for (int s = 32; s > 0; s >>= 1) {
        ls += __shfl_xor(ls, s, 64);
        ts += __shfl_xor(ts, s, 64);
        qs += __shfl_xor(qs, s, 64);
    }
    float fk = (float)K;
    QrRow r;
    r.dz = __fmul_rn(scale / (float)B, -(gsum / kappa) / fk);
    r.loss = ls / fk;
    r.pri = __fadd_rn(fabsf(__fsub_rn(ts / fk, qs / fk)), per_eps);
    return r;
}

// Policy-head gradient of one row: L = -(1/B) sum_b (1/K) sum_i theta_i, so
// the head gradient is the constant -1 / (B K) on lanes < K.  e returns
// mean_i theta_i, wave-reduced (the row's loss is -e / B).
__device__ __forceinline__ float qr_policy_row(float th, int B, int K,
                                               int lane, float& e) {
    e = (lane < K) ? th : 0.f;
    for (int s = 32; s > 0; s >>= 1) e += __shfl_xor(e, s, 64);
    e = e / (float)K;
    return -1.f / (float)(B * K);
}

// ---- PER sampling ----------------------------------------------------------
// 4-ary descent over the binary layout: a stored parent is bit-exactly the
// double-sum of its children, so comparing against grandchildren sums
// reproduces two binary steps with ONE contiguous 32 B load — half the
// dependent-load chain (20 levels -> 10 loads at 1e6 leaves).  NT: deep levels
// are random-access and read once per step, so they bypass L2 and leave the
// hot top of the tree cached.  Returns the leaf NODE (leaf index + tree_cap).
template <bool NT>
__device__ __forceinline__ long per_descend(const double* sum_tree,
                                            long tree_cap, double mass) {
    auto ld = [&](long i, bool deep) {
        return (NT && deep) ? __builtin_nontemporal_load(&sum_tree[i])
                            : sum_tree[i];
    };
    long node = 1;
    while (node < tree_cap / 2) {
        long gb = 4 * node;
        bool deep = gb >= 16384;
        double g0 = ld(gb, deep), g1 = ld(gb + 1, deep),
               g2 = ld(gb + 2, deep);
        double s01 = g0 + g1;
        if (mass <= s01) {
            if (mass <= g0) node = gb;
            else { mass -= g0; node = gb + 1; }
        } else {
            mass -= s01;
            if (mass <= g2) node = gb + 2;
            else { mass -= g2; node = gb + 3; }
        }
    }
    if (node < tree_cap) {                 // odd final level
        double ls = ld(2 * node, node >= 16384);
        if (mass > ls) { mass -= ls; node = 2 * node + 1; }
        else           { node = 2 * node; }
    }
    return node;
}

// beta of the linear schedule at position beta_t
__device__ __forceinline__ float per_beta(long long beta_t, float beta0,
                                          float beta_iters) {
    float frac = fminf((float)((double)beta_t / beta_iters), 1.0f);
    return beta0 + frac * (1.0f - beta0);
}

// IS weight w = (p N)^-beta / max_w, max_w from the smallest priority
__device__ __forceinline__ float per_is_weight(double p, double p_min,
                                               long long n, float beta) {
    double max_w = pow(p_min * (double)n, (double)-beta);
    return (float)(pow(p * (double)n, (double)-beta) / max_w);
}

// Gather tail of both sample helpers: lane 0 holds the drawn slot and has
// written bidx / bw / br / bd; all lanes cooperatively gather the transition
// row into the batch SoA, states into bs_out.  NT keeps the gathered replay
// rows (random, never re-read) out of L2.  NT is the persistent kernel's
// form: its tail crew reads bs / bs2 / ba across a fence-free crew barrier,
// so there the three gather stores are write-through (st_wt).  bidx / bw /
// br / bd are read only behind a grid barrier and stay plain.
template <bool NT>
__device__ __forceinline__ void sample_gather_row(const StepArgs& g,
                                                  float* bs_out, int probe,
                                                  int lane, long idx) {
    auto ld = [](const float* p) {
        return NT ? __builtin_nontemporal_load(p) : *p;
    };
    auto st = [](float* p, float v) {
        if (NT) st_wt(p, v); else *p = v;
    };
    idx = __shfl(idx, 0, 64);
    for (int k = lane; k < g.O; k += 64) {
        st(&bs_out[(long)probe * g.O + k], ld(&g.rs[idx * g.O + k]));
        st(&g.bs2[(long)probe * g.O + k], ld(&g.rs2[idx * g.O + k]));
    }
    for (int k = lane; k < g.A; k += 64)
        st(&g.ba[(long)probe * g.A + k], ld(&g.ra[idx * g.A + k]));
}

// PER sample + gather of one probe by one wave: lane 0 walks the sum tree
// (double, exact) and writes the IS weight, then the gather tail.  epoch /
// beta_t are the schedule values of the step being sampled.
template <bool NT>
__device__ __forceinline__ void per_sample_probe(const StepArgs& g,
                                                 float* bs_out, int probe,
                                                 int lane, long long epoch,
                                                 long long beta_t) {
    long long n = g.cnt->size;
    double total = g.sum_tree[1];
    float beta = per_beta(beta_t, g.per_beta0, g.per_beta_iters);
    long idx = 0;
    if (lane == 0) {
        Philox4 r = philox4(g.seed, (uint64_t)epoch, (uint64_t)probe);
        double mass = (double)u01(r.v[0]) * total;
        idx = per_descend<NT>(g.sum_tree, g.tree_cap, mass) - g.tree_cap;
        if (idx >= n) idx = n - 1;          // fp-roundoff guard at range top
        g.bidx[probe] = idx;
        g.bw[probe] = per_is_weight(g.sum_tree[g.tree_cap + idx] / total,
                                    g.min_tree[1] / total, n, beta);
        g.br[probe] = g.rr[idx];
        g.bd[probe] = g.rd[idx];
    }
    sample_gather_row<NT>(g, bs_out, probe, lane, idx);
}

// Uniform sample + gather of one probe (g.prioritized == 0; no tree is
// touched): the same philox key and counters as the PER draw, so rng_epoch
// means the same in both modes.  The slot is the high half of the 64 x 64-bit
// integer product x * n, x the draw's first two words: every slot of any
// replay size is reachable, where a float32 u01 * n stops at 2^24 distinct
// values.  beta_t is unused; the IS weight is exactly 1.
template <bool NT>
__device__ __forceinline__ void uniform_sample_probe(const StepArgs& g,
                                                     float* bs_out, int probe,
                                                     int lane, long long epoch,
                                                     long long /*beta_t*/) {
    long idx = 0;
    if (lane == 0) {
        unsigned long long n = (unsigned long long)g.cnt->size;
        Philox4 r = philox4(g.seed, (uint64_t)epoch, (uint64_t)probe);
        unsigned long long x = ((unsigned long long)r.v[0] << 32) | r.v[1];
        idx = (long)__umul64hi(x, n);       // floor(x * n / 2^64) < n
        g.bidx[probe] = idx;
        g.bw[probe] = 1.0f;
        g.br[probe] = g.rr[idx];
        g.bd[probe] = g.rd[idx];
    }
    sample_gather_row<NT>(g, bs_out, probe, lane, idx);
}

// the engine's replay mode picks the draw (wave-uniform: a kernel argument)
template <bool NT>
__device__ __forceinline__ void sample_probe(const StepArgs& g, float* bs_out,
                                             int probe, int lane,
                                             long long epoch,
                                             long long beta_t) {
    if (g.prioritized)
        per_sample_probe<NT>(g, bs_out, probe, lane, epoch, beta_t);
    else
        uniform_sample_probe<NT>(g, bs_out, probe, lane, epoch, beta_t);
}

// ---- PER write-back --------------------------------------------------------
// leaf value of a priority
__device__ __forceinline__ double per_leaf_value(float p, float alpha) {
    return pow((double)p, (double)alpha);
}

// Workgroup-wide (256 threads): write the B sampled leaves from pri and fold
// their largest priority into cnt->max_priority.  Ends on a barrier.
__device__ __forceinline__ void per_write_leaves(double* sum_tree,
                                                 double* min_tree,
                                                 long tree_cap,
                                                 const long* idx,
                                                 const float* pri, int B,
                                                 float alpha, Counters* cnt) {
    int tid = threadIdx.x;
    float local_max = 0.f;
    for (int i = tid; i < B; i += 256) {
        float p = pri[i];
        double pa = per_leaf_value(p, alpha);
        long leaf = tree_cap + idx[i];
        sum_tree[leaf] = pa;
        min_tree[leaf] = pa;
        local_max = fmaxf(local_max, p);
    }
    __shared__ float smax[256];
    smax[tid] = local_max;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) smax[tid] = fmaxf(smax[tid], smax[tid + s]);
        __syncthreads();
    }
    if (tid == 0)
        cnt->max_priority = fmaxf(cnt->max_priority, smax[0]);
    __syncthreads();
}

// Workgroup-wide exact level-synchronised repair of the paths above n
// already-written leaves (leaf_of(i) = leaf NODE of item i): per level all
// touched parents are recomputed from their (already final) children.
// Duplicate parents write identical values (benign).  nthr = workgroup size.
template <typename LeafOf>
__device__ __forceinline__ void per_repair_paths(double* sum_tree,
                                                 double* min_tree,
                                                 long tree_cap, int n,
                                                 int nthr, LeafOf leaf_of) {
    long levels = 0;
    for (long c = tree_cap; c > 1; c >>= 1) ++levels;
    for (long lv = 0; lv < levels; ++lv) {
        for (int i = threadIdx.x; i < n; i += nthr) {
            long node = leaf_of(i) >> (lv + 1);
            if (node >= 1) {
                sum_tree[node] = sum_tree[2 * node] + sum_tree[2 * node + 1];
                min_tree[node] = fmin(min_tree[2 * node],
                                      min_tree[2 * node + 1]);
            }
        }
        __syncthreads();
    }
}

// Advance the schedule counters for the NEXT step (they are initialised to 1
// so the first step sees t=1); thread 0 of the step's last kernel.
__device__ __forceinline__ void tick_counters(Counters* cnt) {
    if (threadIdx.x == 0) {
        cnt->beta_t += 1;
        cnt->adam_t_actor += 1;
        cnt->adam_t_critic += 1;
        cnt->rng_epoch += 1;
    }
}

// ---- Adam ----------------------------------------------------------------
// The bias-correction terms 1 - beta^t at step t.  Only these are shared: the
// element update itself stays written out in k_adam_lerp and p_adam_lerp.
// Device code is built with fp-contract=fast, and the compiler already rounds
// the two differently (k_adam_lerp multiplies then adds for both moments,
// p_adam_lerp fuses the second moment into an fma); one inline helper made
// the persistent kernel fuse the first moment too and changed its parameters
// in the last bit.  Sharing it needs explicit fmaf and a deliberate change
// of one path's results.
struct AdamBias { float bc1, bc2; };

__device__ __forceinline__ AdamBias adam_bias(float b1, float b2,
                                              long long t) {
    return {1.f - __powf(b1, (float)t), 1.f - __powf(b2, (float)t)};
}

// ---- global-norm gradient clipping ------------------------------------------
// The rule of torch.nn.utils.clip_grad_norm_, per net: norm = sqrt(sum g^2)
// over the whole gradient slab, scale = min(1, max_norm / (norm + 1e-6)), and
// Adam consumes scale * g (the slab itself stays raw).  The sum is taken in
// double, in one fixed order, by the two helpers below; every path calls them
// over the same chunking, so norm and scale are bitwise equal on all of them.
// No atomics, no float accumulation.
#define GN_CHUNK 4096

__host__ __device__ inline int gn_chunks(long n) {
    return (int)((n + GN_CHUNK - 1) / GN_CHUNK);
}

// Workgroup-wide (256 threads): the sum of squares of chunk `chunk` of the
// slab g[0..n) into gn_part[chunk].  Thread t folds elements t, t + 256, ...
// of the chunk ascending as double(g) * double(g) (exact: 48 bits), then a
// fixed-order LDS tree folds the 256 partials.  red: 256 doubles of LDS.
// Ends on a barrier, so red may be reused at once.
__device__ __forceinline__ void grad_sumsq_chunk(const float* g, long n,
                                                 int chunk, double* gn_part,
                                                 double* red) {
    int tid = threadIdx.x;
    long lo = (long)chunk * GN_CHUNK;
    long hi = lo + GN_CHUNK < n ? lo + GN_CHUNK : n;
    double acc = 0.0;
    for (long i = lo + tid; i < hi; i += 256) {
        double x = (double)g[i];
        acc += x * x;
    }
    red[tid] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    if (tid == 0) gn_part[chunk] = red[0];
    __syncthreads();
}

// The finish, by any one thread (or by many, each for itself): the partials
// summed in ascending chunk order, the norm and the scale Adam multiplies by.
struct GradClip { double norm; float scale; };

__device__ __forceinline__ GradClip grad_clip_finish(const double* gn_part,
                                                     long n,
                                                     double max_norm) {
    double sum = 0.0;
    int nc = gn_chunks(n);
    for (int c = 0; c < nc; ++c) sum += gn_part[c];
    double norm = sqrt(sum);
    return {norm, (float)fmin(1.0, max_norm / (norm + 1e-6))};
}

// Record one net's norm and scale in the statistics block (one thread).
__device__ __forceinline__ void grad_stats_write(GradStats* st, int is_actor,
                                                 GradClip c) {
    if (is_actor) { st->norm_actor = c.norm; st->scale_actor = c.scale; }
    else          { st->norm_critic = c.norm; st->scale_critic = c.scale; }
}

}  // namespace d4pg
