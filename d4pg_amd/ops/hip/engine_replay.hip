// Replay and PER tree kernels: prioritized sampling + batch gather, priority
// write-back (one-workgroup and grid-wide forms), ingestion, synthetic fill and
// tree rebuild.  Used by the row-block and wide paths and by the host replay
// ops; the persistent kernel carries its own p_sample / p_per_update.

namespace d4pg {

// ---- PER sample + gather ---------------------------------------------------
// One wave per probe: lane 0 walks the sum tree (double, exact), all lanes
// then cooperatively gather the transition row into the batch SoA.
// Also computes IS weights w = ((p/total)*N)^-beta / max_w.
__global__ void k_per_sample(
        const double* __restrict__ sum_tree, const double* __restrict__ min_tree,
        long tree_cap,
        const float* __restrict__ rs, const float* __restrict__ ra,
        const float* __restrict__ rr, const float* __restrict__ rs2,
        const float* __restrict__ rd,
        int obs, int act,
        float* __restrict__ bs, float* __restrict__ ba, float* __restrict__ br,
        float* __restrict__ bs2, float* __restrict__ bd,
        float* __restrict__ bw, long* __restrict__ bidx,
        int B, const Counters* __restrict__ cnt,
        float beta0, float beta_iters, uint64_t seed) {
    int probe = blockIdx.x * (blockDim.x / 64) + (threadIdx.x / 64);
    int lane = threadIdx.x & 63;
    if (probe >= B) return;
    if (probe == 0 && lane == 0) {
        // first kernel of the step: reset the per-step loss accumulators
        // (counter increments happen in k_per_update at step end)
        const_cast<Counters*>(cnt)->loss_critic = 0.f;
        const_cast<Counters*>(cnt)->loss_actor = 0.f;
    }

    long long n = cnt->size;
    double total = sum_tree[1];
    float frac = fminf((float)((double)cnt->beta_t / beta_iters), 1.0f);
    float beta = beta0 + frac * (1.0f - beta0);

    long idx;
    if (lane == 0) {
        Philox4 r = philox4(seed, (uint64_t)cnt->rng_epoch, (uint64_t)probe);
        double mass = (double)u01(r.v[0]) * total;
        long node = 1;
        // 4-ary descent over the binary layout: a stored parent is
        // bit-exactly the double-sum of its children, so comparing
        // against grandchildren sums reproduces two binary steps with
        // ONE contiguous 32 B load — half the dependent-load chain
        // (20 levels -> 10 loads at 1e6 leaves).
        while (node < tree_cap / 2) {
            long gb = 4 * node;
            double g0 = sum_tree[gb], g1 = sum_tree[gb + 1],
                   g2 = sum_tree[gb + 2];
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
            double ls = sum_tree[2 * node];
            if (mass > ls) { mass -= ls; node = 2 * node + 1; }
            else           { node = 2 * node; }
        }
        idx = node - tree_cap;
        if (idx >= n) idx = n - 1;          // fp-roundoff guard at range top
        bidx[probe] = idx;
        // IS weight
        double p = sum_tree[tree_cap + idx] / total;
        double p_min = min_tree[1] / total;
        double max_w = pow(p_min * (double)n, (double)-beta);
        bw[probe] = (float)(pow(p * (double)n, (double)-beta) / max_w);
        br[probe] = rr[idx];
        bd[probe] = rd[idx];
    }
    idx = __shfl(idx, 0, 64);
    for (int k = lane; k < obs; k += 64) {
        bs[(long)probe * obs + k] = rs[idx * obs + k];
        bs2[(long)probe * obs + k] = rs2[idx * obs + k];
    }
    for (int k = lane; k < act; k += 64)
        ba[(long)probe * act + k] = ra[idx * act + k];
}

// ---- PER priority write-back (K12 update path) ------------------------------
// Exact level-synchronized tree repair: ONE workgroup; thread i owns probe i;
// per level all touched parents are recomputed from their (already final)
// children.  Duplicate parents write identical values (benign).
__global__ void k_per_update(double* __restrict__ sum_tree,
                             double* __restrict__ min_tree,
                             long tree_cap,
                             const long* __restrict__ idx,
                             const float* __restrict__ pri,
                             int B, float alpha, Counters* cnt) {
    int tid = threadIdx.x;
    // leaves
    float local_max = 0.f;
    for (int i = tid; i < B; i += blockDim.x) {
        float p = pri[i];
        double pa = pow((double)p, (double)alpha);
        long leaf = tree_cap + idx[i];
        sum_tree[leaf] = pa;
        min_tree[leaf] = pa;
        local_max = fmaxf(local_max, p);
    }
    // wg-reduce max priority
    __shared__ float smax[256];
    smax[tid] = local_max;
    __syncthreads();
    for (int s = blockDim.x / 2; s > 0; s >>= 1) {
        if (tid < s) smax[tid] = fmaxf(smax[tid], smax[tid + s]);
        __syncthreads();
    }
    if (tid == 0)
        cnt->max_priority = fmaxf(cnt->max_priority, smax[0]);
    __syncthreads();
    // level-synchronized repair
    long levels = 0;
    for (long c = tree_cap; c > 1; c >>= 1) ++levels;
    for (long lv = 0; lv < levels; ++lv) {
        for (int i = tid; i < B; i += blockDim.x) {
            long node = (tree_cap + idx[i]) >> (lv + 1);
            if (node >= 1) {
                sum_tree[node] = sum_tree[2 * node] + sum_tree[2 * node + 1];
                min_tree[node] = fmin(min_tree[2 * node],
                                      min_tree[2 * node + 1]);
            }
        }
        __syncthreads();
    }
    // last kernel of the step: advance the schedule counters for the NEXT
    // step (counters are initialized to 1 so the first step sees t=1)
    if (tid == 0) {
        cnt->beta_t += 1;
        cnt->adam_t_actor += 1;
        cnt->adam_t_critic += 1;
        cnt->rng_epoch += 1;
    }
}

// ---- PER write-back, wide-batch variant -------------------------------------
// On the wide path (B > 512) the single-workgroup level-synced k_per_update
// serializes (measured 305 us at B=4096); instead: one leaves kernel + one
// grid-wide kernel per four tree levels (k_per_level4), + a tiny counter-
// tick kernel.  Duplicate parents recompute identical values (benign, same
// as the in-wg version).
__global__ void k_per_leaves(double* __restrict__ sum_tree,
                             double* __restrict__ min_tree, long tree_cap,
                             const long* __restrict__ idx,
                             const float* __restrict__ pri,
                             int B, float alpha, Counters* cnt) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < B;
         i += (long)gridDim.x * blockDim.x) {
        float p = pri[i];
        double pa = pow((double)p, (double)alpha);
        long leaf = tree_cap + idx[i];
        sum_tree[leaf] = pa;
        min_tree[leaf] = pa;
        // positive floats compare correctly as int bits
        atomicMax((int*)&cnt->max_priority, __float_as_int(p));
    }
}

// Multi-level path repair: writes heights h0+1 .. h0+nlv along each
// sampled path, every node recomputed directly from the already-correct
// height-h0 snapshot (node at height h0+1+j sums its 2^(j+1) CONTIGUOUS
// height-h0 descendants), so no ordering is needed between the levels
// written by one launch.  Replaces nlv small dispatches (~4.8 us kernel
// floor each on this part) with one.
__global__ void k_per_level4(double* __restrict__ sum_tree,
                             double* __restrict__ min_tree, long tree_cap,
                             const long* __restrict__ idx, int B, long h0,
                             int nlv) {
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
         e < (long)B * nlv; e += (long)gridDim.x * blockDim.x) {
        long i = e / nlv;
        int j = (int)(e % nlv);
        long base = (tree_cap + idx[i]) >> h0;     // height-h0 ancestor
        long node = base >> (j + 1);
        if (node < 1) continue;
        long c0 = node << (j + 1);
        int cnt = 1 << (j + 1);
        // pairwise (binary-tree) combination order, so the written value
        // is BITWISE what the per-level repair would produce — the 4-ary
        // descent depends on parent == sum(children) exactly
        double sv[16], mv[16];
        for (int c = 0; c < cnt; ++c) {
            sv[c] = sum_tree[c0 + c];
            mv[c] = min_tree[c0 + c];
        }
        for (int w = cnt; w > 1; w >>= 1)
            for (int t = 0; t < (w >> 1); ++t) {
                sv[t] = sv[2 * t] + sv[2 * t + 1];
                mv[t] = fmin(mv[2 * t], mv[2 * t + 1]);
            }
        sum_tree[node] = sv[0];
        min_tree[node] = mv[0];
    }
}

__global__ void k_tick_end(Counters* cnt) {
    if (threadIdx.x == 0) {
        cnt->beta_t += 1;
        cnt->adam_t_actor += 1;
        cnt->adam_t_critic += 1;
        cnt->rng_epoch += 1;
    }
}

// ---- replay ingestion (batched add) -----------------------------------------
// T transitions appended at the ring position with priority max_priority^alpha,
// then one level-synced repair pass.  Single workgroup (T can exceed threads).
__global__ void k_replay_add(float* __restrict__ rs, float* __restrict__ ra,
                             float* __restrict__ rr, float* __restrict__ rs2,
                             float* __restrict__ rd,
                             double* __restrict__ sum_tree,
                             double* __restrict__ min_tree,
                             long tree_cap, long capacity,
                             const float* __restrict__ ts,
                             const float* __restrict__ ta,
                             const float* __restrict__ tr,
                             const float* __restrict__ ts2,
                             const float* __restrict__ td,
                             int T, int obs, int act, float alpha,
                             Counters* cnt) {
    int tid = threadIdx.x;
    long pos0 = cnt->pos;
    double pa = pow((double)cnt->max_priority, (double)alpha);
    // copy rows (grid-stride inside the WG over T*max(obs,act) elems)
    for (long e = tid; e < (long)T * obs; e += blockDim.x) {
        long t = e / obs, k = e % obs;
        long slot = (pos0 + t) % capacity;
        rs[slot * obs + k] = ts[t * obs + k];
        rs2[slot * obs + k] = ts2[t * obs + k];
    }
    for (long e = tid; e < (long)T * act; e += blockDim.x) {
        long t = e / act, k = e % act;
        long slot = (pos0 + t) % capacity;
        ra[slot * act + k] = ta[t * act + k];
    }
    for (int t = tid; t < T; t += blockDim.x) {
        long slot = (pos0 + t) % capacity;
        rr[slot] = tr[t];
        rd[slot] = td[t];
        sum_tree[tree_cap + slot] = pa;
        min_tree[tree_cap + slot] = pa;
    }
    __syncthreads();
    long levels = 0;
    for (long c = tree_cap; c > 1; c >>= 1) ++levels;
    for (long lv = 0; lv < levels; ++lv) {
        for (int t = tid; t < T; t += blockDim.x) {
            long slot = (pos0 + t) % capacity;
            long node = (tree_cap + slot) >> (lv + 1);
            if (node >= 1) {
                sum_tree[node] = sum_tree[2 * node] + sum_tree[2 * node + 1];
                min_tree[node] = fmin(min_tree[2 * node],
                                      min_tree[2 * node + 1]);
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        cnt->pos = (pos0 + T) % capacity;
        cnt->size = cnt->size + T > capacity ? capacity : cnt->size + T;
    }
}

// Bulk variant of the row-copy + leaf-init half of k_replay_add: grid-
// stride over T rows (the one-workgroup form serializes at large T —
// GPU-rollout actor ranks push 100k+ transitions per exchange).  The
// caller repairs the tree with the k_tree_build_level sweep (bandwidth-
// cheap) and bumps the counters host-side.
__global__ void k_replay_copy(float* __restrict__ rs, float* __restrict__ ra,
                              float* __restrict__ rr,
                              float* __restrict__ rs2,
                              float* __restrict__ rd,
                              double* __restrict__ sum_tree,
                              double* __restrict__ min_tree,
                              long tree_cap, long capacity, long pos0,
                              const float* __restrict__ ts,
                              const float* __restrict__ ta,
                              const float* __restrict__ tr,
                              const float* __restrict__ ts2,
                              const float* __restrict__ td,
                              int T, int obs, int act, double pa) {
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
         e < (long)T * obs; e += (long)gridDim.x * blockDim.x) {
        long t = e / obs, k = e % obs;
        long slot = (pos0 + t) % capacity;
        rs[slot * obs + k] = ts[t * obs + k];
        rs2[slot * obs + k] = ts2[t * obs + k];
    }
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
         e < (long)T * act; e += (long)gridDim.x * blockDim.x) {
        long t = e / act, k = e % act;
        long slot = (pos0 + t) % capacity;
        ra[slot * act + k] = ta[t * act + k];
    }
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < T;
         t += (long)gridDim.x * blockDim.x) {
        long slot = (pos0 + t) % capacity;
        rr[slot] = tr[t];
        rd[slot] = td[t];
        sum_tree[tree_cap + slot] = pa;
        min_tree[tree_cap + slot] = pa;
    }
}

// ---- synthetic replay fill (bench path: no H2D needed) ----------------------
__global__ void k_synth_fill(float* rs, float* ra, float* rr, float* rs2,
                             float* rd, double* sum_tree, double* min_tree,
                             long tree_cap, long capacity, long n,
                             int obs, int act, uint64_t seed, float alpha) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (long)gridDim.x * blockDim.x) {
        Philox4 r = philox4(seed, 0x5EEDull, (uint64_t)i);
        uint32_t st = r.v[0];
        for (int k = 0; k < obs; ++k) {
            Philox4 q = philox4(seed, 1 + (uint64_t)k, (uint64_t)i);
            rs[i * obs + k] = 2.f * u01(q.v[0]) - 1.f;
            rs2[i * obs + k] = 2.f * u01(q.v[1]) - 1.f;
        }
        for (int k = 0; k < act; ++k) {
            Philox4 q = philox4(seed, 1000 + (uint64_t)k, (uint64_t)i);
            ra[i * act + k] = 2.f * u01(q.v[2]) - 1.f;
        }
        rr[i] = -u01(r.v[1]) * 10.f;
        rd[i] = (u01(r.v[2]) < 0.01f) ? 1.f : 0.f;
        sum_tree[tree_cap + i] = 1.0;     // max_priority(1)^alpha
        min_tree[tree_cap + i] = 1.0;
    }
}

__global__ void k_fill_f64(double* p, long n, double v) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (long)gridDim.x * blockDim.x)
        p[i] = v;
}

// full-tree rebuild after bulk fill: one level at a time, many WGs
__global__ void k_tree_build_level(double* sum_tree, double* min_tree,
                                   long lo, long hi) {
    for (long n = lo + (long)blockIdx.x * blockDim.x + threadIdx.x; n < hi;
         n += (long)gridDim.x * blockDim.x) {
        sum_tree[n] = sum_tree[2 * n] + sum_tree[2 * n + 1];
        min_tree[n] = fmin(min_tree[2 * n], min_tree[2 * n + 1]);
    }
}

}  // namespace d4pg
