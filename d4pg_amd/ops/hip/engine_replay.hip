// Replay and PER tree kernels: prioritized sampling + batch gather, priority
// write-back (one-workgroup and grid-wide forms), ingestion, synthetic fill and
// tree rebuild.  Used by the row-block and wide paths and by the host replay
// ops.  The sampling, leaf-write and path-repair formulas themselves are the
// engine_rowmath.hip helpers, which the persistent kernel's p_sample /
// p_per_update call too.

namespace d4pg {

// ---- sample + gather (PER or uniform) --------------------------------------
// One wave per probe (sample_probe); first kernel of a row-block or wide
// step, reading the schedule position from the device counters.
__global__ void k_per_sample(StepArgs g) {
    int probe = blockIdx.x * (blockDim.x / 64) + (threadIdx.x / 64);
    int lane = threadIdx.x & 63;
    if (probe >= g.B) return;
    if (probe == 0 && lane == 0) {
        // first kernel of the step: reset the per-step loss accumulators
        // (counter increments happen in k_per_update at step end)
        g.cnt->loss_critic = 0.f;
        g.cnt->loss_actor = 0.f;
    }
    sample_probe<false>(g, g.bs, probe, lane, g.cnt->rng_epoch,
                        g.cnt->beta_t);
}

// ---- PER priority write-back (K12 update path) ------------------------------
// ONE workgroup of 256 threads: leaves, exact level-synchronized tree repair,
// then the schedule tick — this is the last kernel of a row-block step.
__global__ void k_per_update(double* __restrict__ sum_tree,
                             double* __restrict__ min_tree,
                             long tree_cap,
                             const long* __restrict__ idx,
                             const float* __restrict__ pri,
                             int B, float alpha, Counters* cnt) {
    per_write_leaves(sum_tree, min_tree, tree_cap, idx, pri, B, alpha, cnt);
    per_repair_paths(sum_tree, min_tree, tree_cap, B, 256,
                     [&](int i) { return tree_cap + idx[i]; });
    tick_counters(cnt);
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
        double pa = per_leaf_value(p, alpha);
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

__global__ void k_tick_end(Counters* cnt) { tick_counters(cnt); }

// ---- replay ingestion (batched add) -----------------------------------------
// T transitions appended at the ring position with priority max_priority^alpha,
// then one level-synced repair pass.  Single workgroup (T can exceed threads).
// Uniform replay passes null trees: the write-side kernels below (and the
// rollouts' emit kernels) then copy rows only.
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
                             long skip, Counters* cnt) {
    int tid = threadIdx.x;
    // skip: rows the host dropped from a call longer than the ring
    long pos0 = (cnt->pos + skip) % capacity;
    const bool trees = sum_tree != nullptr;
    double pa = trees ? per_leaf_value(cnt->max_priority, alpha) : 0.0;
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
        if (trees) {
            sum_tree[tree_cap + slot] = pa;
            min_tree[tree_cap + slot] = pa;
        }
    }
    __syncthreads();
    if (trees)
        per_repair_paths(sum_tree, min_tree, tree_cap, T, blockDim.x, [&](int t) {
            return tree_cap + (pos0 + t) % capacity; });
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
        if (sum_tree) {
            sum_tree[tree_cap + slot] = pa;
            min_tree[tree_cap + slot] = pa;
        }
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
        if (sum_tree) {
            sum_tree[tree_cap + i] = 1.0;     // max_priority(1)^alpha
            min_tree[tree_cap + i] = 1.0;
        }
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
