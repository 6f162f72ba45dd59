// Commit of an overlapped collection window (Engine::collect_*): the rows the
// rollout stream staged are copied into the live replay ring on the learner
// stream, with their PER leaves.
//
// During a window the producer's RollCore points at a staging store of its
// own (five arrays, no trees, its own Counters), so the episode kernels never
// touch what the train step samples.  The commit runs on the learner stream
// after the window's last episode (an event orders the two), so it sees the
// live ring position and max_priority exactly as the steps issued before it
// left them: the result depends on program order only, never on how the two
// streams interleaved.
//
// Everything data-dependent is read on the device — the staged row count (the
// goal producer's is only known there), the live position, the priority — so
// the host does not synchronise before launching.  Plain vector loads and
// stores, no atomics: every destination slot has one writer because the
// staging store is never larger than the ring (collect_alloc refuses that).

namespace d4pg {

struct StageArgs {
    // staging store: rows [0, stage_cnt->size), dense from slot 0
    const float *ss, *sa, *sr, *ss2, *sd;
    Counters* stage_cnt;
    // live replay
    float *rs, *ra, *rr, *rs2, *rd;
    double *sum_tree, *min_tree;       // null: uniform replay
    long tree_cap, capacity;
    Counters* cnt;
    long long* ep_state;               // the producer's per-episode words
    int obs, act;
    float per_alpha;
};

// Dense rows [0, n) of width w to ring slots (pos0 + t) % capacity.  Rows of
// a width that is a multiple of four floats start 16-byte aligned in both
// arrays (the array bases are 256-byte aligned; the pointer test guards
// that), so they move as float4; any other width goes element by element.
__device__ inline void stage_copy_rows(float* __restrict__ dst,
                                       const float* __restrict__ src, long n,
                                       int w, long pos0, long capacity,
                                       long tid, long nthreads) {
    const bool vec = (w & 3) == 0 &&
        ((((uintptr_t)dst) | ((uintptr_t)src)) & 15) == 0;
    if (vec) {
        const int q = w >> 2;
        const float4* s4 = reinterpret_cast<const float4*>(src);
        float4* d4 = reinterpret_cast<float4*>(dst);
        for (long e = tid; e < n * q; e += nthreads) {
            long t = e / q, k = e % q;
            long slot = (pos0 + t) % capacity;
            d4[slot * q + k] = s4[e];
        }
    } else {
        for (long e = tid; e < n * w; e += nthreads) {
            long t = e / w, k = e % w;
            long slot = (pos0 + t) % capacity;
            dst[slot * w + k] = src[e];
        }
    }
}

// Grid-stride over the staged rows; the same plain (temporal) loads and
// stores as k_replay_copy, whose rows the next train steps sample.
__global__ void k_stage_commit(StageArgs a) {
    const long n = a.stage_cnt->size;
    const long pos0 = a.cnt->pos;
    const double pa = a.sum_tree
        ? per_leaf_value(a.cnt->max_priority, a.per_alpha) : 0.0;
    const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long nth = (long)gridDim.x * blockDim.x;
    stage_copy_rows(a.rs, a.ss, n, a.obs, pos0, a.capacity, tid, nth);
    stage_copy_rows(a.rs2, a.ss2, n, a.obs, pos0, a.capacity, tid, nth);
    stage_copy_rows(a.ra, a.sa, n, a.act, pos0, a.capacity, tid, nth);
    for (long t = tid; t < n; t += nth) {
        long slot = (pos0 + t) % a.capacity;
        a.rr[slot] = a.sr[t];
        a.rd[slot] = a.sd[t];
        if (a.sum_tree) {
            a.sum_tree[a.tree_cap + slot] = pa;
            a.min_tree[a.tree_cap + slot] = pa;
        }
    }
}

// One-thread epilogue, after the tree sweep: advance the live ring as
// roll_advance does for an episode's block, leave the block's live base and
// row count in the producer's words (rollout_last_rows) and rewind the
// staging counters for the next window.
__global__ void k_stage_commit_end(StageArgs a) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        const long long n = a.stage_cnt->size;
        const long long pos0 = a.cnt->pos;
        a.ep_state[1] = pos0;
        a.ep_state[2] = n;
        a.cnt->pos = (pos0 + n) % a.capacity;
        long long sz = a.cnt->size + n;
        a.cnt->size = sz > a.capacity ? a.capacity : sz;
        a.stage_cnt->size = 0;
        a.stage_cnt->pos = 0;
    }
}

}  // namespace d4pg
