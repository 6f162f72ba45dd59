// d4pg_amd fused D4PG learner engine — CDNA4 (gfx950 / MI355X) native.
//
// The entire D4PG train step of the reference (ddpg.py:200-255, SURVEY.md §2c
// — PER sample, target forwards, C51 projection, critic CE backward, Adam,
// policy backward, Adam, target soft-update, priority write-back) runs
// on-device.  All state is device-resident: parameters in a flat slab
// (weights stored TRANSPOSED, [in][out], for coalesced forward reads),
// Adam moments, target slabs, the SoA replay store and the prioritized
// sum/min segment trees in HBM, philox4x32 RNG, and
// the beta/Adam step counters.
//
// Three execution paths, selected by batch size (Engine::step_path):
// PERSISTENT (B <= 256, engine_persistent.hip), ROW-BLOCK (256 < B <= 512
// and every split step up to 512, engine_rowblock.hip) and WIDE (B > 512,
// engine_mfma.hip + engine_layer.hip; with EngineCfg.gemm_bf16 its GEMMs take
// the bf16-operand kernels of engine_mfma_bf16.hip).  Forward-only work (actor_forward,
// the device rollout) takes the MFMA forward kernel from 512 rows up and
// the VALU k_fwd below.
//
// This file is the single translation unit ext.hip includes.  The device
// code lives in the parts included here, in dependency order (fragments,
// not stand-alone sources), then engine_host.hip, the host support; the
// host side, the Engine class, follows them: device pool layout, the launch
// sequences of the three paths, hipGraph capture and replay, replay
// ingestion, parameter I/O, the rollout driver.  Every device allocation of
// the engine is a DevicePool, every captured graph a GraphSlot, every stream
// and event an owning handle, and every kernel launch goes through the
// checked launch() (all in engine_host.hip).

#include <string>

#include "engine_common.hip"
#include "engine_rowmath.hip"
#include "engine_replay.hip"
#include "engine_layer.hip"
#include "engine_rowblock.hip"
#include "engine_rollcore.hip"
#include "engine_rollout.hip"
#include "engine_goal.hip"
#include "engine_synth.hip"
#include "engine_eval.hip"
#include "engine_stage.hip"
#include "engine_mfma_tile.hip"
#include "engine_mfma.hip"
#include "engine_mfma_bf16.hip"
#include "engine_persistent.hip"
#include "engine_host.hip"

namespace d4pg {

// ===========================================================================
// Host engine
// ===========================================================================

static long next_pow2(long n) { long c = 1; while (c < n) c <<= 1; return c; }
static int ceil_div(long a, long b) { return (int)((a + b - 1) / b); }

struct Net {
    LayerDesc l[4];
    long n_params;
};

// Lay four layers out back to back in one slab: per layer, transposed
// weight [in1 + in2][out] then bias [out].  dims[i] = {in1, in2, out}.
static Net make_net(const int (&dims)[4][3]) {
    Net n{};
    long off = 0;
    for (int i = 0; i < 4; ++i) {
        int in = dims[i][0] + dims[i][1], out = dims[i][2];
        n.l[i] = LayerDesc{dims[i][0], dims[i][1], out, off,
                           off + (long)in * out};
        off += (long)in * out + out;
    }
    n.n_params = off;
    return n;
}

static Net make_actor_net(int O, int A, int H) {
    return make_net({{O, 0, H}, {H, 0, H}, {H, 0, H}, {H, 0, A}});
}

static Net make_critic_net(int O, int A, int H, int K) {
    return make_net({{O, 0, H}, {H, A, H}, {H, 0, H}, {H, 0, K}});
}

// Host forms of the env observations, for the state-injection test hooks of
// the rollouts and the evaluation.  Pendulum: [cos th, sin th, thdot].
static std::vector<float> pendulum_obs(const float* th, const float* thdot,
                                       long n) {
    std::vector<float> obs(3 * n);
    for (long i = 0; i < n; ++i) {
        obs[i * 3 + 0] = cosf(th[i]);
        obs[i * 3 + 1] = sinf(th[i]);
        obs[i * 3 + 2] = thdot[i];
    }
    return obs;
}

// GoalReach: [pos, goal], D of each.
static std::vector<float> goal_obs(const float* pos, const float* goal,
                                   long n, long D) {
    std::vector<float> obs(2 * n * D);
    for (long i = 0; i < n; ++i)
        for (long k = 0; k < D; ++k) {
            obs[i * 2 * D + k] = pos[i * D + k];
            obs[i * 2 * D + D + k] = goal[i * D + k];
        }
    return obs;
}

class Engine {
public:
    EngineCfg cfg;
    Net anet, cnet;
    Stream stream;
    GraphSlot train_graph_;             // graph_steps train steps
    int graph_steps = 0;

    // step geometry + every workspace pointer, as the kernels take them
    // (scalars filled by the constructor, pointers carved by layout())
    StepArgs ws{};
    float *ing_s, *ing_a, *ing_r, *ing_s2, *ing_d;  // ingestion staging
    float* dw_parts;                                // split-K dW partials
    int ing_cap;

    Engine(const EngineCfg& c) : cfg(c) {
        if (c.hidden + c.act > FWD_XMAX || c.obs > FWD_XMAX)
            throw std::runtime_error("layer fan-in exceeds FWD_XMAX LDS tile");
        if (c.atoms > 64)
            throw std::runtime_error("n_atoms > 64 (softmax is wave-wide)");
        if (c.dist != DIST_CATEGORICAL && c.dist != DIST_QUANTILE)
            throw std::runtime_error("unknown critic head (dist)");
        if (!(c.kappa > 0.f))               // zero, negative or NaN
            throw std::runtime_error(
                "kappa (the quantile head's Huber threshold) must be > 0");
        if (c.gemm_bf16 && c.batch <= 512)
            throw std::runtime_error(
                "gemm_precision='bf16' needs batch > 512: only the wide "
                "train step has bf16 GEMMs, the persistent and row-block "
                "paths (batch <= 512) are fp32 only");
        if (!(c.max_grad_norm >= 0.0))      // negative or NaN
            throw std::runtime_error(
                "max_grad_norm must be >= 0 (0 turns gradient clipping off)");
        anet = make_actor_net(c.obs, c.act, c.hidden);
        cnet = make_critic_net(c.obs, c.act, c.hidden, c.atoms);
        ws.B = c.batch; ws.O = c.obs; ws.A = c.act; ws.H = c.hidden;
        ws.K = c.atoms;
        ws.v_min = c.v_min; ws.v_max = c.v_max; ws.gamma_n = c.gamma_n;
        ws.per_eps = c.per_eps; ws.tau = c.tau;
        ws.lr_actor = c.lr_actor; ws.lr_critic = c.lr_critic;
        ws.per_alpha = c.per_alpha; ws.per_beta0 = c.per_beta0;
        ws.per_beta_iters = (float)c.per_beta_iters;
        ws.is_weighting = c.is_weighting;
        ws.prioritized = c.prioritized; ws.true_td = c.true_td;
        ws.seed = c.seed;
        ws.max_grad_norm = c.max_grad_norm;
        ws.dist = c.dist; ws.kappa = c.kappa;
        ws.tree_cap = has_trees() ? next_pow2(c.capacity) : 0;
        ws.n_actor = anet.n_params; ws.n_critic = cnet.n_params;
        for (int i = 0; i < 4; ++i) {
            ws.al[i] = anet.l[i];
            ws.cl[i] = cnet.l[i];
        }
        HIP_CHECK(hipStreamCreateWithFlags(stream.put(),
                                           hipStreamNonBlocking));
        // co-residency gate for the persistent path: all PNWG workgroups
        // must fit on the device at once or the software grid barrier
        // cannot make progress
        int dev = 0, per_cu = 0;
        HIP_CHECK(hipGetDevice(&dev));
        hipDeviceProp_t prop;
        HIP_CHECK(hipGetDeviceProperties(&prop, dev));
        HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(
            &per_cu, persistent_kernel(), 256, 0));
        persistent_fits_ = (long)per_cu * prop.multiProcessorCount >= PNWG;
        device_ = dev;
        alloc();
    }

    int device_ = 0;

    bool persistent_fits_ = false;

    // The one predicate every tree-touching launch is gated on.  Uniform
    // replay allocates no sum/min trees (tree_cap 0, null pointers): the
    // step samples by integer draw and skips the priority write-back, and
    // the write side copies rows only.
    bool has_trees() const { return cfg.prioritized != 0; }

    // Global-norm gradient clipping is on: the one predicate behind the
    // clip-on kernels and launches.  Off, every launch sequence is the
    // plain one.
    bool clip() const { return cfg.max_grad_norm > 0.0; }

    // The quantile critic head is on: the one predicate behind the QR
    // kernel instantiations and the identity heads.
    bool quantile() const { return cfg.dist == DIST_QUANTILE; }

    // activation of the three critic-family heads (critic, critic_target,
    // the policy chain's critic)
    int head_act() const { return quantile() ? ACT_NONE : ACT_SOFTMAX; }

    // the persistent kernel's instantiation for this engine
    using PersistentKernel = void (*)(StepArgs, int);
    PersistentKernel persistent_kernel() const {
        if (quantile())
            return clip() ? k_step_persistent<true, true>
                          : k_step_persistent<false, true>;
        return clip() ? k_step_persistent<true, false>
                      : k_step_persistent<false, false>;
    }

    // internal tree nodes from the leaves: one bandwidth-bound sweep per
    // level (bulk ingest, synth_fill, once per rollout episode)
    void launch_tree_rebuild(int wgs) {
        if (!has_trees()) return;
        launch_tree_rebuild(wgs, stream, ws.sum_tree, ws.min_tree,
                            ws.tree_cap);
    }

    // the same sweep on the caller's stream over the caller's trees; null
    // trees (uniform replay, or a rollout core pointed at the staging store
    // of an overlapped collection) make it a no-op
    void launch_tree_rebuild(int wgs, hipStream_t st, double* sum_tree,
                             double* min_tree, long tree_cap) {
        if (!sum_tree) return;
        for (long lo = tree_cap / 2; lo >= 1; lo >>= 1)
            launch(k_tree_build_level, wgs, 256, 0, st, sum_tree, min_tree,
                   lo, 2 * lo);
    }

    // the persistent grid barrier's timeout flag (gbar[176]); raised on
    // device when a p_bar spins out, fatal host-side — the engine state
    // must be considered corrupt after it
    void check_bar_error() {
        unsigned long long e = 0;
        HIP_CHECK(hipMemcpy(&e, ws.gbar + 176, 8, hipMemcpyDeviceToHost));
        if (e)
            throw std::runtime_error(
                "persistent grid barrier timed out (desynchronized "
                "workgroups; device state is corrupt) — occupancy check "
                "passed but the grid did not make progress");
    }

    // The one ordering rule of the engine's lifetime, spelled out here and
    // not left to member declaration order: drain the rollout stream FIRST
    // (an open window's episodes read and write the pools), then release
    // graphs and pools, then events and streams.
    ~Engine() {
        if (roll_stream_) (void)hipStreamSynchronize(roll_stream_);
        for (GraphSlot* g : {&train_graph_, &roll_graph_, &stage_graph_,
                             &eval_graph_})
            g->reset();
        for (DevicePool* p : {&pool_, &roll_pool_, &stage_pool_, &eval_pool_})
            p->reset();
        ev_snap_.reset();
        ev_done_.reset();
        roll_stream_.reset();
        stream.reset();
    }

    DevicePool pool_;

    // The main pool's carve sequence (DevicePool::build runs it twice).
    void layout(DevicePool& p) {
        const long B = cfg.batch, O = cfg.obs, A = cfg.act, H = cfg.hidden,
                   K = cfg.atoms;
        const long C = cfg.capacity;
        const long pa = anet.n_params, pc = cnet.n_params;
        ing_cap = 65536;
        p.take(ws.p_actor, pa); p.take(ws.p_actor_t, pa);
        p.take(ws.g_actor, pa);
        p.take(ws.p_critic, pc); p.take(ws.p_critic_t, pc);
        p.take(ws.g_critic, pc);
        p.take(ws.m_actor, pa); p.take(ws.v_actor, pa);
        p.take(ws.m_critic, pc); p.take(ws.v_critic, pc);
        p.take(ws.rs, C * O); p.take(ws.ra, C * A); p.take(ws.rr, C);
        p.take(ws.rs2, C * O); p.take(ws.rd, C);
        if (has_trees()) {
            p.take(ws.sum_tree, 2 * ws.tree_cap);
            p.take(ws.min_tree, 2 * ws.tree_cap);
        } else {
            ws.sum_tree = ws.min_tree = nullptr;
        }
        p.take(ws.cnt, 1);
        p.take(ws.bs, B * O); p.take(ws.bs_b, B * O); p.take(ws.ba, B * A);
        p.take(ws.br, B); p.take(ws.bs2, B * O);
        p.take(ws.bd, B); p.take(ws.bw, B); p.take(ws.pri, B);
        p.take(ws.bidx, B);
        p.take(ws.at_h1, B * H); p.take(ws.at_h2, B * H);
        p.take(ws.at_h3, B * H); p.take(ws.a2, B * A);
        p.take(ws.ct_h1, B * H); p.take(ws.ct_h2, B * H);
        p.take(ws.ct_h3, B * H);
        p.take(ws.p_t, B * K); p.take(ws.m_proj, B * K);
        p.take(ws.c_h1, B * H); p.take(ws.c_h2, B * H); p.take(ws.c_h3, B * H);
        p.take(ws.q, B * K); p.take(ws.dlog, B * K);
        p.take(ws.d3, B * H); p.take(ws.d2, B * H); p.take(ws.d1, B * H);
        p.take(ws.da, B * A);
        p.take(ws.pa_h1, B * H); p.take(ws.pa_h2, B * H);
        p.take(ws.pa_h3, B * H); p.take(ws.a_out, B * A);
        p.take(ws.pc_h1, B * H); p.take(ws.pc_h2, B * H);
        p.take(ws.pc_h3, B * H);
        p.take(ws.pq, B * K); p.take(ws.pd3, B * K);
        p.take(ws.pd2, B * H); p.take(ws.pdh1, B * H);
        p.take(ws.pda, B * A); p.take(ws.adz, B * A);
        p.take(ws.az1, B * H); p.take(ws.az2, B * H); p.take(ws.az3, B * H);
        // split-K disjoint partials: the wide step's dW (max over layers of
        // ksplit * (weights + bias)) and the MFMA heads' forward partials,
        // which actor_forward already needs at B = 512 where the step itself
        // is still row-block.  Segments past the last batch chunk are empty
        // when B is no power-of-two multiple of MT_K; k_mfma_dw zero-fills
        // them
        long dwp = 0;
        if (fwd_uses_mfma(cfg.batch)) {
            auto dw_need = [&](int in_n, int out) {
                long v = (long)dw_ksplit(in_n, out) * ((long)in_n * out + out);
                if (v > dwp) dwp = v;
            };
            auto need = [&](const LayerDesc& l) {
                // dW runs per input block (x1 / x2 separately)
                dw_need(l.in1, l.out);
                if (l.in2 > 0) dw_need(l.in2, l.out);
                if (l.out <= 64) {      // split-K head fwd partials
                    long v2 = (long)head_ksplit(cfg.batch, l.in1 + l.in2) *
                              B * l.out;
                    if (v2 > dwp) dwp = v2;
                }
            };
            for (int i = 0; i < 4; ++i) { need(anet.l[i]); need(cnet.l[i]); }
        }
        p.take(dw_parts, dwp);              // zero-length below 512 rows
        p.take(ws.gbar, 1536);
        p.take(ws.tstamp, 64);
        p.take(ing_s, ing_cap * O); p.take(ing_a, ing_cap * A);
        p.take(ing_r, ing_cap);
        p.take(ing_s2, ing_cap * O); p.take(ing_d, ing_cap);
        // gradient clipping: statistics block and per-chunk partials (last,
        // so every other buffer keeps its offset)
        p.take(ws.gstat, 1);
        p.take(ws.gn_part_a, gn_chunks(pa));
        p.take(ws.gn_part_c, gn_chunks(pc));
    }

    void alloc() {
        pool_.build([&](DevicePool& p) { layout(p); });
        Counters h{};
        h.max_priority = 1.0f;
        // schedule counters pre-advanced: k_per_update increments at step
        // END for the next step, so step 1 must already read Adam t=1.
        // beta_t starts at 0 (reference LinearSchedule returns value_at(0)
        // on its first stateful call, prioritized_replay_memory.py:25-29).
        h.beta_t = 0;
        h.adam_t_actor = h.adam_t_critic = h.rng_epoch = 1;
        HIP_CHECK(hipMemcpy(ws.cnt, &h, sizeof(Counters),
                            hipMemcpyHostToDevice));
        // min-tree neutral element is +inf (memset zero would make every
        // unoccupied leaf the minimum and zero out all IS weights)
        if (has_trees())
            launch(k_fill_f64, 1024, 256, 0, nullptr, ws.min_tree,
                   2 * ws.tree_cap, HUGE_VAL);
        HIP_CHECK(hipDeviceSynchronize());
    }

    // ---------------- forward launches ----------------
    // One layer over `rows` rows of x1 [. x2] with the weights in `slab`.
    FwdJob fwd_job(const float* x1, const float* x2, const float* slab,
                   const LayerDesc& l, float* y, int act_kind, int rows) {
        FwdJob j{};
        j.x1 = x1; j.x2 = x2;
        j.wt = slab + l.w_off; j.bias = slab + l.b_off;
        j.y = y;
        j.B = rows; j.in1 = l.in1; j.in2 = l.in2; j.out = l.out;
        j.act = act_kind;
        j.nwg_b = ceil_div(rows, TB);
        j.nwg_o = ceil_div(l.out, TO);
        return j;
    }
    FwdJob fwd_job(const float* x1, const float* x2, const float* slab,
                   const LayerDesc& l, float* y, int act_kind) {
        return fwd_job(x1, x2, slab, l, y, act_kind, cfg.batch);
    }

    // Forward-only work goes to the matrix cores from this many rows up
    // (the train step has its own split, see step_path()).
    static bool fwd_uses_mfma(int rows) { return rows >= 512; }

    // The split-K factors, for layout() (which sizes dw_parts by them) and
    // the launchers alike: double until the grid covers the chip, as long
    // as K still holds one f32 chunk (MT_K) per segment.  The bf16 kernels
    // take the same factors.
    // dW of one [in_n][out] block, K = the batch:
    int dw_ksplit(int in_n, int out) const {
        int nt = ceil_div(in_n, MT_M) * ceil_div(out, MT_N), ks = 1;
        while (nt * ks < 256 && ks * 2 * MT_K <= cfg.batch) ks *= 2;
        return ks;
    }
    // forward of a narrow head (out <= 64: one column tile), K = in_total:
    static int head_ksplit(int rows, int in_total) {
        int ntm = ceil_div(rows, MT_M), ks = 1;
        while (ntm * ks < 512 && ks * 2 * MT_K <= in_total) ks *= 2;
        return ks;
    }

    // (the launchers the rollout uses take their stream; the train step's
    // run on the engine's)
    void launch_fwd_valu(const FwdJob& j, hipStream_t st) {
        launch(k_fwd, j.nwg_b * j.nwg_o, 256, 0, st, j);
    }
    void launch_fwd_valu(const FwdJob& j) { launch_fwd_valu(j, stream); }

    // bf16 (here and below): the bf16-operand twin of the kernel, same grid
    // and arguments — only the wide train step in gemm_bf16 mode passes it.
    void launch_fwd_mfma(const FwdJob& j, bool bf16, hipStream_t st) {
        int ntm = ceil_div(j.B, MT_M), ntn = ceil_div(j.out, MT_N);
        launch(bf16 ? k_mfma_fwd_bf16 : k_mfma_fwd, ntm * ntn, 256, 0, st,
               j.x1, j.x2, j.wt, j.bias, j.y, j.B, j.in1, j.in2, j.out,
               j.act, 1, nullptr);
    }
    void launch_fwd_mfma(const FwdJob& j, bool bf16 = false) {
        launch_fwd_mfma(j, bf16, stream);
    }

    // Narrow head (out <= 64, incl. the softmax ones): split-K partials in
    // dw_parts + a wave-per-row finish — the M-tile-only grid of a plain
    // launch was chip-starved on both the VALU kernel (~60 us) and MFMA.
    void launch_fwd_mfma_head(const FwdJob& j, bool bf16 = false) {
        int ntm = ceil_div(j.B, MT_M);
        int ks = head_ksplit(j.B, j.in1 + j.in2);
        launch(bf16 ? k_mfma_fwd_bf16 : k_mfma_fwd, ntm * ks, 256, 0, stream,
               j.x1, j.x2, j.wt, j.bias, j.y, j.B, j.in1, j.in2, j.out,
               j.act, ks, dw_parts);
        if (ks > 1)
            launch(k_head_finish, 256, 256, 0, stream, dw_parts, j.bias, j.y,
                   j.B, j.out, ks, j.act);
    }

    // Layers of one phase over the engine's batch (independent of each
    // other; launched back to back).
    void launch_fwd(std::initializer_list<FwdJob> jobs, bool bf16 = false) {
        for (auto& j : jobs) {
            if (!fwd_uses_mfma(j.B)) {
                if (bf16)
                    throw std::runtime_error("no bf16 form of k_fwd");
                launch_fwd_valu(j);
            }
            else if (j.out <= 64) launch_fwd_mfma_head(j, bf16);
            else launch_fwd_mfma(j, bf16);
        }
    }

    // ---------------- backward launches (wide path) ----------------
    // One layer's backward on the matrix cores: dW (+db) into gslab when
    // want_dw, dx1 = (dz @ W[:in1]^T) * act'(h1) and the raw concat slice
    // dx2 = dz @ W[in1:]^T when non-null.
    void launch_bwd(const float* dz, const float* x1, const float* x2,
                    const float* slab, float* gslab, const LayerDesc& l,
                    float* dx1, float* dx2, const float* h1, int prev_act,
                    bool want_dw, bool bf16 = false) {
        int in_total = l.in1 + l.in2;
        auto k_dw = bf16 ? k_mfma_dw_bf16 : k_mfma_dw;
        auto k_dx = bf16 ? k_mfma_dx_bf16 : k_mfma_dx;
        if (want_dw) {
            // split K (= batch) until the grid covers the chip; segments
            // write disjoint partials, k_dw_reduce sums (atomic epilogue
            // retired — see k_dw_reduce comment).
            // Concat layers (in2 > 0) run as TWO GEMMs: the x1 block with
            // fully vectorized staging, and the tiny x2 (action) block
            // separately — one mixed GEMM left its edge tiles on the
            // guarded scalar path, and those straggler wgs held the whole
            // 200-us dispatch (profiles/wide_dissect2)
            auto dw_gemm = [&](const float* xop, int in_n, float* dwt,
                               float* db) {
                int ntm = ceil_div(in_n, MT_M);
                int ntn = ceil_div(l.out, MT_N);
                int ksplit = dw_ksplit(in_n, l.out);
                launch(k_dw, ntm * ntn * ksplit, 256, 0, stream, dz, xop,
                       nullptr, dwt, db, cfg.batch, in_n, 0, l.out, ksplit,
                       dw_parts);
                if (ksplit > 1)
                    launch(k_dw_reduce, 1024, 256, 0, stream, dw_parts, dwt,
                           db, (long)in_n * l.out, l.out, ksplit);
            };
            dw_gemm(x1, l.in1, gslab + l.w_off, gslab + l.b_off);
            if (l.in2 > 0)
                dw_gemm(x2, l.in2, gslab + l.w_off + (long)l.in1 * l.out,
                        nullptr);
        }
        if (dx1) {
            int ntm = ceil_div(cfg.batch, MT_M);
            int ntn = ceil_div(l.in1, MT_N);
            launch(k_dx, ntm * ntn, 256, 0, stream, dz, slab + l.w_off, h1,
                   dx1, cfg.batch, 0, l.in1, l.out, prev_act);
        }
        if (dx2) {
            if (l.in2 <= 8) {
                // action slice: wave-per-row VALU beats a 1-N-tile MFMA
                // grid by ~7x here (see k_dx_narrow comment); fp32 in
                // either precision mode
                launch(k_dx_narrow, 256, 256, 0, stream, dz, slab + l.w_off,
                       nullptr, dx2, cfg.batch, l.in1, in_total, l.out,
                       ACT_NONE);
            } else {
                int ntm = ceil_div(cfg.batch, MT_M);
                int ntn = ceil_div(l.in2, MT_N);
                launch(k_dx, ntm * ntn, 256, 0, stream, dz, slab + l.w_off,
                       nullptr, dx2, cfg.batch, l.in1, in_total, l.out,
                       ACT_NONE);
            }
        }
    }

    // ---------------- the train step (one launch sequence) ----------------
    // Phase mask for split stepping (learner data parallelism: the host
    // all-reduces g_critic / g_actor between the GRADS and APPLY phases,
    // SURVEY §2c collectives list).  PH_ALL == a whole train step.
    enum { PH_CRITIC_GRADS = 1, PH_CRITIC_APPLY = 2,
           PH_ACTOR_GRADS = 4, PH_ACTOR_APPLY = 8, PH_ALL = 15 };

    // Which of the three implementations runs a train step with this mask.
    enum StepPath { PATH_PERSISTENT, PATH_ROWBLOCK, PATH_WIDE };

    StepPath step_path(int mask = PH_ALL) const {
        // the persistent megakernel fuses all phases (so whole steps only)
        // and assumes: probe/row waves cover the batch (B <= PNWG*4),
        // fan-ins fit the LDS x-stage, softmax <= one wave, AND all PNWG
        // workgroups co-resident (the software grid barrier deadlocks
        // otherwise — persistent_fits_ is the ctor's occupancy check; on an
        // occupancy-limited device we fall back to the row-block + hipGraph
        // path instead of corrupting state)
        if (mask == PH_ALL && persistent_fits_ && cfg.batch <= 256 &&
            cfg.obs <= PXMAX && cfg.hidden + cfg.act <= PXMAX &&
            cfg.hidden <= PXMAX && cfg.atoms <= 64)
            return PATH_PERSISTENT;
        // row-block wastes weight bandwidth at large batch (every wave
        // re-streams every weight); the per-layer MFMA path wins there.
        return cfg.batch <= 512 ? PATH_ROWBLOCK : PATH_WIDE;
    }

    void enqueue_persistent(int nsteps) {
        launch(persistent_kernel(), PNWG, 256, 0, stream, ws, nsteps);
    }

    // All four layers' weight gradients of one net in a single k_bwd4
    // launch; in[i] = {dz, x1, x2} of layer i.
    struct DwIn { const float *dz, *x1, *x2; };
    void launch_dw4(const DwIn (&in)[4], const Net& net, float* gslab) {
        BwdJob j[4] = {};
        int wg = 0;
        for (int i = 0; i < 4; ++i) {
            const LayerDesc& l = net.l[i];
            j[i].dz = in[i].dz; j[i].x1 = in[i].x1; j[i].x2 = in[i].x2;
            j[i].dwt = gslab + l.w_off; j[i].dbias = gslab + l.b_off;
            j[i].B = cfg.batch;
            j[i].in1 = l.in1; j[i].in2 = l.in2; j[i].out = l.out;
            j[i].wg0_dw = wg;
            j[i].nwg_dw_i = ceil_div(l.in1 + l.in2, BWT);
            j[i].nwg_dw_o = ceil_div(l.out, BWT);
            wg += j[i].nwg_dw_i * j[i].nwg_dw_o;
        }
        launch(k_bwd4, wg, 256, 0, stream, j[0], j[1], j[2], j[3]);
    }

    void launch_per_sample() {
        launch(k_per_sample, ceil_div(cfg.batch, 4), 256, 0, stream, ws);
    }

    // Adam + target soft-update of one net, fused.  With clipping on, the
    // net's gradient norm and scale come first (inside PH_*_APPLY, so after
    // a data-parallel all-reduce, and inside captured graphs) and the
    // clip-on Adam kernel reads the scale from the statistics block.
    void launch_adam_lerp(bool is_actor) {
        float *p = ws.p_critic, *g = ws.g_critic, *m = ws.m_critic,
              *v = ws.v_critic, *tgt = ws.p_critic_t;
        double* part = ws.gn_part_c;
        long n = cnet.n_params;
        float lr = cfg.lr_critic;
        if (is_actor) {
            p = ws.p_actor; g = ws.g_actor; m = ws.m_actor; v = ws.v_actor;
            tgt = ws.p_actor_t; part = ws.gn_part_a;
            n = anet.n_params; lr = cfg.lr_actor;
        }
        const int ia = is_actor ? 1 : 0;
        if (!clip()) {
            launch(k_adam_lerp, 256, 256, 0, stream, p, g, m, v, tgt, n, lr,
                   0.9f, 0.999f, 1e-8f, cfg.tau, ws.cnt, ia);
            return;
        }
        launch(k_grad_norm, gn_chunks(n), 256, 0, stream, g, n, part);
        launch(k_grad_finish, 1, 64, 0, stream, part, n, cfg.max_grad_norm,
               ws.gstat, ia);
        launch(k_adam_lerp_clip, 256, 256, 0, stream, p, g, m, v, tgt, n, lr,
               0.9f, 0.999f, 1e-8f, cfg.tau, ws.cnt, ia, ws.gstat);
    }

    void enqueue_step_rowblock(int mask) {
        const int B = cfg.batch, H = cfg.hidden;
        int row_wgs = ceil_div(B, 4);
        long smem = rb_lds_bytes(H);
        if (mask & PH_CRITIC_GRADS) {
            launch_per_sample();
            launch(quantile() ? k_critic_rowblock<true>
                              : k_critic_rowblock<false>,
                   row_wgs, 256, smem, stream, ws);
            launch_dw4({{ws.d1, ws.bs, nullptr},
                        {ws.d2, ws.c_h1, ws.ba},
                        {ws.d3, ws.c_h2, nullptr},
                        {ws.dlog, ws.c_h3, nullptr}},
                       cnet, ws.g_critic);
        }
        if (mask & PH_CRITIC_APPLY) launch_adam_lerp(false);
        if (mask & PH_ACTOR_GRADS) {
            launch(quantile() ? k_policy_rowblock<true>
                              : k_policy_rowblock<false>,
                   row_wgs, 256, smem, stream, ws);
            launch_dw4({{ws.az1, ws.bs, nullptr},
                        {ws.az2, ws.pa_h1, nullptr},
                        {ws.az3, ws.pa_h2, nullptr},
                        {ws.adz, ws.pa_h3, nullptr}},
                       anet, ws.g_actor);
        }
        if (mask & PH_ACTOR_APPLY) {
            launch_adam_lerp(true);
            if (has_trees())
                launch(k_per_update, 1, 256, 0, stream, ws.sum_tree,
                       ws.min_tree, ws.tree_cap, ws.bidx, ws.pri, B,
                       cfg.per_alpha, ws.cnt);
            else            // the counters still tick once per step
                launch(k_tick_end, 1, 64, 0, stream, ws.cnt);
        }
    }

    // Per-layer sequence on the matrix cores (B > 512).
    void enqueue_step_wide(int mask) {
        const int B = cfg.batch, K = cfg.atoms;
        const int waves_per_wg = 4;
        // every GEMM below (launch_fwd / launch_bwd) takes bf16 operands in
        // gemm_bf16 mode; the VALU kernels between them stay fp32
        const bool bf = cfg.gemm_bf16 != 0;
        int row_wgs = ceil_div(B, waves_per_wg);

        if (mask & PH_CRITIC_GRADS) {
        launch_per_sample();
        // P2: a_t.L1(s2) | c_t.L1(s2) | c.L1(s)
        launch_fwd({fwd_job(ws.bs2, nullptr, ws.p_actor_t, anet.l[0], ws.at_h1,
                            ACT_RELU),
                    fwd_job(ws.bs2, nullptr, ws.p_critic_t, cnet.l[0], ws.ct_h1,
                            ACT_RELU),
                    fwd_job(ws.bs, nullptr, ws.p_critic, cnet.l[0], ws.c_h1,
                            ACT_RELU)}, bf);
        // P3: a_t.L2 | c.L2(cat c_h1, a)
        launch_fwd({fwd_job(ws.at_h1, nullptr, ws.p_actor_t, anet.l[1],
                            ws.at_h2, ACT_NONE),
                    fwd_job(ws.c_h1, ws.ba, ws.p_critic, cnet.l[1], ws.c_h2,
                            ACT_RELU)}, bf);
        // P4: a_t.L3 | c.L3
        launch_fwd({fwd_job(ws.at_h2, nullptr, ws.p_actor_t, anet.l[2],
                            ws.at_h3, ACT_RELU),
                    fwd_job(ws.c_h2, nullptr, ws.p_critic, cnet.l[2], ws.c_h3,
                            ACT_RELU)}, bf);
        // P5: a_t.L4 tanh | c.L4 softmax -> q
        launch_fwd({fwd_job(ws.at_h3, nullptr, ws.p_actor_t, anet.l[3], ws.a2,
                            ACT_TANH),
                    fwd_job(ws.c_h3, nullptr, ws.p_critic, cnet.l[3], ws.q,
                            head_act())}, bf);
        // P6-8: c_t.L2(cat ct_h1, a2), c_t.L3, c_t.L4 softmax -> p_t
        launch_fwd({fwd_job(ws.ct_h1, ws.a2, ws.p_critic_t, cnet.l[1], ws.ct_h2,
                            ACT_RELU)}, bf);
        launch_fwd({fwd_job(ws.ct_h2, nullptr, ws.p_critic_t, cnet.l[2],
                            ws.ct_h3, ACT_RELU)}, bf);
        launch_fwd({fwd_job(ws.ct_h3, nullptr, ws.p_critic_t, cnet.l[3], ws.p_t,
                            head_act())}, bf);
        // P9+P10 fused: projection + CE grad + priorities
        launch(quantile() ? k_project_ce<true> : k_project_ce<false>,
               min(row_wgs, 256), 256,
               waves_per_wg * 64 * sizeof(float), stream,
               ws.p_t, ws.br, ws.bd, ws.q, ws.bw, ws.m_proj, ws.dlog, ws.pri,
               ws.cnt, B, K, cfg.v_min, cfg.v_max, cfg.gamma_n, cfg.per_eps,
               cfg.is_weighting, cfg.true_td, cfg.kappa);
        // P11-14: critic backward L4..L1
        launch_bwd(ws.dlog, ws.c_h3, nullptr, ws.p_critic, ws.g_critic,
                   cnet.l[3], ws.d3, nullptr, ws.c_h3, ACT_RELU, true, bf);
        launch_bwd(ws.d3, ws.c_h2, nullptr, ws.p_critic, ws.g_critic, cnet.l[2],
                   ws.d2, nullptr, ws.c_h2, ACT_RELU, true, bf);
        launch_bwd(ws.d2, ws.c_h1, ws.ba, ws.p_critic, ws.g_critic, cnet.l[1],
                   ws.d1, nullptr, ws.c_h1, ACT_RELU, true, bf);
        launch_bwd(ws.d1, ws.bs, nullptr, ws.p_critic, ws.g_critic, cnet.l[0],
                   nullptr, nullptr, nullptr, ACT_NONE, true, bf);
        }
        // P15: Adam critic + target soft-update fused
        if (mask & PH_CRITIC_APPLY) launch_adam_lerp(false);
        if (mask & PH_ACTOR_GRADS) {
        // P16: actor.L1(s) | critic'.L1(s)
        launch_fwd({fwd_job(ws.bs, nullptr, ws.p_actor, anet.l[0], ws.pa_h1,
                            ACT_RELU),
                    fwd_job(ws.bs, nullptr, ws.p_critic, cnet.l[0], ws.pc_h1,
                            ACT_RELU)}, bf);
        // P17-19: actor L2, L3, L4
        launch_fwd({fwd_job(ws.pa_h1, nullptr, ws.p_actor, anet.l[1], ws.pa_h2,
                            ACT_NONE)}, bf);
        launch_fwd({fwd_job(ws.pa_h2, nullptr, ws.p_actor, anet.l[2], ws.pa_h3,
                            ACT_RELU)}, bf);
        launch_fwd({fwd_job(ws.pa_h3, nullptr, ws.p_actor, anet.l[3], ws.a_out,
                            ACT_TANH)}, bf);
        // P20-22: critic'(s, a_out)
        launch_fwd({fwd_job(ws.pc_h1, ws.a_out, ws.p_critic, cnet.l[1],
                            ws.pc_h2, ACT_RELU)}, bf);
        launch_fwd({fwd_job(ws.pc_h2, nullptr, ws.p_critic, cnet.l[2], ws.pc_h3,
                            ACT_RELU)}, bf);
        launch_fwd({fwd_job(ws.pc_h3, nullptr, ws.p_critic, cnet.l[3], ws.pq,
                            head_act())}, bf);
        // P23: policy head gradient
        launch(quantile() ? k_policy_grad<true> : k_policy_grad<false>,
               min(row_wgs, 256), 256, 0, stream, ws.pq,
               ws.pd3, ws.cnt, B, K, cfg.v_min, cfg.v_max);
        // P24-26: dX back through critic' (no dW), ending at da
        launch_bwd(ws.pd3, ws.pc_h3, nullptr, ws.p_critic, nullptr, cnet.l[3],
                   ws.pd2, nullptr, ws.pc_h3, ACT_RELU, false, bf);
        launch_bwd(ws.pd2, ws.pc_h2, nullptr, ws.p_critic, nullptr, cnet.l[2],
                   ws.pdh1, nullptr, ws.pc_h2, ACT_RELU, false, bf);
        launch_bwd(ws.pdh1, ws.pc_h1, ws.a_out, ws.p_critic, nullptr, cnet.l[1],
                   nullptr, ws.pda, ws.pc_h1, ACT_RELU, false, bf);
        // P27: tanh backward at actor output
        launch(k_tanh_bwd, ceil_div((long)B * cfg.act, 256), 256, 0, stream,
               ws.pda, ws.a_out, ws.adz, (long)B * cfg.act);
        // P28-31: actor backward L4..L1 (with dW).  az3/az2/az1 are the
        // deltas at the actor's layers 3/2/1, the names they carry on the
        // row-block path: every GEMM's dz outlives the phase (read_buffer)
        launch_bwd(ws.adz, ws.pa_h3, nullptr, ws.p_actor, ws.g_actor, anet.l[3],
                   ws.az3, nullptr, ws.pa_h3, ACT_RELU, true, bf);
        launch_bwd(ws.az3, ws.pa_h2, nullptr, ws.p_actor, ws.g_actor, anet.l[2],
                   ws.az2, nullptr, ws.pa_h2, ACT_NONE, true, bf);
        launch_bwd(ws.az2, ws.pa_h1, nullptr, ws.p_actor, ws.g_actor,
                   anet.l[1], ws.az1, nullptr, ws.pa_h1, ACT_RELU, true, bf);
        launch_bwd(ws.az1, ws.bs, nullptr, ws.p_actor, ws.g_actor, anet.l[0],
                   nullptr, nullptr, nullptr, ACT_NONE, true, bf);
        }
        if (!(mask & PH_ACTOR_APPLY)) return;
        // P32: Adam actor + target soft-update fused (critic target was
        // lerped in P15; ordering matches the row-block/persistent paths)
        launch_adam_lerp(true);
        // P34: PER priority write-back by the per-level grid-wide repair
        // (the one-wg level-synced k_per_update serializes at this size)
        if (has_trees()) {
        launch(k_per_leaves, ceil_div(B, 256), 256, 0, stream, ws.sum_tree,
               ws.min_tree, ws.tree_cap, ws.bidx, ws.pri, B, cfg.per_alpha,
               ws.cnt);
        long levels = 0;
        for (long c = ws.tree_cap; c > 1; c >>= 1) ++levels;
        // 4 heights per dispatch (k_per_level4): 20 launches -> 5
        for (long h0 = 0; h0 < levels; h0 += 4) {
            int nlv = (int)((levels - h0) < 4 ? (levels - h0) : 4);
            launch(k_per_level4, ceil_div((long)B * nlv, 256), 256, 0, stream,
                   ws.sum_tree, ws.min_tree, ws.tree_cap, ws.bidx, B, h0,
                   nlv);
        }
        }
        launch(k_tick_end, 1, 64, 0, stream, ws.cnt);
    }

    void enqueue_step(int mask = PH_ALL) {
        switch (step_path(mask)) {
        case PATH_PERSISTENT: enqueue_persistent(1); break;
        case PATH_ROWBLOCK:   enqueue_step_rowblock(mask); break;
        case PATH_WIDE:       enqueue_step_wide(mask); break;
        }
    }

    void step(int n) {
        bool persistent = step_path() == PATH_PERSISTENT && n > 0;
        if (persistent) {
            // whole multi-step run in ONE launch — zero host dispatch
            // between steps (numerically identical to n single launches)
            enqueue_persistent(n);
        } else {
            for (int i = 0; i < n; ++i) enqueue_step();
        }
        HIP_CHECK(hipStreamSynchronize(stream));
        if (persistent) check_bar_error();
    }

    // Partial step for learner data parallelism: run only the phases in
    // `mask` (PH_* above) and synchronize, so the host can all-reduce the
    // gradient slabs between GRADS and APPLY.  Never takes the persistent
    // megakernel (it fuses all phases); flagship shapes go through the
    // row-block path, wide shapes through the per-layer MFMA path.
    void step_part(int mask) {
        enqueue_step(mask);
        HIP_CHECK(hipStreamSynchronize(stream));
    }

    void invalidate_graph() {
        train_graph_.reset();
        graph_steps = 0;
    }

    void capture(int steps_per_graph) {
        invalidate_graph();
        train_graph_.ensure(stream, [&] {
            for (int i = 0; i < steps_per_graph; ++i) enqueue_step();
        });
        graph_steps = steps_per_graph;
    }

    void replay(int iters) {
        replay_async(iters);
        HIP_CHECK(hipStreamSynchronize(stream));
    }

    // non-blocking variants for overlap with host work
    void replay_async(int iters) {
        if (!train_graph_) throw std::runtime_error("no graph captured");
        for (int i = 0; i < iters; ++i) train_graph_.launch(stream);
    }
    void sync() { HIP_CHECK(hipStreamSynchronize(stream)); }

    // ------------- replay ops -------------
    void synth_fill(long n, uint64_t seed) {
        if (n > cfg.capacity) n = cfg.capacity;
        launch(k_synth_fill, 1024, 256, 0, stream, ws.rs, ws.ra, ws.rr,
               ws.rs2, ws.rd, ws.sum_tree, ws.min_tree, ws.tree_cap,
               cfg.capacity, n, cfg.obs, cfg.act, seed, cfg.per_alpha);
        launch_tree_rebuild(256);
        Counters h{};
        HIP_CHECK(hipMemcpyAsync(&h, ws.cnt, sizeof(h), hipMemcpyDeviceToHost,
                                 stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        h.size = n; h.pos = n % cfg.capacity;
        if (has_trees()) h.max_priority = 1.0f;
        HIP_CHECK(hipMemcpy(ws.cnt, &h, sizeof(h), hipMemcpyHostToDevice));
    }

    void ingest(const float* hs, const float* ha, const float* hr,
                const float* hs2, const float* hd, int T) {
        if (T > ing_cap) throw std::runtime_error("ingest batch too large");
        const int O = cfg.obs, A = cfg.act;
        // One call longer than the ring: rows t and t + capacity share a
        // slot, and the kernels' unordered threads would leave it holding
        // parts of both.  Only the last `capacity` rows survive anyway, so
        // drop the leading ones and start `skip` slots further on; pos
        // still ends at (pos + T) % capacity.
        const long skip = T > cfg.capacity ? T - cfg.capacity : 0;
        hs += skip * O; ha += skip * A; hr += skip;
        hs2 += skip * O; hd += skip;
        T -= (int)skip;
        HIP_CHECK(hipMemcpyAsync(ing_s, hs, (long)T * O * 4,
                                 hipMemcpyHostToDevice, stream));
        HIP_CHECK(hipMemcpyAsync(ing_a, ha, (long)T * A * 4,
                                 hipMemcpyHostToDevice, stream));
        HIP_CHECK(hipMemcpyAsync(ing_r, hr, (long)T * 4,
                                 hipMemcpyHostToDevice, stream));
        HIP_CHECK(hipMemcpyAsync(ing_s2, hs2, (long)T * O * 4,
                                 hipMemcpyHostToDevice, stream));
        HIP_CHECK(hipMemcpyAsync(ing_d, hd, (long)T * 4,
                                 hipMemcpyHostToDevice, stream));
        if (T <= 4096) {
            launch(k_replay_add, 1, 1024, 0, stream, ws.rs, ws.ra, ws.rr,
                   ws.rs2, ws.rd, ws.sum_tree, ws.min_tree, ws.tree_cap,
                   cfg.capacity, ing_s, ing_a, ing_r, ing_s2, ing_d, T, O, A,
                   cfg.per_alpha, skip, ws.cnt);
        } else {
            // bulk path: grid-wide copy + leaf init, then a full
            // bandwidth-bound tree rebuild (far cheaper than one wg
            // chasing 20-level paths for 100k rows)
            Counters h{};
            HIP_CHECK(hipMemcpyAsync(&h, ws.cnt, sizeof(h),
                                     hipMemcpyDeviceToHost, stream));
            HIP_CHECK(hipStreamSynchronize(stream));
            double pa = pow((double)h.max_priority, (double)cfg.per_alpha);
            launch(k_replay_copy, 1024, 256, 0, stream, ws.rs, ws.ra, ws.rr,
                   ws.rs2, ws.rd, ws.sum_tree, ws.min_tree, ws.tree_cap,
                   cfg.capacity, (h.pos + skip) % cfg.capacity, ing_s, ing_a,
                   ing_r, ing_s2, ing_d, T, O, A, pa);
            launch_tree_rebuild(1024);
            h.pos = (h.pos + skip + T) % cfg.capacity;
            h.size = h.size + T > cfg.capacity ? cfg.capacity : h.size + T;
            HIP_CHECK(hipMemcpyAsync(ws.cnt, &h, sizeof(h),
                                     hipMemcpyHostToDevice, stream));
        }
        HIP_CHECK(hipStreamSynchronize(stream));
    }

    // ------------- param I/O (host pointers, already transposed [in][out]) --
    void load_slab(float* dst, const float* src, long n) {
        HIP_CHECK(hipMemcpy(dst, src, n * 4, hipMemcpyHostToDevice));
    }
    void store_slab(float* dst, const float* src, long n) {
        HIP_CHECK(hipMemcpy(dst, src, n * 4, hipMemcpyDeviceToHost));
    }

    // norms and scales of the last step; zeros when clipping is off (the
    // block is cleared at allocation and never written)
    GradStats read_grad_stats() {
        GradStats h{};
        HIP_CHECK(hipMemcpy(&h, ws.gstat, sizeof(h), hipMemcpyDeviceToHost));
        return h;
    }

    Counters read_counters() {
        Counters h{};
        HIP_CHECK(hipMemcpy(&h, ws.cnt, sizeof(h), hipMemcpyDeviceToHost));
        // adam/rng counters are pre-advanced for the NEXT step (init 1 so
        // the first step sees t=1); report steps COMPLETED to the host.
        // beta_t starts at 0 (LinearSchedule value_at(0) on the first
        // sample) and ticks at step end, so its raw value IS steps done.
        h.adam_t_actor -= 1;
        h.adam_t_critic -= 1;
        h.rng_epoch -= 1;
        return h;
    }

    // ---------------- GPU-resident rollouts (device env + K11 + K15) -----
    // Three producers over one scaffold: Pendulum (engine_rollout.hip),
    // GoalReach with HER (engine_goal.hip) and the synthetic-spec envs of
    // any (obs, act) (engine_synth.hip).  They share the device core
    // (engine_rollcore.hip) and, below, the pool builder, fill_core, the
    // policy chain, the episode graph and its runner; one producer is
    // allocated at a time (roll_kind_).  State lives in a separate pool so
    // rollout capacity is independent of the learner batch; the actor
    // weights and the replay are SHARED with the learner (same p_actor
    // slab, same rs/../sum_tree), which is the point: the whole
    // actor->replay->learner loop stays in HBM.
    RollArgs roll_{};
    GoalRollArgs goal_{};
    SynRollArgs syn_{};
    // The synth env's mixing matrices live in the pool as one layer slab
    // ([W; U] is already [in][out], plus a zero bias), so the mixing GEMM
    // is a plain forward job with a concat input.
    float* syn_dyn_ = nullptr;
    LayerDesc syn_dyn_desc_{};
    DevicePool roll_pool_;
    float *r_h1 = nullptr, *r_h2 = nullptr, *r_h3 = nullptr;
    GraphSlot roll_graph_;              // one episode, reset included
    // which producer owns roll_pool_ and the episode graph
    enum { ROLL_NONE = 0, ROLL_PENDULUM = 1, ROLL_GOAL = 2, ROLL_SYNTH = 3 };
    int roll_kind_ = ROLL_NONE;

    // staged: the producer's args pointed at the staging store of an
    // overlapped collection (collect_alloc below)
    RollCore& roll_core(bool staged = false) {
        if (roll_kind_ == ROLL_GOAL) return staged ? goal_st_ : goal_;
        if (roll_kind_ == ROLL_SYNTH) return staged ? syn_st_ : syn_;
        return staged ? roll_st_ : roll_;
    }

    void roll_require(int kind, const char* otherwise) {
        if (roll_kind_ != kind) throw std::runtime_error(otherwise);
    }

    // Everything that reads or moves what an open collection window is
    // using (the producer's env state and words, its pools, the seeds, a
    // host copy of the whole replay) waits for the commit.
    void refuse_in_window(const char* what) {
        if (collect_pending_)
            throw std::runtime_error(
                std::string(what) + ": a collection window is open "
                "(collect_begin ran); call collect_commit first");
    }

    void rollout_free() {
        refuse_in_window("rollout_free / *_rollout_alloc");
        collect_free();                 // the staging store of this producer
        eval_free();                    // the evaluation models this producer
        roll_graph_.reset();
        roll_pool_.reset();
        roll_kind_ = ROLL_NONE;
    }

    // What every producer's args share: geometry, noise, seed and the
    // replay the rows go to, with the refusals that hold for all of them.
    void fill_core(RollCore& c, int M, int nsteps, int horizon, float gamma,
                   int noise_kind, float eps, float ou_theta, float ou_sigma,
                   float ou_mu, uint64_t seed) {
        if (M < 1)
            throw std::runtime_error("rollout: n_envs < 1");
        if (nsteps < 1 || horizon < nsteps)
            throw std::runtime_error("rollout horizon < n_steps");
        c.M = M; c.n = nsteps; c.horizon = horizon;
        c.gamma = gamma; c.eps = eps; c.ou_theta = ou_theta;
        c.ou_sigma = ou_sigma; c.ou_mu = ou_mu; c.ou_dt = 1e-2f;
        c.noise_kind = noise_kind; c.seed = seed;
        c.per_alpha = cfg.per_alpha;
        c.rs = ws.rs; c.ra = ws.ra; c.rr = ws.rr; c.rs2 = ws.rs2; c.rd = ws.rd;
        c.sum_tree = ws.sum_tree; c.min_tree = ws.min_tree;
        c.tree_cap = ws.tree_cap; c.capacity = cfg.capacity;
        c.cnt = ws.cnt;
    }

    // Frees the previous producer's pool and builds this one's.
    // carve(pool) takes each of the producer's own buffers; the core's
    // device words and the policy chain's hidden buffers are taken here.
    template <class Carve>
    void roll_pool_build(RollCore& c, Carve carve) {
        rollout_free();
        roll_pool_.build([&](DevicePool& p) {
            carve(p);
            p.take(c.ep_state, 8);
            const long MH = (long)c.M * cfg.hidden;
            p.take(r_h1, MH); p.take(r_h2, MH); p.take(r_h3, MH);
        });
    }

    // the policy forward obs [M][obs] -> act [M][act] between two ticks
    // on stream st with the weights of `slab`: the engine's stream and
    // ws.p_actor, or the rollout stream and the snapshot p_actor_roll
    void roll_fwd_chain(const float* obs, float* act, int M, hipStream_t st,
                        const float* slab) {
        roll_fwd_chain(obs, act, M, r_h1, r_h2, r_h3, st, slab);
    }

    // the same chain over hidden buffers [M][hidden] of the caller's
    void roll_fwd_chain(const float* obs, float* act, int M, float* h1,
                        float* h2, float* h3, hipStream_t st,
                        const float* slab) {
        // (the tanh head takes the plain MFMA launch here, not the split-K
        // head pair: dw_parts is sized for the learner batch, not for M)
        auto run = [&](const float* x, const LayerDesc& l, float* y,
                       int actk) {
            FwdJob j = fwd_job(x, nullptr, slab, l, y, actk, M);
            if (fwd_uses_mfma(M)) launch_fwd_mfma(j, false, st);
            else launch_fwd_valu(j, st);
        };
        run(obs, anet.l[0], h1, ACT_RELU);
        run(h1, anet.l[1], h2, ACT_NONE);       // fc2->fc2_2 no-act quirk
        run(h2, anet.l[2], h3, ACT_RELU);
        run(h3, anet.l[3], act, ACT_TANH);
    }

    // one whole episode of the allocated producer: on the engine's stream
    // into the live replay with the live actor, or (staged) on the rollout
    // stream into the staging store with the snapshot actor
    void enqueue_episode(bool reset, bool staged = false) {
        hipStream_t st = staged ? roll_stream_ : stream;
        const float* slab = staged ? p_actor_roll : ws.p_actor;
        RollCore& c = roll_core(staged);
        launch(k_roll_begin, 1, 64, 0, st, c);
        if (roll_kind_ == ROLL_GOAL)
            goal_enqueue_ticks(staged ? goal_st_ : goal_, reset, st, slab);
        else if (roll_kind_ == ROLL_SYNTH)
            synth_enqueue_ticks(staged ? syn_st_ : syn_, reset, st, slab);
        else
            pendulum_enqueue_ticks(staged ? roll_st_ : roll_, reset, st,
                                   slab);
        // internal tree nodes: one bandwidth-bound full sweep per episode
        // (vs horizon x per-path repair) — leaves were set at emit; a no-op
        // where the core has no trees (uniform replay, the staging store)
        launch_tree_rebuild(1024, st, c.sum_tree, c.min_tree, c.tree_cap);
    }

    // `episodes` whole episodes and the synchronise after them; with
    // use_graph and reset, one captured graph launched once per episode
    void run_episodes(int episodes, bool reset, bool use_graph) {
        if (use_graph && reset)
            roll_graph_.ensure(stream, [&] { enqueue_episode(true); });
        for (int e = 0; e < episodes; ++e) {
            if (use_graph && reset) roll_graph_.launch(stream);
            else enqueue_episode(reset);
        }
        HIP_CHECK(hipStreamSynchronize(stream));
    }

    // the per-episode device words of the last episode: [0] philox epoch,
    // [1] replay base, [2] rows emitted, and the goal rollout's [3]
    // successes, [4] env steps
    void rollout_words(long long (&w)[5]) {
        if (roll_kind_ == ROLL_NONE)
            throw std::runtime_error("no rollout allocated");
        HIP_CHECK(hipMemcpy(w, roll_core().ep_state, sizeof(w),
                            hipMemcpyDeviceToHost));
    }

    // ---------------- overlapped collection (engine_stage.hip) -----------
    // collect_begin .. collect_commit is one collection WINDOW: the
    // allocated producer's episodes run on a second stream while the
    // learner stream trains, and their rows reach the replay at the commit.
    //
    // Staging, not concurrent ring writes.  The window's episodes run the
    // unchanged episode kernels over a copy of the producer's args whose
    // replay fields point at a staging store (no trees, its own Counters,
    // capacity = max_episodes x rows-per-episode), and read the policy from
    // p_actor_roll, a snapshot of p_actor taken on the learner stream at
    // collect_begin.  Nothing the train step reads is written before the
    // commit, and nothing the episodes read is written by the train step.
    // Env state, n-step rings, the hidden buffers r_h1..3 and the philox
    // epoch (ep_state[0]) are the producer's own and are shared with the
    // sync path, which is refused while a window is open: episodes continue
    // one epoch sequence across sync and staged runs alike.
    //
    // Ordering is by two events and nothing else.  ev_snap_: recorded on
    // the learner stream after the snapshot copy, waited on by the rollout
    // stream before the first episode (it also orders the episodes after
    // any earlier sync rollout, which ran on the learner stream).  ev_done_:
    // recorded on the rollout stream after the last episode, waited on by
    // the learner stream before k_stage_commit.  The host synchronises only
    // at the end of collect_commit.
    //
    // Co-residency of the persistent step.  k_step_persistent's software
    // grid barrier needs its PNWG workgroups resident at once.  Rollout
    // kernels can hold CU slots while it starts, but they wait on nothing
    // the learner produces: their one dependency, ev_snap_, was recorded
    // BEFORE any train launch of the window.  So every rollout kernel runs
    // to completion and frees its slots whatever the learner does, and the
    // persistent grid always becomes resident.  The reverse wait (the
    // commit on ev_done_) sits on the learner stream behind the train
    // launches, not inside one.  Never make the rollout stream wait on
    // learner work issued after collect_begin: that would close a cycle
    // through the barrier.  The episode graph stays a single-stream graph
    // (no cross-stream fork or join is captured); the staged path has its
    // own, because its kernel arguments differ.
    RollArgs roll_st_{};
    GoalRollArgs goal_st_{};
    SynRollArgs syn_st_{};
    DevicePool stage_pool_;
    float *st_rs = nullptr, *st_ra = nullptr, *st_rr = nullptr,
          *st_rs2 = nullptr, *st_rd = nullptr;
    Counters* st_cnt = nullptr;
    float* p_actor_roll = nullptr;
    long stage_rows_ = 0;               // staging capacity in rows
    int collect_max_episodes_ = 0;
    int collect_episodes_ = 0;          // of the open window
    bool collect_pending_ = false;
    Stream roll_stream_;
    Event ev_snap_, ev_done_;
    GraphSlot stage_graph_;             // one staged episode

    void collect_free() {
        stage_graph_.reset();
        stage_pool_.reset();
        collect_max_episodes_ = 0;
        stage_rows_ = 0;
    }

    // rows one episode of the allocated producer writes at most
    long roll_episode_rows() {
        const RollCore& c = roll_core();
        if (roll_kind_ == ROLL_GOAL)
            return goal_episode_max(c.M, c.n, c.horizon);
        return (long)c.M * (c.horizon - c.n + 1);
    }

    void collect_alloc(int max_episodes) {
        refuse_in_window("collect_alloc");
        if (roll_kind_ == ROLL_NONE)
            throw std::runtime_error(
                "collect_alloc: no rollout allocated (call it after a "
                "*_rollout_alloc)");
        if (max_episodes < 1)
            throw std::runtime_error("collect_alloc: max_episodes < 1");
        const long rows = (long)max_episodes * roll_episode_rows();
        if (rows > cfg.capacity)
            throw std::runtime_error(
                "collect_alloc: max_episodes windows of " +
                std::to_string(rows) + " staged rows exceed the replay "
                "capacity " + std::to_string(cfg.capacity) + " (one commit "
                "would map two rows to one slot)");
        collect_free();
        if (!roll_stream_) {
            // below the learner stream where the runtime has priorities
            // (numerically larger = lower); the range is [0, 0] where not
            int least = 0, greatest = 0;
            HIP_CHECK(hipDeviceGetStreamPriorityRange(&least, &greatest));
            // (events first: the stream's presence is what marks all three)
            HIP_CHECK(hipEventCreateWithFlags(ev_snap_.put(),
                                              hipEventDisableTiming));
            HIP_CHECK(hipEventCreateWithFlags(ev_done_.put(),
                                              hipEventDisableTiming));
            HIP_CHECK(hipStreamCreateWithPriority(
                roll_stream_.put(), hipStreamNonBlocking, least));
        }
        const long O = cfg.obs, A = cfg.act;
        stage_pool_.build([&](DevicePool& p) {
            p.take(st_rs, rows * O); p.take(st_ra, rows * A);
            p.take(st_rr, rows);
            p.take(st_rs2, rows * O); p.take(st_rd, rows);
            p.take(st_cnt, 1);
            p.take(p_actor_roll, anet.n_params);
        });
        // the producer's args over the staging store: with null trees
        // roll_leaf_value / roll_write_leaf are no-ops, and k_roll_begin,
        // k_roll_end, k_goal_end and roll_advance work on the staging words
        roll_st_ = roll_; goal_st_ = goal_; syn_st_ = syn_;
        RollCore& c = roll_core(true);
        c.rs = st_rs; c.ra = st_ra; c.rr = st_rr; c.rs2 = st_rs2;
        c.rd = st_rd;
        c.sum_tree = c.min_tree = nullptr;
        c.tree_cap = 0;
        c.capacity = rows;
        c.cnt = st_cnt;
        stage_rows_ = rows;
        collect_max_episodes_ = max_episodes;
    }

    // snapshot the actor, enqueue `episodes` staged episodes on the rollout
    // stream and return without waiting for any of it
    void collect_begin(int episodes, bool use_graph) {
        if (!stage_pool_)
            throw std::runtime_error("collect_begin: collect_alloc first");
        if (collect_pending_)
            throw std::runtime_error(
                "collect_begin: a collection window is already open; call "
                "collect_commit first");
        if (episodes < 1 || episodes > collect_max_episodes_)
            throw std::runtime_error(
                "collect_begin: episodes not in [1, max_episodes = " +
                std::to_string(collect_max_episodes_) + "]");
        HIP_CHECK(hipMemcpyAsync(p_actor_roll, ws.p_actor,
                                 anet.n_params * 4, hipMemcpyDeviceToDevice,
                                 stream));
        HIP_CHECK(hipEventRecord(ev_snap_, stream));
        HIP_CHECK(hipStreamWaitEvent(roll_stream_, ev_snap_, 0));
        collect_pending_ = true;
        collect_episodes_ = episodes;
        if (roll_kind_ == ROLL_GOAL)    // the window's totals, as a run's
            HIP_CHECK(hipMemsetAsync(goal_st_.ep_state + 5, 0, 3 * 8,
                                     roll_stream_));
        if (use_graph)
            stage_graph_.ensure(roll_stream_,
                                [&] { enqueue_episode(true, true); });
        for (int e = 0; e < episodes; ++e) {
            if (use_graph) stage_graph_.launch(roll_stream_);
            else enqueue_episode(true, true);
        }
        HIP_CHECK(hipEventRecord(ev_done_, roll_stream_));
    }

    struct CollectTotals { long long env_steps, rows; };

    // move the window's rows into the live ring on the learner stream, and
    // wait for it
    CollectTotals collect_commit() {
        if (!collect_pending_)
            throw std::runtime_error(
                "collect_commit: no collection window is open");
        HIP_CHECK(hipStreamWaitEvent(stream, ev_done_, 0));
        const RollCore& c = roll_core();
        StageArgs a{};
        a.ss = st_rs; a.sa = st_ra; a.sr = st_rr; a.ss2 = st_rs2;
        a.sd = st_rd;
        a.stage_cnt = st_cnt;
        a.rs = ws.rs; a.ra = ws.ra; a.rr = ws.rr; a.rs2 = ws.rs2;
        a.rd = ws.rd;
        a.sum_tree = ws.sum_tree; a.min_tree = ws.min_tree;
        a.tree_cap = ws.tree_cap; a.capacity = cfg.capacity;
        a.cnt = ws.cnt;
        a.ep_state = c.ep_state;
        a.obs = cfg.obs; a.act = cfg.act;
        a.per_alpha = cfg.per_alpha;
        // sized for the staging store, not the (device-side) row count
        const long work = stage_rows_ * (cfg.obs > 4 ? cfg.obs / 4 : 1);
        int wgs = ceil_div(work, 256);
        launch(k_stage_commit, wgs > 1024 ? 1024 : wgs, 256, 0, stream, a);
        launch_tree_rebuild(1024);
        launch(k_stage_commit_end, 1, 64, 0, stream, a);
        // the window is closed once its work is enqueued, whatever the
        // synchronise reports
        collect_pending_ = false;
        HIP_CHECK(hipStreamSynchronize(stream));
        long long w[8];
        HIP_CHECK(hipMemcpy(w, c.ep_state, sizeof(w),
                            hipMemcpyDeviceToHost));
        CollectTotals t{};
        t.rows = w[2];
        t.env_steps = roll_kind_ == ROLL_GOAL
            ? w[7] : (long long)collect_episodes_ * c.horizon * c.M;
        return t;
    }

    // ---------------- Pendulum rollout (engine_rollout.hip) --------------
    void rollout_alloc(int M, int nsteps, int horizon, float gamma,
                       int noise_kind, float eps, float ou_theta,
                       float ou_sigma, float ou_mu, uint64_t seed) {
        if (cfg.obs != 3 || cfg.act != 1)
            throw std::runtime_error(
                "device rollout models Pendulum dynamics (obs=3, act=1)");
        RollArgs a{};
        fill_core(a, M, nsteps, horizon, gamma, noise_kind, eps, ou_theta,
                  ou_sigma, ou_mu, seed);
        a.O = 3; a.A = 1;
        const long nM = (long)nsteps * M;
        roll_pool_build(a, [&](DevicePool& p) {
            p.take(a.th, M); p.take(a.thdot, M); p.take(a.obs, 3L * M);
            p.take(a.act, M); p.take(a.ou_x, M);
            p.take(a.s_ring, 3 * nM); p.take(a.a_ring, nM);
            p.take(a.r_ring, nM);
        });
        roll_ = a;
        roll_kind_ = ROLL_PENDULUM;
    }

    void pendulum_enqueue_ticks(RollArgs& a, bool reset, hipStream_t st,
                                const float* slab) {
        int wgs = ceil_div(a.M, 256);
        if (reset) launch(k_roll_reset, wgs, 256, 0, st, a);
        int emit_k = 0;
        for (int t = 0; t < a.horizon; ++t) {
            roll_fwd_chain(a.obs, a.act, a.M, st, slab);
            int ek = (t >= a.n - 1) ? emit_k : -1;
            int done = (t == a.horizon - 1) ? 1 : 0;
            launch(k_roll_tick, wgs, 256, 0, st, a, t, t % a.n, ek, done);
            if (ek >= 0) ++emit_k;
        }
        launch(k_roll_end, 1, 64, 0, st, a, (long)emit_k * a.M);
    }

    void rollout_run(int episodes, bool reset, bool use_graph) {
        roll_require(ROLL_PENDULUM, "rollout_alloc first");
        refuse_in_window("rollout_run");
        run_episodes(episodes, reset, use_graph);
    }

    // test hook: inject exact env state (parity vs the numpy oracle)
    void rollout_set_state(const float* th, const float* td, int M) {
        refuse_in_window("rollout_set_state");
        if (roll_kind_ != ROLL_PENDULUM || M != roll_.M)
            throw std::runtime_error("rollout_set_state: bad M");
        HIP_CHECK(hipMemcpy(roll_.th, th, M * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(roll_.thdot, td, M * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(roll_.obs, pendulum_obs(th, td, M).data(),
                            3L * M * 4,
                            hipMemcpyHostToDevice));
        // as k_roll_reset leaves it: the OU process starts at mu
        std::vector<float> ou(M, roll_.ou_mu);
        HIP_CHECK(hipMemcpy(roll_.ou_x, ou.data(), M * 4,
                            hipMemcpyHostToDevice));
    }

    // ---------------- goal rollout + HER (engine_goal.hip) ---------------
    // rows one episode can emit at most: every env runs to the step limit
    // and every step gets a hindsight row
    static long goal_episode_max(long M, long nsteps, long horizon) {
        return M * (horizon - nsteps + 1) + M * horizon;
    }

    void goal_rollout_alloc(int M, int nsteps, int horizon, float gamma,
                            float speed, float tol, float her_ratio,
                            int noise_kind, float eps, float ou_theta,
                            float ou_sigma, float ou_mu, uint64_t seed) {
        if (cfg.act < 1 || cfg.obs != 2 * cfg.act)
            throw std::runtime_error(
                "device goal rollout needs obs = [pos, goal] (obs == 2*act)");
        GoalRollArgs a{};
        fill_core(a, M, nsteps, horizon, gamma, noise_kind, eps, ou_theta,
                  ou_sigma, ou_mu, seed);
        if (M > 65536)
            throw std::runtime_error("goal rollout: n_envs not in [1, 65536]");
        if (horizon >= (1 << 20))
            throw std::runtime_error("goal rollout horizon >= 2^20");
        if (cfg.capacity < goal_episode_max(M, nsteps, horizon))
            throw std::runtime_error(
                "goal rollout: replay capacity below one episode's maximum "
                "M*(horizon-n+1) + M*horizon rows (two rows of one episode "
                "would share a slot)");
        a.D = cfg.act;
        a.speed = speed; a.tol = tol; a.her_ratio = her_ratio;
        const long MD = (long)M * a.D;
        roll_pool_build(a, [&](DevicePool& p) {
            p.take(a.pos, MD); p.take(a.goal, MD); p.take(a.obs, 2 * MD);
            p.take(a.act, MD); p.take(a.ou_x, MD);
            p.take(a.alive, M); p.take(a.len, M); p.take(a.succ, M);
            p.take(a.ep_pos, (horizon + 1) * MD);
            p.take(a.ep_act, horizon * MD);
            p.take(a.count, M); p.take(a.offset, M);
        });
        goal_ = a;
        roll_kind_ = ROLL_GOAL;
    }

    void goal_enqueue_ticks(GoalRollArgs& a, bool reset, hipStream_t st,
                            const float* slab) {
        int wgs = ceil_div(a.M, 256);
        if (reset) launch(k_goal_reset, wgs, 256, 0, st, a);
        for (int t = 0; t < a.horizon; ++t) {
            roll_fwd_chain(a.obs, a.act, a.M, st, slab);
            launch(k_goal_tick, wgs, 256, 0, st, a, t);
        }
        launch(k_goal_count, wgs, 256, 0, st, a);
        launch(k_goal_scan, 1, GOAL_SCAN_THREADS, 0, st, a);
        // one wave per env, four to a workgroup
        int ewgs = ceil_div(a.M, 4);
        launch(k_goal_emit, ewgs > 2048 ? 2048 : ewgs, 256, 0, st, a);
        launch(k_goal_end, 1, 64, 0, st, a);
    }

    // Totals over the episodes of one goal_rollout_run call, read from the
    // device words: rows emitted, successes, env steps (sum of lengths).
    struct GoalTotals { long long rows, successes, env_steps; };

    GoalTotals goal_rollout_run(int episodes, bool reset, bool use_graph) {
        roll_require(ROLL_GOAL, "goal_rollout_alloc first");
        refuse_in_window("goal_rollout_run");
        HIP_CHECK(hipMemsetAsync(goal_.ep_state + 5, 0, 3 * 8, stream));
        run_episodes(episodes, reset, use_graph);
        long long w[3];
        HIP_CHECK(hipMemcpy(w, goal_.ep_state + 5, sizeof(w),
                            hipMemcpyDeviceToHost));
        return {w[0], w[1], w[2]};
    }

    // test hook: inject exact env state, leaving everything else as
    // k_goal_reset leaves it
    void goal_rollout_set_state(const float* pos, const float* goal, int M) {
        refuse_in_window("goal_rollout_set_state");
        if (roll_kind_ != ROLL_GOAL || M != goal_.M)
            throw std::runtime_error("goal_rollout_set_state: bad M");
        const int D = goal_.D;
        const long MD = (long)M * D;
        std::vector<float> obs = goal_obs(pos, goal, M, D),
                           ou(MD, goal_.ou_mu);
        std::vector<int> alive(M, 1);
        HIP_CHECK(hipMemcpy(goal_.pos, pos, MD * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(goal_.goal, goal, MD * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(goal_.obs, obs.data(), 2 * MD * 4,
                            hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(goal_.ep_pos, pos, MD * 4,
                            hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(goal_.ou_x, ou.data(), MD * 4,
                            hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(goal_.alive, alive.data(), M * 4,
                            hipMemcpyHostToDevice));
        std::vector<int> zero(M, 0);
        HIP_CHECK(hipMemcpy(goal_.len, zero.data(), M * 4,
                            hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(goal_.succ, zero.data(), M * 4,
                            hipMemcpyHostToDevice));
    }

    // ---------------- synthetic-spec rollout (engine_synth.hip) ----------
    void synth_rollout_alloc(int M, int nsteps, int horizon, float gamma,
                             float act_high, float proc_sigma,
                             int noise_kind, float eps, float ou_theta,
                             float ou_sigma, float ou_mu, uint64_t seed,
                             const float* W, const float* U) {
        const int O = cfg.obs, A = cfg.act;
        if (O + A > FWD_XMAX)
            throw std::runtime_error(
                "synth rollout: obs + act exceeds FWD_XMAX LDS tile");
        SynRollArgs a{};
        fill_core(a, M, nsteps, horizon, gamma, noise_kind, eps, ou_theta,
                  ou_sigma, ou_mu, seed);
        if (horizon >= (1 << 20) - 2)
            throw std::runtime_error("synth rollout horizon >= 2^20 - 2");
        if (cfg.capacity < (long)M * (horizon - nsteps + 1))
            throw std::runtime_error(
                "synth rollout: replay capacity below one episode's "
                "M*(horizon-n+1) rows (two rows of one episode would share "
                "a slot)");
        a.O = O; a.A = A;
        a.act_high = act_high; a.proc_sigma = proc_sigma;
        const long MO = (long)M * O, MA = (long)M * A;
        const long n_dyn = (long)(O + A) * O;
        float* dyn = nullptr;
        roll_pool_build(a, [&](DevicePool& p) {
            p.take(a.obs, MO); p.take(a.act, MA); p.take(a.act_env, MA);
            p.take(a.z, MO); p.take(a.ou_x, MA);
            p.take(a.s_ring, nsteps * MO); p.take(a.a_ring, nsteps * MA);
            p.take(a.r_ring, (long)nsteps * M);
            p.take(dyn, n_dyn + O);
        });
        // [W; U] then the zero bias the clear left
        HIP_CHECK(hipMemcpy(dyn, W, (long)O * O * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dyn + (long)O * O, U, (long)A * O * 4,
                            hipMemcpyHostToDevice));
        syn_dyn_ = dyn;
        syn_dyn_desc_ = LayerDesc{O, A, O, 0, n_dyn};
        syn_ = a;
        roll_kind_ = ROLL_SYNTH;
    }

    void synth_enqueue_ticks(SynRollArgs& a, bool reset, hipStream_t st,
                             const float* slab) {
        const long elems = (long)a.M * (a.O > a.A ? a.O : a.A);
        int wgs = ceil_div(elems, 256);
        if (wgs > 2048) wgs = 2048;
        // one wave per env, four to a workgroup
        int twgs = ceil_div(a.M, 4);
        if (twgs > 2048) twgs = 2048;
        if (reset) launch(k_syn_reset, wgs, 256, 0, st, a);
        FwdJob mix = fwd_job(a.obs, a.act_env, syn_dyn_, syn_dyn_desc_, a.z,
                             ACT_NONE, a.M);
        int emit_k = 0;
        for (int t = 0; t < a.horizon; ++t) {
            roll_fwd_chain(a.obs, a.act, a.M, st, slab);
            int slot = t % a.n;
            launch(k_syn_act, wgs, 256, 0, st, a, t, slot);
            if (fwd_uses_mfma(a.M)) launch_fwd_mfma(mix, false, st);
            else launch_fwd_valu(mix, st);
            int ek = (t >= a.n - 1) ? emit_k : -1;
            int done = (t == a.horizon - 1) ? 1 : 0;
            launch(k_syn_tick, twgs, 256, 0, st, a, t, slot, ek, done);
            if (ek >= 0) ++emit_k;
        }
        launch(k_roll_end, 1, 64, 0, st, a, (long)emit_k * a.M);
    }

    void synth_rollout_run(int episodes, bool reset, bool use_graph) {
        roll_require(ROLL_SYNTH, "synth_rollout_alloc first");
        refuse_in_window("synth_rollout_run");
        run_episodes(episodes, reset, use_graph);
    }

    // test hook: inject exact env state, leaving the OU process as
    // k_syn_reset leaves it
    void synth_rollout_set_state(const float* state, int M) {
        refuse_in_window("synth_rollout_set_state");
        if (roll_kind_ != ROLL_SYNTH || M != syn_.M)
            throw std::runtime_error("synth_rollout_set_state: bad M");
        HIP_CHECK(hipMemcpy(syn_.obs, state, (long)M * syn_.O * 4,
                            hipMemcpyHostToDevice));
        std::vector<float> ou((long)M * syn_.A, syn_.ou_mu);
        HIP_CHECK(hipMemcpy(syn_.ou_x, ou.data(), ou.size() * 4,
                            hipMemcpyHostToDevice));
    }

    // ---------------- greedy evaluation (engine_eval.hip) ----------------
    // E noise-free envs of the allocated producer's kind, with that
    // producer's env parameters, in a pool of their own (hidden buffers of
    // the policy chain included): nothing training reads is written.  One
    // episode is one single-stream hipGraph, captured on first use after
    // eval_alloc.  rollout_free(), and with it every *_rollout_alloc, drops
    // the evaluation: it models the producer that was allocated.
    EvalArgs eval_{};
    DevicePool eval_pool_;
    float *e_h1 = nullptr, *e_h2 = nullptr, *e_h3 = nullptr;
    GraphSlot eval_graph_;              // one episode, reset included
    // eval_set_state ran: the next episode starts from what it injected
    bool eval_injected_ = false;

    void eval_free() {
        eval_graph_.reset();
        eval_pool_.reset();
        eval_injected_ = false;
    }

    void eval_require() {
        if (!eval_pool_) throw std::runtime_error("eval_alloc first");
    }

    // horizon 0: the rollout's; has_seed false: the rollout seed ^ 0x5EEDE7A1
    void eval_alloc(int E, int horizon, bool has_seed, uint64_t seed,
                    bool fixed_starts) {
        if (roll_kind_ == ROLL_NONE)
            throw std::runtime_error(
                "eval_alloc: no rollout allocated (the evaluation models the "
                "allocated producer's env)");
        if (E < 1 || E > 65536)
            throw std::runtime_error("eval_alloc: n_envs not in [1, 65536]");
        const RollCore& c = roll_core();
        if (horizon == 0) horizon = c.horizon;
        if (horizon < 1 || horizon >= (1 << 20) - 2)
            throw std::runtime_error(
                "eval_alloc: horizon not in [1, 2^20 - 2)");
        eval_free();
        EvalArgs a{};
        a.E = E; a.horizon = horizon; a.fixed_starts = fixed_starts ? 1 : 0;
        a.seed = has_seed ? seed : (c.seed ^ 0x5EEDE7A1ull);
        const int O = cfg.obs, A = cfg.act;
        a.O = O; a.A = A; a.D = A;
        if (roll_kind_ == ROLL_GOAL) {
            a.speed = goal_.speed; a.tol = goal_.tol;
        } else if (roll_kind_ == ROLL_SYNTH) {
            a.act_high = syn_.act_high; a.proc_sigma = syn_.proc_sigma;
        }
        eval_pool_.build([&](DevicePool& p) {
            p.take(a.obs, (long)E * O); p.take(a.act, (long)E * A);
            p.take(a.ret, E); p.take(a.len, E); p.take(a.succ, E);
            p.take(a.words, EVAL_WORDS + 1);
            if (roll_kind_ == ROLL_PENDULUM) {
                p.take(a.th, E); p.take(a.thdot, E);
            } else if (roll_kind_ == ROLL_GOAL) {
                p.take(a.pos, (long)E * A); p.take(a.goal, (long)E * A);
                p.take(a.alive, E);
            } else {
                p.take(a.act_env, (long)E * A); p.take(a.z, (long)E * O);
            }
            const long EH = (long)E * cfg.hidden;
            p.take(e_h1, EH); p.take(e_h2, EH); p.take(e_h3, EH);
        });
        // every episode of a fixed-starts evaluation is episode 1; otherwise
        // k_eval_begin moves 0 on to 1 before the first one
        const long long epoch0 = fixed_starts ? 1 : 0;
        HIP_CHECK(hipMemcpy(a.words + EVAL_EPOCH, &epoch0, 8,
                            hipMemcpyHostToDevice));
        HIP_CHECK(hipDeviceSynchronize());
        eval_ = a;
    }

    void eval_enqueue_episode(bool reset) {
        EvalArgs& a = eval_;
        const int E = a.E;
        int wgs = ceil_div(E, 256);
        launch(k_eval_begin, 1, 64, 0, stream, a);
        auto chain = [&] {
            roll_fwd_chain(a.obs, a.act, E, e_h1, e_h2, e_h3, stream,
                           ws.p_actor);
        };
        if (roll_kind_ != ROLL_SYNTH) {
            const bool pend = roll_kind_ == ROLL_PENDULUM;
            if (reset)
                launch(pend ? k_eval_pend_reset : k_eval_goal_reset, wgs, 256,
                       0, stream, a);
            for (int t = 0; t < a.horizon; ++t) {
                chain();
                launch(pend ? k_eval_pend_tick : k_eval_goal_tick, wgs, 256,
                       0, stream, a, t);
            }
        } else {
            const long elems = (long)E * (a.O > a.A ? a.O : a.A);
            int ewgs = ceil_div(elems, 256);
            if (ewgs > 2048) ewgs = 2048;
            int twgs = ceil_div(E, 4);          // one wave per env
            if (twgs > 2048) twgs = 2048;
            if (reset) launch(k_eval_syn_reset, ewgs, 256, 0, stream, a);
            FwdJob mix = fwd_job(a.obs, a.act_env, syn_dyn_, syn_dyn_desc_,
                                 a.z, ACT_NONE, E);
            for (int t = 0; t < a.horizon; ++t) {
                chain();
                launch(k_eval_syn_act, ewgs, 256, 0, stream, a);
                if (fwd_uses_mfma(E)) launch_fwd_mfma(mix);
                else launch_fwd_valu(mix);
                launch(k_eval_syn_tick, twgs, 256, 0, stream, a, t);
            }
        }
        launch(k_eval_reduce, 1, EVAL_REDUCE_THREADS, 0, stream, a);
    }

    // `episodes` evaluation episodes; the result words sum over them
    void eval_run(int episodes, bool use_graph) {
        eval_require();
        if (episodes < 1)
            throw std::runtime_error(
                "eval_run: episodes < 1 (the result words would count no "
                "env episode)");
        HIP_CHECK(hipMemsetAsync(eval_.words, 0, EVAL_WORDS * 8, stream));
        for (int e = 0; e < episodes; ++e) {
            if (eval_injected_) {
                eval_injected_ = false;
                eval_enqueue_episode(false);
            } else if (use_graph) {
                eval_graph_.ensure(stream,
                                   [&] { eval_enqueue_episode(true); });
                eval_graph_.launch(stream);
            } else {
                eval_enqueue_episode(true);
            }
        }
        HIP_CHECK(hipStreamSynchronize(stream));
    }

    struct EvalResults {
        double sum, min, max;
        long long successes, env_steps, count, episode, episodes;
    };
    static_assert(sizeof(EvalResults) == EVAL_WORDS * 8, "result words");

    // the one 64-byte device-to-host copy of an evaluation
    EvalResults eval_results() {
        eval_require();
        EvalResults r{};
        HIP_CHECK(hipMemcpy(&r, eval_.words, sizeof(r),
                            hipMemcpyDeviceToHost));
        return r;
    }

    // per-env results of the last episode
    void eval_arrays(double* ret, int* len, int* succ) {
        eval_require();
        const long E = eval_.E;
        HIP_CHECK(hipMemcpy(ret, eval_.ret, E * 8, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(len, eval_.len, E * 4, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(succ, eval_.succ, E * 4, hipMemcpyDeviceToHost));
    }

    // test hook: inject exact env state for the next episode, leaving
    // everything else as the evaluation reset leaves it.  Pendulum: x = th,
    // y = thdot [E]; GoalReach: x = pos, y = goal [E][D]; synthetic: x =
    // state [E][obs], y unused.
    void eval_set_state(const float* x, const float* y, long nx, long ny) {
        eval_require();
        EvalArgs& a = eval_;
        const long E = a.E;
        auto up = [&](void* dst, const void* src, long bytes) {
            HIP_CHECK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
        };
        if (roll_kind_ == ROLL_PENDULUM) {
            if (nx != E || ny != E)
                throw std::runtime_error("eval_set_state: th/thdot not [E]");
            up(a.th, x, E * 4); up(a.thdot, y, E * 4);
            up(a.obs, pendulum_obs(x, y, E).data(), 3 * E * 4);
        } else if (roll_kind_ == ROLL_GOAL) {
            const long D = a.D, ED = E * D;
            if (nx != ED || ny != ED)
                throw std::runtime_error("eval_set_state: pos/goal not [E][D]");
            std::vector<int> alive(E, 1);
            up(a.pos, x, ED * 4); up(a.goal, y, ED * 4);
            up(a.obs, goal_obs(x, y, E, D).data(), 2 * ED * 4);
            up(a.alive, alive.data(), E * 4);
        } else {
            if (nx != E * a.O)
                throw std::runtime_error("eval_set_state: state not [E][obs]");
            up(a.obs, x, E * a.O * 4);
        }
        HIP_CHECK(hipMemset(a.ret, 0, E * 8));
        HIP_CHECK(hipMemset(a.len, 0, E * 4));
        HIP_CHECK(hipMemset(a.succ, 0, E * 4));
        // the clears went to the null stream; the episode kernels run on
        // the engine's non-blocking stream
        HIP_CHECK(hipDeviceSynchronize());
        eval_injected_ = true;
    }

    // actor forward for eval/smoke: x[B,obs] (device via staging) -> a[B,act]
    void actor_forward(const float* hx, float* hy, int n) {
        // reuse batch buffers (requires n <= batch)
        if (n > cfg.batch) throw std::runtime_error("actor_forward: n > batch");
        HIP_CHECK(hipMemcpyAsync(ws.bs, hx, (long)n * cfg.obs * 4,
                                 hipMemcpyHostToDevice, stream));
        launch_fwd({fwd_job(ws.bs, nullptr, ws.p_actor, anet.l[0], ws.pa_h1,
                            ACT_RELU)});
        launch_fwd({fwd_job(ws.pa_h1, nullptr, ws.p_actor, anet.l[1], ws.pa_h2,
                            ACT_NONE)});
        launch_fwd({fwd_job(ws.pa_h2, nullptr, ws.p_actor, anet.l[2], ws.pa_h3,
                            ACT_RELU)});
        launch_fwd({fwd_job(ws.pa_h3, nullptr, ws.p_actor, anet.l[3], ws.a_out,
                            ACT_TANH)});
        HIP_CHECK(hipMemcpyAsync(hy, ws.a_out, (long)n * cfg.act * 4,
                                 hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
    }
};

}  // namespace d4pg
