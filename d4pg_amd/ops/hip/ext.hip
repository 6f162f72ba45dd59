// Python bindings for the fused D4PG engine (torch extension).
// Single translation unit: includes engine.hip (kernels + host engine).

#include "engine.hip"

#include <torch/extension.h>

#include <memory>
#include <unordered_map>

namespace d4pg {

static std::unordered_map<int64_t, std::unique_ptr<Engine>> g_engines;
static int64_t g_next = 1;

static Engine& get(int64_t h) {
    auto it = g_engines.find(h);
    if (it == g_engines.end())
        throw std::runtime_error("invalid engine handle");
    return *it->second;
}

static int64_t create(int64_t obs, int64_t act, int64_t hidden, int64_t atoms,
                      int64_t batch, int64_t capacity, double v_min,
                      double v_max, double gamma_n, double tau,
                      double lr_actor, double lr_critic, double per_alpha,
                      double per_beta0, int64_t per_beta_iters,
                      double per_eps, int64_t seed, bool is_weighting,
                      bool prioritized, bool true_td, bool gemm_bf16,
                      double max_grad_norm, const std::string& dist,
                      double kappa) {
    EngineCfg c{};
    if (dist == "categorical") c.dist = DIST_CATEGORICAL;
    else if (dist == "quantile") c.dist = DIST_QUANTILE;
    else throw std::runtime_error(
        "unknown critic dist '" + dist +
        "' (expected 'categorical' or 'quantile')");
    c.kappa = (float)kappa;             // the engine refuses <= 0 and NaN
    c.obs = (int)obs; c.act = (int)act; c.hidden = (int)hidden;
    c.atoms = (int)atoms; c.batch = (int)batch;
    c.capacity = capacity;
    c.v_min = (float)v_min; c.v_max = (float)v_max;
    c.gamma_n = (float)gamma_n; c.tau = (float)tau;
    c.lr_actor = (float)lr_actor; c.lr_critic = (float)lr_critic;
    c.per_alpha = (float)per_alpha; c.per_beta0 = (float)per_beta0;
    c.per_beta_iters = per_beta_iters; c.per_eps = (float)per_eps;
    c.seed = (uint64_t)seed; c.is_weighting = is_weighting ? 1 : 0;
    c.prioritized = prioritized ? 1 : 0; c.true_td = true_td ? 1 : 0;
    c.gemm_bf16 = gemm_bf16 ? 1 : 0;
    c.max_grad_norm = max_grad_norm;    // the engine refuses < 0 and NaN
    int64_t h = g_next++;
    g_engines[h] = std::make_unique<Engine>(c);
    return h;
}

static void destroy(int64_t h) { g_engines.erase(h); }

static py::dict info(int64_t h) {
    Engine& e = get(h);
    py::dict d;
    d["n_params_actor"] = e.anet.n_params;
    d["n_params_critic"] = e.cnet.n_params;
    d["tree_cap"] = e.ws.tree_cap;      // 0 on uniform replay (no trees)
    d["prioritized"] = e.cfg.prioritized != 0;
    d["true_td"] = e.cfg.true_td != 0;
    d["gemm_precision"] = e.cfg.gemm_bf16 ? "bf16" : "fp32";
    d["max_grad_norm"] = e.cfg.max_grad_norm;
    d["dist"] = e.quantile() ? "quantile" : "categorical";
    d["kappa"] = (double)e.cfg.kappa;
    d["persistent"] = e.step_path() == Engine::PATH_PERSISTENT;
    d["seed"] = (int64_t)e.cfg.seed;
    // episodes one collection window can hold; 0 before collect_alloc
    d["collect_max_episodes"] = e.collect_max_episodes_;
    auto layers = [](const Net& net) {
        py::list out;
        for (const LayerDesc& l : net.l) {
            py::dict ld;
            ld["in1"] = l.in1; ld["in2"] = l.in2; ld["out"] = l.out;
            ld["w_off"] = l.w_off; ld["b_off"] = l.b_off;
            out.append(ld);
        }
        return out;
    };
    d["actor_layers"] = layers(e.anet);
    d["critic_layers"] = layers(e.cnet);
    return d;
}

static torch::Tensor f32_contig(torch::Tensor t) {
    return t.to(torch::kFloat32).contiguous().cpu();
}

// which: 0 actor, 1 actor_target, 2 critic, 3 critic_target
static float* slab_ptr(Engine& e, int64_t which, long& n) {
    switch (which) {
        case 0: n = e.anet.n_params; return e.ws.p_actor;
        case 1: n = e.anet.n_params; return e.ws.p_actor_t;
        case 2: n = e.cnet.n_params; return e.ws.p_critic;
        case 3: n = e.cnet.n_params; return e.ws.p_critic_t;
        case 4: n = e.anet.n_params; return e.ws.g_actor;
        case 5: n = e.cnet.n_params; return e.ws.g_critic;
        case 6: n = e.anet.n_params; return e.ws.m_actor;
        case 7: n = e.anet.n_params; return e.ws.v_actor;
        case 8: n = e.cnet.n_params; return e.ws.m_critic;
        case 9: n = e.cnet.n_params; return e.ws.v_critic;
    }
    throw std::runtime_error("bad slab id");
}

static void load_slab(int64_t h, int64_t which, torch::Tensor flat) {
    Engine& e = get(h);
    long n;
    float* dst = slab_ptr(e, which, n);
    auto t = f32_contig(flat);
    TORCH_CHECK(t.numel() == n, "slab size mismatch");
    e.load_slab(dst, t.data_ptr<float>(), n);
}

static torch::Tensor store_slab(int64_t h, int64_t which) {
    Engine& e = get(h);
    long n;
    float* src = slab_ptr(e, which, n);
    auto out = torch::empty({n}, torch::kFloat32);
    e.store_slab(out.data_ptr<float>(), src, n);
    return out;
}

static void synth_fill(int64_t h, int64_t n, int64_t seed) {
    get(h).synth_fill(n, (uint64_t)seed);
}

static void ingest(int64_t h, torch::Tensor s, torch::Tensor a,
                   torch::Tensor r, torch::Tensor s2, torch::Tensor d) {
    Engine& e = get(h);
    auto ts = f32_contig(s), ta = f32_contig(a), tr = f32_contig(r),
         ts2 = f32_contig(s2), td = f32_contig(d);
    int T = (int)tr.numel();
    TORCH_CHECK(ts.numel() == (long)T * e.cfg.obs, "bad states shape");
    TORCH_CHECK(ta.numel() == (long)T * e.cfg.act, "bad actions shape");
    e.ingest(ts.data_ptr<float>(), ta.data_ptr<float>(), tr.data_ptr<float>(),
             ts2.data_ptr<float>(), td.data_ptr<float>(), T);
}

// exact-resume support: restore the schedule counters to "steps_done
// completed" (adam/rng pre-advanced to steps_done+1, beta_t = steps_done —
// the same convention Engine::alloc establishes at step 0)
static void set_seed(int64_t h, int64_t seed) {
    Engine& e = get(h);
    e.refuse_in_window("set_seed");
    e.cfg.seed = e.ws.seed = (uint64_t)seed;
    // the seed is baked into captured kernel ARGUMENTS (k_per_sample /
    // k_step_persistent take it by value), so a previously captured
    // hipGraph would silently keep sampling with the stale seed —
    // invalidate it; FusedEngine.set_seed resets _captured so the next
    // train_steps() recaptures with the new seed.
    e.invalidate_graph();
}

static void set_schedule(int64_t h, int64_t steps_done, double max_priority) {
    Engine& e = get(h);
    Counters c{};
    HIP_CHECK(hipMemcpy(&c, e.ws.cnt, sizeof(c), hipMemcpyDeviceToHost));
    c.beta_t = steps_done;
    c.adam_t_actor = c.adam_t_critic = c.rng_epoch = steps_done + 1;
    c.max_priority = (float)max_priority;
    HIP_CHECK(hipMemcpy(e.ws.cnt, &c, sizeof(c), hipMemcpyHostToDevice));
}

// on-HBM replay snapshot: SoA rows [0, size) + both segment trees (zero-
// length on uniform replay)
static py::dict replay_state(int64_t h) {
    Engine& e = get(h);
    e.refuse_in_window("replay_state (state save)");
    Counters c{};
    HIP_CHECK(hipMemcpy(&c, e.ws.cnt, sizeof(c), hipMemcpyDeviceToHost));
    long n = c.size;
    const int O = e.cfg.obs, A = e.cfg.act;
    py::dict d;
    auto grab = [&](const float* src, long rows, long w) {
        auto t = torch::empty({rows, w}, torch::kFloat32);
        if (rows)
            HIP_CHECK(hipMemcpy(t.data_ptr<float>(), src, rows * w * 4,
                                hipMemcpyDeviceToHost));
        return t;
    };
    d["s"] = grab(e.ws.rs, n, O);
    d["a"] = grab(e.ws.ra, n, A);
    d["r"] = grab(e.ws.rr, n, 1);
    d["s2"] = grab(e.ws.rs2, n, O);
    d["d"] = grab(e.ws.rd, n, 1);
    auto st = torch::empty({2 * e.ws.tree_cap}, torch::kFloat64);
    auto mt = torch::empty({2 * e.ws.tree_cap}, torch::kFloat64);
    if (e.has_trees()) {
        HIP_CHECK(hipMemcpy(st.data_ptr<double>(), e.ws.sum_tree,
                            2 * e.ws.tree_cap * 8, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(mt.data_ptr<double>(), e.ws.min_tree,
                            2 * e.ws.tree_cap * 8, hipMemcpyDeviceToHost));
    }
    d["sum_tree"] = st;
    d["min_tree"] = mt;
    d["size"] = c.size;
    d["pos"] = c.pos;
    d["max_priority"] = c.max_priority;
    return d;
}

static void load_replay_state(int64_t h, torch::Tensor s, torch::Tensor a,
                              torch::Tensor r, torch::Tensor s2,
                              torch::Tensor dn, torch::Tensor sum_tree,
                              torch::Tensor min_tree, int64_t size,
                              int64_t pos, double max_priority) {
    Engine& e = get(h);
    e.refuse_in_window("load_replay_state (state load)");
    const int O = e.cfg.obs, A = e.cfg.act;
    long n = size;
    TORCH_CHECK(sum_tree.numel() == 2 * e.ws.tree_cap &&
                    min_tree.numel() == 2 * e.ws.tree_cap,
                "tree size mismatch: the snapshot holds ", sum_tree.numel(),
                " sum-tree nodes, this engine ", 2 * e.ws.tree_cap,
                e.has_trees() ? " (prioritized replay)"
                              : " (uniform replay keeps no trees)");
    auto put = [&](float* dst, torch::Tensor t, long rows, long w) {
        auto tt = f32_contig(t);
        TORCH_CHECK(tt.numel() == rows * w, "replay slab size mismatch");
        if (rows)
            HIP_CHECK(hipMemcpy(dst, tt.data_ptr<float>(), rows * w * 4,
                                hipMemcpyHostToDevice));
    };
    put(e.ws.rs, s, n, O);
    put(e.ws.ra, a, n, A);
    put(e.ws.rr, r, n, 1);
    put(e.ws.rs2, s2, n, O);
    put(e.ws.rd, dn, n, 1);
    auto st = sum_tree.to(torch::kFloat64).contiguous().cpu();
    auto mt = min_tree.to(torch::kFloat64).contiguous().cpu();
    if (e.has_trees()) {
        HIP_CHECK(hipMemcpy(e.ws.sum_tree, st.data_ptr<double>(),
                            2 * e.ws.tree_cap * 8, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(e.ws.min_tree, mt.data_ptr<double>(),
                            2 * e.ws.tree_cap * 8, hipMemcpyHostToDevice));
    }
    Counters c{};
    HIP_CHECK(hipMemcpy(&c, e.ws.cnt, sizeof(c), hipMemcpyDeviceToHost));
    c.size = size;
    c.pos = pos;
    c.max_priority = (float)max_priority;
    HIP_CHECK(hipMemcpy(e.ws.cnt, &c, sizeof(c), hipMemcpyHostToDevice));
}

static void step(int64_t h, int64_t n) { get(h).step((int)n); }
static void step_part(int64_t h, int64_t mask) {
    get(h).step_part((int)mask);
}

// Zero-copy torch view of an engine slab (params/grads/moments) ON DEVICE,
// so torch.distributed collectives (RCCL over xGMI) can all-reduce /
// broadcast engine state in place — the learner-DP and local-SGD paths.
// The tensor aliases engine memory: keep the engine alive while using it.
static torch::Tensor device_tensor(int64_t h, int64_t which) {
    Engine& e = get(h);
    long n;
    float* p = slab_ptr(e, which, n);
    return torch::from_blob(
        p, {n}, torch::TensorOptions().dtype(torch::kFloat32)
                    .device(torch::kCUDA, e.device_));
}
static void capture(int64_t h, int64_t n) { get(h).capture((int)n); }
static void replay(int64_t h, int64_t iters) { get(h).replay((int)iters); }
static void replay_async(int64_t h, int64_t iters) {
    get(h).replay_async((int)iters);
}
static void sync(int64_t h) { get(h).sync(); }

static py::dict counters(int64_t h) {
    Counters c = get(h).read_counters();
    py::dict d;
    d["beta_t"] = c.beta_t;
    d["adam_t_actor"] = c.adam_t_actor;
    d["adam_t_critic"] = c.adam_t_critic;
    // steps completed, like the adam counters: the NEXT step draws its
    // probes with philox epoch rng_epoch + 1
    d["rng_epoch"] = c.rng_epoch;
    d["size"] = c.size;
    d["pos"] = c.pos;
    d["max_priority"] = c.max_priority;
    d["loss_critic"] = c.loss_critic;
    d["loss_actor"] = c.loss_actor;
    return d;
}

// gradient-clip statistics of the last step (zeros with clipping off): one
// small device-to-host copy, no launch
static py::dict grad_stats(int64_t h) {
    GradStats g = get(h).read_grad_stats();
    py::dict d;
    d["norm_actor"] = g.norm_actor;
    d["norm_critic"] = g.norm_critic;
    d["scale_actor"] = g.scale_actor;
    d["scale_critic"] = g.scale_critic;
    return d;
}

// ---- GPU-resident rollout (device Pendulum + K11 noise + K15 fold) ----
static void rollout_alloc(int64_t h, int64_t M, int64_t n_steps,
                          int64_t horizon, double gamma, int64_t noise_kind,
                          double eps, double ou_theta, double ou_sigma,
                          double ou_mu, int64_t seed) {
    get(h).rollout_alloc((int)M, (int)n_steps, (int)horizon, (float)gamma,
                         (int)noise_kind, (float)eps, (float)ou_theta,
                         (float)ou_sigma, (float)ou_mu, (uint64_t)seed);
}

static void rollout_run(int64_t h, int64_t episodes, bool reset,
                        bool use_graph) {
    get(h).rollout_run((int)episodes, reset, use_graph);
}

static void rollout_set_state(int64_t h, torch::Tensor th,
                              torch::Tensor thdot) {
    Engine& e = get(h);
    auto t1 = f32_contig(th), t2 = f32_contig(thdot);
    TORCH_CHECK(t1.numel() == t2.numel(), "th/thdot size mismatch");
    e.rollout_set_state(t1.data_ptr<float>(), t2.data_ptr<float>(),
                        (int)t1.numel());
}

// what the info dicts of the two static-count rollouts share
static py::dict static_rollout_info(const RollCore& c) {
    py::dict d;
    d["M"] = c.M;
    d["n"] = c.n;
    d["horizon"] = c.horizon;
    d["emits_per_episode"] = (long)(c.horizon - c.n + 1) * c.M;
    d["env_steps_per_episode"] = (long)c.horizon * c.M;
    return d;
}

static py::dict rollout_info(int64_t h) {
    return static_rollout_info(get(h).roll_);
}

// ---- GPU-resident goal rollout + HER relabel (engine_goal.hip) ----
static void goal_rollout_alloc(int64_t h, int64_t M, int64_t n_steps,
                               int64_t horizon, double gamma, double speed,
                               double tol, double her_ratio,
                               int64_t noise_kind, double eps,
                               double ou_theta, double ou_sigma, double ou_mu,
                               int64_t seed) {
    get(h).goal_rollout_alloc((int)M, (int)n_steps, (int)horizon,
                              (float)gamma, (float)speed, (float)tol,
                              (float)her_ratio, (int)noise_kind, (float)eps,
                              (float)ou_theta, (float)ou_sigma, (float)ou_mu,
                              (uint64_t)seed);
}

// (env_steps, rows_emitted, successes) over the episodes of this call
static py::tuple goal_rollout_run(int64_t h, int64_t episodes, bool reset,
                                  bool use_graph) {
    Engine::GoalTotals t = get(h).goal_rollout_run((int)episodes, reset,
                                                   use_graph);
    return py::make_tuple((int64_t)t.env_steps, (int64_t)t.rows,
                          (int64_t)t.successes);
}

static void goal_rollout_set_state(int64_t h, torch::Tensor pos,
                                   torch::Tensor goal) {
    Engine& e = get(h);
    auto t1 = f32_contig(pos), t2 = f32_contig(goal);
    TORCH_CHECK(t1.numel() == t2.numel(), "pos/goal size mismatch");
    TORCH_CHECK(t1.numel() % e.cfg.act == 0, "pos is not [M, act]");
    e.goal_rollout_set_state(t1.data_ptr<float>(), t2.data_ptr<float>(),
                             (int)(t1.numel() / e.cfg.act));
}

static py::dict goal_rollout_info(int64_t h) {
    Engine& e = get(h);
    e.roll_require(Engine::ROLL_GOAL, "goal_rollout_alloc first");
    long long w[5];
    e.rollout_words(w);
    py::dict d;
    d["M"] = e.goal_.M;
    d["D"] = e.goal_.D;
    d["n"] = e.goal_.n;
    d["horizon"] = e.goal_.horizon;
    d["episode_max_rows"] = Engine::goal_episode_max(e.goal_.M, e.goal_.n,
                                                     e.goal_.horizon);
    d["episode"] = (int64_t)w[0];
    d["base"] = (int64_t)w[1];
    d["rows"] = (int64_t)w[2];
    d["successes"] = (int64_t)w[3];
    d["env_steps"] = (int64_t)w[4];
    return d;
}

// test hook: the last episode as recorded on the device
static py::dict goal_rollout_episode(int64_t h) {
    Engine& e = get(h);
    e.roll_require(Engine::ROLL_GOAL, "goal_rollout_alloc first");
    const GoalRollArgs& a = e.goal_;
    const long M = a.M, D = a.D, HOR = a.horizon;
    auto f32 = [&](const float* src, std::vector<int64_t> shape) {
        auto t = torch::empty(shape, torch::kFloat32);
        HIP_CHECK(hipMemcpy(t.data_ptr<float>(), src, t.numel() * 4,
                            hipMemcpyDeviceToHost));
        return t;
    };
    auto i32 = [&](const int* src) {
        auto t = torch::empty({M}, torch::kInt32);
        HIP_CHECK(hipMemcpy(t.data_ptr<int>(), src, M * 4,
                            hipMemcpyDeviceToHost));
        return t;
    };
    py::dict d;
    d["ep_pos"] = f32(a.ep_pos, {HOR + 1, M, D});
    d["ep_act"] = f32(a.ep_act, {HOR, M, D});
    d["goal"] = f32(a.goal, {M, D});
    d["len"] = i32(a.len);
    d["succ"] = i32(a.succ);
    return d;
}

// ---- GPU-resident synthetic-spec rollout (engine_synth.hip) ----
static void synth_rollout_alloc(int64_t h, int64_t M, int64_t n_steps,
                                int64_t horizon, double gamma,
                                double act_high, double proc_sigma,
                                int64_t noise_kind, double eps,
                                double ou_theta, double ou_sigma,
                                double ou_mu, int64_t seed, torch::Tensor W,
                                torch::Tensor U) {
    Engine& e = get(h);
    auto tw = f32_contig(W), tu = f32_contig(U);
    const int64_t O = e.cfg.obs, A = e.cfg.act;
    if (tw.dim() != 2 || tw.size(0) != O || tw.size(1) != O)
        throw std::runtime_error("synth rollout: W is not [obs][obs]");
    if (tu.dim() != 2 || tu.size(0) != A || tu.size(1) != O)
        throw std::runtime_error("synth rollout: U is not [act][obs]");
    e.synth_rollout_alloc((int)M, (int)n_steps, (int)horizon, (float)gamma,
                          (float)act_high, (float)proc_sigma,
                          (int)noise_kind, (float)eps, (float)ou_theta,
                          (float)ou_sigma, (float)ou_mu, (uint64_t)seed,
                          tw.data_ptr<float>(), tu.data_ptr<float>());
}

static void synth_rollout_run(int64_t h, int64_t episodes, bool reset,
                              bool use_graph) {
    get(h).synth_rollout_run((int)episodes, reset, use_graph);
}

static void synth_rollout_set_state(int64_t h, torch::Tensor state) {
    Engine& e = get(h);
    auto t = f32_contig(state);
    TORCH_CHECK(t.numel() % e.cfg.obs == 0, "state is not [M, obs]");
    e.synth_rollout_set_state(t.data_ptr<float>(),
                              (int)(t.numel() / e.cfg.obs));
}

static py::dict synth_rollout_info(int64_t h) {
    Engine& e = get(h);
    e.roll_require(Engine::ROLL_SYNTH, "synth_rollout_alloc first");
    long long w[5];
    e.rollout_words(w);
    py::dict d = static_rollout_info(e.syn_);
    d["O"] = e.syn_.O;
    d["A"] = e.syn_.A;
    d["episode"] = (int64_t)w[0];
    d["base"] = (int64_t)w[1];
    return d;
}

// ---- overlapped collection (engine_stage.hip) ----
static void collect_alloc(int64_t h, int64_t max_episodes) {
    if (max_episodes < 1 || max_episodes > (1 << 30))
        throw std::runtime_error("collect_alloc: max_episodes < 1");
    get(h).collect_alloc((int)max_episodes);
}

static void collect_begin(int64_t h, int64_t episodes, bool use_graph) {
    // clamped before the narrowing cast; the engine refuses both ends
    episodes = std::min<int64_t>(std::max<int64_t>(episodes, 0), 1 << 30);
    get(h).collect_begin((int)episodes, use_graph);
}

// (env_steps, rows) of the committed window
static py::tuple collect_commit(int64_t h) {
    Engine::CollectTotals t = get(h).collect_commit();
    return py::make_tuple((int64_t)t.env_steps, (int64_t)t.rows);
}

static bool collect_pending(int64_t h) { return get(h).collect_pending_; }

// ---- device greedy evaluation (engine_eval.hip) ----
static void eval_alloc(int64_t h, int64_t E, int64_t horizon, bool has_seed,
                       int64_t seed, bool fixed_starts) {
    // range checks before the narrowing casts
    if (E < 1 || E > 65536)
        throw std::runtime_error("eval_alloc: n_envs not in [1, 65536]");
    if (horizon < 0 || horizon >= (1 << 20) - 2)
        throw std::runtime_error("eval_alloc: horizon not in [1, 2^20 - 2)");
    get(h).eval_alloc((int)E, (int)horizon, has_seed, (uint64_t)seed,
                      fixed_starts);
}

static void eval_run(int64_t h, int64_t episodes, bool use_graph) {
    get(h).eval_run((int)episodes, use_graph);
}

static py::dict eval_results(int64_t h) {
    Engine::EvalResults r = get(h).eval_results();
    py::dict d;
    d["sum"] = r.sum;
    d["min"] = r.min;
    d["max"] = r.max;
    d["successes"] = (int64_t)r.successes;
    d["env_steps"] = (int64_t)r.env_steps;
    d["count"] = (int64_t)r.count;
    d["episode"] = (int64_t)r.episode;
    d["episodes"] = (int64_t)r.episodes;
    return d;
}

// per-env (ret float64, len int32, succ int32) of the last episode
static py::tuple eval_arrays(int64_t h) {
    Engine& e = get(h);
    e.eval_require();
    const int64_t E = e.eval_.E;
    auto ret = torch::empty({E}, torch::kFloat64);
    auto len = torch::empty({E}, torch::kInt32);
    auto succ = torch::empty({E}, torch::kInt32);
    e.eval_arrays(ret.data_ptr<double>(), len.data_ptr<int>(),
                  succ.data_ptr<int>());
    return py::make_tuple(ret, len, succ);
}

static void eval_set_state(int64_t h, torch::Tensor x, torch::Tensor y) {
    auto t1 = f32_contig(x), t2 = f32_contig(y);
    get(h).eval_set_state(t1.data_ptr<float>(), t2.data_ptr<float>(),
                          t1.numel(), t2.numel());
}

// test hook: what eval_alloc settled on
static py::dict eval_info(int64_t h) {
    Engine& e = get(h);
    e.eval_require();
    py::dict d;
    d["E"] = e.eval_.E;
    d["horizon"] = e.eval_.horizon;
    d["seed"] = e.eval_.seed;
    d["fixed_starts"] = (bool)e.eval_.fixed_starts;
    return d;
}

// Host copy of `count` replay rows starting at ring slot `base` (wrapping),
// in ring order.
static py::tuple replay_slice(int64_t h, int64_t base, int64_t count) {
    Engine& e = get(h);
    const long C = e.cfg.capacity;
    TORCH_CHECK(base >= 0 && base < C && count >= 0 && count <= C,
                "replay_slice out of range");
    const int O = e.cfg.obs, A = e.cfg.act;
    const long first = std::min<long>(count, C - base);
    auto grab = [&](const float* src, long w) {
        auto t = torch::empty({count, w}, torch::kFloat32);
        if (first)
            HIP_CHECK(hipMemcpy(t.data_ptr<float>(), src + base * w,
                                first * w * 4, hipMemcpyDeviceToHost));
        if (count > first)
            HIP_CHECK(hipMemcpy(t.data_ptr<float>() + first * w, src,
                                (count - first) * w * 4,
                                hipMemcpyDeviceToHost));
        return t;
    };
    return py::make_tuple(grab(e.ws.rs, O), grab(e.ws.ra, A),
                          grab(e.ws.rr, 1), grab(e.ws.rs2, O),
                          grab(e.ws.rd, 1));
}

// (base, rows) of the last rollout episode, of any kind
static py::tuple rollout_last(int64_t h) {
    long long w[5];
    get(h).rollout_words(w);
    return py::make_tuple((int64_t)w[1], (int64_t)w[2]);
}

// test hook (the evaluation's no-side-effects check snapshots them): all
// eight per-episode device words of the allocated rollout
static torch::Tensor rollout_words(int64_t h) {
    Engine& e = get(h);
    if (e.roll_kind_ == Engine::ROLL_NONE)
        throw std::runtime_error("no rollout allocated");
    auto t = torch::empty({8}, torch::kInt64);
    HIP_CHECK(hipMemcpy(t.data_ptr<int64_t>(), e.roll_core().ep_state, 64,
                        hipMemcpyDeviceToHost));
    return t;
}

static torch::Tensor actor_forward(int64_t h, torch::Tensor x) {
    Engine& e = get(h);
    auto t = f32_contig(x);
    int n = (int)(t.numel() / e.cfg.obs);
    auto out = torch::empty({n, (long)e.cfg.act}, torch::kFloat32);
    e.actor_forward(t.data_ptr<float>(), out.data_ptr<float>(), n);
    return out;
}

// Debug/parity access: copy a named device buffer to a CPU tensor.
static torch::Tensor read_buffer(int64_t h, std::string name) {
    Engine& e = get(h);
    const int B = e.cfg.batch, O = e.cfg.obs, A = e.cfg.act,
              H = e.cfg.hidden, K = e.cfg.atoms;
    // the persistent path double-buffers bs by step parity; resolve the
    // buffer the LAST completed step actually used
    if (name == "bs" && e.step_path() == Engine::PATH_PERSISTENT) {
        Counters c = e.read_counters();
        if (c.beta_t > 0 && ((c.beta_t - 1) & 1))
            name = "bs_b";
    }
    const auto i64 = torch::kInt64, f64 = torch::kFloat64;
    struct Ent {
        const char* name;
        const void* p;
        std::vector<long> shape;
        torch::ScalarType dtype = torch::kFloat32;
    };
    std::vector<Ent> tab = {
        {"bs", e.ws.bs, {B, O}},
        {"bs_b", e.ws.bs_b, {B, O}},
        {"ba", e.ws.ba, {B, A}},
        {"br", e.ws.br, {B}},
        {"bs2", e.ws.bs2, {B, O}},
        {"bd", e.ws.bd, {B}},
        {"bw", e.ws.bw, {B}},
        {"pri", e.ws.pri, {B}},
        {"bidx", e.ws.bidx, {B}, i64},
        {"a2", e.ws.a2, {B, A}},
        {"p_t", e.ws.p_t, {B, K}},
        {"m_proj", e.ws.m_proj, {B, K}},
        {"q", e.ws.q, {B, K}},
        {"pq", e.ws.pq, {B, K}},
        {"a_out", e.ws.a_out, {B, A}},
        {"dlog", e.ws.dlog, {B, K}},
        {"c_h1", e.ws.c_h1, {B, H}},
        {"c_h2", e.ws.c_h2, {B, H}},
        {"c_h3", e.ws.c_h3, {B, H}},
        {"at_h1", e.ws.at_h1, {B, H}},
        // the wide step's remaining GEMM inputs and outputs (per-GEMM
        // tests, tests/test_gpu_wide_bf16.py)
        {"at_h2", e.ws.at_h2, {B, H}},
        {"at_h3", e.ws.at_h3, {B, H}},
        {"ct_h1", e.ws.ct_h1, {B, H}},
        {"ct_h2", e.ws.ct_h2, {B, H}},
        {"ct_h3", e.ws.ct_h3, {B, H}},
        {"d1", e.ws.d1, {B, H}},
        {"d2", e.ws.d2, {B, H}},
        {"d3", e.ws.d3, {B, H}},
        {"pa_h1", e.ws.pa_h1, {B, H}},
        {"pa_h2", e.ws.pa_h2, {B, H}},
        {"pa_h3", e.ws.pa_h3, {B, H}},
        {"pc_h1", e.ws.pc_h1, {B, H}},
        {"pc_h2", e.ws.pc_h2, {B, H}},
        {"pc_h3", e.ws.pc_h3, {B, H}},
        {"pd3", e.ws.pd3, {B, K}},
        {"pd2", e.ws.pd2, {B, H}},
        {"pdh1", e.ws.pdh1, {B, H}},
        {"pda", e.ws.pda, {B, A}},
        {"adz", e.ws.adz, {B, A}},
        {"az1", e.ws.az1, {B, H}},
        {"az2", e.ws.az2, {B, H}},
        {"az3", e.ws.az3, {B, H}},
        {"tstamp", e.ws.tstamp, {64}, i64},
        {"sum_tree", e.ws.sum_tree, {2 * e.ws.tree_cap}, f64},
        {"min_tree", e.ws.min_tree, {2 * e.ws.tree_cap}, f64},
        // per-chunk sums of squares of the gradient slabs (clipping on)
        {"gn_part_actor", e.ws.gn_part_a, {gn_chunks(e.anet.n_params)}, f64},
        {"gn_part_critic", e.ws.gn_part_c, {gn_chunks(e.cnet.n_params)}, f64},
    };
    if (e.stage_pool_) {
        // the actor snapshot and the staging store of an overlapped
        // collection (whole store; rows past the staged count are stale)
        const long S = e.stage_rows_;
        tab.insert(tab.end(),
                   {{"p_actor_roll", e.p_actor_roll, {e.anet.n_params}},
                    {"stage_s", e.st_rs, {S, O}},
                    {"stage_a", e.st_ra, {S, A}},
                    {"stage_r", e.st_rr, {S}},
                    {"stage_s2", e.st_rs2, {S, O}},
                    {"stage_d", e.st_rd, {S}}});
    }
    for (const Ent& ent : tab) {
        if (name != ent.name) continue;
        auto out = torch::empty(ent.shape, ent.dtype);
        if (out.numel())                // zero: the trees of a uniform engine
            HIP_CHECK(hipMemcpy(out.data_ptr(), ent.p,
                                out.numel() * out.element_size(),
                                hipMemcpyDeviceToHost));
        return out;
    }
    throw std::runtime_error("unknown buffer " + name);
}

}  // namespace d4pg

PYBIND11_MODULE(TORCH_EXTENSION_NAME, mod) {
    // gemm_bf16, max_grad_norm, dist and kappa are the trailing arguments
    // with defaults
    mod.def("create", &d4pg::create,
            py::arg("obs"), py::arg("act"), py::arg("hidden"),
            py::arg("atoms"), py::arg("batch"), py::arg("capacity"),
            py::arg("v_min"), py::arg("v_max"), py::arg("gamma_n"),
            py::arg("tau"), py::arg("lr_actor"), py::arg("lr_critic"),
            py::arg("per_alpha"), py::arg("per_beta0"),
            py::arg("per_beta_iters"), py::arg("per_eps"), py::arg("seed"),
            py::arg("is_weighting"), py::arg("prioritized"),
            py::arg("true_td"),
            py::arg("gemm_bf16") = false,
            py::arg("max_grad_norm") = 0.0,
            py::arg("dist") = "categorical", py::arg("kappa") = 1.0);
    mod.def("destroy", &d4pg::destroy);
    mod.def("info", &d4pg::info);
    mod.def("load_slab", &d4pg::load_slab);
    mod.def("store_slab", &d4pg::store_slab);
    mod.def("synth_fill", &d4pg::synth_fill);
    mod.def("ingest", &d4pg::ingest);
    mod.def("set_seed", &d4pg::set_seed);
    mod.def("set_schedule", &d4pg::set_schedule);
    mod.def("replay_state", &d4pg::replay_state);
    mod.def("load_replay_state", &d4pg::load_replay_state);
    mod.def("step", &d4pg::step);
    mod.def("step_part", &d4pg::step_part);
    mod.def("device_tensor", &d4pg::device_tensor);
    mod.def("capture", &d4pg::capture);
    mod.def("replay", &d4pg::replay);
    mod.def("replay_async", &d4pg::replay_async);
    mod.def("sync", &d4pg::sync);
    mod.def("counters", &d4pg::counters);
    mod.def("grad_stats", &d4pg::grad_stats);
    mod.def("rollout_alloc", &d4pg::rollout_alloc);
    mod.def("rollout_run", &d4pg::rollout_run);
    mod.def("rollout_set_state", &d4pg::rollout_set_state);
    mod.def("rollout_info", &d4pg::rollout_info);
    mod.def("goal_rollout_alloc", &d4pg::goal_rollout_alloc);
    mod.def("goal_rollout_run", &d4pg::goal_rollout_run);
    mod.def("goal_rollout_set_state", &d4pg::goal_rollout_set_state);
    mod.def("goal_rollout_info", &d4pg::goal_rollout_info);
    mod.def("goal_rollout_episode", &d4pg::goal_rollout_episode);
    mod.def("synth_rollout_alloc", &d4pg::synth_rollout_alloc);
    mod.def("synth_rollout_run", &d4pg::synth_rollout_run);
    mod.def("synth_rollout_set_state", &d4pg::synth_rollout_set_state);
    mod.def("synth_rollout_info", &d4pg::synth_rollout_info);
    mod.def("collect_alloc", &d4pg::collect_alloc);
    mod.def("collect_begin", &d4pg::collect_begin);
    mod.def("collect_commit", &d4pg::collect_commit);
    mod.def("collect_pending", &d4pg::collect_pending);
    mod.def("eval_alloc", &d4pg::eval_alloc);
    mod.def("eval_run", &d4pg::eval_run);
    mod.def("eval_results", &d4pg::eval_results);
    mod.def("eval_arrays", &d4pg::eval_arrays);
    mod.def("eval_set_state", &d4pg::eval_set_state);
    mod.def("eval_info", &d4pg::eval_info);
    mod.def("rollout_words", &d4pg::rollout_words);
    mod.def("replay_slice", &d4pg::replay_slice);
    mod.def("rollout_last", &d4pg::rollout_last);
    mod.def("actor_forward", &d4pg::actor_forward);
    mod.def("read_buffer", &d4pg::read_buffer);
}
