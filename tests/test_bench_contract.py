"""The driver depends on bench.py's exact output contract: one JSON line
from rank 0 with the BASELINE metric/config fields.  Pin it (CPU fallback
path; the GPU and multirank paths emit through the same code)."""

import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


AUX_KEYS = ("env_steps_per_sec_1actor", "env_steps_per_sec_vector64",
            "env_steps_per_sec_gpu_rollout8192")


def _run_bench(*extra):
    res = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"),
         "--steps", "8", "--warmup", "2", *extra],
        capture_output=True, text=True, timeout=600, cwd=REPO)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, "exactly one JSON line expected"
    return json.loads(lines[0])


def test_bench_full_adds_aux_metrics():
    """--full carries the actor-side figures a plain run leaves out."""
    out = _run_bench("--full")
    assert out["steps"] == 8 and out["ms_per_step"] > 0
    assert out["env_steps_per_sec_1actor"] > 0
    assert out["env_steps_per_sec_vector64"] > 0
    if out["config"]["device"] == "cuda":
        assert out["env_steps_per_sec_gpu_rollout8192"] > 0
    else:
        assert out["env_steps_per_sec_gpu_rollout8192"] is None


def test_bench_dump_outputs_reproducible(tmp_path):
    """--dump-outputs writes the learner state of the last timed step as
    float32 .npy files; fixed seeds make two runs agree bit for bit."""
    import numpy as np
    dirs = [str(tmp_path / "a"), str(tmp_path / "b")]
    for d in dirs:
        _run_bench("--dump-outputs", d)
    names = sorted(os.listdir(dirs[0]))
    assert names == sorted(os.listdir(dirs[1]))
    assert {"actor.npy", "actor_target.npy", "critic.npy",
            "critic_target.npy"} <= set(names)
    total = 0
    for n in names:
        a = np.load(os.path.join(dirs[0], n))
        b = np.load(os.path.join(dirs[1], n))
        assert a.dtype == np.float32 and a.size > 0
        assert np.isfinite(a).all(), n
        np.testing.assert_array_equal(a, b, err_msg=n)
        total += a.nbytes
    assert total <= 64 * 2 ** 20
    # 10 optimizer steps moved the online nets off their targets
    act = np.load(os.path.join(dirs[0], "actor.npy"))
    tgt = np.load(os.path.join(dirs[0], "actor_target.npy"))
    assert act.shape == tgt.shape and not np.array_equal(act, tgt)


def test_bench_json_contract():
    out = _run_bench()
    # a plain run measures the headline only
    assert not any(k in out for k in AUX_KEYS)
    # driver-contract fields (brief): metric/value/unit/n_gpus/steps/
    # warmup/ms_per_step/higher_is_better/scaling/vs_baseline/dtype/data/
    # config{model, global_batch, seq_len, parallelism}
    assert out["metric"].startswith("learner grad-steps/sec")
    assert out["unit"] == "grad_steps/s"
    assert out["n_gpus"] == 1 and out["steps"] == 8 and out["warmup"] == 2
    assert out["higher_is_better"] is True
    assert out["scaling"] == "weak"
    assert out["vs_baseline"] is None          # reference publishes none
    assert out["dtype"] == "fp32"
    assert "synthetic" in out["data"]
    cfg = out["config"]
    assert cfg["global_batch"] == 64 and cfg["seq_len"] is None
    assert cfg["n_step"] == 5 and cfg["prioritized_replay"] is True
    assert cfg["replay_capacity"] == 1_000_000
    assert out["value"] > 0 and out["ms_per_step"] > 0
    # timing identity: value == n_gpus * steps / elapsed
    ident = out["n_gpus"] * 1000.0 / out["ms_per_step"]
    assert abs(out["value"] - ident) < 1e-6 * out["value"]
