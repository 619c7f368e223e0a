"""bench.py's N > 1 control flow, executed on the one GPU of the test box (missing 1).

The measured multi-GPU configuration is one rank per GPU over RCCL (backend "nccl"), which cannot put two ranks on one
device; before round 5 the `world > 1` code of bench.py -- self-launch of the ranks, process group, max-reduced timed
regions, the clinic on every rank, one JSON line from rank 0 only -- had therefore never executed anywhere.  With
``RPO_BENCH_BACKEND=gloo`` the ranks share cuda:0 and the collectives are issued by the host between hipGraph segments
(the scheme of test_trainer_gpu.py::test_data_parallel_graph_segments_on_gpu); everything else is the code the driver's
8-GPU run goes through.  The line is labelled a control-flow check: two processes time-slicing one GPU say nothing about
scaling.
"""
import json
import os
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_bench(extra_env, args, budget):
    """bench.py as a fresh process (started before anything here touches the GPU in ITS address space: no re-exec of a GPU
    process); returns (returncode or None when it had to be ended, stdout, stderr)."""
    env = dict(os.environ)
    env.update(extra_env)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    p = subprocess.Popen([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT, env=env,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, start_new_session=True)
    try:
        out, err = p.communicate(timeout=budget)
        return p.returncode, out, err
    except subprocess.TimeoutExpired:
        import signal
        os.killpg(p.pid, signal.SIGKILL)                         # exactly the process group started above (launcher + ranks)
        out, err = p.communicate()
        return None, out, err


@pytest.mark.timeout(900, method="thread")
def test_bench_two_ranks_over_gloo_on_one_gpu():
    """`bench.py --gpus 2 --steps 20 --warmup 5 --full --no-cpu-baseline` (a multi-GPU run with its clinic and cart_sac leg)
    through the gloo switch: exit code 0 from the launcher (i.e. from every rank), ONE JSON line on stdout (rank 1 prints
    nothing there), and the keys a SCALE run is checked by."""
    args = ["--gpus", "2", "--steps", "20", "--warmup", "5", "--full", "--no-cpu-baseline"]
    t0 = time.time()
    for attempt in range(3):
        # two processes time-slicing one GPU through gloo stall once in ~20 runs on this pool (see
        # test_data_parallel_graph_segments_on_gpu): a stalled attempt is ended and repeated; three in a row FAIL
        rc, out, err = _run_bench({"RPO_BENCH_BACKEND": "gloo"}, args, budget=280)
        if rc is not None:
            break
    assert rc is not None, "bench.py --gpus 2 over gloo did not finish within 280 s, three times in a row\n" + err[-3000:]
    assert rc == 0, err[-4000:]
    lines = [l for l in out.split("\n") if l.strip()]
    assert len(lines) == 1, out                                  # rank 0's line and nothing else on stdout
    r = json.loads(lines[0])
    cfg = r["config"]
    assert r["n_gpus"] == 2 and r["steps"] == 20 and r["warmup"] == 5 and r["scaling"] == "weak"
    assert cfg["global_envs"] == 8192 and cfg["envs_per_gpu"] == 4096
    assert cfg["data_parallel_path"] is True
    assert cfg["collectives_per_update"] == 1.25                 # one per critic update + one per policy step (policy_fre 4)
    assert "graphs_replayed_on_all_ranks" in cfg and "graph_capture_fell_back_to_eager" in cfg
    assert cfg["collective_backend"] == "gloo" and cfg["rccl_ranks"] == 0
    assert cfg["collectives_in_graph"] is False                  # host-driven collectives cannot be captured
    assert cfg["allreduce_bytes"]["critic_update"] > 0
    assert "control_flow_check" in r and "NOT a scaling figure" in r["control_flow_check"]
    assert r["value"] > 0 and abs(r["value"] - 8192 * 20 / (r["ms_per_step"] * 20e-3)) < 1e-6 * r["value"]
    assert r["timed_regions"] >= 1 and r["ms_per_step_min"] <= r["ms_per_step"] <= r["ms_per_step_max"]
    roof = r["roofline"]                                         # every rank ran the clinic, rank 0's figures are printed
    assert roof["frac"] > 0 and roof["bound"] in ("hbm", "mfma") and "2-rank run" in roof["note"]
    assert "cart_sac_env_steps_per_s" in r                       # config 4's algorithm on the same ranks
    assert "cpu_baseline" not in r                               # rank 0 at N = 1 only
    os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
    with open(os.path.join(ROOT, "gpurun_out", "bench_gloo_2ranks.json"), "w") as f:
        json.dump(dict(line=r, seconds=time.time() - t0, attempts=attempt + 1), f, indent=1)


@pytest.mark.timeout(900, method="thread")
def test_scale_preflight_over_gloo_on_one_gpu():
    """tools/scale_preflight.py -- what to run FIRST on a multi-GPU box -- in its control-flow form: two ranks
    sharing this GPU over gloo, config 4's algorithm at 512 lanes per rank, 64 iterations: one JSON verdict, replicas bit-equal
    after 64 iterations with graph segments AND with eager launches, the lanes sharded, microseconds per iteration for the
    plain process and the two-rank run."""
    import signal
    cmd = [sys.executable, os.path.join(ROOT, "tools", "scale_preflight.py"), "--gpus", "2", "--backend", "gloo", "--lanes", "512",
           "--quick"]
    out = err = ""
    rc = None
    for attempt in range(3):                                     # (two processes time-slicing one GPU through gloo: see above)
        env = dict(os.environ)
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        p = subprocess.Popen(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, start_new_session=True)
        try:
            out, err = p.communicate(timeout=280)
            rc = p.returncode
            break
        except subprocess.TimeoutExpired:
            os.killpg(p.pid, signal.SIGKILL)
            out, err = p.communicate()
    assert rc is not None, "scale_preflight over gloo did not finish within 280 s, three times in a row\n" + err[-3000:]
    lines = [l for l in out.splitlines() if l.strip().startswith("{")]
    assert len(lines) == 1, out + err[-3000:]
    v = json.loads(lines[0])
    assert rc == 0 and v["verdict"] == "ok", json.dumps(v, indent=1)[:4000]
    assert v["ranks"] == 2 and v["backend"] == "gloo" and v["iterations"] == 64
    assert v["replicas_bit_equal_after_64_iterations"] is True
    nr = v["legs"]["n_ranks"]["result"]
    assert nr["world"] == 2 and nr["lanes_per_rank"] == 512 and nr["data_parallel_path"] and nr["lanes_differ_between_ranks"]
    assert nr["rccl_ranks"] == 0 and nr["collectives_in_graph"] is False          # gloo: host-driven collectives between segments
    assert v["legs"]["n_ranks_eager"]["result"]["replicas_bit_equal"] is True
    assert v["us_per_iteration"]["plain_process"] > 0 and v["us_per_iteration"]["n_ranks"] > 0
    assert "control-flow form" in v["note"]
    os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
    with open(os.path.join(ROOT, "gpurun_out", "scale_preflight_gloo.json"), "w") as f:
        json.dump(v, f, indent=1)


@pytest.mark.timeout(900, method="thread")
def test_bench_dump_outputs_are_reproducible(tmp_path):
    """`bench.py --dump-outputs DIR`: what the last of exactly `--steps` timed steps computed -- its transitions, the
    observations, parameters and targets after the update, the losses -- as float32 / float64 .npy files of at most 64 MB,
    the same from two runs with the same arguments (every input comes from fixed seeds)."""
    import numpy as np
    args = ["--steps", "24", "--warmup", "4", "--no-extras", "--no-cpu-baseline", "--no-clinic"]
    runs = []
    for i in range(2):
        d = os.path.join(str(tmp_path), "run%d" % i)
        rc, out, err = _run_bench({}, args + ["--dump-outputs", d], budget=400)
        assert rc == 0, err[-4000:]
        r = json.loads(out.strip().splitlines()[-1])
        assert r["steps"] == 24 and r["timed_regions"] == 1
        runs.append({f[:-len(".npy")]: np.load(os.path.join(d, f)) for f in os.listdir(d)})
    a, b = runs
    assert sorted(a) == sorted(b)
    assert {"params", "critic_target", "obs", "transition_state", "transition_action", "transition_next_state", "loss_critic"} <= set(a)
    assert a["transition_state"].shape == (4096, 6) and a["obs"].shape == (4096, 6)
    assert sum(v.nbytes for v in a.values()) <= 64 * 2 ** 20
    for k in a:
        assert a[k].dtype in (np.float32, np.float64), (k, a[k].dtype)
        assert np.isfinite(a[k]).all(), k
        np.testing.assert_allclose(a[k], b[k], rtol=1e-5, atol=1e-6, err_msg=k)


def test_lanes_sweep_rows_carry_both_rooflines():
    """bench.py's `lanes_sweep`: whole iterations -- rollout only, rollout + the batch-256 update -- with
    env-steps/s and the fractions of the f32 MFMA peak and of the HBM roofline.  Here at two small sizes (the bench runs 4096 /
    65 536 / 2^20); a size that cannot run is reported in its row, not raised."""
    import torch
    sys.path.insert(0, ROOT)
    import bench
    os.environ.setdefault("RPO_VERBOSE", "0")
    res = bench.lanes_sweep(torch.device("cuda"), [512, 8192])
    assert [r["lanes"] for r in res["rows"]] == [512, 8192] and "flop" in res["note"]
    for r in res["rows"]:
        assert "error" not in r, r
        for mode in ("rollout_only", "with_update"):
            m = r[mode]
            assert m["env_steps_per_s"] > 0 and 0 < m["frac_of_f32_mfma_peak"] < 1 and 0 < m["frac_of_hbm_roofline"] < 1
            assert abs(m["env_steps_per_s"] - r["lanes"] / (m["ms_per_step"] * 1e-3)) < 1e-6 * m["env_steps_per_s"]
        assert r["with_update"]["ms_per_step"] > r["rollout_only"]["ms_per_step"]
    bad = bench.lanes_sweep(torch.device("cuda"), [-5])          # (make_trainer refuses: the row says so)
    assert "error" in bad["rows"][0]
