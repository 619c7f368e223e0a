#!/usr/bin/env python
"""What it costs to feed EVOPF-v0's days from a table instead of drawing them from Philox, on one MI355X (GPU box).

    python tools/bench_scenarios.py [--reps R] [--out profiles/eval_scenarios_bench.json]

EVOPF-RPODDPG with bench.py's hyper-parameters after 32 vector steps on 16 lanes; the days are the ones the Philox streams deal
under the evaluation's seed (``env.scenarios(1024, seed)``), so both forms compute the same thing and their results are compared
bit for bit before anything is timed.
* ``evaluate``: ``evaluate(1024, seed)`` (Philox-dealt, the stepwise path) and ``evaluate(1024, seed, scenarios=S)`` (table-fed),
  run ALTERNATELY, --reps rounds after one warm-up round (which also uploads the table: the device copy is cached); wall clock
  around a device synchronisation, host work and the copy back included.  Reported: median, min, max in milliseconds and the
  ratio of the medians.
* ``step``: the step kernel alone on 1 024 lanes, ``rpo_evopf_step`` against ``rpo_evopf_step_scenario``, alternately: one sample
  is the device time of `inner` = 12 back-to-back launches after a reset between two events, divided by `inner` (hours 1..12 of
  the day: both kernels fetch data in every launch of a sample).  Median, min, max in microseconds.
* ``table``: ``rpo_evopf_scenario_table`` for 1 024 lanes, the same way, and ``env.scenarios(1024)`` as wall clock (kernel, copy
  back, the host object).
No threshold: nobody has measured this before; the expectation is only that the table's loads are not dearer than the Philox
rounds and the logf / tanf / acosf chain they replace.  The work runs in a child process under a time limit (``timeout -k 10``).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EPISODES = 1024
SEED = 11


def _stat(xs, digits=3):
    return dict(median=round(statistics.median(xs), digits), min=round(min(xs), digits), max=round(max(xs), digits))


def child(reps):
    import numpy as np
    import torch
    from bench import make_trainer
    from rpo_amd import ops
    dev = torch.device("cuda")
    tr = make_trainer(16, dev, max_epochs=1000, capacity=64, workload="evopf_ddpg")
    env = tr.base_env
    tr.vec.reset()
    tr.run_steps(32)
    S = env.scenarios(EPISODES, SEED)
    # ---- whole evaluations, alternately
    wall = dict(philox=[], table=[])
    for rnd in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a = tr.evaluate(EPISODES, seed=SEED)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        b = tr.evaluate(EPISODES, seed=SEED, scenarios=S)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if rnd == 0:
            assert a.path == b.path == "stepwise"
            for f in a.FIELDS:
                assert np.array_equal(getattr(a, f), getattr(b, f)), f
        else:
            wall["philox"].append((t1 - t0) * 1e3)
            wall["table"].append((t2 - t1) * 1e3)
    evaluate = dict(episodes=EPISODES, horizon=a.horizon, path=a.path, bits_equal=True, philox_ms=_stat(wall["philox"]),
                    table_ms=_stat(wall["table"]),
                    table_over_philox=round(statistics.median(wall["table"]) / statistics.median(wall["philox"]), 4),
                    return_mean=float(a.ret.mean()), violation_rate=a.violation_rate())
    # ---- the step kernel alone
    day = torch.arange(EPISODES, dtype=torch.int32, device=dev)
    plain = env.make_vec(EPISODES, seed=SEED, stats_cap=2)
    fed = env.make_vec(EPISODES, seed=SEED, stats_cap=2, scenario=(S.table(dev), day))
    action = tr.evaluate(16, seed=SEED, record=True).trajectory.action[:, 0]
    action = torch.tensor(np.tile(action, (EPISODES // 16, 1)), device=dev)
    rows = torch.zeros(EPISODES, env.kernels.ring_floats, device=dev)
    inner = 12
    samples = dict(philox=[], table=[])
    for rnd in range(reps + 2):
        for name, v in (("philox", plain), ("table", fed)):
            v.reset()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                v.step(action, rows=rows, cap_steps=1, auto_reset=False)
            e1.record()
            e1.synchronize()
            if rnd >= 2:
                samples[name].append(e0.elapsed_time(e1) * 1e3 / inner)
    assert torch.equal(plain.internal.view(torch.int32), fed.internal.view(torch.int32))
    step = dict(lanes=EPISODES, inner=inner, philox_us=_stat(samples["philox"]), table_us=_stat(samples["table"]),
                table_over_philox=round(statistics.median(samples["table"]) / statistics.median(samples["philox"]), 4))
    # ---- the table itself
    out = torch.empty(EPISODES, ops.SCEN_DAY, device=dev)
    t_us, t_wall = [], []
    for rnd in range(reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            ops.evopf_scenario_table(env.kernels, out, None, SEED, 0)
        e1.record()
        e1.synchronize()
        t0 = time.perf_counter()
        env.scenarios(EPISODES, SEED)
        t1 = time.perf_counter()
        if rnd >= 2:
            t_us.append(e0.elapsed_time(e1) * 1e3 / inner)
            t_wall.append((t1 - t0) * 1e3)
    table = dict(lanes=EPISODES, kernel_us=_stat(t_us), env_scenarios_ms=_stat(t_wall), bytes=int(out.numel() * 4))
    print("SCEN_BENCH " + json.dumps(dict(device=torch.cuda.get_device_name(0), reps=reps, evaluate=evaluate, step=step, table=table)),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_scenarios_bench.json"))
    ap.add_argument("--limit", type=int, default=400, help="seconds for the whole measurement")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.reps)
    p = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps)],
                       stdout=subprocess.PIPE, text=True)
    if p.returncode != 0:                                        # (a fault, an abort, a time limit: nothing more is started)
        print(p.stdout[-2000:])
        sys.exit("bench_scenarios: ended with status %d" % p.returncode)
    tag = "SCEN_BENCH "
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith(tag)][-1][len(tag):])
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
