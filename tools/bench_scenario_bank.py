#!/usr/bin/env python
"""What it costs to train EVOPF-v0 on a scenario bank instead of the Philox-drawn days, on one MI355X (GPU box).

    python tools/bench_scenario_bank.py [--reps R] [--out profiles/scenario_bank_bench.json]

tools/bench_scenarios.py's method: bits first, then the forms run ALTERNATELY, --reps rounds after two warm-up rounds; median, min
and max of the rounds.
* ``step``: the step kernel alone on 1 024 lanes with ``auto_reset = 1``: ``rpo_evopf_step`` (Philox) against
  ``rpo_evopf_step_bank`` with the "uniform" and the "cycle" deal.  The bank is the 1 024 days the Philox streams deal those lanes
  (``env.scenarios(1024, seed)``), so under "cycle" with stride 1 024 lane i plays its Philox day in episode 0: the bank step's
  state after hours 1..12 is compared bit for bit with the Philox step's, and the "uniform" step's with the table-fed step
  (``rpo_evopf_step_scenario``) on the days ``rpo_evopf_bank_days`` names, before anything is timed.  One sample is the device
  time of `inner` = 24 back-to-back launches after a reset between two events, divided by `inner`: a whole day, the last launch
  of which rolls every lane over to its next episode (the Philox step draws hour 0 of the next day there, the bank step deals the
  next day and reads it).  Microseconds.
* ``train``: ``run_steps(steps)`` of EVOPF-RPODDPG with bench.py's hyper-parameters on 1 024 lanes in hipGraph windows, without a
  bank against ``scenarios=`` that bank (deal "uniform"), alternately on two trainers; wall clock around a device synchronisation,
  milliseconds per vector step.
* ``days``: ``rpo_evopf_bank_days`` for 1 024 lanes, and ``trainer.scenario_days()`` as wall clock (kernel and copy back).
Nobody has measured this before.  The expectation is "no difference outside the spread", as for the table-fed step: the bank step
adds one Philox block per obs() call (the "uniform" deal) or a 64-bit remainder (the "cycle" deal) and reads 52 table words in
place of seven Philox blocks.  The verdict the file records: a bank step is ``slower`` when its median exceeds the Philox step's
median by more than the min-max spread of the Philox step in the same run.  The work runs in a child process under a time limit
(``timeout -k 10``).
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

LANES = 1024
SEED = 11


def _stat(xs, digits=3):
    return dict(median=round(statistics.median(xs), digits), min=round(min(xs), digits), max=round(max(xs), digits))


def child(reps, steps):
    import numpy as np
    import torch
    from bench import make_trainer
    from rpo_amd import ops
    dev = torch.device("cuda")
    small = make_trainer(16, dev, max_epochs=1000, capacity=64, workload="evopf_ddpg")
    env = small.base_env
    small.vec.reset()
    small.run_steps(32)
    S = env.scenarios(LANES, SEED)
    table = S.table(dev)
    # ---- the step kernel alone: bits first
    vecs = dict(philox=env.make_vec(LANES, seed=SEED, stats_cap=2),
                uniform=env.make_vec(LANES, seed=SEED, stats_cap=2, bank=(table, "uniform", LANES)),
                cycle=env.make_vec(LANES, seed=SEED, stats_cap=2, bank=(table, "cycle", LANES)))
    day = torch.empty(LANES, dtype=torch.int32, device=dev)
    ops.evopf_bank_days(day, None, LANES, "uniform", LANES, SEED, 0)
    fed = env.make_vec(LANES, seed=SEED, stats_cap=2, scenario=(table, day))
    action = small.evaluate(16, seed=SEED, record=True).trajectory.action[:, 0]
    action = torch.tensor(np.tile(action, (LANES // 16, 1)), device=dev)
    rows = torch.zeros(LANES, env.kernels.ring_floats, device=dev)
    for v in list(vecs.values()) + [fed]:
        v.reset()
        for _ in range(12):
            v.step(action, rows=rows, cap_steps=1, auto_reset=v is not fed)
    as_bits = lambda v: v.internal.view(torch.int32)
    assert torch.equal(as_bits(vecs["philox"]), as_bits(vecs["cycle"])) and torch.equal(as_bits(fed), as_bits(vecs["uniform"]))
    assert not torch.equal(as_bits(vecs["philox"]), as_bits(vecs["uniform"]))
    inner = 24
    samples = {k: [] for k in vecs}
    for rnd in range(reps + 2):
        for name, v in vecs.items():
            v.ep_count.zero_()
            v.reset()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                v.step(action, rows=rows, cap_steps=1, auto_reset=True)
            e1.record()
            e1.synchronize()
            if rnd >= 2:
                samples[name].append(e0.elapsed_time(e1) * 1e3 / inner)
    for v in vecs.values():
        assert int(v.ep_count.min()) == int(v.ep_count.max()) == 1 and int(v.ep_len.max()) == 0     # every lane rolled over once
    spread = max(samples["philox"]) - min(samples["philox"])
    med = {k: statistics.median(x) for k, x in samples.items()}
    step = dict(lanes=LANES, inner=inner, auto_reset=1, bits_equal=True, philox_us=_stat(samples["philox"]),
                bank_uniform_us=_stat(samples["uniform"]), bank_cycle_us=_stat(samples["cycle"]),
                philox_spread_us=round(spread, 3),
                uniform_over_philox=round(med["uniform"] / med["philox"], 4), cycle_over_philox=round(med["cycle"] / med["philox"], 4),
                uniform_slower=bool(med["uniform"] - med["philox"] > spread), cycle_slower=bool(med["cycle"] - med["philox"] > spread))
    # ---- whole training iterations in graph windows
    del small
    trainers = dict(philox=make_trainer(LANES, dev, max_epochs=10 ** 9, capacity=64, workload="evopf_ddpg", use_graph=True, seed=SEED),
                    bank=make_trainer(LANES, dev, max_epochs=10 ** 9, capacity=64, workload="evopf_ddpg", use_graph=True, seed=SEED,
                                      scenarios=S, deal="uniform"))
    wall = {k: [] for k in trainers}
    for tr in trainers.values():
        tr.vec.reset()
        tr.run_steps(96)                                         # every window of the steady state is captured
    for rnd in range(reps + 1):
        for name, tr in trainers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.run_steps(steps)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if rnd >= 1:
                wall[name].append((t1 - t0) * 1e3 / steps)
    for tr in trainers.values():
        assert not tr._graphs.capture_failed and bool(torch.isfinite(tr.agent.flat.data).all())
    spread_t = max(wall["philox"]) - min(wall["philox"])
    train = dict(lanes=LANES, steps=steps, deal="uniform", bank_days=len(S), philox_ms_per_step=_stat(wall["philox"], 4),
                 bank_ms_per_step=_stat(wall["bank"], 4), philox_spread_ms=round(spread_t, 4),
                 bank_over_philox=round(statistics.median(wall["bank"]) / statistics.median(wall["philox"]), 4),
                 bank_slower=bool(statistics.median(wall["bank"]) - statistics.median(wall["philox"]) > spread_t))
    # ---- asking which day a lane is on
    tr = trainers["bank"]
    d_us, d_wall = [], []
    for rnd in range(reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            ops.evopf_bank_days(day, tr.vec.ep_count, len(S), "uniform", LANES, SEED, 0)
        e1.record()
        e1.synchronize()
        t0 = time.perf_counter()
        tr.scenario_days()
        t1 = time.perf_counter()
        if rnd >= 2:
            d_us.append(e0.elapsed_time(e1) * 1e3 / inner)
            d_wall.append((t1 - t0) * 1e3)
    days = dict(lanes=LANES, kernel_us=_stat(d_us), scenario_days_ms=_stat(d_wall))
    print("BANK_BENCH " + json.dumps(dict(device=torch.cuda.get_device_name(0), reps=reps, step=step, train=train, days=days)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--steps", type=int, default=192, help="vector steps per timed run_steps call")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scenario_bank_bench.json"))
    ap.add_argument("--limit", type=int, default=400, help="seconds for the whole measurement")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.reps, a.steps)
    p = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps),
                        "--steps", str(a.steps)], stdout=subprocess.PIPE, text=True)
    if p.returncode != 0:                                        # (a fault, an abort, a time limit: nothing more is started)
        print(p.stdout[-2000:])
        sys.exit("bench_scenario_bank: ended with status %d" % p.returncode)
    tag = "BANK_BENCH "
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith(tag)][-1][len(tag):])
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
