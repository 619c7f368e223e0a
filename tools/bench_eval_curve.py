#!/usr/bin/env python
"""What an evaluation point costs a training run on one MI355X (GPU box); prints ONE JSON line.

    timeout -k 10 900 python tools/bench_eval_curve.py [--rounds 3] [--points 8] [--out profiles/eval_curve_bench.json]

For cart-RPODDPG and pendulum-RPODDPG at 4096 lanes (bench.py's hyper-parameters, eval_fre 500), the wall time of the same
region -- run_steps(points * eval_fre, eval=...) followed by a read of the results and a device synchronise -- in five legs:

  a  eval=False                                   (training alone)
  b  eval=True, the host-driven eval()            (today's default)
  c  eval=True, curve mode, 10 episodes per point, overlapped on the evaluation stream
  d  the same with schedule eval_overlap=0        (in order on the training stream)
  e  curve mode, 1024 episodes per point, overlapped

One trainer per leg (b shares a's), every leg warmed by one untimed region (graph captures, allocations), then --rounds
rounds that alternate the legs; medians.  Reported: the five times, the added time per evaluation point of b..e over a, the
share of eval() in leg b's wall time, and the time of one rpo_eval_summarize at 10 / 1024 / 2^20 episodes (events around
100 back-to-back calls).  One process; run it under its own time limit.

    timeout -k 10 900 python tools/bench_eval_curve.py --keep-best [--rounds 3] [--points 8] [--out profiles/eval_keep_best_bench.json]

The ``keep_best`` leg instead: what keeping the best policy on the device (``rpo_eval_keep_best`` behind every point's summary)
adds to a point.  For both workloads, 10 and 1024 episodes per point, overlapped and in order: two trainers of the same build,
``keep_best=True`` and off (off: the launches of curve mode as it was), the same region, one untimed round and --rounds
alternating rounds; medians, every sample, and the added time per point.  And the device time of ``rpo_eval_keep_best`` alone
on a span of the cart actor's length, on the taken and on the not-taken branch (events around 100 back-to-back calls).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from bench import make_trainer, spin_up  # noqa: E402

LANES, EVAL_FRE = 4096, 500
LEGS = (("a_no_eval", None, {}), ("b_eval", None, {}), ("c_curve10_overlap", 10, dict(eval_overlap=1)),
        ("d_curve10_inorder", 10, dict(eval_overlap=0)), ("e_curve1024_overlap", 1024, dict(eval_overlap=1)))


def trainer(workload, episodes, schedule):
    kw = {} if episodes is None else dict(eval_episodes=episodes)
    tr = make_trainer(LANES, torch.device("cuda"), 10 ** 9, capacity=64, workload=workload, eval_fre=EVAL_FRE,
                      schedule=schedule or None, **kw)
    tr.vec.reset()
    return tr


def region(tr, n, evaluate):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tr.run_steps(n, eval=evaluate)
    points = len(tr.eval_curve)                                 # (curve mode: the harvest; empty otherwise)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, points


def summarize_us(n, reps=100):
    from rpo_amd import ops
    dev = torch.device("cuda")
    acc = torch.rand(n, ops.EVAL_LEN, device=dev)
    acc[:, 7] = torch.full((n,), 40, dtype=torch.int32, device=dev).view(torch.float32)
    ctrl = torch.zeros(ops.CTRL_LEN, dtype=torch.int64, device=dev)
    row = torch.zeros(ops.CURVE_LEN, dtype=torch.float64, device=dev)
    ws = torch.zeros(ops.CURVE_WS, dtype=torch.float64, device=dev)
    for _ in range(5):
        ops.eval_summarize(acc, ctrl, row, ws)
    times = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            ops.eval_summarize(acc, ctrl, row, ws)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3 / reps)
    return statistics.median(times)


def keep_best_us(n_params, taken, reps=100):
    """Device time of one rpo_eval_keep_best on a span of n_params floats.  taken: every call's return is strictly higher
    than the incumbent's (decide writes, the copy runs); otherwise every call after the first ties and loses."""
    from rpo_amd import ops
    dev = torch.device("cuda")
    src, best = torch.rand(n_params, device=dev), torch.zeros(n_params, device=dev)
    rows = torch.zeros(reps + 6, ops.CURVE_LEN, dtype=torch.float64, device=dev)
    rows[:, 12] = 200.0                                         # RPO_CURVE_LENGTH (no violating step: safe)
    best_row = torch.zeros(ops.CURVE_LEN, dtype=torch.float64, device=dev)
    best_point = torch.full((1,), -1, dtype=torch.int64, device=dev)
    times = []
    for _ in range(6):
        best_point.fill_(-1)
        rows[:, 2] = torch.arange(reps + 6, device=dev, dtype=torch.float64) if taken else 1.0   # RPO_CURVE_STATS: the return
        for k in range(5):
            ops.eval_keep_best(src, best, rows[k], best_row, best_point, k, 0.0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for k in range(5, reps + 5):
            ops.eval_keep_best(src, best, rows[k], best_row, best_point, k, 0.0)
        e1.record()
        torch.cuda.synchronize()
        assert int(best_point.cpu()[0]) == (reps + 4 if taken else 0)
        times.append(e0.elapsed_time(e1) * 1e3 / reps)
    return dict(median=statistics.median(times[1:]), all=times[1:])


def keep_best_leg(a):
    n = a.points * EVAL_FRE
    line = dict(tool="bench_eval_curve --keep-best", device=torch.cuda.get_device_name(0), lanes=LANES, eval_fre=EVAL_FRE,
                iterations=n, points=a.points, rounds=a.rounds, configs={})
    span = None
    for workload in ("cart_ddpg", "pen_ddpg"):
        line["configs"][workload] = {}
        for episodes in (10, 1024):
            for overlap in (1, 0):
                trs = {}
                for name, kw in (("off", {}), ("on", dict(keep_best=True))):
                    tr = make_trainer(LANES, torch.device("cuda"), 10 ** 9, capacity=64, workload=workload, eval_fre=EVAL_FRE,
                                      schedule=dict(eval_overlap=overlap), eval_episodes=episodes, **kw)
                    tr.vec.reset()
                    trs[name] = tr
                times = {name: [] for name in trs}
                for rnd in range(a.rounds + 1):                 # round 0: untimed warm-up of both
                    for name in (("off", "on") if rnd % 2 else ("on", "off")):
                        before = len(trs[name].eval_curve)
                        t, points = region(trs[name], n, True)
                        assert points - before == a.points, (name, points, before)
                        if rnd:
                            times[name].append(t)
                assert trs["on"].best is not None and trs["off"].best is None
                lo, hi = trs["on"].agent.flat.actor_range
                span = hi - lo if workload == "cart_ddpg" else span
                med = {name: statistics.median(ts) for name, ts in times.items()}
                line["configs"][workload]["%d_%s" % (episodes, "overlap" if overlap else "inorder")] = dict(
                    wall_s=med, all_s=times, span_floats=hi - lo, best_point=trs["on"].best.point,
                    added_ms_per_point=(med["on"] - med["off"]) * 1e3 / a.points,
                    spread_ms_per_point={name: (max(ts) - min(ts)) * 1e3 / a.points for name, ts in times.items()})
                del trs
                torch.cuda.empty_cache()
    line["us_per_keep_best"] = dict(span_floats=span, taken=keep_best_us(span, True), not_taken=keep_best_us(span, False))
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--points", type=int, default=8)
    ap.add_argument("--out", default=None)
    ap.add_argument("--keep-best", action="store_true", help="the keep_best leg instead of legs a..e")
    a = ap.parse_args()
    os.environ["RPO_VERBOSE"] = "0"
    n = a.points * EVAL_FRE
    spin_up(torch.device("cuda"))
    if a.keep_best:
        s = json.dumps(keep_best_leg(a))
        print(s)
        if a.out:
            with open(a.out, "w") as f:
                f.write(s + "\n")
        return
    line = dict(tool="bench_eval_curve", device=torch.cuda.get_device_name(0), lanes=LANES, eval_fre=EVAL_FRE, iterations=n,
                points=a.points, rounds=a.rounds, configs={})
    for workload in ("cart_ddpg", "pen_ddpg"):
        trs = {}
        for name, episodes, schedule in LEGS:
            trs[name] = trs["a_no_eval"] if name == "b_eval" else trainer(workload, episodes, schedule)
        times = {name: [] for name, _, _ in LEGS}
        for rnd in range(a.rounds + 1):                         # round 0: untimed warm-up of every leg
            for name, episodes, _ in LEGS:
                before = len(trs[name].eval_curve)
                t, points = region(trs[name], n, name != "a_no_eval")
                if episodes is not None:
                    assert points - before == a.points, (name, points, before)
                if rnd:
                    times[name].append(t)
        med = {name: statistics.median(ts) for name, ts in times.items()}
        row = dict(wall_s=med, all_s=times,
                   added_ms_per_point={name: (med[name] - med["a_no_eval"]) * 1e3 / a.points for name in med if name != "a_no_eval"})
        row["eval_share_of_leg_b"] = (med["b_eval"] - med["a_no_eval"]) / med["b_eval"]
        row["us_per_iteration_no_eval"] = med["a_no_eval"] * 1e6 / n
        row["c_over_b"] = row["added_ms_per_point"]["c_curve10_overlap"] / row["added_ms_per_point"]["b_eval"]
        line["configs"][workload] = row
        del trs
        torch.cuda.empty_cache()
    line["us_per_summarize"] = {str(k): summarize_us(k) for k in (10, 1024, 1 << 20)}
    s = json.dumps(line)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
