#!/usr/bin/env python
"""trainer.evaluate() vs eval() on one MI355X (GPU box); prints ONE JSON line.

    python tools/bench_eval.py [--reps R] [--sizes 4096,65536,1048576] [--out FILE]
    python tools/bench_eval.py --profile-only [--sizes 65536]     # fused evaluations only, for a rocprofv3 pass:
    rocprofv3 --kernel-trace --stats -d DIR -o eval -- python tools/bench_eval.py --profile-only

Per configuration (cart-RPODDPG, cart-RPOSAC, pendulum-RPODDPG: fused; EVOPF-RPODDPG: stepwise only) a trainer with
bench.py's hyper-parameters is trained for a few vector steps (a policy that has left its initialisation), then:
  * eval() wall time, evaluate(10) on both paths (`fused_eval` 1 / 0), median of --reps calls after one warm-up call;
  * the fused path at --sizes episodes: wall time, episodes/s, env-steps/s (the live steps the episodes took) and the
    actor's algorithmic f32 FLOP over those steps as a share of the 157.3 TFLOP/s f32 MFMA peak (a lower bound: the
    finished lanes of a live 16-lane tile still go through the MLP).
Every call ends with a host read of the results (evaluate()'s .cpu(), eval()'s), so wall times include the device work.
Run each GPU step under its own time limit (timeout -k 10 ...).
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

from bench import ROLLOUT_FLOP_PER_LANE, make_trainer  # noqa: E402

PEAK_F32_MFMA = 157.3e12
CONFIGS = [("cart_ddpg", True), ("cart_sac", True), ("pen_ddpg", True), ("evopf_ddpg", False)]


def timed(fn, reps):
    fn()                                                        # warm-up (allocations, first launches)
    ts, out = [], None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), out


def trainer(workload):
    tr = make_trainer(64 if not workload.startswith("evopf") else 16, torch.device("cuda"), max_epochs=1000,
                      capacity=64, workload=workload)
    tr.vec.reset()
    tr.run_steps(32)
    torch.cuda.synchronize()
    return tr


def evaluate_path(tr, fused, **kw):
    tr.schedule["fused_eval"] = int(fused)
    try:
        return tr.evaluate(**kw)
    finally:
        tr.schedule["fused_eval"] = 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="4096,65536,1048576")
    ap.add_argument("--profile-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sizes = [int(x) for x in a.sizes.split(",") if x]
    if a.profile_only:
        tr = trainer("cart_ddpg")
        for n in sizes:
            for _ in range(3):
                tr.evaluate(n, seed=7)
        torch.cuda.synchronize()
        print(json.dumps(dict(profile_only=True, sizes=sizes)))
        return
    line = dict(tool="bench_eval", device=torch.cuda.get_device_name(0), reps=a.reps, configs={})
    for workload, has_fused in CONFIGS:
        tr = trainer(workload)
        row = dict(horizon=None)
        t, res = timed(lambda: tr.eval(), a.reps)
        row["eval_s"] = t
        t, r = timed(lambda: evaluate_path(tr, False, episodes=10, seed=3), a.reps)
        row.update(horizon=r.horizon, evaluate10_stepwise_s=t, evaluate10_stepwise_env_steps=int(r.length.sum()))
        if has_fused:
            t, r = timed(lambda: evaluate_path(tr, True, episodes=10, seed=3), a.reps)
            assert r.path == "fused"
            row.update(evaluate10_fused_s=t, evaluate10_fused_env_steps=int(r.length.sum()),
                       speedup_vs_eval=row["eval_s"] / t)
            row["fused"] = {}
            flop = ROLLOUT_FLOP_PER_LANE + (2 * 256 if tr._gauss_policy else 0)    # (RPOSAC: the second head)
            for n in sizes:
                t, r = timed(lambda: tr.evaluate(n, seed=5), max(1, min(a.reps, 3)))
                steps = int(r.length.sum())
                row["fused"][str(n)] = dict(wall_s=t, episodes_per_s=n / t, env_steps=steps, env_steps_per_s=steps / t,
                                            mean_length=steps / n, violation_rate=r.violation_rate(),
                                            mfma_share_lower_bound=flop * steps / t / PEAK_F32_MFMA)
        line["configs"][workload] = row
        del tr
        torch.cuda.empty_cache()
    s = json.dumps(line)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
