#!/usr/bin/env python
"""trainer.evaluate() vs eval() on one MI355X (GPU box); prints ONE JSON line.

    python tools/bench_eval.py [--reps R] [--sizes 4096,65536,1048576] [--out FILE]
    python tools/bench_eval.py --profile-only [--sizes 65536]     # fused evaluations only, for a rocprofv3 pass:
    rocprofv3 --kernel-trace --stats -d DIR -o eval -- python tools/bench_eval.py --profile-only
    python tools/bench_eval.py --record [--reps R] [--sizes 10,1024,65536] [--out profiles/eval_record_bench.json]
    python tools/bench_eval.py --constraints [--reps R] [--sizes 10,1024,65536] [--out profiles/eval_constraints_bench.json]
    python tools/bench_eval.py --obs-noise [--reps R] [--sizes 10,1024,65536] [--out profiles/eval_noise_bench.json]
    python tools/bench_eval.py --budgets [--reps R] [--sizes 10,1024,65536] [--out profiles/eval_budgets_bench.json]
    python tools/bench_eval.py --policies [--reps R] [--sizes 10,1024,65536] [--out profiles/eval_policies_bench.json]
    python tools/bench_eval.py --noise-sweep [--reps R] [--sizes 10,1024,65536] [--out profiles/eval_noise_sweep_bench.json]

Per configuration (cart-RPODDPG, cart-RPOSAC, pendulum-RPODDPG: fused; EVOPF-RPODDPG: stepwise only) a trainer with
bench.py's hyper-parameters is trained for a few vector steps (a policy that has left its initialisation), then:
  * eval() wall time, evaluate(10) on both paths (`fused_eval` 1 / 0), median of --reps calls after one warm-up call;
  * the fused path at --sizes episodes: wall time, episodes/s, env-steps/s (the live steps the episodes took) and the
    actor's algorithmic f32 FLOP over those steps as a share of the 157.3 TFLOP/s f32 MFMA peak (a lower bound: the
    finished lanes of a live 16-lane tile still go through the MLP).
--record: the cost of evaluate(record=...) (the per-step trajectory).  Fused cart-RPODDPG and pendulum-RPODDPG at --sizes
episodes, stepwise EVOPF-RPODDPG at 10 and 1024: the legs record=False / record=64 / record=True are timed ALTERNATELY, --reps
rounds after one warm-up round, and reported as medians with the min-max spread of each leg (a leg's cost over record=False
means something only beyond that spread).  A record=True leg includes the read-back and the numpy views of the trace.
--constraints: the cost of evaluate(constraints=True) (the per-constraint report), by the same method.  Fused cart-RPODDPG at
--sizes episodes, stepwise EVOPF-RPODDPG at 10 and 1024: the legs constraints=False / constraints=True (and, on the fused path,
record=True for comparison) alternate; per size the ratio of the medians constraints=True / constraints=False is reported next
to the two legs' own min-max spreads.
--obs-noise: the cost of evaluate(obs_noise=sigma) (sensor noise drawn inside the kernel), by the same method.  Fused
cart-RPODDPG and pendulum-RPOSAC at --sizes episodes, stepwise EVOPF-RPODDPG at 10 and 1024: the legs obs_noise=None /
obs_noise=sigma of ONE build alternate (sigma 0.05; EVOPF-v0 1e-3); the ratio of the medians is reported next to the legs' own
spreads.  A noisy policy takes other episodes than a clean one, so every leg also reports the env steps it took and its time
per env step.
--budgets: ONE evaluate_budgets() call with B = 8 budgets (eval_steps 0..7 at the trainer's eval_lr) against the 8 evaluate()
calls it is defined by, in ONE build, by the same method (alternating rounds, medians and min-max spreads of the whole call's
wall time, read-backs included).  Fused cart-RPODDPG and pendulum-RPOSAC at --sizes episodes, stepwise EVOPF-RPODDPG at 10
(where evaluate_budgets() runs those 8 calls itself: the ratio there measures only its bookkeeping).  Reported per size: the two
legs, the ratio sweep / eight calls, and the sweep against ONE evaluate() call at the largest budget (the claim to test:
about one call's time while B x episodes lanes do not fill the chip).
--policies: ONE evaluate_policies() call with P = 8 distinct actor spans (the live actor and 7 seeded perturbations of it)
against the 8 evaluate() calls under using_policy() it is defined by and against ONE plain evaluate(), in ONE build, by the same
method.  Fused cart-RPODDPG and pendulum-RPOSAC at --sizes episodes.  Reported per size: the three legs, the ratios sweep / eight
calls and sweep / one call, and the padded lanes of the launch.
--noise-sweep: ONE evaluate_noise() call with S = 8 noise levels (0, 0.005, 0.01, 0.02, 0.05, 0.1, 0.2 and a per-column vector;
EVOPF-v0: a thousandth of them) against the 8 evaluate(obs_noise=) calls it is defined by and against ONE such call (sigma
0.05), in ONE build, by the same method.  Fused cart-RPODDPG and pendulum-RPOSAC at --sizes episodes, stepwise EVOPF-RPODDPG at
10 (where evaluate_noise() runs those 8 calls itself: the ratio there measures only its bookkeeping).  Reported per size: the
three legs, the ratios sweep / eight calls and sweep / one call, and the padded lanes of the launch.
--evopf-fused: evaluate() on EVOPF-v0 under schedule fused_eval_evopf=1 (rpo_evopf_evaluate) against the stepwise path of the
same build, whose kernels are the ones from before that switch existed: EVOPF-RPODDPG and EVOPF-RPOSAC after 32 training steps,
at 10, 1024 and 16384 episodes (--sizes), the two legs alternating, medians and min-max spreads of the whole call's wall time,
the time per env step of a lane (the call over its horizon) and whether fused is faster by more than both legs' spreads; the
two legs must return the same bits.  --out profiles/eval_evopf_fused_bench.json.
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
from rpo_amd import ops  # noqa: E402

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


def alternating(legs, reps):
    """legs: {name: fn}; one warm-up round, then `reps` rounds of every leg in turn -> {name: dict(median_s, min_s, max_s)}."""
    ts = {k: [] for k in legs}
    for rnd in range(reps + 1):
        for k, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rnd:
                ts[k].append(time.perf_counter() - t0)
    return {k: dict(median_s=statistics.median(v), min_s=min(v), max_s=max(v)) for k, v in ts.items()}


def record_bench(a, sizes):
    line = dict(tool="bench_eval --record", device=torch.cuda.get_device_name(0), reps=a.reps, configs={})
    for workload, has_fused in (("cart_ddpg", True), ("pen_ddpg", True), ("evopf_ddpg", False)):
        tr = trainer(workload)
        row = {}
        for n in (sizes if has_fused else [10, 1024]):
            legs = {"record_false": lambda: tr.evaluate(n, seed=5)}
            if n > 64:
                legs["record_64"] = lambda: tr.evaluate(n, seed=5, record=64)
            legs["record_true"] = lambda: tr.evaluate(n, seed=5, record=True)
            res = alternating(legs, a.reps)
            r = tr.evaluate(n, seed=5, record=True)
            assert r.path == ("fused" if has_fused else "stepwise")
            base = res["record_false"]["median_s"]
            for k in res:
                res[k]["over_record_false_s"] = res[k]["median_s"] - base
            tj = r.trajectory
            width = ops.trace_layout(tj.obs.shape[2], tj.proposal.shape[2], tj.action.shape[2])[1]
            res.update(horizon=r.horizon, env_steps=int(r.length.sum()), path=r.path, trace_bytes_record_true=4 * r.horizon * n * width)
            row[str(n)] = res
            del r, tj
        line["configs"][workload] = row
        del tr
        torch.cuda.empty_cache()
    return line


def constraints_bench(a, sizes):
    line = dict(tool="bench_eval --constraints", device=torch.cuda.get_device_name(0), reps=a.reps, configs={})
    for workload, has_fused in (("cart_ddpg", True), ("evopf_ddpg", False)):
        tr = trainer(workload)
        row = {}
        for n in (sizes if has_fused else [10, 1024]):
            legs = {"constraints_false": lambda: tr.evaluate(n, seed=5),
                    "constraints_true": lambda: tr.evaluate(n, seed=5, constraints=True)}
            if has_fused:
                legs["record_true"] = lambda: tr.evaluate(n, seed=5, record=True)
            res = alternating(legs, a.reps)
            r = tr.evaluate(n, seed=5, constraints=True)
            assert r.path == ("fused" if has_fused else "stepwise")
            base = res["constraints_false"]["median_s"]
            for k in list(res):
                res[k]["ratio_to_constraints_false"] = res[k]["median_s"] / base
            k = tr.kernels
            res.update(horizon=r.horizon, env_steps=int(r.length.sum()), path=r.path,
                       report_bytes=4 * n * ops.con_width(k.ineq_num, k.eq_num))
            row[str(n)] = res
            del r
        line["configs"][workload] = row
        del tr
        torch.cuda.empty_cache()
    return line


def noise_bench(a, sizes):
    line = dict(tool="bench_eval --obs-noise", device=torch.cuda.get_device_name(0), reps=a.reps, configs={})
    for workload, has_fused in (("cart_ddpg", True), ("pen_sac", True), ("evopf_ddpg", False)):
        tr = trainer(workload)
        sigma = 0.05 if has_fused else 1e-3
        row = {}
        for n in (sizes if has_fused else [10, 1024]):
            legs = {"obs_noise_none": lambda: tr.evaluate(n, seed=5, obs_noise=None),
                    "obs_noise_sigma": lambda: tr.evaluate(n, seed=5, obs_noise=sigma)}
            res = alternating(legs, a.reps)
            base = res["obs_noise_none"]["median_s"]
            for k, fn in legs.items():
                r = fn()
                assert r.path == ("fused" if has_fused else "stepwise") and (r.obs_noise is None) == (k == "obs_noise_none")
                steps = int(r.length.sum())
                res[k].update(ratio_to_obs_noise_none=res[k]["median_s"] / base, env_steps=steps,
                              s_per_env_step=res[k]["median_s"] / steps, violation_rate=r.violation_rate())
            res.update(horizon=r.horizon, path=r.path, sigma=sigma)
            row[str(n)] = res
            del r
        line["configs"][workload] = row
        del tr
        torch.cuda.empty_cache()
    return line


def budgets_bench(a, sizes):
    line = dict(tool="bench_eval --budgets", device=torch.cuda.get_device_name(0), reps=a.reps, configs={})
    budgets = list(range(8))
    for workload, has_fused in (("cart_ddpg", True), ("pen_sac", True), ("evopf_ddpg", False)):
        tr = trainer(workload)
        row = {}
        for n in (sizes if has_fused else [10]):
            legs = {"evaluate_budgets": lambda: tr.evaluate_budgets(n, eval_steps=budgets, seed=5),
                    "eight_evaluate_calls": lambda: [tr.evaluate(n, seed=5, eval_steps=b, eval_lr=tr.eval_lr) for b in budgets],
                    "one_evaluate_call": lambda: tr.evaluate(n, seed=5, eval_steps=budgets[-1], eval_lr=tr.eval_lr)}
            res = alternating(legs, a.reps)
            s, calls = legs["evaluate_budgets"](), legs["eight_evaluate_calls"]()
            assert s.path == ("fused" if has_fused else "sweep")
            for g, r in enumerate(calls):                        # faster and different is not faster: the same bits
                assert all(getattr(s[g], f).tobytes() == getattr(r, f).tobytes() for f in r.FIELDS), (workload, n, g)
            res.update(ratio_to_eight_calls=res["evaluate_budgets"]["median_s"] / res["eight_evaluate_calls"]["median_s"],
                       ratio_to_one_call=res["evaluate_budgets"]["median_s"] / res["one_evaluate_call"]["median_s"],
                       budgets=budgets, lanes=len(budgets) * n, horizon=s.horizon, path=s.path, env_steps=int(s.length.sum()),
                       violation_rate=s.violation_rate().tolist())
            row[str(n)] = res
            del s, calls
        line["configs"][workload] = row
        del tr
        torch.cuda.empty_cache()
    return line


def policies_bench(a, sizes):
    line = dict(tool="bench_eval --policies", device=torch.cuda.get_device_name(0), reps=a.reps, configs={})
    for workload in ("cart_ddpg", "pen_sac"):
        tr = trainer(workload)
        live = tr.policy_params()
        gen = torch.Generator(device="cpu").manual_seed(7)
        policies = [None] + [live * (1.0 + 0.05 * torch.randn(live.numel(), generator=gen).to(live.device)) for _ in range(7)]
        row = {}
        for n in sizes:
            def eight():
                out = []
                for p in policies:
                    with tr.using_policy(p):
                        out.append(tr.evaluate(n, seed=5))
                return out
            legs = {"evaluate_policies": lambda: tr.evaluate_policies(policies, n, seed=5),
                    "eight_evaluate_calls": eight,
                    "one_evaluate_call": lambda: tr.evaluate(n, seed=5)}
            res = alternating(legs, a.reps)
            s, calls = legs["evaluate_policies"](), eight()
            assert s.path == "fused"
            for g, r in enumerate(calls):                        # faster and different is not faster: the same bits
                assert all(getattr(s[g], f).tobytes() == getattr(r, f).tobytes() for f in r.FIELDS), (workload, n, g)
            res.update(ratio_to_eight_calls=res["evaluate_policies"]["median_s"] / res["eight_evaluate_calls"]["median_s"],
                       ratio_to_one_call=res["evaluate_policies"]["median_s"] / res["one_evaluate_call"]["median_s"],
                       policies=len(policies), lanes=len(policies) * ((n + 63) // 64 * 64), horizon=s.horizon, path=s.path,
                       env_steps=int(s.length.sum()), violation_rate=s.violation_rate().tolist(),
                       ret_mean=s.ret_mean().tolist())
            row[str(n)] = res
            del s, calls
        line["configs"][workload] = row
        del tr
        torch.cuda.empty_cache()
    return line


def noise_sweep_bench(a, sizes):
    line = dict(tool="bench_eval --noise-sweep", device=torch.cuda.get_device_name(0), reps=a.reps, configs={})
    for workload, has_fused in (("cart_ddpg", True), ("pen_sac", True), ("evopf_ddpg", False)):
        tr = trainer(workload)
        unit = 1.0 if has_fused else 1e-3
        O = tr.kernels.obs_dim
        levels = [unit * x for x in (0.0, 0.005, 0.01, 0.02, 0.05, 0.1, 0.2)] + [[unit * 0.05 * (q % 2) for q in range(O)]]
        row = {}
        for n in (sizes if has_fused else [10]):
            legs = {"evaluate_noise": lambda: tr.evaluate_noise(n, obs_noise=levels, seed=5),
                    "eight_evaluate_calls": lambda: [tr.evaluate(n, seed=5, obs_noise=lv) for lv in levels],
                    "one_evaluate_call": lambda: tr.evaluate(n, seed=5, obs_noise=levels[4])}
            res = alternating(legs, a.reps)
            s, calls = legs["evaluate_noise"](), legs["eight_evaluate_calls"]()
            assert s.path == ("fused" if has_fused else "sweep")
            for g, r in enumerate(calls):                        # faster and different is not faster: the same bits
                assert all(getattr(s[g], f).tobytes() == getattr(r, f).tobytes() for f in r.FIELDS), (workload, n, g)
            res.update(ratio_to_eight_calls=res["evaluate_noise"]["median_s"] / res["eight_evaluate_calls"]["median_s"],
                       ratio_to_one_call=res["evaluate_noise"]["median_s"] / res["one_evaluate_call"]["median_s"],
                       levels=s.levels.tolist(), lanes=len(levels) * ((n + 63) // 64 * 64), horizon=s.horizon, path=s.path,
                       env_steps=int(s.length.sum()), violation_rate=s.violation_rate().tolist(), ret_mean=s.ret_mean().tolist(),
                       tolerance=s.tolerance())
            row[str(n)] = res
            del s, calls
        line["configs"][workload] = row
        del tr
        torch.cuda.empty_cache()
    return line


def evopf_fused_bench(a, sizes):
    line = dict(tool="bench_eval --evopf-fused", device=torch.cuda.get_device_name(0), reps=a.reps,
                lane_steps_per_launch=ops.EVOPF_EVAL_LANE_STEPS, configs={})

    def leg(tr, on, n):
        tr.schedule["fused_eval_evopf"] = on
        try:
            return tr.evaluate(n, seed=5)
        finally:
            tr.schedule["fused_eval_evopf"] = 0
    for workload in ("evopf_ddpg", "evopf_sac"):
        tr = trainer(workload)
        row = {}
        for n in sizes:
            legs = {"fused": lambda: leg(tr, 1, n), "stepwise": lambda: leg(tr, 0, n)}
            res = alternating(legs, a.reps)
            f, s = legs["fused"](), legs["stepwise"]()
            assert f.path == "fused" and s.path == "stepwise"
            assert all(getattr(f, k).tobytes() == getattr(s, k).tobytes() for k in f.FIELDS), (workload, n)   # the same bits
            steps = int(f.length.sum())
            for k in res:
                res[k]["s_per_env_step_of_a_lane"] = res[k]["median_s"] / f.horizon      # the call over its 24 serial steps
            spread = max(res["fused"]["max_s"] - res["fused"]["min_s"], res["stepwise"]["max_s"] - res["stepwise"]["min_s"])
            res.update(ratio_fused_to_stepwise=res["fused"]["median_s"] / res["stepwise"]["median_s"],
                       faster_beyond_spreads=bool(res["stepwise"]["median_s"] - res["fused"]["median_s"] > spread),
                       horizon=f.horizon, env_steps=steps, launches=-(-f.horizon // max(1, min(f.horizon, ops.EVOPF_EVAL_LANE_STEPS // n))))
            row[str(n)] = res
            del f, s
        line["configs"][workload] = row
        del tr
        torch.cuda.empty_cache()
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="4096,65536,1048576")
    ap.add_argument("--profile-only", action="store_true")
    ap.add_argument("--record", action="store_true")
    ap.add_argument("--constraints", action="store_true")
    ap.add_argument("--obs-noise", action="store_true")
    ap.add_argument("--budgets", action="store_true")
    ap.add_argument("--policies", action="store_true")
    ap.add_argument("--noise-sweep", action="store_true")
    ap.add_argument("--evopf-fused", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sizes = [int(x) for x in a.sizes.split(",") if x]
    if a.evopf_fused:
        s = json.dumps(evopf_fused_bench(a, [10, 1024, 16384] if a.sizes == ap.get_default("sizes") else sizes))
        print(s)
        if a.out:
            with open(a.out, "w") as f:
                f.write(s + "\n")
        return
    if a.record or a.constraints or a.obs_noise or a.budgets or a.policies or a.noise_sweep:
        small = [10, 1024, 65536] if a.sizes == ap.get_default("sizes") else sizes
        bench = noise_sweep_bench if a.noise_sweep else policies_bench if a.policies else budgets_bench if a.budgets else noise_bench if a.obs_noise else (constraints_bench if a.constraints else record_bench)
        s = json.dumps(bench(a, small))
        print(s)
        if a.out:
            with open(a.out, "w") as f:
                f.write(s + "\n")
        return
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
