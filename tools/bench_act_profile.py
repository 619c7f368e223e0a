#!/usr/bin/env python
"""trainer.act(obs, profile=True) on one MI355X (GPU box): one profiled call against the K + 1 plain calls it replaces and against
one plain call at the budget K.

    python tools/bench_act_profile.py [--reps R] [--out profiles/act_profile_bench.json]

The method is tools/bench_act.py's.  Per configuration (cart-RPODDPG, pendulum-RPOSAC; bench.py's hyper-parameters, a few vector
steps of training), per n (4 096 and 65 536 rows of recorded observations, repeated) and per budget K (10 and 50):
  * the legs ``profile`` (one ``act(profile=True, eval_steps=K)``: the fused row-tile launch), ``sweep`` (the K + 1 calls
    ``act(eval_steps=b, form=1)``, b = 0..K) and ``plain`` (one ``act(eval_steps=K, form=1)``) are timed ALTERNATELY, --reps rounds
    after two warm-up rounds, every leg with ``out=`` (no allocation).  One sample is the device time of `inner` back-to-back
    repetitions of the leg between two events, divided by `inner`.
  * reported per leg: median, min and max in microseconds; for ``profile`` also the ratios sweep / profile and profile / plain
    and the profile's 16 (K + 1) n bytes of stores as a share of the 6.29 TB/s achievable HBM bandwidth (the store roofline).
    A difference between two legs means something only beyond their min-max spreads.
Each configuration runs in a child process of its own under a time limit (``timeout -k 10``); the first failure ends the run.

    python tools/bench_act_profile.py --evopf [--reps R] [--out profiles/act_profile_evopf_bench.json]

The EVOPF-v0 leg (EVOPF-RPODDPG, EVOPF-RPOSAC with bench.py's hyper-parameters: the 256-wide networks, policies after 32 vector
steps of training on 16 lanes), per n (4, 1 024 and 4 096 rows of recorded observations, repeated) and per budget K (10 and 50),
the same method: ``profile`` = one ``act(profile=True, eval_steps=K)`` under schedule ``profile_evopf=1`` (the proposal launches +
``rpo_evopf_project_profile`` + the residual kernel), ``sweep`` = the same call under ``profile_evopf=0`` (K + 1 stepwise
``act()`` calls: the kernels every earlier version ran, so the baseline) and ``plain`` = one ``act(eval_steps=K)``.  The two
profiles are compared bit for bit before anything is timed.  Reported besides the legs: sweep / profile and profile / plain.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_ACHIEVABLE = 6.29e12
CONFIGS = ["cart_ddpg", "pen_sac"]
SIZES = [4096, 65536]
BUDGETS = [10, 50]
EVOPF_CONFIGS = ["evopf_ddpg", "evopf_sac"]
EVOPF_SIZES = [4, 1024, 4096]


def child(workload, reps):
    import torch
    from bench import make_trainer
    evopf = workload.startswith("evopf")
    tr = make_trainer(16 if evopf else 64, torch.device("cuda"), max_epochs=1000, capacity=64, workload=workload)
    tr.vec.reset()
    tr.run_steps(32)
    t = tr.evaluate(16 if evopf else 256, seed=11, record=True).trajectory
    obs = torch.tensor(t.obs[t.valid], device=tr.device)
    rows = []
    for n in (EVOPF_SIZES if evopf else SIZES):
        x = obs.repeat((n + obs.shape[0] - 1) // obs.shape[0], 1)[:n].contiguous()
        for K in BUDGETS:
            outs = dict(profile=None, sweep=None, plain=None)
            inner = 10 if n <= 4096 else 4
            inners = dict(profile=inner, sweep=inner, plain=inner)
            if evopf:                                            # (a sweep at K = 50 is 51 calls of up to 50 GRG iterations)
                inners = dict(profile=8, sweep=1, plain=8)
                tr.schedule["profile_evopf"] = 1
                one = tr.act(x, profile=True, eval_steps=K)
                tr.schedule["profile_evopf"] = 0
                swept = tr.act(x, profile=True, eval_steps=K)
                assert one.path == "stepwise" and swept.path == "sweep"
                assert torch.equal(one.profile.data, swept.profile.data) and torch.equal(one.iters, swept.iters)   # the same bits
                del one, swept

            def run(name):
                if evopf:
                    tr.schedule["profile_evopf"] = int(name == "profile")
                    if name == "plain":
                        outs[name] = tr.act(x, eval_steps=K, out=outs[name])
                    else:
                        outs[name] = tr.act(x, profile=True, eval_steps=K, out=outs[name])
                elif name == "profile":
                    outs[name] = tr.act(x, profile=True, eval_steps=K, out=outs[name])
                elif name == "plain":
                    outs[name] = tr.act(x, eval_steps=K, form=1, out=outs[name])
                else:
                    for b in range(K + 1):
                        outs[name] = tr.act(x, eval_steps=b, form=1, out=outs[name])
            samples = {name: [] for name in outs}
            for rnd in range(reps + 2):
                for name in outs:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(inners[name]):
                        run(name)
                    e1.record()
                    e1.synchronize()
                    if rnd >= 2:
                        samples[name].append(e0.elapsed_time(e1) * 1e3 / inners[name])
            med = {name: statistics.median(s) for name, s in samples.items()}
            iters = outs["profile"].iters.float()
            for name, s in samples.items():
                row = dict(workload=workload, n=n, K=K, leg=name, path=outs[name].path, inner=inners[name], median_us=round(med[name], 3),
                           min_us=round(min(s), 3), max_us=round(max(s), 3))
                if name == "profile":
                    nbytes = 16 * (K + 1) * n
                    row.update(sweep_over_profile=round(med["sweep"] / med[name], 3), profile_over_plain=round(med[name] / med["plain"], 3),
                               profile_bytes=nbytes, store_roofline_share=round(nbytes / (med[name] * 1e-6) / HBM_ACHIEVABLE, 4),
                               iters_mean=round(float(iters.mean()), 3), iters_max=int(iters.max()))
                rows.append(row)
    print("ACT_PROFILE_BENCH " + json.dumps(rows), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--evopf", action="store_true", help="the EVOPF-v0 leg (schedule profile_evopf) instead of the classic-control one")
    ap.add_argument("--out", default=None, help="default: profiles/act_profile_bench.json, profiles/act_profile_evopf_bench.json with --evopf")
    ap.add_argument("--limit", type=int, default=240, help="seconds per configuration")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.reps)
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "act_profile_evopf_bench.json" if a.evopf else "act_profile_bench.json")
    rows = []
    for w in (EVOPF_CONFIGS if a.evopf else CONFIGS):
        p = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", w,
                            "--reps", str(a.reps)], stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:                                    # (a fault, an abort, a time limit: nothing more is started)
            print(p.stdout[-2000:])
            sys.exit("bench_act_profile: %s ended with status %d" % (w, p.returncode))
        tag = "ACT_PROFILE_BENCH "
        rows += json.loads([ln for ln in p.stdout.splitlines() if ln.startswith(tag)][-1][len(tag):])
        print("bench_act_profile: %s done" % w, file=sys.stderr, flush=True)
    import torch
    res = dict(device=torch.cuda.get_device_name(0), reps=a.reps, hbm_achievable=HBM_ACHIEVABLE, rows=rows)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
