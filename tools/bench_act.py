#!/usr/bin/env python
"""trainer.act() on one MI355X (GPU box): the fused launch against the stepwise path, and its forms against each other.

    python tools/bench_act.py [--reps R] [--out profiles/act_bench.json]

Per configuration (cart-RPODDPG, pendulum-RPOSAC; bench.py's hyper-parameters, a few vector steps of training) and per n
(1, 256, 4096, 65 536, 2^20 rows of recorded observations, repeated):
  * the legs ``stepwise`` (schedule fused_act=0) and ``fused`` (form 0: the library's size rule) -- and at 65 536 and 2^20 rows
    also ``tile`` (form 1), ``stream_g1`` (form 2) and ``stream_g4`` (form 3) -- are timed ALTERNATELY, --reps rounds after two
    warm-up rounds, every leg with ``out=`` (no allocation).  One sample is the device time of `inner` back-to-back calls
    between two events, divided by `inner` (small n: the time of a call is its launches' latency, so a sample spans many).
  * reported per leg: median, min and max in microseconds and the actor's algorithmic f32 FLOP (67 584 per row) as a share of
    the 157.3 TFLOP/s f32 MFMA peak.  A difference between two legs means something only beyond their min-max spreads.
Each configuration runs in a child process of its own under a time limit (``timeout -k 10``); the first failure ends the run.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_F32_MFMA = 157.3e12
FLOP_PER_ROW = 67584
CONFIGS = ["cart_ddpg", "pen_sac"]
SIZES = [1, 256, 4096, 65536, 1 << 20]
FORMS = [("tile", 1), ("stream_g1", 2), ("stream_g4", 3)]


def child(workload, reps):
    import torch
    from bench import make_trainer
    tr = make_trainer(64, torch.device("cuda"), max_epochs=1000, capacity=64, workload=workload)
    tr.vec.reset()
    tr.run_steps(32)
    t = tr.evaluate(256, seed=11, record=True).trajectory
    obs = torch.tensor(t.obs[t.valid], device=tr.device)
    rows = []
    for n in SIZES:
        x = obs.repeat((n + obs.shape[0] - 1) // obs.shape[0], 1)[:n].contiguous()
        legs = [("stepwise", None), ("fused", 0)] + (FORMS if n >= 65536 else [])
        outs = {name: None for name, _ in legs}
        inner = 50 if n <= 4096 else (8 if n <= 65536 else 2)

        def run(name, form):
            if form is None:
                tr.schedule["fused_act"] = 0
                outs[name] = tr.act(x, out=outs[name])
                tr.schedule["fused_act"] = 1
            else:
                outs[name] = tr.act(x, out=outs[name], form=form)
        samples = {name: [] for name, _ in legs}
        for rnd in range(reps + 2):
            for name, form in legs:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(inner):
                    run(name, form)
                e1.record()
                e1.synchronize()
                if rnd >= 2:
                    samples[name].append(e0.elapsed_time(e1) * 1e3 / inner)
        for name, _ in legs:
            s = samples[name]
            med = statistics.median(s)
            rows.append(dict(workload=workload, n=n, leg=name, path=outs[name].path, form=outs[name].form, inner=inner,
                             median_us=round(med, 3), min_us=round(min(s), 3), max_us=round(max(s), 3),
                             peak_share=round(n * FLOP_PER_ROW / (med * 1e-6) / PEAK_F32_MFMA, 4)))
    print("ACT_BENCH " + json.dumps(rows), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "act_bench.json"))
    ap.add_argument("--limit", type=int, default=240, help="seconds per configuration")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.reps)
    rows = []
    for w in CONFIGS:
        p = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", w,
                            "--reps", str(a.reps)], stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:                                    # (a fault, an abort, a time limit: nothing more is started)
            print(p.stdout[-2000:])
            sys.exit("bench_act: %s ended with status %d" % (w, p.returncode))
        rows += json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("ACT_BENCH ")][-1][len("ACT_BENCH "):])
    import torch
    res = dict(device=torch.cuda.get_device_name(0), reps=a.reps, flop_per_row=FLOP_PER_ROW, peak_f32_mfma=PEAK_F32_MFMA, rows=rows)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
