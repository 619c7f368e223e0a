#!/usr/bin/env python
"""The 3 x bf16 split-precision streaming forward (ops.tuning(fwd_bf16x3=1), csrc/mlp_stream_bf16x3.h) against the exact-f32
streaming forward on one MI355X (GPU box): time and error.

    python tools/bench_forward_bf16x3.py [--reps R] [--out profiles/fwd_bf16x3_bench.json]

Method of tools/bench_act.py: device events, every shape warmed up (two rounds), then --reps ALTERNATING rounds of switch 0 / 1
in one process; one sample is the device time of `inner` back-to-back calls divided by `inner`.  Legs, at 65 536 and 2^20 rows:
  * ``critic_save``: rpo_mlp_forward of a 6 + 2 -> 128 -> 256 -> 1 critic with x0 and h1 saved;
  * ``multi4``: rpo_mlp_forward_multi of 4 such target networks, nothing saved;
  * ``error``: h1 of both forms against float64 from the form's own x0 (RMS, max |err| / (|relu(x0)| |W0|^T + |b0|)): the figures of
    tests/test_forward_bf16x3_gpu.py's criterion (split <= 2 x exact);
and ``large_batch``: time per iteration of bench.py's large_batch configuration (RPODDPG, CartSafe-v0, 4096 lanes, one 2^20-row
batch per vector step, hipGraph windows), one trainer per setting, alternating.
Reported per leg: median / min / max in microseconds per setting and the ratio exact / split of the medians; for the exact
setting the algorithmic f32 FLOP as a share of the 157.3 TFLOP/s f32 MFMA peak (for the split setting the time alone: a share
of the f32 peak is not its name).  Each part runs in a child process of its own under a time limit; the first failure ends the run.
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_F32_MFMA = 157.3e12
S, A, E, H = 6, 2, 128, 256
FLOP_PER_ROW = 2 * (S + A) * E + 2 * E * H + 2 * H
SIZES = [65536, 1 << 20]


def _critic(torch, ops, seed):
    torch.manual_seed(seed)
    lin = {k: torch.nn.Linear(i, o) for k, (i, o) in dict(s=(S, E), a=(A, E), h=(E, H), o=(H, 1)).items()}
    t = {}
    for name, (k, attr) in dict(Ws=("s", "weight"), bs=("s", "bias"), Wa=("a", "weight"), ba=("a", "bias"), W0=("h", "weight"),
                                b0=("h", "bias"), W1=("o", "weight"), b1=("o", "bias")).items():
        t[name] = getattr(lin[k], attr).detach().to("cuda").contiguous()
    return ops.MlpDesc(t, S, A, E, H, 1, False), t


def _timed(torch, legs, reps, inner):
    """legs: {name: callable}; alternating rounds -> {name: [us per call]}"""
    samples = {name: [] for name in legs}
    for rnd in range(reps + 2):
        for name, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            e1.synchronize()
            if rnd >= 2:
                samples[name].append(e0.elapsed_time(e1) * 1e3 / inner)
    return samples


def _row(leg, n, samples, flop):
    med = {k: statistics.median(v) for k, v in samples.items()}
    row = dict(leg=leg, n=n, ratio_exact_over_split=round(med["exact"] / med["split"], 4),
               exact_peak_share=None if flop is None else round(flop / (med["exact"] * 1e-6) / PEAK_F32_MFMA, 4))
    for k, v in samples.items():
        row[k] = dict(median_us=round(med[k], 2), min_us=round(min(v), 2), max_us=round(max(v), 2))
    return row


def child_forward(reps):
    import torch
    from rpo_amd import ops
    nets = [_critic(torch, ops, 20 + k) for k in range(4)]
    rows = []
    for n in SIZES:
        g = torch.Generator(device="cuda").manual_seed(n)
        wide = torch.randn(n, S + A + 3, device="cuda", generator=g)
        s, a = wide[:, 1:1 + S], wide[:, 1 + S:1 + S + A]
        out, x0, h1 = (torch.empty(n, w, device="cuda") for w in (1, E, H))
        outs = [torch.empty(n, 1, device="cuda") for _ in range(4)]
        desc, t = nets[0]

        def one(split):
            with ops.tuning(fwd_bf16x3=split):
                ops.mlp_forward(desc, s, a, out, x0, h1)

        def multi(split):
            with ops.tuning(fwd_bf16x3=split):
                ops.mlp_forward_multi([(nets[k][0], s, a, outs[k], None, None) for k in range(4)])
        inner = 8 if n <= 65536 else 2
        rows.append(_row("critic_save", n, _timed(torch, dict(exact=lambda: one(0), split=lambda: one(1)), reps, inner),
                         n * FLOP_PER_ROW))
        rows.append(_row("multi4", n, _timed(torch, dict(exact=lambda: multi(0), split=lambda: multi(1)), reps, inner),
                         4 * n * FLOP_PER_ROW))
        err = dict(leg="error", n=n, u=2.0 ** -24)
        W0, b0 = t["W0"].double(), t["b0"].double()
        for name, split in (("exact", 0), ("split", 1)):
            one(split)
            torch.cuda.synchronize()
            rms2, worst = 0.0, 0.0
            for lo in range(0, n, 1 << 17):                      # (float64 in slabs)
                r = x0[lo:lo + (1 << 17)].double().clamp_min(0.0)
                e = (h1[lo:lo + (1 << 17)].double() - (r @ W0.t() + b0)).abs()
                rms2 += float((e * e).sum())
                worst = max(worst, float((e / (r @ W0.abs().t() + b0.abs())).max()))
            err[name] = dict(rms=math.sqrt(rms2 / (n * H)), max_over_absab=worst)
        rows.append(err)
    print("BF16X3_BENCH " + json.dumps(rows), flush=True)


def child_trainer(reps):
    import torch
    from bench import make_trainer
    from rpo_amd import ops
    lanes, steps = 4096, 8
    trs = {}
    for name, split in (("exact", 0), ("split", 1)):
        with ops.tuning(fwd_bf16x3=split):                      # (read at launch: the windows captured here keep the setting)
            torch.manual_seed(5)
            trs[name] = make_trainer(lanes, torch.device("cuda"), 10 ** 9, capacity=64, workload="cart_ddpg", batch_size=256 * lanes)
            trs[name].vec.reset()
            trs[name].run_steps(32)
    torch.cuda.synchronize()

    def run(name, split):
        with ops.tuning(fwd_bf16x3=split):
            trs[name].run_steps(steps)
    samples = _timed(torch, dict(exact=lambda: run("exact", 0), split=lambda: run("split", 1)), reps, 1)
    samples = {k: [x / steps for x in v] for k, v in samples.items()}
    for tr in trs.values():
        tr._harvest(final=True)
    row = _row("large_batch", 256 * lanes, samples, None)
    row["unit"] = "us per iteration (one vector step of %d lanes + one update on %d rows)" % (lanes, 256 * lanes)
    print("BF16X3_BENCH " + json.dumps([row]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fwd_bf16x3_bench.json"))
    ap.add_argument("--limit", type=int, default=240, help="seconds per part")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        return dict(forward=child_forward, trainer=child_trainer)[a.child](a.reps)
    rows = []
    for part in ("forward", "trainer"):
        p = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", part,
                            "--reps", str(a.reps)], stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:                                    # (a fault, an abort, a time limit: nothing more is started)
            print(p.stdout[-2000:])
            sys.exit("bench_forward_bf16x3: %s ended with status %d" % (part, p.returncode))
        rows += json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("BF16X3_BENCH ")][-1][len("BF16X3_BENCH "):])
    import torch
    res = dict(device=torch.cuda.get_device_name(0), reps=a.reps, flop_per_row=FLOP_PER_ROW, peak_f32_mfma=PEAK_F32_MFMA, rows=rows)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
