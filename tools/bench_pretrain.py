#!/usr/bin/env python
"""trainer.pretrain() on one MI355X (GPU box): what a cloning step costs, and what cloning the OPF controller gives.

    python tools/bench_pretrain.py [--reps R] [--steps S] [--lr LR] [--out profiles/pretrain_bench.json]

Timing -- the ``evopf256`` RPODDPG / RPOSAC and the cart RPODDPG configurations of tests/test_train_step_golden.py::build_trainer,
batch 256, 512 random demonstrations: microseconds per cloning step (gather, actor forward, head, actor backward, clip + Adam),
``eager`` (64 steps launched one by one) against ``graph`` (four replays of a captured 16-step window), timed ALTERNATELY by the
method of tools/bench_act.py: --reps rounds after two warm-up rounds, one sample = the device time of 64 steps between two
events / 64; median, min and max per leg.  A difference means something only beyond the min-max spreads.

Outcome -- ``evopf256`` RPODDPG at its initial weights: ``evaluate(1024, seed=0)`` return, violation rate and mean
``opf_gap(pe="free")`` before and after ``pretrain`` (--steps steps of batch 256 at --lr) on the demonstrations of
``evaluate_opf(1024, seed=1, record=True)``; the same after one DAgger round (label the pretrained policy's own recorded
observations with ``Demonstrations.label``, extend, pretrain again); and ``evaluate_opf(1024, seed=0)``'s own figures.  The
mean return is taken over the episodes without a non-finite step (``nonfinite_episodes`` counts the others: the OPF controller
steps the solver's last iterate in an infeasible hour).  No threshold is set on any of them: the JSON is where they are
written down.
Each part runs in a child process of its own under a time limit (``timeout -k 10``); the first failure ends the run.  Reads
nothing outside the tree.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

TIMING = ["ddpg:evopf256", "sac:evopf256", "ddpg:cart"]
BATCH, WINDOW, INNER = 256, 16, 64


def build(algo, envname, **kw):
    import torch
    from rpo_amd import ops
    from test_train_step_golden import build_trainer
    torch.manual_seed(123)
    return build_trainer(algo, envname, ops, torch.device("cuda"), num_envs=16, **kw)


def timing_child(config, reps):
    import numpy as np
    import torch
    from rpo_amd.algo import Demonstrations
    from rpo_amd.algo import pretrain as pt
    from rpo_amd.algo.trainer import _GraphCache
    algo, envname = config.split(":")
    tr = build(algo, envname, use_graph=True)
    k = tr.kernels
    rng = np.random.RandomState(0)
    lo, hi = tr.base_env.box_constraint_partial
    obs = rng.uniform(0.1, 0.8, (512, k.obs_dim)).astype(np.float32)
    tgt = (np.asarray(lo) + (np.asarray(hi) - np.asarray(lo)) * rng.uniform(0, 1, (512, k.partial_dim))).astype(np.float32)
    d = Demonstrations(obs, tgt)
    with torch.no_grad():
        run = pt.BCStep(tr, d.table(tr.device), BATCH, tr.agent.lr_actor, 1, None, 0.98, WINDOW)
        fl = tr.agent.flat
        fl.gradient(fl.actor_range).zero_()
        graphs = _GraphCache(True, warm=1)
        window = lambda: [run.step(i) for i in range(WINDOW)]                                  # noqa: E731
        legs = {"eager": lambda: [window() for _ in range(INNER // WINDOW)],
                "graph": lambda: [graphs.run(("bc", WINDOW), window) for _ in range(INNER // WINDOW)]}
        samples = {name: [] for name in legs}
        for rnd in range(reps + 2):
            for name, fn in legs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if rnd >= 2:
                    samples[name].append(e0.elapsed_time(e1) * 1e3 / INNER)
    assert graphs.entries[("bc", WINDOW)]["graph"] is not None and not graphs.capture_failed
    rows = [dict(config=config, leg=name, batch=BATCH, median_us=round(statistics.median(s), 3), min_us=round(min(s), 3),
                 max_us=round(max(s), 3)) for name, s in samples.items()]
    print("PRETRAIN_BENCH " + json.dumps(rows), flush=True)


def outcome_child(steps, lr):
    import numpy as np
    from rpo_amd.algo import Demonstrations
    tr = build("ddpg", "evopf256", use_graph=True)
    env = tr.base_env

    def figures(res, gap=True):
        ok = ~res.nonfinite                                      # (an infeasible hour steps the solver's last iterate: not finite)
        out = dict(ret_mean=float(res.ret[ok].mean()), nonfinite_episodes=int(res.nonfinite.sum()),
                   violation_rate=float(res.violation_rate()))
        if gap:
            g = res.trajectory.opf_gap(env, pe="free")
            out.update(opf_gap_free_mean=g.mean(), opf_converged_rate=g.converged_rate())
        return out

    rows = {}
    rows["before"] = figures(tr.evaluate(1024, seed=0, record=True))
    b = tr.evaluate_opf(1024, seed=1, record=True)
    d = Demonstrations.from_trajectory(b.trajectory, env, mask=b.opf_converged)
    r = tr.pretrain(d, steps=steps, batch_size=BATCH, lr=lr, seed=0)
    rows["pretrain"] = dict(rows=len(d), dropped=d.dropped, steps=steps, batch_size=BATCH, lr=r.lr,
                            loss_first20=float(r.loss[:20].mean()), loss_last20=float(r.loss[-20:].mean()))
    after = tr.evaluate(1024, seed=0, record=True)
    rows["after"] = figures(after)
    t = after.trajectory
    visited = t.obs[t.valid & np.isfinite(t.obs).all(axis=2)]
    lab = Demonstrations.label(env, visited)
    d.extend(lab)
    r = tr.pretrain(d, steps=steps, batch_size=BATCH, lr=lr, seed=1)
    rows["dagger"] = dict(labelled=len(lab), unlabelled=lab.dropped, rows=len(d), loss_first20=float(r.loss[:20].mean()),
                          loss_last20=float(r.loss[-20:].mean()))
    rows["after_dagger"] = figures(tr.evaluate(1024, seed=0, record=True))
    o = tr.evaluate_opf(1024, seed=0)
    rows["opf"] = dict(figures(o, gap=False), converged_rate=float(o.opf_converged.sum()) / float(o.length.sum()))
    print("PRETRAIN_BENCH " + json.dumps(rows), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pretrain_bench.json"))
    ap.add_argument("--limit", type=int, default=300, help="seconds per part")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child == "outcome":
        return outcome_child(a.steps, a.lr)
    if a.child:
        return timing_child(a.child, a.reps)
    parts = []
    for part in TIMING + ["outcome"]:
        p = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", part,
                            "--reps", str(a.reps), "--steps", str(a.steps), "--lr", str(a.lr)], stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:                                    # (a fault, an abort, a time limit: nothing more is started)
            print(p.stdout[-2000:])
            sys.exit("bench_pretrain: %s ended with status %d" % (part, p.returncode))
        parts.append(json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("PRETRAIN_BENCH ")][-1][len("PRETRAIN_BENCH "):]))
    import torch
    res = dict(device=torch.cuda.get_device_name(0), reps=a.reps, timing=[r for rows in parts[:-1] for r in rows], outcome=parts[-1])
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
