#!/usr/bin/env python
"""The device AC-OPF solver of EVOPF-v0 (``EVOPFEnv.opf``, rpo_evopf_opf) on one MI355X (GPU box): what it computes on the
fixture's states, states per second, and what ``opf_gap`` costs next to the ``evaluate()`` that produced its trajectory.

    python tools/bench_opf.py [--reps R] [--out profiles/opf_bench.json]
    python tools/bench_opf.py --free [--reps R] [--out profiles/opf_free_bench.json]

* ``accuracy``: all 384 states of tests/golden/evopf_opf.npz against the float64 helper tests/evopf_opf_f64.py: the converged
  share, the iteration histogram, the largest |cost - helper's cost|, the largest float64 infeasibility of the returned points
  (and of the helper's own), the largest |returned cost - float64 obj_fn of the returned point|.
* ``throughput``: n = 4, 1 024 and 16 384 states (the fixture's, repeated), the three sizes timed ALTERNATELY, --reps rounds after
  two warm-up rounds, with ``out=`` (no allocation).  One sample is the device time of `inner` back-to-back calls between two
  events, divided by `inner`; reported: median, min, max in microseconds and states per second at the median.
* ``gap``: EVOPF-RPODDPG with bench.py's hyper-parameters after 32 vector steps on 16 lanes; ``evaluate(1024, record=True)`` and
  ``trajectory.opf_gap(env)`` on its 1 024-episode trajectory, timed alternately as wall clock around a device synchronisation
  (both include their host work and copies); the gap's mean, median and converged share.
* ``comparator``: there is no earlier version of this capability.  Where scipy is importable, SLSQP (float64) on the first
  --slsqp states of the fixture, on the CPU of the box this runs on; otherwise the time recorded in the fixture by the machine
  that made it, which is another machine.
``--free``: the free-pe instance (``EVOPFEnv.opf(pe="free")``, rpo_evopf_opf_free) next to the fixed-pe one, re-measured in the same
run (``fixed_pe_before`` repeats the committed profiles/opf_bench.json for reference):
* ``accuracy``: all 384 observations of tests/golden/evopf_opf_free.npz against the float64 helper tests/evopf_opf_free_f64.py: the
  converged split against the helper's and SLSQP's classes, the iteration histograms, the largest |objective - helper's| and
  |objective - SLSQP's|, the largest float64 infeasibility over the 58 bounds and the equations, the share of pe at a bound.
* ``throughput``: n = 4, 1 024 and 16 384 states, the free and the fixed-pe kernel (the same demands, the fixture's pe) and the three
  sizes timed ALTERNATELY as above; per size the two medians, their ratio and both kernels' mean iteration counts.
* ``evaluate_opf``: ``evaluate_opf(1024)`` and ``evaluate(1024)`` on the same seed, timed alternately as wall clock around a device
  synchronisation; the converged share and the two mean returns.
No threshold: the figures are reported as they come out.  The work runs in a child process under a time limit (``timeout -k 10``).
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = [4, 1024, 16384]
GOLDEN = os.path.join(ROOT, "tests", "golden", "evopf_opf.npz")
GOLDEN_FREE = os.path.join(ROOT, "tests", "golden", "evopf_opf_free.npz")


def child(reps, n_slsqp):
    import numpy as np
    import torch
    import evopf_opf_f64 as opf64
    from bench import make_trainer
    from oracle import evopf as ev
    dev = torch.device("cuda")
    tr = make_trainer(16, dev, max_epochs=1000, capacity=64, workload="evopf_ddpg")
    env = tr.base_env
    with np.load(GOLDEN) as z:
        z = {k: z[k] for k in z.files}
    demand, pe = torch.tensor(z["demand"], dtype=torch.float32, device=dev), torch.tensor(z["pe"], dtype=torch.float32, device=dev)
    # ---- accuracy on the 384 states
    got = env.opf(demand, pe=pe).numpy()
    d64, pe64 = demand.cpu().numpy().astype(np.float64), pe.cpu().numpy().astype(np.float64)
    ref = opf64.solve_many(d64, pe64)
    both = got["converged"] & ref["converged"]
    a = got["action"].astype(np.float64)
    accuracy = dict(states=int(len(both)), converged=int(got["converged"].sum()), converged_share=float(got["converged"].mean()),
                    flags_equal_helper=bool(np.array_equal(got["converged"], ref["converged"])),
                    flags_equal_slsqp_classes=bool(np.array_equal(got["converged"], z["slsqp_eq_resid"] < 1e-6)),
                    iteration_histogram=np.bincount(got["iters"]).tolist(), helper_iteration_histogram=np.bincount(ref["iters"]).tolist(),
                    iterations_equal_helper=int((got["iters"] == ref["iters"]).sum()),
                    max_cost_dev_vs_helper=float(np.abs(got["cost"] - ref["cost"])[both].max()),
                    max_cost_dev_vs_slsqp=float(np.abs(got["cost"] - z["slsqp_cost"])[both].max()),
                    max_infeasibility=float(opf64.infeasibility(d64[both], a[both]).max()),
                    helper_max_infeasibility=float(opf64.infeasibility(d64[both], ref["action"][both]).max()),
                    max_cost_dev_vs_f64_obj_fn=float(np.abs(got["cost"] - ev.obj_fn(a))[both].max()))
    # ---- throughput
    xs = {n: (demand.repeat((n + 383) // 384, 1)[:n].contiguous(), pe.repeat((n + 383) // 384, 1)[:n].contiguous()) for n in SIZES}
    outs = {n: env.opf(*xs[n][:1], pe=xs[n][1]) for n in SIZES}
    inner = {4: 20, 1024: 10, 16384: 3}
    samples = {n: [] for n in SIZES}
    for rnd in range(reps + 2):
        for n in SIZES:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner[n]):
                env.opf(xs[n][0], pe=xs[n][1], out=outs[n])
            e1.record()
            e1.synchronize()
            if rnd >= 2:
                samples[n].append(e0.elapsed_time(e1) * 1e3 / inner[n])
    throughput = []
    for n in SIZES:
        med = statistics.median(samples[n])
        throughput.append(dict(n=n, inner=inner[n], median_us=round(med, 3), min_us=round(min(samples[n]), 3),
                               max_us=round(max(samples[n]), 3), states_per_second=round(n / (med * 1e-6), 1),
                               converged_share=float(outs[n].converged_rate())))
    # ---- opf_gap next to evaluate()
    tr.vec.reset()
    tr.run_steps(32)
    wall = dict(evaluate=[], opf_gap=[])
    gap = None
    for rnd in range(min(reps, 5) + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = tr.evaluate(1024, seed=11, record=True)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        gap = res.trajectory.opf_gap(env)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if rnd >= 1:
            wall["evaluate"].append((t1 - t0) * 1e3)
            wall["opf_gap"].append((t2 - t1) * 1e3)
    feasible = gap.feasible_only(res.trajectory.viol_thresh)
    gap_row = dict(episodes=1024, steps=int(gap.valid.sum()), path=res.path,
                   evaluate_ms=dict(median=round(statistics.median(wall["evaluate"]), 3), min=round(min(wall["evaluate"]), 3), max=round(max(wall["evaluate"]), 3)),
                   opf_gap_ms=dict(median=round(statistics.median(wall["opf_gap"]), 3), min=round(min(wall["opf_gap"]), 3), max=round(max(wall["opf_gap"]), 3)),
                   converged_share=gap.converged_rate(), gap_mean=gap.mean(), gap_median=gap.quantile(0.5), gap_min=gap.quantile(0.0),
                   feasible_only_steps=int(np.isfinite(feasible.gap).sum()), feasible_only_gap_mean=feasible.mean())
    # ---- the comparator
    try:
        sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
        from make_evopf_opf import slsqp
        secs = [slsqp(d64[i], pe64[i])[3] for i in range(n_slsqp)]
        comparator = dict(solver="scipy SLSQP, float64, on this box's CPU", states=n_slsqp, ms_per_state_median=round(statistics.median(secs) * 1e3, 3),
                          ms_per_state_mean=round(sum(secs) / len(secs) * 1e3, 3))
    except ImportError:
        comparator = dict(solver="scipy SLSQP, float64: the time recorded in the fixture, on the machine that made it (not this one)",
                          states=int(len(z["slsqp_seconds"])), ms_per_state_median=round(float(np.median(z["slsqp_seconds"])) * 1e3, 3),
                          ms_per_state_mean=round(float(z["slsqp_seconds"].mean()) * 1e3, 3))
    print("OPF_BENCH " + json.dumps(dict(device=torch.cuda.get_device_name(0), reps=reps, accuracy=accuracy, throughput=throughput,
                                         gap=gap_row, comparator=comparator)), flush=True)


def child_free(reps):
    import numpy as np
    import torch
    import evopf_opf_free_f64 as free64
    from bench import make_trainer
    from oracle import evopf as ev
    dev = torch.device("cuda")
    tr = make_trainer(16, dev, max_epochs=1000, capacity=64, workload="evopf_ddpg")
    env = tr.base_env
    with np.load(GOLDEN_FREE) as z:
        z = {k: z[k] for k in z.files}
    with np.load(GOLDEN) as zf:
        pe_fixed = torch.tensor(zf["pe"], dtype=torch.float32, device=dev)
    obs = torch.tensor(z["obs"], dtype=torch.float32, device=dev)
    # ---- accuracy on the 384 observations
    got = env.opf(obs, pe="free").numpy()
    o64 = obs.cpu().numpy().astype(np.float64)
    ref = free64.solve_free_many(o64)
    both = got["converged"] & ref["converged"]
    a = got["action"].astype(np.float64)
    hi, lo = ev.battery_bounds(o64[:, 28:33])
    pe = a[:, 38:]
    accuracy = dict(states=int(len(both)), converged=int(got["converged"].sum()), not_converged=int((~got["converged"]).sum()),
                    not_converged_rows=np.nonzero(~got["converged"])[0].tolist(),
                    flags_equal_helper=bool(np.array_equal(got["converged"], ref["converged"])),
                    flags_equal_slsqp_classes=bool(np.array_equal(got["converged"], z["slsqp_eq_resid"] < 1e-6)),
                    iteration_histogram=np.bincount(got["iters"]).tolist(), helper_iteration_histogram=np.bincount(ref["iters"]).tolist(),
                    iterations_equal_helper=int((got["iters"] == ref["iters"]).sum()),
                    max_objective_dev_vs_helper=float(np.abs(got["objective"] - ref["objective"])[both].max()),
                    max_f64_objective_dev_vs_helper=float(np.abs(free64.objective(o64, a) - ref["objective"])[both].max()),
                    max_objective_dev_vs_slsqp=float(np.abs(got["objective"] - z["slsqp_objective"])[both].max()),
                    max_infeasibility=float(free64.infeasibility(o64[both], a[both]).max()),
                    helper_max_infeasibility=float(free64.infeasibility(o64[both], ref["action"][both]).max()),
                    max_cost_dev_vs_f64_obj_fn=float(np.abs(got["cost"] - ev.obj_fn(a))[both].max()),
                    pe_at_a_bound_share=float((np.minimum(hi - pe, pe - lo)[both] <= 1e-3).mean()))
    # ---- throughput: the free and the fixed-pe kernel, alternately
    xs = {n: (obs.repeat((n + 383) // 384, 1)[:n].contiguous(), pe_fixed.repeat((n + 383) // 384, 1)[:n].contiguous()) for n in SIZES}
    calls = {"free": lambda n, out=None: env.opf(xs[n][0], pe="free", out=out),
             "fixed": lambda n, out=None: env.opf(xs[n][0], pe=xs[n][1], out=out)}
    outs = {(k, n): calls[k](n) for k in calls for n in SIZES}
    inner = {4: 20, 1024: 10, 16384: 3}
    samples = {key: [] for key in outs}
    for rnd in range(reps + 2):
        for n in SIZES:
            for k in calls:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(inner[n]):
                    calls[k](n, outs[(k, n)])
                e1.record()
                e1.synchronize()
                if rnd >= 2:
                    samples[(k, n)].append(e0.elapsed_time(e1) * 1e3 / inner[n])
    throughput = []
    for n in SIZES:
        row = dict(n=n, inner=inner[n])
        for k in calls:
            sm = samples[(k, n)]
            med = statistics.median(sm)
            row[k] = dict(median_us=round(med, 3), min_us=round(min(sm), 3), max_us=round(max(sm), 3),
                          states_per_second=round(n / (med * 1e-6), 1), converged_share=float(outs[(k, n)].converged_rate()),
                          mean_iterations=round(float(outs[(k, n)].info[:, 2].mean()), 3))
        row["free_over_fixed"] = round(row["free"]["median_us"] / row["fixed"]["median_us"], 4)
        throughput.append(row)
    # ---- evaluate_opf next to evaluate()
    tr.vec.reset()
    tr.run_steps(32)
    wall = dict(evaluate=[], evaluate_opf=[])
    for rnd in range(min(reps, 5) + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = tr.evaluate(1024, seed=11)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        ctl = tr.evaluate_opf(1024, seed=11)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if rnd >= 1:
            wall["evaluate"].append((t1 - t0) * 1e3)
            wall["evaluate_opf"].append((t2 - t1) * 1e3)
    ms = lambda v: dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3))       # noqa: E731
    live = np.arange(ctl.horizon)[None, :] < ctl.length[:, None]
    ok = (ctl.opf_converged | ~live).all(axis=1)
    eval_row = dict(episodes=1024, horizon=ctl.horizon, evaluate_path=res.path, evaluate_ms=ms(wall["evaluate"]),
                    evaluate_opf_ms=ms(wall["evaluate_opf"]), opf_converged_share=float(ctl.opf_converged[live].mean()),
                    opf_mean_iterations=float(ctl.opf_iters[live].mean()),
                    # an episode that met an infeasible hour stepped the solver's last iterate there: it is flagged, and left
                    # out of the means below
                    opf_all_converged_episodes=int(ok.sum()), opf_nonfinite_episodes=int(ctl.nonfinite.sum()),
                    return_opf_mean=float(ctl.ret[ok].mean()), return_policy_mean=float(res.ret[ok].mean()),
                    paired_return_diff_mean=float((ctl.ret - res.ret)[ok].mean()),
                    paired_return_diff_stderr=float((ctl.ret - res.ret)[ok].std() / np.sqrt(max(int(ok.sum()), 1))),
                    opf_violation_rate=ctl.violation_rate(), policy_violation_rate=res.violation_rate(),
                    opf_max_eq=float(ctl.max_eq[ok].max()), opf_max_ineq=float(ctl.max_ineq[ok].max()))
    before = None
    try:
        with open(os.path.join(ROOT, "profiles", "opf_bench.json")) as f:
            before = json.load(f)["throughput"]
    except (OSError, KeyError, ValueError):
        pass
    print("OPF_BENCH " + json.dumps(dict(device=torch.cuda.get_device_name(0), reps=reps, accuracy=accuracy, throughput=throughput,
                                         evaluate_opf=eval_row, fixed_pe_before=before)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--free", action="store_true", help="the free-pe instance next to the fixed-pe one -> profiles/opf_free_bench.json")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--slsqp", type=int, default=48, help="states the SLSQP comparator solves")
    ap.add_argument("--out", default=None, help="default: profiles/opf_bench.json, with --free profiles/opf_free_bench.json")
    ap.add_argument("--limit", type=int, default=400, help="seconds for the whole measurement")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child_free(a.reps) if a.free else child(a.reps, a.slsqp)
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "opf_free_bench.json" if a.free else "opf_bench.json")
    p = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps),
                        "--slsqp", str(a.slsqp)] + (["--free"] if a.free else []), stdout=subprocess.PIPE, text=True)
    if p.returncode != 0:                                        # (a fault, an abort, a time limit: nothing more is started)
        print(p.stdout[-2000:])
        sys.exit("bench_opf: ended with status %d" % p.returncode)
    tag = "OPF_BENCH "
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith(tag)][-1][len(tag):])
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
