"""The safety filter of EVOPF-v0 (``EVOPFEnv.nearest_feasible`` / rpo_evopf_nearest, ``trainer.evaluate_filtered``) on the MI355X:
its accuracy against the float64 yardstick, its device time next to the free-pe OPF, and whole episodes through it next to the
policy alone and the OPF controller.

    python tools/bench_nearest.py [--rounds R] [--out profiles/nearest_bench.json]

* ``accuracy``: the 70 rows and three families of targets of tests/golden/evopf_nearest.npz against tests/evopf_nearest_f64.py -- per
  family the converged counts, the iteration range and the number of rows whose count differs from the helper's, the largest
  residual and float64 infeasibility of the converged points, the worst |distance - helper's| next to its allowance (1e-4 +
  |lambda_helper|_inf |eq_resid_64(y)|_1) and, for the already feasible targets, the largest ``moved`` next to the helper's own.
* ``device_time``: microseconds per call of ``nearest_feasible`` and of ``opf(pe="free")`` on the same observations at 4 / 1024 /
  16384 rows, measured alternately in one run with device events: medians and min-max of R rounds (9).
* ``episodes``: wall time of ``evaluate_filtered(1024)`` next to ``evaluate(1024)`` and ``evaluate_opf(1024)``, alternately, medians
  and min-max of R rounds; return, violation rate and converged rate of policy / filtered / OPF on the same episodes.
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
GOLDEN = os.path.join(ROOT, "tests", "golden", "evopf_nearest.npz")
TOL = 1e-4


def child(rounds):
    import numpy as np
    import torch
    import evopf_nearest_f64 as near64
    import evopf_opf_free_f64 as free64
    from bench import make_trainer
    from oracle import evopf as ev
    dev = torch.device("cuda")
    tr = make_trainer(16, dev, max_epochs=1000, capacity=64, workload="evopf_ddpg")
    env = tr.base_env
    with np.load(GOLDEN) as z:
        z = {k: z[k] for k in z.files}
    obs = torch.tensor(z["obs"], device=dev)
    o64 = z["obs"].astype(np.float64)
    # ---- accuracy on the 70 rows, every family
    accuracy = {}
    for fam in near64.FAMILIES:
        t32 = z["target_" + fam].astype(np.float32)
        ref = near64.solve_nearest_many(o64, t32.astype(np.float64), tol=TOL, max_iters=40)
        got = env.nearest_feasible(obs, torch.tensor(t32, device=dev), tol=TOL, max_iters=40).numpy()
        conv = got["converged"]
        a = got["action"][conv].astype(np.float64)
        eq1 = np.abs(ev.eq_resid(o64[conv], a)).sum(axis=1)
        allow = 1e-4 + np.abs(ref["lam"][conv]).max(axis=1) * eq1
        dev_d = np.abs(got["distance"][conv] - ref["distance"][conv])
        row = dict(rows=int(len(conv)), converged=int(conv.sum()), helper_converged=int(ref["converged"].sum()),
                   flags_equal_helper=bool(np.array_equal(conv, ref["converged"])),
                   iterations=[int(got["iters"][conv].min()), int(got["iters"][conv].max())],
                   helper_iterations=[int(ref["iters"][conv].min()), int(ref["iters"][conv].max())],
                   rows_whose_iterations_differ=int((got["iters"][conv] != ref["iters"][conv]).sum()),
                   max_residual=float(got["residual"][conv].max()),
                   max_infeasibility=float(free64.infeasibility(o64[conv], a).max()),
                   helper_max_infeasibility=float(free64.infeasibility(o64[conv], ref["action"][conv]).max()),
                   max_distance_dev_vs_helper=float(dev_d.max()), min_allowance=float(allow.min()),
                   worst_dev_over_allowance=float((dev_d / allow).max()),
                   max_distance_dev_vs_slsqp=float(np.abs(got["distance"][conv] - z["slsqp_objective_" + fam][conv]).max()),
                   max_distance=float(got["distance"][conv].max()))
        if fam == "feasible":
            own = float(near64.moved(o64[conv], ref["action"][conv], t32[conv].astype(np.float64)).max())
            row.update(max_moved=float(got["moved"][conv].max()), helper_max_moved=own, moved_bound=4 * own)
        accuracy[fam] = row
    # ---- device time: the filter and the free-pe OPF on the same observations, alternately
    t_all = torch.tensor(z["target_uniform"].astype(np.float32), device=dev)
    feas = torch.arange(65, device=dev)                          # (the feasible rows: an infeasible one runs to max_iters)
    xs = {n: (obs[feas].repeat((n + 64) // 65, 1)[:n].contiguous(), t_all[feas].repeat((n + 64) // 65, 1)[:n].contiguous()) for n in SIZES}
    calls = {"nearest": lambda n, out=None: env.nearest_feasible(xs[n][0], xs[n][1], out=out),
             "opf_free": lambda n, out=None: env.opf(xs[n][0], pe="free", out=out)}
    outs = {(k, n): calls[k](n) for k in calls for n in SIZES}
    inner = {4: 20, 1024: 10, 16384: 3}
    samples = {key: [] for key in outs}
    for rnd in range(rounds + 2):
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
    device_time = []
    for n in SIZES:
        row = dict(n=n, inner=inner[n])
        for k in calls:
            sm = samples[(k, n)]
            med = statistics.median(sm)
            row[k] = dict(median_us=round(med, 3), min_us=round(min(sm), 3), max_us=round(max(sm), 3),
                          rows_per_second=round(n / (med * 1e-6), 1), converged_share=float(outs[(k, n)].converged_rate()),
                          mean_iterations=round(float(outs[(k, n)].info[:, 2].mean()), 3))
        row["nearest_over_opf_free"] = round(row["nearest"]["median_us"] / row["opf_free"]["median_us"], 4)
        device_time.append(row)
    # (nearest_feasible's call includes the torch ops around the launch: the target gather and ``moved``)
    # ---- whole episodes: policy, policy + filter, OPF -- alternately, on the same episodes
    tr.vec.reset()
    tr.run_steps(32)
    wall = dict(evaluate=[], evaluate_filtered=[], evaluate_opf=[])
    for rnd in range(rounds + 1):
        stamps = []
        for name in wall:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = getattr(tr, name)(1024, seed=11)
            torch.cuda.synchronize()
            stamps.append((name, (time.perf_counter() - t0) * 1e3, res))
        if rnd >= 1:
            for name, ms_, _ in stamps:
                wall[name].append(ms_)
    pol, fil, ctl = (s[2] for s in stamps)
    ms = lambda v: dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3))       # noqa: E731
    live = np.arange(fil.horizon)[None, :] < fil.length[:, None]
    ok = (fil.filter_converged | ~live).all(axis=1) & (ctl.opf_converged | ~live).all(axis=1)
    rec = tr.evaluate_filtered(64, seed=11, record=True).trajectory
    conv64 = tr.evaluate_filtered(64, seed=11).filter_converged
    episodes = dict(episodes=1024, horizon=fil.horizon, evaluate_path=pol.path, evaluate_ms=ms(wall["evaluate"]),
                    evaluate_filtered_ms=ms(wall["evaluate_filtered"]), evaluate_opf_ms=ms(wall["evaluate_opf"]),
                    filter_converged_share=float(fil.filter_converged[live].mean()), opf_converged_share=float(ctl.opf_converged[live].mean()),
                    filter_mean_iterations=float(fil.filter_iters[live].mean()), filter_mean_distance_converged_steps=float(fil.filter_distance[fil.filter_converged].mean()),
                    # an episode that met an infeasible hour stepped the policy's own action there (fallback="policy"): such
                    # episodes are left out of the paired means below
                    all_converged_episodes=int(ok.sum()),
                    return_policy_mean=float(pol.ret[ok].mean()), return_filtered_mean=float(fil.ret[ok].mean()),
                    return_opf_mean=float(ctl.ret[ok].mean()),
                    paired_filtered_minus_policy_mean=float((fil.ret - pol.ret)[ok].mean()),
                    paired_opf_minus_filtered_mean=float((ctl.ret - fil.ret)[ok].mean()),
                    policy_violation_rate=pol.violation_rate(), filtered_violation_rate=fil.violation_rate(),
                    opf_violation_rate=ctl.violation_rate(),
                    filtered_max_eq=float(fil.max_eq[ok].max()), filtered_max_ineq=float(fil.max_ineq[ok].max()),
                    policy_max_eq=float(pol.max_eq[ok].max()), policy_max_ineq=float(pol.max_ineq[ok].max()),
                    recorded_64_converged_steps_max_eq=float(rec.eq[conv64].max()), recorded_64_converged_steps_max_ineq=float(rec.ineq[conv64].max()))
    print("NEAREST_BENCH " + json.dumps(dict(device=torch.cuda.get_device_name(0), rounds=rounds, tol=TOL, max_iters=40, accuracy=accuracy,
                                             device_time=device_time, episodes=episodes)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nearest_bench.json"))
    ap.add_argument("--limit", type=int, default=400, help="seconds for the whole measurement")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.rounds)
    p = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", "--rounds", str(a.rounds)],
                       stdout=subprocess.PIPE, text=True)
    if p.returncode != 0:                                        # (a fault, an abort, a time limit: nothing more is started)
        print(p.stdout[-2000:])
        sys.exit("bench_nearest: ended with status %d" % p.returncode)
    tag = "NEAREST_BENCH "
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith(tag)][-1][len(tag):])
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
