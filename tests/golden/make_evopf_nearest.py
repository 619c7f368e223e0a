"""tests/golden/evopf_nearest.npz: the targets of tests/test_evopf_nearest.py / tests/test_evopf_nearest_gpu.py for the 70 rows of
``evopf_opf_free_f64.fixture_rows()``, with an INDEPENDENT solver's answer to each.

    python tests/golden/make_evopf_nearest.py           (needs scipy; the tests do not)

Three families of targets [70, 14] (``partial_actions`` order), each deterministic (tests/evopf_nearest_f64.py): ``uniform`` in the
box of every controlled variable (default_rng(101)); ``near``, the free-pe fixture's ``slsqp_point`` plus 0.2 half-widths of
Gaussian noise (default_rng(102)); ``feasible``, the float64 helper's own answer to ``uniform`` (its target of ``uniform`` on the 5 rows it does not converge on).  For each row and family scipy's
SLSQP (float64) minimises ``0.5 * sum_k (y_k - t_k)^2 / s_k^2`` over (pg, qg, vm, va at the non-slack buses, pe) subject to
``eq_resid = 0`` (analytic Jacobian ``jac_free``), the bounds on pg, qg, vm and the battery box of the row's state of charge, from
the flat start.  ``ftol`` is tight and the objective SLSQP ends with is stored even where it reports a stalled line search.
Stored per family: the targets, SLSQP's objective, point [43] and final max |eq_resid|; once: the row indices and observations.
"""
import os
import sys

import numpy as np
from scipy.optimize import minimize

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import evopf_nearest_f64 as near  # noqa: E402
import evopf_opf_free_f64 as free  # noqa: E402
from oracle import evopf as ev  # noqa: E402


def slsqp(obs, target):
    base = free.flat_start(obs)
    s = obs[None]
    w = near.default_weight(obs)
    hi, lo = free.box(obs)

    def full(x):
        a = base.copy()
        a[free.XIDX] = x
        return a

    def grad(x):
        g = np.zeros(free.NX)
        g[near.PX] = w * (x[near.PX] - target)
        return g
    bounds = [(None, None)] * free.NX
    for b, l, h in zip(free.BIDX, lo, hi):
        bounds[b] = (l, h)
    cons = dict(type="eq", fun=lambda x: ev.eq_resid(s, full(x)[None])[0], jac=lambda x: free.jac_free(full(x)))
    r = minimize(lambda x: 0.5 * float((w * (x[near.PX] - target) ** 2).sum()), base[free.XIDX], jac=grad, bounds=bounds,
                 constraints=[cons], method="SLSQP", options=dict(ftol=1e-14, maxiter=1000))
    a = full(r.x)
    return a, float(r.fun), float(np.abs(ev.eq_resid(s, a[None])).max())


if __name__ == "__main__":
    rows, obs32 = free.fixture_rows()
    obs = obs32.astype(np.float64)                               # the float32 observations the kernel reads, as float64
    with np.load(os.path.join(HERE, "evopf_opf_free.npz")) as z:
        point = z["slsqp_point"][rows]
    uniform = near.target_uniform(obs)
    targets = dict(uniform=uniform, near=near.target_near(obs, point), feasible=near.target_feasible(obs, uniform))
    out = dict(rows=rows, obs=obs32)
    for fam in near.FAMILIES:
        res = [slsqp(obs[i], targets[fam][i]) for i in range(len(rows))]
        eq = np.array([r[2] for r in res])
        print("%s: feasible %d, infeasible %d, other %d" % (fam, (eq < 1e-6).sum(), (eq > 1e-3).sum(), ((eq >= 1e-6) & (eq <= 1e-3)).sum()))
        out["target_" + fam] = targets[fam]
        out["slsqp_objective_" + fam] = np.array([r[1] for r in res])
        out["slsqp_point_" + fam] = np.stack([r[0] for r in res])
        out["slsqp_eq_resid_" + fam] = eq
    np.savez_compressed(os.path.join(HERE, "evopf_nearest.npz"), **out)
