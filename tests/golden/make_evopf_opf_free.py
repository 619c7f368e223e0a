"""tests/golden/evopf_opf_free.npz: the 384 free-pe single-step AC-OPF observations of tests/test_evopf_opf_free.py with an
INDEPENDENT solver's answer.

    python tests/golden/make_evopf_opf_free.py           (needs scipy; the tests do not)

Observations: ``evopf_opf_free_f64.fixture_obs()``.  For each one scipy's SLSQP (float64) minimises ``oracle.evopf.obj_fn + (WE /
WG) * price * sum(pe)`` over (pg, qg, vm, va at the non-slack buses, pe) subject to ``eq_resid = 0`` (analytic Jacobian: ``eq_jac``
with the battery columns at their true sign +1, ``jac_free``), the bounds on pg, qg, vm and the battery box of the row's state of
charge, from the flat start of the interior-point method.  Stored: the observations, SLSQP's objective, obj_fn, point [43], final
max |eq_resid|, and its wall time per state on the machine that made the file.  A final equality residual below 1e-6 marks the
state as feasible, above 1e-3 as infeasible (SLSQP stops at a point of least infeasibility there).
"""
import os
import sys
import time

import numpy as np
from scipy.optimize import minimize

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import evopf_opf_free_f64 as free  # noqa: E402
from oracle import evopf as ev  # noqa: E402


def slsqp(obs):
    base = free.flat_start(obs)
    s = obs[None]
    pc = free.default_pe_cost(obs)
    hi, lo = free.box(obs)

    def full(x):
        a = base.copy()
        a[free.XIDX] = x
        return a

    def grad(x):
        g = np.zeros(free.NX)
        g[:free.NG] = free.COST2 * x[:free.NG] + free.COST1
        g[free.NX - free.NE:] = pc
        return g
    bounds = [(None, None)] * free.NX
    for b, l, h in zip(free.BIDX, lo, hi):
        bounds[b] = (l, h)
    cons = dict(type="eq", fun=lambda x: ev.eq_resid(s, full(x)[None])[0], jac=lambda x: free.jac_free(full(x)))
    t = time.perf_counter()
    r = minimize(lambda x: ev.obj_fn(full(x)[None])[0] + pc @ x[free.NX - free.NE:], base[free.XIDX], jac=grad, bounds=bounds,
                 constraints=[cons], method="SLSQP", options=dict(ftol=1e-12, maxiter=500))
    dt = time.perf_counter() - t
    a = full(r.x)
    cost = float(ev.obj_fn(a[None])[0])
    return a, cost + float(pc @ a[ev.GRID.pe0:]), cost, float(np.abs(ev.eq_resid(s, a[None])).max()), dt


if __name__ == "__main__":
    obs = free.fixture_obs()
    res = [slsqp(obs[i]) for i in range(obs.shape[0])]
    point = np.stack([r[0] for r in res])
    objective, cost, eq, secs = (np.array([r[k] for r in res]) for k in (1, 2, 3, 4))
    print("feasible %d, infeasible %d, other %d; %.1f ms per state" % ((eq < 1e-6).sum(), (eq > 1e-3).sum(),
                                                                        ((eq >= 1e-6) & (eq <= 1e-3)).sum(), secs.mean() * 1e3))
    print("infeasible states:", np.nonzero(eq > 1e-3)[0], eq[eq > 1e-3])
    np.savez_compressed(os.path.join(HERE, "evopf_opf_free.npz"), obs=obs, slsqp_objective=objective, slsqp_cost=cost,
                        slsqp_point=point, slsqp_eq_resid=eq, slsqp_seconds=secs)
