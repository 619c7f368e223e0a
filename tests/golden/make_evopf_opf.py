"""tests/golden/evopf_opf.npz: the 384 single-step AC-OPF states of tests/test_evopf_opf.py with an INDEPENDENT solver's answer.

    python tests/golden/make_evopf_opf.py           (needs scipy; the tests do not)

States: ``evopf_opf_f64.fixture_states()`` -- ``oracle.evopf.episode_demand(11, lanes 0..7, episodes 0..1, t = 0..23)`` and pe
zero on even lanes, one uniform draw in the B_PMIN / B_PMAX box per odd lane.  For each state scipy's SLSQP (float64) minimises
``oracle.evopf.obj_fn`` over (pg, qg, vm, va at the non-slack buses) subject to ``eq_resid = 0`` (analytic Jacobian ``eq_jac``)
and the bounds on pg, qg, vm, from the flat start of the interior-point method.  Stored: demand, pe, SLSQP's cost, point [43],
final max |eq_resid|, and its wall time per state on the machine that made the file.  A final equality residual below 1e-6 marks
the state as feasible, above 1e-3 as infeasible (SLSQP stops at a point of least infeasibility there).
"""
import os
import sys
import time

import numpy as np
from scipy.optimize import minimize

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import evopf_opf_f64 as opf  # noqa: E402
from oracle import evopf as ev  # noqa: E402


def slsqp(demand, pe):
    base = opf.flat_start(pe)
    s = demand[None]

    def full(x):
        a = base.copy()
        a[opf.XIDX] = x
        return a[None]

    def grad(x):
        g = np.zeros(opf.NX)
        g[:opf.NG] = opf.COST2 * x[:opf.NG] + opf.COST1
        return g
    bounds = [(lo, hi) for lo, hi in zip(opf.XMIN, opf.XMAX)] + [(None, None)] * (opf.NX - opf.NBND)
    cons = dict(type="eq", fun=lambda x: ev.eq_resid(s, full(x))[0], jac=lambda x: ev.eq_jac(full(x))[0][:, opf.XIDX])
    t = time.perf_counter()
    r = minimize(lambda x: ev.obj_fn(full(x))[0], base[opf.XIDX], jac=grad, bounds=bounds, constraints=[cons], method="SLSQP",
                 options=dict(ftol=1e-12, maxiter=500))
    dt = time.perf_counter() - t
    a = full(r.x)
    return a[0], float(ev.obj_fn(a)[0]), float(np.abs(ev.eq_resid(s, a)).max()), dt


if __name__ == "__main__":
    demand, pe = opf.fixture_states()
    res = [slsqp(demand[i], pe[i]) for i in range(demand.shape[0])]
    point = np.stack([r[0] for r in res])
    cost, eq, secs = (np.array([r[k] for r in res]) for k in (1, 2, 3))
    print("feasible %d, infeasible %d, other %d; %.1f ms per state" % ((eq < 1e-6).sum(), (eq > 1e-3).sum(),
                                                                        ((eq >= 1e-6) & (eq <= 1e-3)).sum(), secs.mean() * 1e3))
    print("infeasible states:", np.nonzero(eq > 1e-3)[0], eq[eq > 1e-3])
    np.savez_compressed(os.path.join(HERE, "evopf_opf.npz"), demand=demand, pe=pe, slsqp_cost=cost, slsqp_point=point,
                        slsqp_eq_resid=eq, slsqp_seconds=secs)
