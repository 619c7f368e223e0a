"""Float64 yardstick of the single-step AC-OPF of EVOPF-v0 with the battery power FREE (``EVOPFEnv.opf(pe="free")`` /
``rpo_evopf_opf_free``).  Test infrastructure only, numpy only.

The problem, per observation: minimise ``obj_fn(pg) + pe_cost . pe`` over x = (pg[5], qg[5], vm[14], va at the 13 non-slack buses,
pe[5]) subject to the 28 equalities ``eq_resid = 0``, the 48 box bounds on pg, qg, vm and the 10 battery bounds
``battery_bounds(soc)`` of the row's state of charge -- 58 inequalities.  ``pe_cost`` None: (WE / WG) * the row's current price in
every component, with which the optimum maximises ``oracle.evopf.step``'s one-step reward.

The method is tests/evopf_opf_f64.py's (same flat start -- pe at the middle of its box --, sigma, xi and stop test), with five more
bounded variables and gamma <- sigma z^T mu / 58.  The full 70 x 70 system goes to ``numpy.linalg.solve``: nothing of the kernel's
elimination (generator AND battery variables eliminated by hand, one row per lane, dynamic pivots) is shared with this file.

The battery columns of the Jacobian: ``oracle.evopf.eq_jac`` keeps the reference's literal -1 (DESIGN hazard E1) although
``eq_resid`` adds pg + pe; ``jac_free`` below puts the TRUE derivative +1 there (tests/test_evopf_opf_free.py holds it to central
differences of ``eq_resid``).
"""
import numpy as np

import evopf_opf_f64 as opf64
from evopf_opf_f64 import COST1, COST2, GAMMA0, GRID, NB, NEQ, NG, SIGMA, XI, XMAX, XMIN, Z0, lagr_hessian
from oracle import evopf as ev

NE = GRID.ne
SOC0, PRICE0 = 2 * NB, 2 * NB + NE                            # columns of an observation: state of charge, current price
XIDX = np.concatenate([opf64.XIDX, GRID.pe0 + np.arange(NE)])  # x as positions of the 43-vector: ..., then pe
NX = len(XIDX)                                                # 42
NBND0 = opf64.NBND                                            # 24 bounded variables of the fixed-pe problem (pg, qg, vm): x[:24]
BIDX = np.concatenate([np.arange(NBND0), np.arange(NX - NE, NX)])   # the 29 bounded components of x (pe last)
NBND = len(BIDX)                                              # -> 58 inequalities


def default_pe_cost(obs):
    """(WE / WG) * current price, [5]."""
    return np.full(NE, ev.WE / ev.WG * float(obs[PRICE0]))


def box(obs):
    """(upper, lower) bounds of the 29 bounded variables of one observation."""
    p_max, p_min = ev.battery_bounds(np.asarray(obs, dtype=np.float64)[SOC0:SOC0 + NE])
    return np.concatenate([XMAX, p_max]), np.concatenate([XMIN, p_min])


def jac_free(action, grid=GRID):
    """d eq_resid / d x [28, 42] at one action [43]: ``eq_jac``'s columns with the battery columns at their true sign, +1 in the
    real-power equation of bus spv[j]."""
    J = ev.eq_jac(action[None], grid)[0][:, XIDX].copy()
    J[:, NX - NE:] = 0.0
    J[np.asarray(grid.spv), NX - NE + np.arange(NE)] = 1.0
    return J


def flat_start(obs, grid=GRID):
    """Middle of every box (pe included), angles zero (the slack's: slack_va) -> [43]."""
    hi, lo = box(obs)
    a = np.zeros(grid.ydim)
    a[XIDX[BIDX]] = 0.5 * (hi + lo)
    a[grid.va0 + opf64.SLACK] = grid.slack_va[0]
    return a


def infeasibility(obs, action):
    """max(|eq_resid|_inf, largest excess over any of the 58 bounds) of rows [n, 43] against observations [n, 57], float64."""
    obs, action = np.asarray(obs, dtype=np.float64), np.asarray(action, dtype=np.float64)
    eq = np.abs(ev.eq_resid(obs, action)).max(axis=1)
    return np.maximum(eq, ev.ineq_resid(obs, action).max(axis=1))


def objective(obs, action, pe_cost=None):
    """obj_fn + pe_cost . pe of rows, float64 (pe_cost None: the default of every row; or [5] / [n, 5])."""
    obs, action = np.asarray(obs, dtype=np.float64), np.asarray(action, dtype=np.float64)
    pc = (ev.WE / ev.WG) * obs[:, PRICE0:PRICE0 + 1] if pe_cost is None else np.asarray(pe_cost, dtype=np.float64)
    return ev.obj_fn(action) + (pc * action[:, GRID.pe0:]).sum(axis=1)


def solve_free(obs, pe_cost=None, tol=1e-4, max_iters=40, grid=GRID):
    """One observation [57]; pe_cost [5] or None.  -> dict(action [43], cost = obj_fn, objective = cost + pe_cost . pe, iters,
    converged, residual): ``residual`` the largest of the three stop quantities at exit."""
    obs = np.asarray(obs, dtype=np.float64)
    s = obs[None, :2 * NB]
    pc = default_pe_cost(obs) if pe_cost is None else np.broadcast_to(np.asarray(pe_cost, dtype=np.float64), (NE,))
    hi, lo = box(obs)
    a = flat_start(obs, grid)
    xb = a[XIDX[BIDX]]
    z = np.maximum(-np.concatenate([xb - hi, lo - xb]), Z0)
    gamma = GAMMA0
    mu = gamma / z
    lam = np.zeros(NEQ)
    it, converged = 0, False
    with np.errstate(all="ignore"):
        while True:
            x = a[XIDX]
            g = ev.eq_resid(s, a[None], grid)[0]
            J = jac_free(a, grid)
            h = np.concatenate([x[BIDX] - hi, lo - x[BIDX]])
            df = np.zeros(NX)
            df[:NG] = COST2 * x[:NG] + COST1
            df[NX - NE:] = pc
            dmu = np.zeros(NX)
            dmu[BIDX] = mu[:NBND] - mu[NBND:]
            lx = df + J.T @ lam + dmu
            residual = max(np.abs(g).max(), h.max(), np.abs(lx).max(), float(z @ mu))
            if residual < tol:                                  # (a NaN compares False: not converged)
                converged = True
                break
            if it >= max_iters:
                break
            M = np.zeros((NX, NX))
            M[:NX - NE, :NX - NE] = lagr_hessian(a, lam, grid)[np.ix_(opf64.XIDX, opf64.XIDX)]
            M[np.arange(NG), np.arange(NG)] += COST2
            M[BIDX, BIDX] += mu[:NBND] / z[:NBND] + mu[NBND:] / z[NBND:]
            N = lx.copy()
            N[BIDX] += (mu[:NBND] * h[:NBND] + gamma) / z[:NBND] - (mu[NBND:] * h[NBND:] + gamma) / z[NBND:]
            K = np.zeros((NX + NEQ, NX + NEQ))
            K[:NX, :NX], K[:NX, NX:], K[NX:, :NX] = M, J.T, J
            try:
                sol = np.linalg.solve(K, np.concatenate([-N, -g]))
            except np.linalg.LinAlgError:
                sol = np.full(NX + NEQ, np.nan)
            dx, dlam = sol[:NX], sol[NX:]
            dz = -h - z - np.concatenate([dx[BIDX], -dx[BIDX]])
            dm = -mu + (gamma - mu * dz) / z
            neg = dz < 0
            alpha_p = min(XI * np.min(z[neg] / -dz[neg]), 1.0) if neg.any() else 1.0
            neg = dm < 0
            alpha_d = min(XI * np.min(mu[neg] / -dm[neg]), 1.0) if neg.any() else 1.0
            a = a.copy()
            a[XIDX] += alpha_p * dx
            z = z + alpha_p * dz
            lam = lam + alpha_d * dlam
            mu = mu + alpha_d * dm
            gamma = SIGMA * float(z @ mu) / (2 * NBND)
            it += 1
    cost = float(ev.obj_fn(a[None], grid)[0])
    return dict(action=a, cost=cost, objective=cost + float(pc @ a[grid.pe0:]), iters=it, converged=converged,
                residual=float(residual))


def solve_free_many(obs, pe_cost=None, tol=1e-4, max_iters=40, grid=GRID):
    """Rows of ``solve_free`` -> dict of arrays (action [n, 43], cost, objective, iters, converged, residual)."""
    obs = np.asarray(obs, dtype=np.float64)
    pc = None if pe_cost is None else np.broadcast_to(np.asarray(pe_cost, dtype=np.float64), (obs.shape[0], NE))
    res = [solve_free(obs[i], None if pc is None else pc[i], tol, max_iters, grid) for i in range(obs.shape[0])]
    return dict(action=np.stack([r["action"] for r in res]), cost=np.array([r["cost"] for r in res]),
                objective=np.array([r["objective"] for r in res]), iters=np.array([r["iters"] for r in res], dtype=np.int32),
                converged=np.array([r["converged"] for r in res], dtype=bool), residual=np.array([r["residual"] for r in res]))


def fixture_obs(grid=GRID):
    """The 384 observations [384, 57] of tests/golden/evopf_opf_free.npz: the demands of ``evopf_opf_f64.fixture_states()`` (lanes
    0..7, episodes 0..1, hours 0..23 of seed 11; lane outermost, then episode, then hour), the price window
    ``episode_price(11, [lane], ep, t)`` of the same lane, episode and hour, and a state of charge per row from
    numpy.random.default_rng(2): one permutation of the rows, its first half uniform in [B_LOW, B_HIGH], the next quarter B_INIT,
    the rest drawn from {B_LOW, B_HIGH}."""
    demand, _ = opf64.fixture_states(grid)
    n = demand.shape[0]
    price = np.concatenate([ev.episode_price(11, np.array([lane]), ep, t) for lane in range(8) for ep in range(2)
                            for t in range(ev.T)])
    rng = np.random.default_rng(2)
    order = rng.permutation(n)
    soc = np.full((n, NE), ev.B_INIT)
    soc[order[:n // 2]] = rng.uniform(ev.B_LOW, ev.B_HIGH, size=(n // 2, NE))
    rest = order[n // 2 + n // 4:]
    soc[rest] = rng.choice([ev.B_LOW, ev.B_HIGH], size=(len(rest), NE))
    return np.concatenate([demand, soc, price], axis=1)


def fixture_rows():
    """The 70 rows of tests/test_evopf_opf_free_gpu.py: the fixture's first 65 observations plus its infeasible ones (SLSQP's final
    equality residual > 1e-3) behind them -> (row indices [70], observations [70, 57] float32)."""
    import os
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "evopf_opf_free.npz")) as z:
        obs, infeas = z["obs"], z["slsqp_eq_resid"] > 1e-3
    rows = np.concatenate([np.arange(65), np.setdiff1d(np.nonzero(infeas)[0], np.arange(65))])
    assert len(rows) == 70
    return rows, obs[rows].astype(np.float32)
