"""Float64 yardstick of the safety filter of EVOPF-v0 (``EVOPFEnv.nearest_feasible`` / ``rpo_evopf_nearest``): the feasible
dispatch nearest to a policy's action.  Test infrastructure only, numpy only.

The problem, per observation: minimise ``0.5 * sum_k w_k (y_k - t_k)^2`` over the 14 controlled components k (the env's
``partial_actions``: pg at the four non-slack generators, vm at the five generator buses, pe[5]) of x = (pg[5], qg[5], vm[14], va
at the 13 non-slack buses, pe[5]), subject to the 28 equalities ``eq_resid = 0`` and the 58 bounds of the free-pe OPF
(tests/evopf_opf_free_f64.py: pg, qg, vm boxes and ``battery_bounds(soc)``).  ``w_k`` None: 1 / s_k^2 with s_k the half-width of
the variable's own box in this problem (per row for pe), 0 where s_k <= 1e-6 -- the distance in box units.

The method is tests/evopf_opf_free_f64.py's, constant for constant (flat start -- NOT the target --, sigma, xi, the stop test, gamma
<- sigma z^T mu / 58); the objective alone differs: gradient w (x - t) and a diagonal Hessian w on the controlled components.  The
full 70 x 70 system goes to ``numpy.linalg.solve``: nothing of the kernel's elimination is shared with this file.
"""
import numpy as np

import evopf_opf_f64 as opf64
from evopf_opf_f64 import GAMMA0, GRID, NEQ, SIGMA, XI, Z0, lagr_hessian
from evopf_opf_free_f64 import BIDX, NBND, NE, NX, XIDX, box, flat_start, jac_free
from oracle import evopf as ev

PARTIAL = np.asarray(GRID.partial_actions)                     # the 14 controlled components of the 43-vector, the env's order
NP = len(PARTIAL)
PX = np.array([int(np.nonzero(XIDX == k)[0][0]) for k in PARTIAL])        # ... as positions of x
PB = np.array([int(np.nonzero(XIDX[BIDX] == k)[0][0]) for k in PARTIAL])  # ... and of the 29 bounded variables
HALF_MIN = 1e-6


def half_widths(obs):
    """s [14]: half the width of every controlled variable's own box, one observation."""
    hi, lo = box(obs)
    return 0.5 * (hi[PB] - lo[PB])


def default_weight(obs):
    """1 / s^2, 0 where s <= 1e-6 -> [14]."""
    s = half_widths(obs)
    w = np.zeros(NP)
    w[s > HALF_MIN] = 1.0 / s[s > HALF_MIN] ** 2
    return w


def distance(action, target, weight):
    """0.5 * sum w (y - t)^2 of rows: action [n, 43], target [n, 14], weight [n, 14] -> [n], float64."""
    action, target = np.asarray(action, dtype=np.float64), np.asarray(target, dtype=np.float64)
    return 0.5 * (np.asarray(weight, dtype=np.float64) * (action[:, PARTIAL] - target) ** 2).sum(axis=1)


def moved(obs, action, target):
    """|y - t| / s in box units, rows -> [n, 14] (inf / nan where the box is empty)."""
    s = np.stack([half_widths(o) for o in np.asarray(obs, dtype=np.float64)])
    with np.errstate(all="ignore"):
        return np.abs(np.asarray(action, dtype=np.float64)[:, PARTIAL] - np.asarray(target, dtype=np.float64)) / s


def solve_nearest(obs, target, weight=None, tol=1e-4, max_iters=40, grid=GRID):
    """One observation [57], target [14] (``partial_actions`` order), weight [14] or None.  -> dict(action [43], distance, iters,
    converged, residual, lam [28]): ``residual`` the largest of the three stop quantities at exit, ``lam`` the multipliers of the
    equalities there."""
    obs = np.asarray(obs, dtype=np.float64)
    s = obs[None, :2 * opf64.NB]
    t = np.asarray(target, dtype=np.float64)
    w = default_weight(obs) if weight is None else np.asarray(weight, dtype=np.float64)
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
            df[PX] = w * (x[PX] - t)
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
            M[PX, PX] += w
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
        dist = 0.5 * float((w * (a[PARTIAL] - t) ** 2).sum())
    return dict(action=a, distance=dist, iters=it, converged=converged, residual=float(residual), lam=lam)


def solve_nearest_many(obs, target, weight=None, tol=1e-4, max_iters=40, grid=GRID):
    """Rows of ``solve_nearest`` -> dict of arrays (action [n, 43], distance, iters, converged, residual, lam [n, 28]); weight None,
    [14] or [n, 14]."""
    obs, target = np.asarray(obs, dtype=np.float64), np.asarray(target, dtype=np.float64)
    w = None if weight is None else np.broadcast_to(np.asarray(weight, dtype=np.float64), (obs.shape[0], NP))
    res = [solve_nearest(obs[i], target[i], None if w is None else w[i], tol, max_iters, grid) for i in range(obs.shape[0])]
    return dict(action=np.stack([r["action"] for r in res]), distance=np.array([r["distance"] for r in res]),
                iters=np.array([r["iters"] for r in res], dtype=np.int32), converged=np.array([r["converged"] for r in res], dtype=bool),
                residual=np.array([r["residual"] for r in res]), lam=np.stack([r["lam"] for r in res]))


# ------------------------------------------------------------------------------------------------ the targets of the tests
FAMILIES = ("uniform", "near", "feasible")
SEED_UNIFORM, SEED_NEAR = 101, 102


def target_uniform(obs):
    """(a) uniform in the box of each controlled variable, numpy.random.default_rng(101), rows in order -> [n, 14]."""
    rng = np.random.default_rng(SEED_UNIFORM)
    out = []
    for o in np.asarray(obs, dtype=np.float64):
        hi, lo = box(o)
        out.append(lo[PB] + rng.uniform(size=NP) * (hi[PB] - lo[PB]))
    return np.stack(out)


def target_near(obs, point):
    """(b) ``point`` [n, 43] (the fixture's slsqp_point) plus 0.2 half-widths of Gaussian noise, numpy.random.default_rng(102)."""
    rng = np.random.default_rng(SEED_NEAR)
    obs = np.asarray(obs, dtype=np.float64)
    s = np.stack([half_widths(o) for o in obs])
    return np.asarray(point, dtype=np.float64)[:, PARTIAL] + 0.2 * s * rng.standard_normal((obs.shape[0], NP))


def target_feasible(obs, uniform, tol=1e-4, max_iters=40):
    """(c) the helper's own answer to (a): an already feasible target (a row it does not converge on keeps its target of (a):
    the last iterate of an infeasible problem may hold NaNs)."""
    r = solve_nearest_many(obs, uniform, tol=tol, max_iters=max_iters)
    return np.where(r["converged"][:, None], r["action"][:, PARTIAL], uniform)
