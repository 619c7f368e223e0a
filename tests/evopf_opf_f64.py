"""Float64 yardstick of the single-step AC-OPF of EVOPF-v0 (``EVOPFEnv.opf`` / ``rpo_evopf_opf``).  Test infrastructure only,
numpy only.

The problem, per state: minimise ``obj_fn`` over x = (pg[5], qg[5], vm[14], va at the 13 non-slack buses) subject to the 28
equalities ``eq_resid = 0`` and the 48 box bounds on pg, qg, vm; the demand and the battery power ``pe`` are data, the slack
angle is ``slack_va``.  The method is a primal-dual interior point in the form of MATPOWER's MIPS (Wang, Murillo-Sanchez,
Zimmerman, Thomas 2007; MATPOWER manual app. A), restated on ``oracle.evopf``'s functions:

    slacks z > 0 on the bounds h(x) + z = 0, multipliers mu, lambda; gamma the barrier parameter
    L_x = grad f + J^T lambda + (mu_u - mu_l)
    M   = hess f + hess(lambda^T g) + diag(mu_u / z_u + mu_l / z_l)
    N   = L_x + (mu_u h_u + gamma) / z_u - (mu_l h_l + gamma) / z_l
    [[M, J^T], [J, 0]] (dx, dlambda) = (-N, -g);  dz = -h - z - dh;  dmu = -mu + (gamma - mu dz) / z
    step lengths to the boundary times xi (capped at 1), gamma <- sigma z^T mu / 48

It stops when max(|g|_inf, max h), |L_x|_inf and z^T mu are all below ``tol`` (plain, not MIPS's scaled quantities).  The
full 65 x 65 system goes to ``numpy.linalg.solve``: nothing of the kernel's elimination (generator variables eliminated, one row
per thread, dynamic pivots) is shared with this file.

``eq_resid`` is injection minus flow, so the Hessian of lambda^T g is MINUS the second derivatives of the bus powers weighted
by lambda.  With G[i,k] = Yr[k,i], B[i,k] = Yi[k,i] (``_flows`` multiplies the voltage ROW vector into Ybus), th = va_i - va_k,

    a = G cos th + B sin th        P_i = V_i sum_k V_k a_ik
    b = G sin th - B cos th        Q_i = V_i sum_k V_k b_ik
    c = lp_i a + lq_i b            F   = sum_ik V_i V_k c_ik          (= lambda^T (P, Q))
    d = -lp_i b + lq_i a           (= dc/dth; dd/dth = -c)

    F_VV   = c + c^T
    F_thth = V V^T (c + c^T) - diag(V (c V + c^T V))
    F_thV  = diag(d V - d^T V) + V[:, None] (d - d^T)
"""
import numpy as np

from oracle import evopf as ev

GRID = ev.GRID
NB, NG = GRID.nbus, GRID.ng
SLACK = int(GRID.slack[0])
# x = (pg, qg, vm, va at the non-slack buses) as positions of the 43-vector
XIDX = np.concatenate([np.arange(GRID.va0), GRID.va0 + np.setdiff1d(np.arange(NB), GRID.slack)])
NX, NEQ, NBND = len(XIDX), GRID.eq_num, 2 * NG + NB          # 37, 28, 24 bounded variables -> 48 inequalities
XMAX = np.concatenate([GRID.pmax, GRID.qmax, GRID.vmax])
XMIN = np.concatenate([GRID.pmin, GRID.qmin, GRID.vmin])
COST2 = 2.0 * GRID.quad * GRID.genbase ** 2 / GRID.obj_scale   # d2 f / d pg2
COST1 = GRID.lin * GRID.genbase / GRID.obj_scale               # d f / d pg at pg = 0
SIGMA, XI, Z0, GAMMA0 = 0.1, 0.99995, 1.0, 1.0


def lagr_hessian(action, lam, grid=GRID):
    """Hessian of lam^T eq_resid with respect to the 43-vector ``action`` [43] -> [43, 43]; only the (vm, va) block is
    non-zero (pg, qg, pe enter eq_resid linearly)."""
    vm, va = action[grid.vm0:grid.va0], action[grid.va0:grid.pe0]
    lp, lq = lam[:NB, None], lam[NB:, None]
    G, B = grid.Yr.T, grid.Yi.T
    th = va[:, None] - va[None, :]
    a = G * np.cos(th) + B * np.sin(th)
    b = G * np.sin(th) - B * np.cos(th)
    c = lp * a + lq * b
    d = -lp * b + lq * a
    cs = c + c.T
    f_vv = cs
    f_tt = np.outer(vm, vm) * cs - np.diag(vm * (cs @ vm))
    f_tv = np.diag(d @ vm - d.T @ vm) + vm[:, None] * (d - d.T)
    h = np.zeros((grid.ydim, grid.ydim))
    sv, st = slice(grid.vm0, grid.va0), slice(grid.va0, grid.pe0)
    h[sv, sv], h[st, st], h[st, sv], h[sv, st] = -f_vv, -f_tt, -f_tv, -f_tv.T
    return h


def flat_start(pe, grid=GRID):
    """Middle of every box, angles zero (the slack's: slack_va), the given pe -> [43]."""
    a = np.zeros(grid.ydim)
    a[:NBND] = 0.5 * (XMAX + XMIN)
    a[grid.va0 + SLACK] = grid.slack_va[0]
    a[grid.pe0:] = pe
    return a


def infeasibility(demand, action, grid=GRID):
    """max(|eq_resid|_inf, largest excess over a bound of pg, qg, vm) of rows [n, 43] against demands [n, >= 28], float64."""
    action = np.asarray(action, dtype=np.float64)
    eq = np.abs(ev.eq_resid(np.asarray(demand, dtype=np.float64), action, grid)).max(axis=1)
    xb = action[:, :NBND]
    return np.maximum(eq, np.maximum(xb - XMAX, XMIN - xb).max(axis=1))


def solve(demand, pe=None, tol=1e-4, max_iters=40, grid=GRID):
    """One state: demand [>= 28] (pd, qd), pe [5] (None: zeros).  -> dict(action [43], cost, iters, converged, residual):
    ``residual`` is the largest of the three stop quantities at exit, ``iters`` the number of steps taken."""
    s = np.asarray(demand, dtype=np.float64)[None, :2 * NB]
    pe = np.zeros(grid.ne) if pe is None else np.asarray(pe, dtype=np.float64)
    a = flat_start(pe, grid)
    h = np.concatenate([a[:NBND] - XMAX, XMIN - a[:NBND]])
    z = np.maximum(-h, Z0)
    gamma = GAMMA0
    mu = gamma / z
    lam = np.zeros(NEQ)
    it, converged = 0, False
    while True:
        g = ev.eq_resid(s, a[None], grid)[0]
        J = ev.eq_jac(a[None], grid)[0][:, XIDX]
        h = np.concatenate([a[:NBND] - XMAX, XMIN - a[:NBND]])
        df = np.zeros(NX)
        df[:NG] = COST2 * a[:NG] + COST1
        dmu = np.zeros(NX)
        dmu[:NBND] = mu[:NBND] - mu[NBND:]
        lx = df + J.T @ lam + dmu
        with np.errstate(all="ignore"):
            residual = max(np.abs(g).max(), h.max(), np.abs(lx).max(), float(z @ mu))
        if residual < tol:
            converged = True
            break
        if it >= max_iters:
            break
        with np.errstate(all="ignore"):
            M = lagr_hessian(a, lam, grid)[np.ix_(XIDX, XIDX)]
            M[np.arange(NG), np.arange(NG)] += COST2
            M[np.arange(NBND), np.arange(NBND)] += mu[:NBND] / z[:NBND] + mu[NBND:] / z[NBND:]
            N = lx.copy()
            N[:NBND] += (mu[:NBND] * h[:NBND] + gamma) / z[:NBND] - (mu[NBND:] * h[NBND:] + gamma) / z[NBND:]
            K = np.zeros((NX + NEQ, NX + NEQ))
            K[:NX, :NX], K[:NX, NX:], K[NX:, :NX] = M, J.T, J
            try:
                sol = np.linalg.solve(K, np.concatenate([-N, -g]))
            except np.linalg.LinAlgError:
                sol = np.full(NX + NEQ, np.nan)
            dx, dlam = sol[:NX], sol[NX:]
            dh = np.concatenate([dx[:NBND], -dx[:NBND]])
            dz = -h - z - dh
            dm = -mu + (gamma - mu * dz) / z
            neg = dz < 0
            alpha_p = min(XI * np.min(z[neg] / -dz[neg]), 1.0) if neg.any() else 1.0
            neg = dm < 0
            alpha_d = min(XI * np.min(mu[neg] / -dm[neg]), 1.0) if neg.any() else 1.0
            a[XIDX] += alpha_p * dx
            z = z + alpha_p * dz
            lam = lam + alpha_d * dlam
            mu = mu + alpha_d * dm
            gamma = SIGMA * float(z @ mu) / (2 * NBND)
        it += 1
    return dict(action=a, cost=float(ev.obj_fn(a[None], grid)[0]), iters=it, converged=converged, residual=float(residual))


def solve_many(demand, pe=None, tol=1e-4, max_iters=40, grid=GRID):
    """Rows of ``solve`` -> dict of arrays (action [n, 43], cost, iters, converged, residual)."""
    demand = np.asarray(demand, dtype=np.float64)
    res = [solve(demand[i], None if pe is None else pe[i], tol, max_iters, grid) for i in range(demand.shape[0])]
    return dict(action=np.stack([r["action"] for r in res]), cost=np.array([r["cost"] for r in res]),
                iters=np.array([r["iters"] for r in res], dtype=np.int32),
                converged=np.array([r["converged"] for r in res], dtype=bool),
                residual=np.array([r["residual"] for r in res]))


def fixture_states(grid=GRID):
    """The 384 states of tests/golden/evopf_opf.npz: demand [384, 28] of lanes 0..7, episodes 0..1, hours 0..23 of seed 11 (lane
    outermost, then episode, then hour) and pe [384, 5]: zero on even lanes, one uniform draw in the B_PMIN / B_PMAX box per odd
    lane (numpy.random.default_rng(1), lanes in loop order)."""
    rng = np.random.default_rng(1)
    demand, pes = [], []
    for lane in range(8):
        pe = rng.uniform(ev.ETA_OUT * ev.B_PMIN, ev.B_PMAX / ev.ETA_IN, size=grid.ne) if lane % 2 else np.zeros(grid.ne)
        for ep in range(2):
            for t in range(ev.T):
                demand.append(ev.episode_demand(11, np.array([lane]), ep, t, grid)[0])
                pes.append(pe)
    return np.stack(demand), np.stack(pes)
