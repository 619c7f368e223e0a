"""Float64 yardstick of the single-step AC-OPF of EVOPF-v0 (``EVOPFEnv.opf`` / ``rpo_evopf_opf``).  Test infrastructure only,
numpy only.  First half: the helper ``solve`` (the method, iterated).  Second half, on tests/evopf_f64.py's arithmetics: ``step_ref``
(ONE iteration from a given state, with the error bound of the float32 kernel's every output), ``emu_opf`` (the kernel in float32),
the constants C_REF measured from it, and the inputs of tests/test_evopf_opf_f64_gpu.py.

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


class Prob(object):
    """The data of one problem family: the grid (Ybus, index sets) for ``oracle.evopf``'s functions, the 24 upper and lower
    bounds of (pg, qg, vm) and the cost derivatives.  ``PROB64``: the reference's float64 case; ``prob_of_table``: the float32
    constants table the kernel reads, as float64 numbers."""

    def __init__(self, grid, xmax, xmin, cost2, cost1):
        self.grid, self.xmax, self.xmin, self.cost2, self.cost1 = grid, xmax, xmin, cost2, cost1


PROB64 = Prob(GRID, XMAX, XMIN, COST2, COST1)


def ip_eval(prob, s, a, lam, z, mu):
    """What one iterate is judged by: g, J (columns XIDX), h, L_x and the stop quantities (``residual`` their largest)."""
    grid = prob.grid
    g = ev.eq_resid(s, a[None], grid)[0]
    J = ev.eq_jac(a[None], grid)[0][:, XIDX]
    h = np.concatenate([a[:NBND] - prob.xmax, prob.xmin - a[:NBND]])
    df = np.zeros(NX)
    df[:NG] = prob.cost2 * a[:NG] + prob.cost1
    dmu = np.zeros(NX)
    dmu[:NBND] = mu[:NBND] - mu[NBND:]
    lx = df + J.T @ lam + dmu
    with np.errstate(all="ignore"):
        residual = max(np.abs(g).max(), h.max(), np.abs(lx).max(), float(z @ mu))
        feas, grad, comp = max(np.abs(g).max(), h.max()), np.abs(lx).max(), float(z @ mu)
    return dict(g=g, J=J, h=h, lx=lx, residual=residual, feas=feas, grad=grad, comp=comp)


def ip_advance(prob, e, a, lam, z, mu, gamma):
    """One interior-point iteration from (a, lam, z, mu, gamma), ``e`` = ip_eval there: the full 65 x 65 system through LAPACK.
    -> (a, lam, z, mu, gamma) of the next iterate and dict(alpha_p, alpha_d, sol)."""
    grid = prob.grid
    g, J, h, lx = e["g"], e["J"], e["h"], e["lx"]
    a = a.copy()
    with np.errstate(all="ignore"):
        M = lagr_hessian(a, lam, grid)[np.ix_(XIDX, XIDX)]
        M[np.arange(NG), np.arange(NG)] += prob.cost2
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
    return (a, lam, z, mu, gamma), dict(alpha_p=alpha_p, alpha_d=alpha_d, sol=sol)


def flat_state(pe, prob=PROB64):
    """(a, lam, z, mu, gamma) of the flat start."""
    a = flat_start(pe, prob.grid)
    h = np.concatenate([a[:NBND] - prob.xmax, prob.xmin - a[:NBND]])
    z = np.maximum(-h, Z0)
    gamma = GAMMA0
    return a, np.zeros(NEQ), z, gamma / z, gamma


def solve(demand, pe=None, tol=1e-4, max_iters=40, grid=GRID):
    """One state: demand [>= 28] (pd, qd), pe [5] (None: zeros).  -> dict(action [43], cost, iters, converged, residual):
    ``residual`` is the largest of the three stop quantities at exit, ``iters`` the number of steps taken.  The iteration itself is
    ``ip_eval`` / ``ip_advance``, which ``step_ref`` holds the kernel to one step at a time."""
    prob = PROB64 if grid is GRID else Prob(grid, XMAX, XMIN, COST2, COST1)
    s = np.asarray(demand, dtype=np.float64)[None, :2 * NB]
    pe = np.zeros(grid.ne) if pe is None else np.asarray(pe, dtype=np.float64)
    st = flat_state(pe, prob)
    it, converged = 0, False
    while True:
        e = ip_eval(prob, s, *st[:4])
        if e["residual"] < tol:
            converged = True
            break
        if it >= max_iters:
            break
        st, _ = ip_advance(prob, e, *st)
        it += 1
    a = st[0]
    return dict(action=a, cost=float(ev.obj_fn(a[None], grid)[0]), iters=it, converged=converged, residual=float(e["residual"]))


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


# =====================================================================================================================
# One iteration at a time: the kernel's formulas ONCE against an arithmetic ``A`` of tests/evopf_f64.py (B64E: float64 with the
# running error bound in units of eps32 -- the bound of ``step_ref``; F32E: one float32 rounding per operation in the kernel's
# order -- the emulation ``emu_opf``), the float64 VALUES from the full 65 x 65 system above.
#
# The bound of the linear solve.  evopf_f64.py's |inv K| ((|K| + m_K) |sol| + |rhs| + m_rhs) is the first-order error of a
# componentwise backward-stable elimination.  The kernel's is a Gauss-Jordan elimination with partial pivoting on a matrix whose
# rows differ in scale by mu / z (up to 1e12 on the states below): that is neither invariant under row scaling nor backward stable
# (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., theorem 14.5), and the faithful float32 emulation exceeds that
# bound by up to 1e6 on the synthetic states and 1e5 on late trajectory iterates.  The bound here is the one that theorem gives for
# the elimination actually performed, still componentwise and never a norm:
#     |inv K| ((|L| |U| + m_K) |sol| + |rhs| + m_rhs) + |inv U| |U| |sol|
# with L, U the factors of the kernel's pivot rule in float64 (``pivoted_factors``).  |L| |U| >= |K|, so it is never tighter than
# the other, and it equals it where the pivots do not grow and U is well conditioned (the early iterates).
#
# State row (RPO_EVOPF_OPF_STATE = 168 floats): action[43] | lambda[28] | z_u[24] | z_l[24] | mu_u[24] | mu_l[24] | gamma, the
# bounded variables in the order of XMAX / XMIN.  Tolerance of an element = MARGIN (4) * C_REF[group] * eps32 * bound.
# =====================================================================================================================
import evopf_f64 as E  # noqa: E402
from evopf_f64 import B64E, EPS32, F32E, MARGIN, V  # noqa: E402

OPF_STATE = E.DEF["RPO_EVOPF_OPF_STATE"]
S_X, S_LAM, S_ZU, S_ZL = slice(0, 43), slice(43, 71), slice(71, 95), slice(95, 119)
S_MUU, S_MUL, S_GAMMA = slice(119, 143), slice(143, 167), 167
GROUP_COLS = {"opf_x": S_X, "opf_lam": S_LAM, "opf_zmu": slice(71, 168)}
NVAR, NKKT = 2 * NB - 1, 2 * NB - 1 + NEQ                    # 27 voltage unknowns, 55 rows of the reduced system
VAR_X = [E.VM0 + k for k in range(NB)] + [E.VA0 + k for k in range(1, NB)]      # action index of voltage lane k (bus 0: slack)
BND_EQ = [E.SPV[g] for g in range(NG)] + [NB + E.SPV[g] for g in range(NG)]    # equation of generator variable b < 10
BND_LANE = [NVAR + e for e in BND_EQ] + list(range(NB))                       # lane that owns bounded variable b

# measured by test_evopf_opf.py::test_yardstick_constants from emu_opf on the CPU, on the inputs of test_evopf_opf_f64_gpu.py
# (trajectory states of the 70 fixture rows, opf_states under both tables), never from a device
C_REF = {
    "opf_x": 0.46,         # measured 0.449: x after one step
    "opf_lam": 0.32,       # measured 0.309: lambda after one step
    "opf_zmu": 0.47,       # measured 0.455: slacks, multipliers and gamma after one step
    "opf_stop": 0.215,     # measured 0.205: the three stop quantities and residual
    "opf_cost": 0.215,     # measured 0.205: cost (next to the explicit half ulp of the table's coefficients, cost_ref)
}
MUTATIONS = ("untransposed", "cs_no_ct", "thth_no_diag", "thv_no_diag", "hess_sign", "no_sig_vm", "kdiag_no_sig", "rhs_plus_g",
             "dzl_sign", "xi_one", "alpha_p_for_mu", "gamma_24", "tie_highest", "no_c1")


def ratios(group, got, ref_vals, ref_mag, extra=0.0):
    """|got - ref| / (MARGIN * C_REF[group] * eps32 * bound) per element, the rule of evopf_f64.ratios with this file's constants
    (evopf_f64.C_REF is iterated by its own tests and stays theirs).  -> (ratios, not judged): an element whose bound or float64
    value is not finite is not judged (ratio 0, counted); a NaN from the kernel where float64 is finite is inf.  ``extra``: an
    explicit term of the tolerance in units of eps32, outside the measured constant (as evopf_f64's intrinsic term)."""
    got, ref_vals, ref_mag = (np.asarray(x, np.float64) for x in (got, ref_vals, ref_mag))
    tol = MARGIN * C_REF[group] * EPS32 * ref_mag + EPS32 * np.asarray(extra, np.float64)
    with np.errstate(all="ignore"):
        err = np.abs(got - ref_vals)
        unj = ~np.isfinite(tol) | ~np.isfinite(ref_vals)
        r = np.where(err == 0, 0.0, err / np.maximum(tol, E.ef.TINY))
        r = np.where(unj, 0.0, np.where(np.isnan(r), np.inf, r))
    return r, unj


def prob_of_table(consts):
    """The problem the KERNEL solves: the float32 constants table as float64 numbers."""
    import copy
    t = np.asarray(consts, np.float32).astype(np.float64)
    seg = lambda name, n: t[E.OFF[name]:E.OFF[name] + n]                                                   # noqa: E731
    grid = copy.copy(GRID)
    grid.Yr, grid.Yi = seg("YR", NB * NB).reshape(NB, NB), seg("YI", NB * NB).reshape(NB, NB)
    return Prob(grid, np.concatenate([seg("PMAX", NG), seg("QMAX", NG), seg("VMAX", NB)]),
                np.concatenate([seg("PMIN", NG), seg("QMIN", NG), seg("VMIN", NB)]), 2.0 * seg("QUAD", NG), seg("LIN", NG))


def shifted_table(consts, phi=0.125, f=3, t=6):
    """The table with a phase shifter of ``phi`` rad on the transformer between buses f and t (4 and 7 of the IEEE numbering): Ybus
    stops being symmetric, which the case's own (no shifter) is exactly -- on it, reading Yr / Yi transposed or not is the same
    thing, and no test on the committed table could tell."""
    out = np.asarray(consts, np.float32).copy()
    yr, yi = (out[E.OFF[k]:E.OFF[k] + NB * NB].reshape(NB, NB) for k in ("YR", "YI"))
    assert yr[f, t] != 0 or yi[f, t] != 0
    for (i, k), ang in (((f, t), phi), ((t, f), -phi)):
        y = complex(yr[i, k], yi[i, k]) * complex(np.cos(ang), np.sin(ang))
        yr[i, k], yi[i, k] = y.real, y.imag
    return out


def _add(a, b):
    return b if a is None else (a if b is None else a + b)


def _neg(a):
    return None if a is None else -a


def _mul(a, b):
    return None if (a is None or b is None) else a * b


def _fma(A, a, b, c):
    """fmaf(a, b, c); c None = 0."""
    if a is None or b is None:
        return c
    if c is None:
        return a * b
    return E.fma(a, b, c) if A is F32E else a * b + c


def wave_sum_rows(A, lanes):
    """rpo_wave_sum_rows over 64 lanes (None = 0): per 16-lane row u_l = (v_l + v_l+8) + (v_l+4 + v_l+12), (u_0 + u_2) + (u_1 + u_3);
    then (r0 + r1) + (r2 + r3)."""
    v = list(lanes) + [None] * (64 - len(lanes))
    rows = []
    for r in range(4):
        w = v[16 * r:16 * r + 16]
        u = [_add(_add(w[j], w[j + 8]), _add(w[j + 4], w[j + 12])) for j in range(4)]
        rows.append(_add(_add(u[0], u[2]), _add(u[1], u[3])))
    return _add(_add(rows[0], rows[1]), _add(rows[2], rows[3]))


NEAR = 8.0                 # a losing candidate of a maximum counts while it lies within NEAR * eps32 * (both bounds) of the winner


def _max2(A, a, b):
    """fmaxf(a, b).  It is continuous, so no case is split, but its error is that of whichever candidate wins in float32: under
    B64E the bound is the larger of the two wherever the loser lies within NEAR * eps32 * (m_a + m_b) of the winner."""
    if A is F32E:
        return np.fmax(a, b)
    a, b = V.of(a), V.of(b)
    with np.errstate(all="ignore"):
        first = (a.v >= b.v) | np.isnan(b.v)
        near = np.abs(a.v - b.v) <= NEAR * EPS32 * (a.m + b.m)
        return V(np.where(first, a.v, b.v), np.where(near, np.fmax(a.m, b.m), np.where(first, a.m, b.m)))


def _min2(A, a, b):
    return -_max2(A, -a, -b)


def _maxs(A, xs):
    acc = None
    for x in xs:
        if x is not None:
            acc = x if acc is None else _max2(A, acc, x)
    return acc


def state_cols(A, state):
    """[n, 168] float32 -> dict of column lists of ``A``."""
    c = E.cols(A, state)
    return dict(x=c[S_X], lam=c[S_LAM], zu=c[S_ZU], zl=c[S_ZL], muu=c[S_MUU], mul=c[S_MUL], gamma=c[S_GAMMA])


def kkt(A, c, s, st, mut=()):
    """The lanes' rows of [[H_vv + Sigma, J_v^T], [J_v, -S D^-1 S^T]] | rhs in the kernel's formulas (csrc/evopf_opf.hip), with
    everything the step needs afterwards and the stop quantities at ``st``.  Entries: None = structural zero."""
    x, lam, gamma = st["x"], st["lam"], st["gamma"]
    f = E.flows(A, c, x)
    g = E.eq_resid(A, c, s, x, f)
    hi, lo = c.pmax + c.qmax + c.vmax, c.pmin + c.qmin + c.vmin
    hu, hl, sig, nbar, dmu = [], [], [], [], []
    for b in range(NBND):
        zu, zl, mu_u, mu_l = st["zu"][b], st["zl"][b], st["muu"][b], st["mul"][b]
        hu.append(x[b] - hi[b])
        hl.append(lo[b] - x[b])
        sig.append(mu_u / zu + mu_l / zl)
        nbar.append((mu_u * hu[b] + gamma) / zu - (mu_l * hl[b] + gamma) / zl)
        dmu.append(mu_u - mu_l)
    lxu, du, nu, kdiag = [], [], [], []
    for b in range(2 * NG):
        lam_e = lam[BND_EQ[b]]
        if b < NG:
            c2 = A.k(2.0) * c.quad[b]
            df = c2 * x[b] if "no_c1" in mut else c2 * x[b] + c.lin[b]
            lxu.append(df + lam_e + dmu[b])
            du.append(c2 + sig[b])
            kdiag.append(A.k(-1.0) / (c2 if "kdiag_no_sig" in mut else du[b]))
        else:
            lxu.append(lam_e + dmu[b])
            du.append(sig[b])
            kdiag.append(A.k(-1.0) / du[b])
        nu.append(lxu[b] + nbar[b])
    # Hessian coefficients of bus m against bus n (zero off the branch pattern: both admittances are)
    vmag = [x[E.VM0 + n] for n in range(NB)]
    csn, ddn, csv, dv = [[None] * NB for _ in range(NB)], [[None] * NB for _ in range(NB)], [None] * NB, [None] * NB
    cs, sn = f["cs"], f["sn"]
    for m in range(NB):
        lpm, lqm = lam[m], lam[NB + m]
        for n in range(NB):
            if not c.adj[m][n] and not c.adj[n][m]:
                continue
            if "untransposed" in mut:
                gmn, bmn, gnm, bnm = c.yr[m][n], c.yi[m][n], c.yr[n][m], c.yi[n][m]
            else:
                gmn, bmn, gnm, bnm = c.yr[n][m], c.yi[n][m], c.yr[m][n], c.yi[m][n]
            if m == n:
                amn, bbmn, anm, bbnm = gmn, -bmn, gnm, -bnm
            else:
                C, S = cs[m] * cs[n] + sn[m] * sn[n], sn[m] * cs[n] - cs[m] * sn[n]
                amn, bbmn = gmn * C + bmn * S, gmn * S - bmn * C
                anm, bbnm = gnm * C - bnm * S, -gnm * S - bnm * C
            lpn, lqn = lam[n], lam[NB + n]
            cmn, cnm = lpm * amn + lqm * bbmn, lpn * anm + lqn * bbnm
            dmn, dnm = -lpm * bbmn + lqm * amn, -lpn * bbnm + lqn * anm
            csn[m][n] = cmn if "cs_no_ct" in mut else cmn + cnm
            ddn[m][n] = dmn - dnm
            csv[m] = _fma(A, csn[m][n], vmag[n], csv[m])
            dv[m] = _fma(A, ddn[m][n], vmag[n], dv[m])
    jac = [[E.jac_entry(A, c, f, e, var) for var in range(E.PE0)] for e in range(NEQ)]
    K = [[None] * NKKT for _ in range(NKKT)]
    rhs, lxv = [None] * NKKT, []
    for k in range(NVAR):
        is_vm = k < NB
        m = k if is_vm else k - (NB - 1)
        for col in range(NVAR):
            col_vm = col < NB
            n = col if col_vm else col - (NB - 1)
            same = m == n
            if is_vm:
                if col_vm:
                    v = _neg(csn[m][n])
                else:
                    v = _neg(dv[m]) if (same and "thv_no_diag" not in mut) else _mul(vmag[n], ddn[m][n])
            elif col_vm:
                v = _neg(_add(dv[m] if (same and "thv_no_diag" not in mut) else None, _mul(vmag[m], ddn[m][n])))
            else:
                v = _add(_mul(vmag[m], csv[m]) if (same and "thth_no_diag" not in mut) else None,
                         _neg(_mul(_mul(vmag[m], vmag[n]), csn[m][n])))
            if "hess_sign" in mut:
                v = _neg(v)
            if is_vm and k == col and "no_sig_vm" not in mut:
                v = _add(v, sig[2 * NG + m])
            K[k][col] = v
        jtl = None
        for e in range(NEQ):
            K[k][NVAR + e] = jac[e][VAR_X[k]]
            jtl = _fma(A, jac[e][VAR_X[k]], lam[e], jtl)
        lxv.append(jtl + dmu[2 * NG + m] if is_vm else jtl)
        rhs[k] = -(lxv[k] + nbar[2 * NG + m]) if is_vm else -lxv[k]
    for e in range(NEQ):
        for col in range(NVAR):
            K[NVAR + e][col] = jac[e][VAR_X[col]]
        rhs[NVAR + e] = -g[e]
    for b in range(2 * NG):
        e = BND_EQ[b]
        K[NVAR + e][NVAR + e] = kdiag[b]
        q = nu[b] / du[b]
        rhs[NVAR + e] = q + g[e] if "rhs_plus_g" in mut else q - g[e]
    # stop quantities: max(|g|_inf, max h), |L_x|_inf, z^T mu in the wave's order
    zero = A.k(0.0)
    feas = _maxs(A, [A.abs(v) for v in g] + hu + hl + [zero])
    grad = _maxs(A, [A.abs(v) for v in lxv + lxu])
    lanes = [None] * 64
    for b in range(NBND):
        lanes[BND_LANE[b]] = st["zu"][b] * st["muu"][b] + st["zl"][b] * st["mul"][b]
    comp = wave_sum_rows(A, lanes)
    resid = _max2(A, _max2(A, feas, grad), comp)
    return dict(K=K, rhs=rhs, g=g, hu=hu, hl=hl, nu=nu, du=du, lxv=lxv, lxu=lxu, feas=feas, grad=grad, comp=comp, resid=resid)


def advance(A, st, q, delta, mut=()):
    """From the solution ``delta`` [55] of the reduced system: the eliminated generator steps, dz, dmu, the two step lengths, the
    updates and gamma, in the kernel's formulas.  -> (next state as state_cols, alpha_p, alpha_d)."""
    x, lam, gamma = st["x"], st["lam"], st["gamma"]
    one, zero = A.k(1.0), A.k(0.0)
    xi = one if "xi_one" in mut else A.k(XI)
    dx = [None] * NBND
    for b in range(2 * NG):
        dx[b] = (-q["nu"][b] - delta[NVAR + BND_EQ[b]]) / q["du"][b]
    for m in range(NB):
        dx[2 * NG + m] = delta[m]
    dzu, dzl, dmu_u, dmu_l, qp, qd = [], [], [], [], [], []
    for b in range(NBND):
        zu, zl, mu_u, mu_l = st["zu"][b], st["zl"][b], st["muu"][b], st["mul"][b]
        dzu.append(-q["hu"][b] - zu - dx[b])
        dzl.append((-q["hl"][b] - zl - dx[b]) if "dzl_sign" in mut else (-q["hl"][b] - zl + dx[b]))
        dmu_u.append(-mu_u + (gamma - mu_u * dzu[b]) / zu)
        dmu_l.append(-mu_l + (gamma - mu_l * dzl[b]) / zl)
        qp.append(_max2(A, _max2(A, -dzu[b] / zu, -dzl[b] / zl), zero))
        qd.append(_max2(A, _max2(A, -dmu_u[b] / mu_u, -dmu_l[b] / mu_l), zero))
    qp, qd = _maxs(A, qp), _maxs(A, qd)
    alpha_p = A.where(A.val(qp) > 0, _min2(A, xi / qp, one), one)
    alpha_d = A.where(A.val(qd) > 0, _min2(A, xi / qd, one), one)
    if "alpha_p_for_mu" in mut:
        alpha_d = alpha_p
    nx = list(x)
    for b in range(2 * NG):
        nx[b] = x[b] + alpha_p * dx[b]
    for k in range(NVAR):
        nx[VAR_X[k]] = x[VAR_X[k]] + alpha_p * delta[k]
    nlam = [lam[e] + alpha_d * delta[NVAR + e] for e in range(NEQ)]
    nzu = [st["zu"][b] + alpha_p * dzu[b] for b in range(NBND)]
    nzl = [st["zl"][b] + alpha_p * dzl[b] for b in range(NBND)]
    nmu = [st["muu"][b] + alpha_d * dmu_u[b] for b in range(NBND)]
    nml = [st["mul"][b] + alpha_d * dmu_l[b] for b in range(NBND)]
    lanes = [None] * 64
    for b in range(NBND):
        lanes[BND_LANE[b]] = nzu[b] * nmu[b] + nzl[b] * nml[b]
    ngamma = A.k(SIGMA) * wave_sum_rows(A, lanes) / A.k(float(NBND if "gamma_24" in mut else 2 * NBND))
    return dict(x=nx, lam=nlam, zu=nzu, zl=nzl, muu=nmu, mul=nml, gamma=ngamma), alpha_p, alpha_d


def _pack(A, st, n, what):
    cols_ = st["x"] + st["lam"] + st["zu"] + st["zl"] + st["muu"] + st["mul"] + [st["gamma"]]
    fn = A.val if what == "val" else A.mag
    return np.stack([np.broadcast_to(np.asarray(fn(v)), (n,)) for v in cols_], axis=1)


def _dense(A, K, rhs, n):
    kv, km = np.zeros((n, NKKT, NKKT + 1)), np.zeros((n, NKKT, NKKT + 1))
    for r in range(NKKT):
        for col, v in enumerate(K[r] + [rhs[r]]):
            if v is not None:
                kv[:, r, col], km[:, r, col] = A.val(v), A.mag(v)
    return kv, km


def split_state(row):
    """One state row [168] float64 -> (a, lam, z, mu, gamma) of ip_eval / ip_advance."""
    return (row[S_X].copy(), row[S_LAM].copy(), np.concatenate([row[S_ZU], row[S_ZL]]), np.concatenate([row[S_MUU], row[S_MUL]]),
            float(row[S_GAMMA]))


def join_state(a, lam, z, mu, gamma):
    return np.concatenate([a, lam, z, mu, [gamma]])


def pivoted_factors(k_):
    """|L| |U| (in the rows' own order) and U of the elimination the kernel performs on ``k_`` [55, 55], in float64: the pivot of
    column k is the largest |entry| among the rows that own none yet, the lowest row among equals; rows are not swapped."""
    n = k_.shape[0]
    a, low, u, used = k_.copy(), np.zeros((n, n)), np.zeros((n, n)), np.zeros(n, bool)
    for k in range(n):
        p = int(np.where(used, -1.0, np.abs(a[:, k])).argmax())
        used[p] = True
        f = np.where(used, 0.0, a[:, k] / a[p, k])
        low[:, k], u[k] = np.abs(f), a[p]
        low[p, k] = 1.0
        a = a - np.outer(f, a[p])
    return low @ np.abs(u), u


def step_ref(consts, demand, state, bound=True):
    """One interior-point iteration in float64 from the float32 states [n, 168] for the demands [n, >= 28], on the constants
    table the kernel reads.  Values: ip_eval / ip_advance, the full 65 x 65 system through LAPACK, the statement of the method that
    ``solve`` iterates (``consts`` None: the reference's float64 case and the state as given -- solve()'s own iteration).
    -> dict(state [n, 168] the next state, stop [n, 4] = (feasibility, |L_x|, z^T mu, residual) AT THE INPUT STATE, alpha [n, 2] =
    (alpha_p, alpha_d)) and, with ``bound``, state_m / stop_m / alpha_m: the bound of each in units of eps32.  The bound is built
    on the REDUCED system in the kernel's formulas under B64E (``kkt``): every entry carries its running bound, the solution gets
    the componentwise |inv K| ((|L| |U| + m_K) |sol| + |rhs| + m_rhs) + |inv U| |U| |sol| (below), and ``advance`` propagates it to
    first order through the
    eliminated steps, the quotient maxima, the step lengths and the updates (min(xi / q, 1) and the maxima are continuous: no case
    split).  An element whose bound is not finite is not judged (``ratios`` counts it)."""
    prob = PROB64 if consts is None else prob_of_table(consts)
    demand = np.asarray(demand)
    state = np.asarray(state) if consts is None else np.asarray(state, np.float32)
    n = state.shape[0]
    s64, st64 = demand.astype(np.float64)[:, :2 * NB], state.astype(np.float64)
    out = dict(state=np.zeros((n, OPF_STATE)), stop=np.zeros((n, 4)), alpha=np.zeros((n, 2)))
    sol = np.zeros((n, NX + NEQ))
    for r in range(n):
        cur = split_state(st64[r])
        e = ip_eval(prob, s64[r][None], *cur[:4])
        nxt, info = ip_advance(prob, e, *cur)
        out["state"][r] = join_state(*nxt)
        out["stop"][r] = e["feas"], e["grad"], e["comp"], e["residual"]
        out["alpha"][r] = info["alpha_p"], info["alpha_d"]
        sol[r] = info["sol"]
    nonfinite = ~np.isfinite(st64).all(axis=1)                    # a NaN in the state: nothing to hold the kernel to but NaNs
    out["state"][nonfinite], out["stop"][nonfinite] = np.nan, np.nan
    if not bound:
        return out
    with np.errstate(all="ignore"):
        c = E.Tab(B64E, consts)
        st = state_cols(B64E, state)
        q = kkt(B64E, c, E.cols(B64E, np.asarray(demand, np.float32)[:, :2 * NB]), st)
        kv, km = _dense(B64E, q["K"], q["rhs"], n)
        sol55 = sol[:, 2 * NG:]                                   # (vm, va at the non-slack buses, dlambda): the reduced unknowns
        bnd = np.full((n, NKKT), np.inf)
        for r in range(n):
            if not np.isfinite(kv[r]).all():
                continue
            k_, x_ = kv[r, :, :NKKT], np.abs(sol55[r])
            lu, u = pivoted_factors(k_)
            try:
                inner = (lu + km[r, :, :NKKT]) @ x_ + np.abs(kv[r, :, NKKT]) + km[r, :, NKKT]
                bnd[r] = np.abs(np.linalg.inv(k_)) @ inner + np.abs(np.linalg.inv(u)) @ (np.abs(u) @ x_)
            except np.linalg.LinAlgError:
                pass
        delta = [V(sol55[:, k], bnd[:, k]) for k in range(NKKT)]
        nxt, ap, ad = advance(B64E, st, q, delta)
        out["state_m"] = _pack(B64E, nxt, n, "mag")
        out["reduced_dev"] = np.abs(_pack(B64E, nxt, n, "val") - out["state"])      # reduced against full system, for the record
        out["stop_m"] = E.mag(B64E, [q["feas"], q["grad"], q["comp"], q["resid"]])
        out["alpha_m"] = E.mag(B64E, [ap, ad])
        # first order only: where a step length is not pinned to a quarter of itself (eps32 * MARGIN * its bound against its value:
        # the solution of a system beyond float32, late iterates of infeasible problems), the products alpha * dx are not bounded
        # by first-order terms and the row is not judged
        out["first_order"] = np.isfinite(out["alpha_m"]).all(axis=1) & \
            (MARGIN * EPS32 * out["alpha_m"] <= FIRST_ORDER * np.abs(out["alpha"])).all(axis=1)
    return out


FIRST_ORDER = 0.25


def check_step(ref, got_state):
    """Every component of the state after one step against ``step_ref``'s, group by group -> ({group: worst ratio}, rows not
    judged [n] bool: a bound that is not finite, or ``first_order`` False)."""
    out, left = {}, ~ref["first_order"]
    for group, sl in GROUP_COLS.items():
        r, unj = ratios(group, np.asarray(got_state)[:, sl], ref["state"][:, sl], ref["state_m"][:, sl])
        left = left | unj.any(axis=1)
    for group, sl in GROUP_COLS.items():
        r, _ = ratios(group, np.asarray(got_state)[:, sl], ref["state"][:, sl], ref["state_m"][:, sl])
        out[group] = float(r[~left].max()) if (~left).any() else 0.0
    return out, left


def check_stop(ref, got):
    """The stop quantities at the INPUT state: ``got`` [n, 4] (feasibility, |L_x|, z^T mu, residual) or [n] (residual alone, what
    the kernel reports) -> (worst ratio, rows not judged)."""
    got = np.asarray(got)
    sl = slice(0, 4) if got.ndim == 2 else 3
    r, unj = ratios("opf_stop", got, ref["stop"][:, sl], ref["stop_m"][:, sl])
    r, unj = (r, unj) if got.ndim == 1 else (r.max(axis=1), unj.any(axis=1))
    return (float(r[~unj].max()) if (~unj).any() else 0.0), unj


def cost_ref(consts, action):
    """``obj_fn`` in float64 at the float32 points [n, 43] and the bound of the kernel's cost (quad pg pg + lin pg per generator,
    rpo_wave_sum_rows, + const) in units of eps32; the table's entries are the float32 roundings of the reference's coefficients,
    half an ulp each on |quad pg^2|, |lin pg| and |const|: the explicit term.  -> (values, bound, explicit term)."""
    c = E.Tab(B64E, consts)
    a = E.cols(B64E, np.asarray(action, np.float32))
    parts = [c.quad[g] * a[g] * a[g] + c.lin[g] * a[g] for g in range(NG)]
    cost = wave_sum_rows(B64E, parts) + c.const
    tab = sum(np.abs((c.quad[g] * a[g] * a[g]).v) + np.abs((c.lin[g] * a[g]).v) for g in range(NG)) + np.abs(c.const.v)
    return ev.obj_fn(np.asarray(action, np.float32).astype(np.float64)), B64E.mag(cost), 0.5 * tab


# ---------------------------------------------------------------------------------------------------- the float32 emulation
def emu_gj_exact(m, highest=False):
    """gj_dynamic<0, 55, 0, 56, PickExact64> on [n, 55, 56]: the pivot of column k is the largest |entry| among the rows that own
    none yet, compared exactly, the LOWEST row among equals (``highest``: the seeded mutation); if no candidate compares equal
    (NaNs), the lowest free row.  Rows are not swapped.  -> (pivots [n, 55], mycol [n, 55], the picks as (column at pick time
    [n, 55, 55], free [n, 55, 55], pick [n, 55]) for ``check_picks``)."""
    n, rows, _ = m.shape
    piv, mycol = np.ones((n, rows), np.float32), np.zeros((n, rows), np.int64)
    used = np.zeros((n, rows), bool)
    ar = np.arange(n)
    seen, free, picks = np.zeros((n, rows, rows), np.float32), np.zeros((n, rows, rows), bool), np.zeros((n, rows), np.int64)
    one = np.float32(1.0)
    with np.errstate(all="ignore"):
        for k in range(rows):
            mag = np.where(used, np.float32(0.0), np.abs(m[:, :, k]))
            top = np.fmax.reduce(mag, axis=1)
            cand = ~used & (mag == top[:, None])
            none = ~cand.any(axis=1)
            cand[none] = ~used[none]
            p = (rows - 1 - cand[:, ::-1].argmax(axis=1)) if highest else cand.argmax(axis=1)
            seen[:, k], free[:, k], picks[:, k] = m[:, :, k], ~used, p
            pk = m[ar, p, k].copy()
            fct = (-m[:, :, k] * (one / pk)[:, None]).astype(np.float32)
            fct[ar, p] = 0
            used[ar, p], mycol[ar, p], piv[ar, p] = True, k, pk
            m[:, :, k + 1:] = E.fma(fct[:, :, None], m[ar, p, k + 1:][:, None, :], m[:, :, k + 1:])
    return piv, mycol, (seen, free, picks)


def check_picks(trace):
    """The picker's rule held against what it was shown, independently of how it picked: at every column the pick is free, no
    free row is larger in magnitude, and no free row of equal magnitude has a lower index.  Rows with a NaN candidate in a column
    are left out.  -> number of violations."""
    seen, free, picks = trace
    n, rows, _ = seen.shape
    bad = 0
    with np.errstate(all="ignore"):
        mag = np.where(free, np.abs(seen.astype(np.float64)), -1.0)
        for k in range(rows):
            ok = ~np.isnan(np.where(free[:, k], seen[:, k], 0.0)).any(axis=1)
            pm = mag[np.arange(n), k, picks[:, k]]
            lower = (mag[:, k] == pm[:, None]) & (np.arange(rows)[None] < picks[:, k][:, None])
            bad += int((ok & ((pm < 0) | (mag[:, k] > pm[:, None]).any(axis=1) | lower.any(axis=1))).sum())
    return bad


def flat_state32(consts, pe):
    """The kernel's flat start as state rows [n, 168] float32: middle of every box (0.5f * (hi + lo)), angles 0 but the slack's,
    the given pe, z = max(hi - x0, 1), max(x0 - lo, 1), mu = gamma / z, lambda = 0, gamma = 1."""
    t = np.asarray(consts, np.float32)
    pe = np.asarray(pe, np.float32)
    n = pe.shape[0]
    seg = lambda name, k: t[E.OFF[name]:E.OFF[name] + k]                                                   # noqa: E731
    hi = np.concatenate([seg("PMAX", NG), seg("QMAX", NG), seg("VMAX", NB)])
    lo = np.concatenate([seg("PMIN", NG), seg("QMIN", NG), seg("VMIN", NB)])
    st = np.zeros((n, OPF_STATE), np.float32)
    x0 = np.float32(0.5) * (hi + lo)
    st[:, :NBND] = x0
    st[:, E.VA0] = t[E.OFF["VA_INIT"]]
    st[:, E.PE0:43] = pe
    st[:, S_ZU], st[:, S_ZL] = np.fmax(hi - x0, np.float32(Z0)), np.fmax(x0 - lo, np.float32(Z0))
    st[:, S_MUU], st[:, S_MUL] = np.float32(GAMMA0) / st[:, S_ZU], np.float32(GAMMA0) / st[:, S_ZL]
    st[:, S_GAMMA] = GAMMA0
    return st


def emu_opf(consts, demand, pe_or_state, tol, max_iters, mut=()):
    """evopf_opf_kernel in float32 (F32E: one rounding per operation in the kernel's order, its fmaf's as fused, the wave sums in
    lane order, PickExact64's pivots).  ``pe_or_state``: pe [n, 5] or None (the flat start) or states [n, 168].
    -> dict(action [n, 43], info [n, 4] = (cost, residual, iterations, converged), state [n, 168], stop [n, 3] the stop quantities at
    exit, picks: violations of the pivot rule counted by check_picks over every elimination)."""
    demand = np.asarray(demand, np.float32)[:, :2 * NB]
    n = demand.shape[0]
    if pe_or_state is not None and np.asarray(pe_or_state).shape[1] == OPF_STATE:
        state = np.asarray(pe_or_state, np.float32).copy()
    else:
        state = flat_state32(consts, np.zeros((n, NG), np.float32) if pe_or_state is None else pe_or_state)
    c = E.Tab(F32E, consts)
    tol32 = np.float32(tol)
    info, stop = np.zeros((n, 4), np.float32), np.zeros((n, 3), np.float32)
    active, iters, bad_picks = np.ones(n, bool), np.zeros(n, np.int64), 0
    with np.errstate(all="ignore"):
        while active.any():
            idx = np.nonzero(active)[0]
            st = state_cols(F32E, state[idx])
            q = kkt(F32E, c, E.cols(F32E, demand[idx]), st, mut)
            k = len(idx)
            three = E.val(F32E, [q["feas"], q["grad"], q["comp"]])
            nan = np.isnan(E.val(F32E, q["g"] + q["hu"] + q["lxv"] + q["lxu"] + [q["comp"]])).any(axis=1)
            resid = np.where(nan, np.float32(np.nan), np.broadcast_to(q["resid"], (k,))).astype(np.float32)
            conv = ~nan & (resid < tol32)
            done = conv | (iters[idx] >= max_iters)
            info[idx, 1], info[idx, 3], stop[idx] = resid, conv, three
            active[idx[done]] = False
            if done.all():
                break
            kv, _ = _dense(F32E, q["K"], q["rhs"], k)
            m = kv.astype(np.float32)
            piv, mycol, trace = emu_gj_exact(m, "tie_highest" in mut)
            bad_picks += check_picks(trace)
            vec = np.zeros((k, NKKT), np.float32)
            np.put_along_axis(vec, mycol, m[:, :, NKKT] / piv, axis=1)
            nxt, _, _ = advance(F32E, st, q, [vec[:, j] for j in range(NKKT)], mut)
            new = _pack(F32E, nxt, k, "val").astype(np.float32)
            go = idx[~done]
            state[go] = new[~done]
            iters[go] += 1
        pg = state[:, :NG]
        parts = [c.quad[g] * pg[:, g] * pg[:, g] + c.lin[g] * pg[:, g] for g in range(NG)]
        info[:, 0] = wave_sum_rows(F32E, parts) + c.const
    info[:, 2] = iters
    return dict(action=state[:, S_X].copy(), info=info, state=state, stop=stop, picks=bad_picks)


# ---------------------------------------------------------------------------------------------------- inputs built to go wrong
LAMBDA_SCALE = 0.3         # the helper's converged multipliers in float64, 69 converged of the fixture's first 70 states: rms 0.283,
                           # largest 0.557 (real-power rows about 0.4, reactive-power rows below 0.01)
N_SPECIAL = 10


def fixture_rows():
    """The 70 rows of test_evopf_opf_gpu._setup: the fixture's first 65 states plus its 5 infeasible ones (SLSQP's final equality
    residual > 1e-3), as the kernel's float32 inputs -> (demand [70, 28], pe [70, 5])."""
    import os
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "evopf_opf.npz")) as z:
        demand, pe, infeas = z["demand"], z["pe"], z["slsqp_eq_resid"] > 1e-3
    rows = np.concatenate([np.arange(65), np.setdiff1d(np.nonzero(infeas)[0], np.arange(65))])
    assert len(rows) == 70
    return demand[rows].astype(np.float32), pe[rows].astype(np.float32)


def opf_states(n, seed, consts=None):
    """(demand [n, 28], state [n, 168]) float32, n >= 10, every term of the iteration carrying weight: x an operating point of
    evopf_f64.make_rows (demands of Philox episodes, completed basic actions + 0.02 N(0, 1)); lambda = LAMBDA_SCALE * N(0, 1); on
    the odd rows z log-uniform over 1e-6 .. 1, gamma log-uniform over 1e-6 .. 1, mu = gamma / z times a log-uniform factor in
    0.1 .. 10; on the even rows and the first ten the same over 1e-2 .. 1, 1e-3 .. 1e-1 and 0.5 .. 2.  (Slacks drawn apart from x
    leave h + z far from 0, so most steps are cut to alpha ~ z; with z down to 1e-6 about three quarters of the wide rows have a
    step length no float32 solve pins down -- step_ref's ``first_order`` -- and are not judged; the narrower rows are.)  The first
    ten rows: 0 lambda = 0 (the Hessian vanishes); 1 a hundred times the scale on the real-power multiplier of load bus 9 (index
    8); 2 an active bound, z_u = 1e-6 with x = hi - z_u, on |v| of bus 1 and on pg of generator 1; 3..6 pe on the corners of the
    battery box (all high, all low, alternating both ways); 7 a pivot tie in the first column: lambda = 0 and Sigma of |v| at
    bus 0 set to EXACTLY the largest |d g / d v_0| of the float32 Jacobian, so lane 0 and an equation lane compare equal and
    PickExact64's lowest-lane rule decides; 8 the kernel's flat start itself; 9 a NaN in lambda."""
    assert n >= N_SPECIAL
    consts = E.consts_table() if consts is None else consts
    s, a = E.make_rows(n, seed, edges=False, consts=consts)
    rng = np.random.RandomState(1000 + seed)
    st = np.zeros((n, OPF_STATE), np.float32)
    st[:, S_X] = a
    st[:, S_LAM] = LAMBDA_SCALE * rng.randn(n, NEQ)
    lu = lambda lo, hi, shape: np.exp(rng.uniform(np.log(lo), np.log(hi), shape))                         # noqa: E731
    tame = ((np.arange(n) < N_SPECIAL) | (np.arange(n) % 2 == 0))[:, None]
    gamma = np.where(tame, lu(1e-3, 1e-1, (n, 1)), lu(1e-6, 1.0, (n, 1)))
    st[:, S_GAMMA] = gamma[:, 0]
    for sz, sm in ((S_ZU, S_MUU), (S_ZL, S_MUL)):
        z = np.where(tame, lu(1e-2, 1.0, (n, NBND)), lu(1e-6, 1.0, (n, NBND)))
        st[:, sz], st[:, sm] = z, gamma / z * np.where(tame, lu(0.5, 2.0, (n, NBND)), lu(0.1, 10.0, (n, NBND)))
    t = np.asarray(consts, np.float32)
    st[0, S_LAM] = 0.0
    st[1, S_LAM.start + 8] = 100.0 * LAMBDA_SCALE
    for b, hi in ((2 * NG + 1, t[E.OFF["VMAX"] + 1]), (1, t[E.OFF["PMAX"] + 1])):
        st[2, S_ZU.start + b] = 1e-6
        st[2, b] = hi - np.float32(1e-6)
    hi_pe, lo_pe = np.float32(ev.B_PMAX / ev.ETA_IN), np.float32(ev.ETA_OUT * ev.B_PMIN)
    alt = np.arange(NG) % 2 == 0
    st[3, E.PE0:43], st[4, E.PE0:43] = hi_pe, lo_pe
    st[5, E.PE0:43], st[6, E.PE0:43] = np.where(alt, hi_pe, lo_pe), np.where(alt, lo_pe, hi_pe)
    st[7, S_LAM] = 0.0
    c = E.Tab(F32E, consts)
    x7 = E.cols(F32E, st[7:8, S_X])
    f = E.flows(F32E, c, x7)
    col0 = [E.jac_entry(F32E, c, f, e, E.VM0) for e in range(NEQ)]
    top = np.float32(max(abs(float(v[0])) for v in col0 if v is not None))
    b0 = 2 * NG
    st[7, S_ZU.start + b0] = st[7, S_ZL.start + b0] = 1.0
    st[7, S_MUU.start + b0] = st[7, S_MUL.start + b0] = top * np.float32(0.5)
    st[8] = flat_state32(consts, np.zeros((1, NG), np.float32))[0]
    st[9, S_LAM.start + 3] = np.nan
    return s[:, :2 * NB].copy(), st


def trajectory_states(run, kmax=12):
    """The states after k = 0 .. kmax iterations, each one step (max_iters = 1, tol = 1e-30: no lane stops) from the one before;
    ``run(state_in or None, max_iters)`` -> state_out [n, 168] is the kernel or the emulation.  -> [kmax + 1, n, 168] float32."""
    out = [np.asarray(run(None, 0), np.float32)]
    for _ in range(kmax):
        out.append(np.asarray(run(out[-1], 1), np.float32))
    return np.stack(out)


def helper_iterates(prob, demand, pe, kmax, tol=None):
    """The float64 helper's iterates from the flat start, rows [n]: states [kmax + 1, n, 168] and the residual at each
    [kmax + 1, n].  With ``tol`` a row stops where its residual falls below it (later entries repeat the last iterate)."""
    demand, pe = np.asarray(demand, np.float64)[:, :2 * NB], np.asarray(pe, np.float64)
    n = demand.shape[0]
    states, resid = np.zeros((kmax + 1, n, OPF_STATE)), np.zeros((kmax + 1, n))
    for r in range(n):
        st = flat_state(pe[r], prob)
        for k in range(kmax + 1):
            e = ip_eval(prob, demand[r][None], *st[:4])
            states[k, r], resid[k, r] = join_state(*st), e["residual"]
            if k < kmax and not (tol is not None and e["residual"] < tol):
                st, _ = ip_advance(prob, e, *st)
    return states, resid


def iteration_classes(demand, pe, tol, max_iters=40):
    """Of the helper on rows [n]: (iterations, converged, decisive): ``decisive`` = the float64 residual lies outside [tol / 2,
    2 tol] at EVERY iterate up to the stop, so no float32 rounding of a residual can move the stop by an iteration."""
    _, resid = helper_iterates(PROB64, demand, pe, max_iters, tol)
    with np.errstate(all="ignore"):
        below = resid < tol
    conv = below.any(axis=0)
    iters = np.where(conv, below.argmax(axis=0), max_iters)
    upto = np.arange(max_iters + 1)[:, None] <= iters[None]
    decisive = ~(upto & (resid >= tol / 2) & (resid <= 2 * tol)).any(axis=0)
    return iters.astype(np.int32), conv, decisive


def trajectory_ratios(consts, demand, pe, got_states):
    """Whole trajectories: got_states[k] = the state after k iterations from the flat start (max_iters = k, tol tiny) against the
    k-th iterate of the float64 helper on the table's constants, within the SUM of the k single-step tolerances along the float64
    trajectory (the rule of evopf_f64.check_momentum).  Rows with a step that is not judged on the way are left out from there
    on.  -> (ratios [kmax + 1, n] worst over the components, left out [kmax + 1, n])."""
    kmax = len(got_states) - 1
    states, _ = helper_iterates(prob_of_table(consts), demand, pe, kmax)
    n = states.shape[1]
    # the flat start itself: x0 = 0.5f * (hi + lo) is one rounding, z = max(hi - x0, 1) and mu = gamma / z inherit it and add
    # their own -- under two ulps of each component
    tol_sum, left = 2.0 * EPS32 * np.abs(states[0]), np.zeros(n, bool)
    scale = np.zeros(OPF_STATE)
    for group, sl in GROUP_COLS.items():
        scale[sl] = MARGIN * C_REF[group] * EPS32
    out, outl = np.zeros((kmax + 1, n)), np.zeros((kmax + 1, n), bool)
    for k in range(kmax + 1):
        with np.errstate(all="ignore"):
            err = np.abs(np.asarray(got_states[k], np.float64) - states[k])
            r = np.where(err == 0, 0.0, err / np.maximum(tol_sum, E.ef.TINY))
            bad = ~np.isfinite(tol_sum).all(axis=1) | left
            out[k], outl[k] = np.where(bad, 0.0, np.where(np.isnan(r), np.inf, r).max(axis=1)), bad
        if k < kmax:
            ref = step_ref(consts, demand, states[k].astype(np.float32))
            left = left | ~ref["first_order"]
            # (the float32 rounding of the float64 iterate the bound is evaluated at: half an ulp of each component)
            tol_sum += scale * ref["state_m"] + 0.5 * EPS32 * np.abs(states[k + 1])
    return out, outl
