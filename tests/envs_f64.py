"""Float64 restatement of the env-step, constraint and projection kernels (csrc/cartsafe_dev.h: cart_lane, eq_ineq, reduced_grad,
cart_explore_project, lagrangian_row, complete_bwd_row; csrc/pendulum_dev.h: pend_lane, set_eq, ipg_row, pend_explore_project,
project_batchref_body / _wide, lagrangian_row, complete_bwd_row), the edge inputs that exercise them, and the yardstick that
turns "close to float64" into a number.  Not collected; used by test_envs_f64.py (CPU) and test_envs_f64_gpu.py.

Every formula is written ONCE, from the reference's lines (the ones the device headers cite: cartpole.py:170-229,369-408,
pendulum.py:80-128,256-343, rpo_ddpg.py:266-286), against an arithmetic ``A`` and is run three ways:

    B64   float64 values, each carrying a first-order running error bound in units of eps32 (class ``V``): the yardstick;
    F32   numpy float32, one rounding per operation, in the kernels' operation order, no contraction: the float32 emulation,
          from which the C_REF_* below are measured and on which the mutations of test_envs_f64.py are shown to fail;
    (the kernels themselves, whose outputs the same ``check_*`` functions judge in test_envs_f64_gpu.py).

Only the kernels' float32 inputs enter (the constants table of oracle.cartsafe.Constants.as_array() is one of them); every
other constant is the reference's float64 value in B64 and its float32 rounding in F32.

Running error bound ("magnitude sum").  With u = one rounding, a value r computed from a and b carries
    a +- b:  m = m_a + m_b + |r|          a b:  m = |a| m_b + |b| m_a + |r|          a / b:  m = m_a / |b| + |r| m_b / |b| + |r|
    sin / cos:  |cos| m_a + 2 |r|  (sinf / cosf are good to two roundings)            inputs: m = 0, constants: m = |c| if inexact
so a cancelling expression keeps the bound of its operands -- (theta + pi) mod 2 pi - pi the size of theta + pi,
b - (a_x C_p + a_y C_o) after completion the size of |a_x C_p| + |a_y C_o| although the value is 0, g = |a|^2 - 32 the size of 32,
4/3 - ... in the cart's denominator the size of 4/3 -- and fmod(x, c) adds floor(|x / c|) roundings of c.  A float32 evaluation is
expected within a small multiple c of EPS32 * m on EVERY element; c is measured per output group as C_REF_* (never from a kernel),
and the GPU tolerance is MARGIN * C_REF_* * EPS32 * m.

Discontinuities.  Masks and signs are step functions: a predicate whose float64 margin lies within GUARD * EPS32 * m of 0
(GUARD = MARGIN * C_REF of the predicate's expression) is AMBIGUOUS and either value is accepted -- by enumeration for the
per-lane forms (up to three per row, a row with more is left out), by widening for the batch-coupled sum -- and at most AMBIG_CAP
of the rows of one comparison may be ambiguous, whatever the kernel did.  The projection loop is compared ONE iteration at a
time from the kernel's own previous iterate (corr_momentum = 0: (a_x, a_y) is the whole loop state), never as a trajectory.
"""
import itertools
import math

import numpy as np

from oracle import cartsafe as ocs
from oracle import pendulum as opd

EPS32 = float(np.finfo(np.float32).eps)              # 2^-23
TINY = 1e-30
MARGIN = 4.0                                         # GPU tolerance = MARGIN * C_REF_* * EPS32 * magnitude sum
AMBIG_CAP = 0.02                                     # share of rows of one comparison that may carry an ambiguous predicate
MAX_ENUM = 3                                         # ambiguous predicates per row accepted by enumeration
FLT_MAX = float(np.finfo(np.float32).max)
HALF_DENORM = 2.0 ** -150                            # a float32 product below this rounds to 0 (gradual underflow, round to even)

# The yardstick: max over the yardstick inputs (``cart_rows`` / ``pend_rows``: every edge row and the random rows, both partial
# values) of |float32 - float64| / (EPS32 * magnitude sum), the float32 side being THIS file's formulas under F32 on the CPU
# (never a kernel).  Measured by tests/test_envs_f64.py::test_yardstick, which recomputes them and fails on a drift beyond 2x.
C_REF = {
    "cart_viol": 0.47,       # measured 0.468: eq / ineq violations of the step (h, relu(g_j))
    "cart_next": 0.49,       # measured 0.484: next x, x_dot, theta, theta_dot
    "cart_acc": 0.23,        # measured 0.223: xacc, thetaacc
    "pend_obs": 0.44,        # measured 0.432: cos / sin of the pre-step theta (columns 0..1 of the row)
    "pend_viol": 0.42,       # measured 0.420: h, relu(g)
    "pend_next": 0.50,       # measured 0.491: next cos, sin, theta_dot, l, l_dot and the internal theta
    "pend_reward": 0.46,     # measured 0.456: 1 / (100 |angle_normalize(theta)| + 1)
    "cart_resid": 0.50,      # measured 0.500: eq_resid / ineq_resid
    "cart_ipg": 0.37,        # measured 0.366: ineq_partial_grad's two components
    "cart_cbwd": 0.48,       # measured 0.477: backward of complete_partial
    "cart_lag": 0.42,        # measured 0.420: per-row d/d action and distances of the Lagrangian term
    "pend_resid": 0.42,      # measured 0.420
    "pend_ipg": 0.43,        # measured 0.430
    "pend_cbwd": 0.50,       # measured 0.493
    "pend_lag": 0.49,        # measured 0.489
    "cart_act": 0.49,        # measured 0.486: exploration + complete_partial (the budget-0 action under explicit noise)
    "pend_act": 0.47,        # measured 0.461
    "cart_grg": 0.50,        # measured 0.499: one GRG iteration (a_p, a_o) -> (a_p, a_o), and the residuals of an iterate
    "pend_grg": 0.50,        # measured 0.496: one row-wise GRG iteration, and the residuals of an iterate
    "batch_grg": 0.46,       # measured 0.458: one batch-coupled GRG iteration (depth-weighted bound of the sum)
    "cart_pred": 0.50,       # measured 0.500: a_p G_r[i] - d_r[i]
    "pend_pred": 0.40,       # measured 0.397: a_x dgp - bgp (row-wise; the n^2 of the coupled form are the same expression)
    "stop_pred": 0.50,       # measured 0.500: |h| - corr_eps, g - corr_eps (the residual expressions: the larger of both envs)
    "sign_pred": 0.26,       # measured 0.258: n_c x_dot
}


def tol_c(group):
    return MARGIN * C_REF[group]


# ===================================================================================================== arithmetics
class V(object):
    """float64 value(s) with the running error bound m (units of eps32) of the float32 evaluation of the same expression."""
    __slots__ = ("v", "m")

    def __init__(self, v, m=0.0):
        self.v = np.asarray(v, dtype=np.float64)
        self.m = np.asarray(m, dtype=np.float64)

    @staticmethod
    def of(x):
        return x if isinstance(x, V) else V(x, 0.0)

    @staticmethod
    def _own(r, am, bm):
        """The operation's own rounding: |r|, or 0 where both operands are exact (m = 0) and r is a float32 -- then the float32
        operation returns r itself (the float64 r is the correctly rounded result, and a float32 that is the nearest float64 is
        the nearest float32).  This keeps m = 0 along exact chains: 10 * 1 - 10, 4 * 8 - 32, 16 + 16 - 32."""
        with np.errstate(all="ignore"):
            exact = (am == 0) & (bm == 0) & (r.astype(np.float32).astype(np.float64) == r)
            # beyond the float32 range the float32 operation overflows where float64 goes on: nothing downstream is bounded
            return np.where(exact, 0.0, np.where(np.abs(r) > FLT_MAX, np.inf, np.abs(r)))

    def __add__(self, o):
        o = V.of(o)
        r = self.v + o.v
        return V(r, self.m + o.m + V._own(r, self.m, o.m))
    __radd__ = __add__

    def __sub__(self, o):
        o = V.of(o)
        r = self.v - o.v
        return V(r, self.m + o.m + V._own(r, self.m, o.m))

    def __rsub__(self, o):
        return V.of(o) - self

    def __mul__(self, o):
        o = V.of(o)
        r = self.v * o.v
        return V(r, np.abs(self.v) * o.m + np.abs(o.v) * self.m + V._own(r, self.m, o.m))
    __rmul__ = __mul__

    def __truediv__(self, o):
        o = V.of(o)
        r = self.v / o.v
        return V(r, self.m / np.abs(o.v) + np.abs(r) * o.m / np.abs(o.v) + V._own(r, self.m, o.m))

    def __rtruediv__(self, o):
        return V.of(o) / self

    def __neg__(self):
        return V(-self.v, self.m)


class B64(object):
    """float64 with bounds."""
    name = "b64"

    @staticmethod
    def k(c):
        c = float(c)
        return V(c, 0.0 if float(np.float32(c)) == c else abs(c))

    @staticmethod
    def inp(x):
        return V(np.asarray(x, dtype=np.float32).astype(np.float64), 0.0)

    @staticmethod
    def val(x):
        return V.of(x).v

    @staticmethod
    def mag(x):
        x = V.of(x)
        return np.broadcast_to(x.m, x.v.shape)

    @staticmethod
    def sin(x):
        r = np.sin(x.v)
        return V(r, np.abs(np.cos(x.v)) * x.m + 2 * np.abs(r))

    @staticmethod
    def cos(x):
        r = np.cos(x.v)
        return V(r, np.abs(np.sin(x.v)) * x.m + 2 * np.abs(r))

    @staticmethod
    def abs(x):
        return V(np.abs(x.v), x.m)

    @staticmethod
    def where(c, a, b):
        a, b = V.of(a), V.of(b)
        return V(np.where(c, a.v, b.v), np.where(c, a.m, b.m))

    @classmethod
    def maximum(cls, a, b):
        a, b = V.of(a), V.of(b)
        return cls.where((a.v >= b.v) | np.isnan(b.v), a, b)           # fmaxf: a NaN operand loses

    @classmethod
    def minimum(cls, a, b):
        a, b = V.of(a), V.of(b)
        return cls.where((a.v <= b.v) | np.isnan(b.v), a, b)

    @staticmethod
    def fmod(x, c):
        r = np.fmod(x.v, c.v)
        return V(r, x.m + np.floor(np.abs(x.v / c.v)) * c.m)


class B64X(B64):
    """B64 on float64 inputs as they are (the reference's own golden states): to hold the restatement against the reference."""
    @staticmethod
    def inp(x):
        return V(np.asarray(x, dtype=np.float64), 0.0)


class F32(object):
    """numpy float32: one rounding per operation, no contraction."""
    name = "f32"

    @staticmethod
    def k(c):
        return np.float32(c)

    @staticmethod
    def inp(x):
        return np.asarray(x, dtype=np.float32)

    @staticmethod
    def val(x):
        return np.asarray(x)

    @staticmethod
    def mag(x):
        return np.zeros(np.shape(x))

    sin = staticmethod(np.sin)
    cos = staticmethod(np.cos)
    abs = staticmethod(np.abs)
    where = staticmethod(np.where)
    maximum = staticmethod(np.fmax)
    minimum = staticmethod(np.fmin)
    fmod = staticmethod(np.fmod)


def _clip(A, x, lim):
    """fminf(fmaxf(x, -lim), lim): exact; a NaN comes out as -lim, as on the device (the step kernels flag it before)."""
    return A.minimum(A.maximum(x, A.k(-lim)), A.k(lim))


def _sign_of(A, prod):
    """np.sign of the product as the kernel writes it: 0 -> 0 (+0 / -0 kept), NaN -> NaN."""
    v = A.val(prod)
    s = np.where(v > 0, 1.0, np.where(v < 0, -1.0, v))
    return A.inp(s.astype(np.float32))


# ===================================================================================================== CartSafe
class CartTab(object):
    """The float32[35] constants table (include/rpo_hip.h: RPO_CART_CONSTS_LEN) as inputs of ``A``."""

    def __init__(self, A, table, partial):
        t = np.asarray(table, dtype=np.float32)
        assert t.shape == (35,)
        f = lambda v: A.inp(np.float32(v))                      # noqa: E731
        self.C = [f(t[0]), f(t[1])]
        self.C_p, self.C_o_inv, self.b = f(t[2]), f(t[3]), f(t[4])
        self.G = [f(v) for v in t[5:17]]
        self.d = [f(v) for v in t[17:23]]
        self.G_r = [f(v) for v in t[23:29]]
        self.d_r = [f(v) for v in t[29:35]]
        self.partial = int(partial)


def cart_eq_ineq(A, c, a0, a1):
    """eq_resid cartpole.py:375-376, ineq_resid :378-379 (signed)."""
    h = c.b - (a0 * c.C[0] + a1 * c.C[1])
    g = [(a0 * c.G[2 * i] + a1 * c.G[2 * i + 1]) - c.d[i] for i in range(6)]
    return h, g


def cart_step(A, state, action, table, partial, sign=None, mut=()):
    """cartpole.py:170-229 for float32 (state [n,6], action [n,2]).  Returns dict: h, g (list of 6 relu'd violations), ns (list of
    the 6 next-state entries), prod (n_c x_dot, the argument of np.sign).  ``sign``: use this sign instead of np.sign(prod)."""
    with np.errstate(all="ignore"):
        c = CartTab(A, table, partial)
        state, action = np.asarray(state), np.asarray(action)
        x, xd, _, th, thd, tha_prev = (A.inp(state[:, i]) for i in range(6))
        a0, a1 = A.inp(action[:, 0]), A.inp(action[:, 1])
        f0, f1 = _clip(A, a0, 10.0), _clip(A, a1, 10.0)                                    # :170-173
        v0, v1 = (f0, f1) if "viol_clipped" in mut else (a0, a1)                           # :229: the UN-clipped action
        h, g = cart_eq_ineq(A, c, v0, v1)
        g = [A.maximum(gi, A.k(0.0)) for gi in g]
        force = f0 * A.k(math.cos(ocs.DELTA[0])) + f1 * A.k(math.cos(ocs.DELTA[1]))         # :178
        force_y = f0 * A.k(math.sin(ocs.DELTA[0])) + f1 * A.k(math.sin(ocs.DELTA[1]))       # :179
        sn, cs = A.sin(th), A.cos(th)
        td2 = thd * thd
        K = A.k
        tha_nc = tha_prev
        for _ in range(2 if "nc_new_thetaacc" in mut else 1):
            n_c = force_y + K(ocs.TOTAL_MASS) * K(ocs.GRAVITY) - K(ocs.POLEMASS_LENGTH) * (tha_nc * sn + td2 * cs)   # :183
            prod = n_c * xd
            sg = _sign_of(A, prod) if sign is None else A.inp(np.asarray(sign, np.float32))   # :184
            if "sign0_is_1" in mut:
                sg = A.where(A.val(prod) == 0, A.k(1.0), sg)
            temp = (force + K(ocs.POLEMASS_LENGTH) * td2 * (sn + K(ocs.MU_C) * sg * cs)) / K(ocs.TOTAL_MASS) \
                + K(ocs.MU_C) * K(ocs.GRAVITY) * sg                                         # :185-186
            thacc = (K(ocs.GRAVITY) * sn - cs * temp - K(ocs.MU_P) * thd / K(ocs.POLEMASS_LENGTH)) / \
                (K(ocs.LENGTH) * (K(4.0) / K(3.0) - K(ocs.MASSPOLE) * cs * (cs - K(ocs.MU_C) * K(ocs.GRAVITY) * sg)
                                  / K(ocs.TOTAL_MASS)))                                     # :187-189
            xacc = (force + K(ocs.POLEMASS_LENGTH) * (td2 * sn - thacc * cs) - K(ocs.MU_C) * n_c * sg) / K(ocs.TOTAL_MASS)
            tha_nc = thacc
        ns = [x + K(ocs.TAU) * xd, xd + K(ocs.TAU) * xacc, xacc, th + K(ocs.TAU) * thd, thd + K(ocs.TAU) * thacc, thacc]
        return dict(h=h, g=g, ns=ns, prod=prod)


X_LIM32 = np.float32(2.4)                                   # the float32 neighbours of the two thresholds, for the edge rows
TH_LIM32 = np.float32(ocs.THETA_THRESHOLD)


def cart_terminated_ref(ns32):
    """cartpole.py:208-213 in float64 on the STORED float32 next state, 2.4 and 12 degrees as float64 constants."""
    x, th = np.asarray(ns32)[:, 0].astype(np.float64), np.asarray(ns32)[:, 3].astype(np.float64)
    return (x < -ocs.X_THRESHOLD) | (x > ocs.X_THRESHOLD) | (th < -ocs.THETA_THRESHOLD) | (th > ocs.THETA_THRESHOLD)


def _below(c):
    """The largest float32 not above the float64 c."""
    f = np.float32(c)
    return f if float(f) <= c else np.nextafter(f, np.float32(-np.inf))


def cart_terminated_f32(ns32, mut=()):
    """The kernel's float32 predicate (cart_lane): x > X_hi <=> x > 2.4 for every float32 x when X_hi is the largest float32 not
    above 2.4 (``naive_thresholds``: the rounded constants 2.4f and 0.20943952f, which lie ABOVE the float64 thresholds)."""
    xl = X_LIM32 if "naive_thresholds" in mut else _below(ocs.X_THRESHOLD)
    tl = TH_LIM32 if "naive_thresholds" in mut else _below(ocs.THETA_THRESHOLD)
    x, th = np.asarray(ns32, np.float32)[:, 0], np.asarray(ns32, np.float32)[:, 3]
    return (x < -xl) | (x > xl) | (th < -tl) | (th > tl)


def cart_complete(A, c, ap):
    """complete_partial, cartpole.py:369-373: the other component."""
    return (c.b - ap * c.C_p) * c.C_o_inv


def cart_reduced_grad(A, c, ap, mask=None, mut=()):
    """ineq_partial_grad, cartpole.py:396-403.  Returns (grad, [margins a_p G_r[i] - d_r[i]]); ``mask`` [n,6] overrides the
    predicates."""
    margins = [ap * c.G_r[i] - c.d_r[i] for i in range(6)]
    grad = None
    for i in range(6):
        if mask is not None:
            on = np.asarray(mask)[..., i]
        else:
            on = (A.val(margins[i]) >= 0) if "ge_reduced" in mut else (A.val(margins[i]) > 0)
        term = A.where(on, c.G_r[i], A.k(0.0))
        grad = (A.k(0.0) + term) if grad is None else grad + term
    return grad, margins


def cart_grg_step(A, table, partial, ap, ao, lr, momentum=0.0, old=None, mask=None, mut=()):
    """One iteration of grad_steps (rpo_ddpg.py:266-286, corr_mode 0) on (a_p, a_o).  Returns (ap', ao', (sp, so), margins)."""
    with np.errstate(all="ignore"):
        c = table if isinstance(table, CartTab) else CartTab(A, table, partial)
        ap, ao = _as(A, ap), _as(A, ao)
        gp, margins = cart_reduced_grad(A, c, ap, mask, mut)
        go = -(gp * c.C_p) * c.C_o_inv                                                     # cartpole.py:407
        lr = A.inp(np.float32(lr))
        if old is None:
            sp, so = lr * gp, lr * go
        else:
            m = A.inp(np.float32(momentum))
            sp, so = lr * gp + m * _as(A, old[0]), lr * go + m * _as(A, old[0 if "mom_wrong_old" in mut else 1])
        return ap - sp, ao - so, (sp, so), margins


def cart_split(partial, a):
    a = np.asarray(a)
    return (a[..., 0], a[..., 1]) if partial == 0 else (a[..., 1], a[..., 0])


def cart_join(partial, ap, ao):
    return np.stack([ap, ao] if partial == 0 else [ao, ap], axis=-1)


def explore(A, ap_in, noise, eps_t, lo, hi):
    """ddpg_pa.py:108-110: clip(ap + eps_t noise, lo, hi), a NaN passed through (rpo_clamp)."""
    ap = A.inp(ap_in)
    if noise is None:
        return ap
    pre = ap + A.inp(np.float32(eps_t)) * A.inp(noise)
    out = A.minimum(A.maximum(pre, A.inp(np.float32(lo))), A.inp(np.float32(hi)))
    return A.where(np.isnan(A.val(pre)), pre, out)


def cart_project_f32(table, partial, ap_in, K, lr, corr_eps, momentum=0.0, noise=None, eps_t=0.0, lo=-10.0, hi=10.0, mut=()):
    """The float32 emulation of cart_explore_project with the profile of every budget: planes [K + 1, n, 4] = (a0, a1, eq_resid,
    max_j ineq_resid) of the iterate after min(b, iters) steps, and iters [n]."""
    A = F32
    with np.errstate(all="ignore"):
        c = CartTab(A, table, partial)
        ap = explore(A, ap_in, noise, eps_t, lo, hi)
        ao = cart_complete(A, c, A.inp(ap_in) if "complete_unnoised" in mut else ap)
        n = ap.shape[0]
        old = (np.zeros(n, np.float32), np.zeros(n, np.float32))
        live = np.ones(n, bool)
        iters = np.zeros(n, np.int32)
        planes = np.zeros((K + 1, n, 4), np.float32)
        eps = np.float32(corr_eps)
        for k in range(K + 1):
            a = cart_join(partial, ap, ao)
            h, g = cart_eq_ineq(A, c, a[:, 0], a[:, 1])
            mx = np.max(np.stack(g, axis=1), axis=1)
            planes[k] = np.stack([a[:, 0], a[:, 1], h, mx], axis=1)
            if k == K:
                break
            viol = (np.abs(h) > eps) | (mx > eps)
            if k > 0 or "no_k0" in mut:
                live = live & viol
            nap, nao, (sp, so), _ = cart_grg_step(A, c, partial, ap, ao, lr, momentum, old, mut=mut)
            ap, ao = np.where(live, nap, ap), np.where(live, nao, ao)
            old = (np.where(live, sp, old[0]), np.where(live, so, old[1]))
            iters += live
        return planes, iters


def cart_lagrangian_t64(table, partial, action, nu, scale):
    """nu . relu(g(a)) (Dual.forward on ineq_dist, rpo_ddpg.py:312-319) written as a function and differentiated by torch float64
    autograd: (per-row loss, dist [n,6], scale * d/d action [n,2])."""
    import torch
    t = np.asarray(table, np.float32).astype(np.float64)
    G, d = torch.from_numpy(t[5:17].reshape(6, 2)), torch.from_numpy(t[17:23])
    a = torch.from_numpy(np.asarray(action, np.float32).astype(np.float64)).requires_grad_(True)
    dist = torch.relu(a @ G.T - d)
    row = dist @ torch.from_numpy(np.asarray(nu, np.float32).astype(np.float64))
    ga, = torch.autograd.grad(float(np.float32(scale)) * row.sum(), (a,))
    return row.detach().numpy(), dist.detach().numpy(), ga.numpy()


def _cols(A, x, exact):
    """The columns of x as inputs of ``A``.  ``exact`` (B64 only; tests/update_f64.py): float64 values are taken as they are
    instead of through their float32 rounding -- the value a float64 chain hands on, not a kernel's output."""
    x = np.asarray(x, np.float64 if exact else np.float32)
    return [V(x[..., i]) if exact else A.inp(x[..., i]) for i in range(x.shape[-1])]


def cart_lagrangian(A, table, partial, action, nu, scale, mask=None, exact=False):
    """lagrangian_row + the scale of the elementwise launch, with bounds: dict(dist [6], g0, g1, margins [6]); ``mask`` [n,6]
    overrides the predicates g_j > 0 of the gradient.  ``exact``: see ``_cols``."""
    with np.errstate(all="ignore"):
        c = CartTab(A, table, partial)
        h, g = cart_eq_ineq(A, c, *_cols(A, action, exact))
        nu = [A.inp(np.float32(v)) for v in nu]
        g0 = g1 = None
        for j in range(6):
            on = A.val(g[j]) > 0 if mask is None else np.asarray(mask)[:, j]
            t0, t1 = A.where(on, nu[j] * c.G[2 * j], A.k(0.0)), A.where(on, nu[j] * c.G[2 * j + 1], A.k(0.0))
            g0, g1 = (A.k(0.0) + t0, A.k(0.0) + t1) if g0 is None else (g0 + t0, g1 + t1)
        s = A.inp(np.float32(scale))
        return dict(dist=[A.maximum(gj, A.k(0.0)) for gj in g], g0=s * g0, g1=s * g1, margins=g)


def cart_complete_bwd(A, table, partial, ga, exact=False):
    """d/d ap of the loss through complete_partial (cartpole.py:369-373): g_p + (-(C_p C_o_inv)) g_o.  ``exact``: see ``_cols``."""
    with np.errstate(all="ignore"):
        c = CartTab(A, table, partial)
        g0, g1 = _cols(A, ga, exact)
        gp, go = (g0, g1) if partial == 0 else (g1, g0)
        k = -(c.C_p * c.C_o_inv)
        return gp + k * go


def cart_complete_bwd_fd(table, partial, ga):
    """The same by differentiating complete_partial (a linear map: the central difference is exact) in float64."""
    c = CartTab(B64, table, partial)
    f = lambda ap: np.stack([ap, B64.val(cart_complete(B64, c, V(ap)))], axis=-1)     # noqa: E731  (a_p, a_o)
    jac = (f(np.float64(1.0)) - f(np.float64(-1.0))) / 2.0
    gp, go = cart_split(partial, np.asarray(ga, np.float32).astype(np.float64))
    return gp * jac[0] + go * jac[1]


# ===================================================================================================== SpringPendulum
class PendEq(object):
    """set_eq, pendulum.py:264-288, from the observation (cos, sin, theta_dot, l, l_dot)."""

    def __init__(self, A, cs, sn, thd, l, ld, mut=()):
        K = A.k
        self.C_p, self.C_o = sn, cs
        self.C_o_inv = K(1.0) / cs
        # l m thd thd as the kernels associate it, ((l m) thd) thd; ``oracle_order``: (l m) (thd thd), numpy's l * M * thdot ** 2
        kin = (l * K(opd.M)) * (thd * thd) if "oracle_order" in mut else l * K(opd.M) * thd * thd
        self.b = (-K(opd.M_DT)) * ld - (kin - K(opd.K) * (l - K(opd.L0)) - K(opd.M) * K(opd.G) * cs)   # :287


def pend_eq_of_obs(A, obs, mut=()):
    obs = np.asarray(obs, np.float32)
    return PendEq(A, *(A.inp(obs[:, i]) for i in range(5)), mut=mut)


def angle_cost(A, th, mut=()):
    """|angle_normalize(theta)|, pendulum.py:106,367-368.  For -pi < theta < pi (every float32 strictly inside (-pi32, pi32)) the
    value is |theta| exactly and the kernel computes it so; outside, ((theta + pi) mod 2 pi) - pi with the bound it has."""
    K = A.k
    x = th + K(math.pi)
    an = A.fmod(x, K(2 * math.pi))
    an = A.where(A.val(an) < 0, an + K(2 * math.pi), an)
    wrapped = A.abs(an - K(math.pi))
    if "reward_fmod" in mut:
        return wrapped
    inside = np.abs(A.val(th)) < float(np.float32(math.pi))
    return A.where(inside, A.abs(th), wrapped)


def pend_step(A, internal, action, mut=()):
    """pendulum.py:80-128 for float32 (internal [n,4] = theta, theta_dot, l, l_dot; action [n,2]).  Returns dict: obs (cos, sin of
    the pre-step theta), h, g (relu'd), nth (un-stored next theta), next (ncs, nsn, nthdot clipped, nl, nldot), reward."""
    with np.errstate(all="ignore"):
        internal, action = np.asarray(internal), np.asarray(action)
        th, thd, l, ld = (A.inp(internal[:, i]) for i in range(4))
        ax, ay = A.inp(action[:, 0]), A.inp(action[:, 1])
        K = A.k
        sn, cs = A.sin(th), A.cos(th)
        e = PendEq(A, cs, sn, thd, l, ld)
        fx, fy = _clip(A, ax, opd.MAX_TORQUE), _clip(A, ay, opd.MAX_TORQUE)                 # :85-88
        vx, vy = (fx, fy) if "viol_clipped" in mut else (ax, ay)                           # :128: the UN-clipped action
        h = e.b - (vx * e.C_p + vy * e.C_o)                                                # :298-300
        g = A.maximum(vx * vx + vy * vy - K(opd.MAX_SUMMATION), K(0.0))                     # :302-311
        fth = (-fy) * sn + fx * cs                                                         # :95
        fl = fy * cs + fx * sn                                                             # :96
        costs = angle_cost(A, th, mut)                                     # :106
        thacc = (fth - K(opd.M) * (K(opd.G) * sn + K(2.0) * ld * thd)) / (l * K(opd.M))     # :109
        lacc = (fl - K(opd.M) * K(opd.G) * cs + K(opd.M) * l * thd * thd - K(opd.K) * (l - K(opd.L0))) / K(opd.M)   # :110
        nthd = thd + thacc * K(opd.DT)
        nld = ld + lacc * K(opd.DT)
        if "clip_before_theta" in mut:
            nthd = _clip(A, nthd, opd.MAX_SPEED)
        nth = th + (thd if "explicit_theta" in mut else nthd) * K(opd.DT)                   # semi-implicit in theta :119
        nl = l + ld * K(opd.DT)                                                            # explicit in l :120
        nthd_c = _clip(A, nthd, opd.MAX_SPEED)                                             # :122
        reward = K(1.0) / (K(100.0) * costs + K(1.0))
        return dict(obs=[cs, sn], h=h, g=g, nth=nth, next=[A.cos(nth), A.sin(nth), nthd_c, nl, nld], reward=reward)


def pend_terminated_ref(nint32):
    """pendulum.py:124 in float64 on the STORED float32 (theta, ., l, .), pi / 12 as a float64 constant."""
    th, l = np.asarray(nint32)[:, 0].astype(np.float64), np.asarray(nint32)[:, 2].astype(np.float64)
    return (l <= 0.5) | (l >= 1.5) | (th >= np.pi / 12) | (th <= -np.pi / 12)


def pend_terminated_f32(nint32):
    """The kernel's float32 predicate: >= against float32(pi / 12), which lies above pi / 12 -- so v >= pi/12 <=> v >= pi/12f."""
    th, l = np.asarray(nint32, np.float32)[:, 0], np.asarray(nint32, np.float32)[:, 2]
    lim = np.float32(np.pi / 12)
    return (l <= np.float32(0.5)) | (l >= np.float32(1.5)) | (th >= lim) | (th <= -lim)


def pend_resid(A, e, ax, ay):
    return e.b - (ax * e.C_p + ay * e.C_o), ax * ax + ay * ay - A.k(opd.MAX_SUMMATION)


def pend_complete(A, e, ax):
    return (e.b - ax * e.C_p) * e.C_o_inv                                                  # :256-262


def pend_dgp_bgp(A, e, ax, ay):
    Gx, Gy = A.k(2.0) * ax, A.k(2.0) * ay                                                  # set_ineq :296
    return Gx - Gy * (e.C_o_inv * e.C_p), A.k(opd.MAX_SUMMATION) - (e.b * e.C_o_inv) * Gy  # :334-336


def _as(A, x):
    return x if isinstance(x, V) else A.inp(x)


def pend_grg_step(A, e, ax, ay, lr, momentum=0.0, old=None, mask=None, mut=()):
    """One row-wise iteration (pendulum.py:331-343 for B = 1 inside rpo_ddpg.py:266-286).  Returns (ax', ay', (sx, sy), margin)."""
    with np.errstate(all="ignore"):
        ax, ay = _as(A, ax), _as(A, ay)
        dgp, bgp = pend_dgp_bgp(A, e, ax, ay)
        bm = ax * dgp - bgp                                                                # :337
        on = np.asarray(mask) if mask is not None else (A.val(bm) >= 0 if "ge_ipg" in mut else A.val(bm) > 0)
        gx = A.where(on, dgp, A.k(0.0))                                                    # :339
        gy = -(gx * e.C_p) * e.C_o_inv                                                     # :342
        lr = A.inp(np.float32(lr))
        if old is None:
            sx, sy = lr * gx, lr * gy
        else:
            m = A.inp(np.float32(momentum))
            sx, sy = lr * gx + m * _as(A, old[0]), lr * gy + m * _as(A, old[0 if "mom_wrong_old" in mut else 1])
        return ax - sx, ay - sy, (sx, sy), bm


def pend_project_f32(obs, ap_in, K, lr, corr_eps, momentum=0.0, noise=None, eps_t=0.0, lo=-6.0, hi=6.0, mut=()):
    """The float32 emulation of pend_explore_project with the profile of every budget (see cart_project_f32; the reported
    residuals are those of this file's unfused formulas)."""
    A = F32
    with np.errstate(all="ignore"):
        e = pend_eq_of_obs(A, obs, mut)
        ax = explore(A, ap_in, noise, eps_t, lo, hi)
        ay = pend_complete(A, e, A.inp(ap_in) if "complete_unnoised" in mut else ax)
        n = ax.shape[0]
        old = (np.zeros(n, np.float32), np.zeros(n, np.float32))
        live = np.ones(n, bool)
        iters = np.zeros(n, np.int32)
        planes = np.zeros((K + 1, n, 4), np.float32)
        eps = np.float32(corr_eps)
        for k in range(K + 1):
            h, g = pend_resid(A, e, ax, ay)
            planes[k] = np.stack([ax, ay, h, g], axis=1)
            if k == K:
                break
            viol = (np.abs(h) > eps) | (g > eps)
            if k > 0 or "no_k0" in mut:
                live = live & viol
            nx, ny, (sx, sy), _ = pend_grg_step(A, e, ax, ay, lr, momentum, old, mut=mut)
            ax, ay = np.where(live, nx, ax), np.where(live, ny, ay)
            old = (np.where(live, sx, old[0]), np.where(live, sy, old[1]))
            iters += live
        return planes, iters


def batch_depth(n):
    """Longest chain of additions a term of the coupled sum passes through: 16 + 4 in the register-tiled form (n <= 256), a
    quarter of the batch + 2 with one thread per sample."""
    return 20 if n <= 256 else (n + 3) // 4 + 2


def _batch_sum_f32(sel, n):
    """Row sums of the float32 [n, n] matrix of selected dgp_j in the kernels' order: n <= 256 -- project_batchref_wide: lane c of
    16 adds j = 64 q + 4 c + m in the order (q, m), then the xor / mirror butterfly; otherwise project_batchref_body<1>: four
    accumulators over j mod 4 (the tail into the first), (g0 + g1) + (g2 + g3)."""
    if n <= 256:
        pad = np.zeros((n, 256), np.float32)
        pad[:, :n] = sel
        lanes = pad.reshape(n, 4, 16, 4)                               # [i, q, c, m]
        part = np.zeros((n, 16), np.float32)
        for q in range(4):
            for m in range(4):
                part = part + lanes[:, q, :, m]
        while part.shape[1] > 1:
            part = part[:, 0::2] + part[:, 1::2]
        return part[:, 0]
    acc = [np.zeros(n, np.float32) for _ in range(4)]
    full = n // 4 * 4
    for j in range(0, full, 4):
        for u in range(4):
            acc[u] = acc[u] + sel[:, j + u]
    for j in range(full, n):
        acc[0] = acc[0] + sel[:, j]
    return (acc[0] + acc[1]) + (acc[2] + acc[3])


def pend_batch_step(A, e, ax, ay, lr, momentum=0.0, old=None, mut=()):
    """One batch-coupled iteration, pendulum.py:337-339 for B > 1: grad_i = sum_j 1[a_x,i dgp_j - bgp_i > 0] dgp_j.  Returns
    (ax', ay', (sx, sy), margins [n, n], dgp [n]); under B64 the sum carries the depth-weighted bound."""
    with np.errstate(all="ignore"):
        ax, ay = _as(A, ax), _as(A, ay)
        n = A.val(ax).shape[0]
        dgp, bgp = pend_dgp_bgp(A, e, ax, ay)
        if A is F32:
            prod = ax[:, None] * dgp[None, :]
            bm = prod - bgp[:, None]
            on = (bm >= 0) if "ge_coupled" in mut else (bm > 0)
            if "drop_last" in mut:
                on[:, n - 1] = False
            grad = _batch_sum_f32(np.where(on, dgp[None, :], np.float32(0.0)).astype(np.float32), n)
        else:
            bm = V(ax.v[:, None], ax.m[:, None] if ax.m.ndim else ax.m) * V(dgp.v[None, :], np.broadcast_to(dgp.m, dgp.v.shape)[None, :]) \
                - V(bgp.v[:, None], np.broadcast_to(bgp.m, bgp.v.shape)[:, None])
            on = bm.v > 0
            dm = np.broadcast_to(dgp.m, dgp.v.shape)
            grad = V((on * dgp.v[None, :]).sum(axis=1),
                     (on * dm[None, :]).sum(axis=1) + batch_depth(n) * (on * np.abs(dgp.v)[None, :]).sum(axis=1))
        gy = -(grad * e.C_p) * e.C_o_inv
        lr = A.inp(np.float32(lr))
        if old is None:
            sx, sy = lr * grad, lr * gy
        else:
            m = A.inp(np.float32(momentum))
            sx, sy = lr * grad + m * _as(A, old[0]), lr * gy + m * _as(A, old[0 if "mom_wrong_old" in mut else 1])
        return ax - sx, ay - sy, (sx, sy), bm, dgp


def pend_batch_project_f32(obs, ap, K, lr, corr_eps, momentum=0.0, mut=()):
    """The float32 emulation of rpo_pendulum_project_batchref at the budget K: (action [n,2], iterations)."""
    A = F32
    with np.errstate(all="ignore"):
        e = pend_eq_of_obs(A, obs)
        ax = A.inp(ap)
        ay = pend_complete(A, e, ax)
        n = ax.shape[0]
        old = (np.zeros(n, np.float32), np.zeros(n, np.float32))
        eps = np.float32(corr_eps)
        live = np.ones(n, bool)
        k = 0
        for k in range(K + 1):
            if k == K:
                break
            h, g = pend_resid(A, e, ax, ay)
            viol = (np.abs(h) > eps) | (g > eps)
            if "per_row_stop" in mut:
                if k > 0:
                    live = live & viol
                if not live.any():
                    break
            elif k > 0 and not viol.any():                               # batch-global stop test, rpo_ddpg.py:271-272
                break
            nx, ny, (sx, sy), _, _ = pend_batch_step(A, e, ax, ay, lr, momentum, old, mut=mut)
            ax, ay = np.where(live, nx, ax), np.where(live, ny, ay)
            old = (np.where(live, sx, old[0]), np.where(live, sy, old[1]))
        return np.stack([ax, ay], axis=1), k


def pend_lagrangian_t64(action, nu0, scale):
    """nu0 relu(|a|^2 - 32) (pendulum.py:302-311; rpo_sac.py:326-335) differentiated by torch float64 autograd:
    (dist [n], scale * d/d action [n,2]).  relu'(0) = 0: g = 0 gives gradient 0 exactly."""
    import torch
    a = torch.from_numpy(np.asarray(action, np.float32).astype(np.float64)).requires_grad_(True)
    dist = torch.relu((a * a).sum(dim=1) - opd.MAX_SUMMATION)
    ga, = torch.autograd.grad(float(np.float32(scale)) * float(np.float32(nu0)) * dist.sum(), (a,))
    return dist.detach().numpy(), ga.numpy()


def pend_lagrangian(A, action, nu0, scale, mask=None, exact=False):
    """lagrangian_row: dict(dist, g0, g1, margin g); ``mask`` [n] overrides the predicate g > 0 of the gradient.  ``exact``: see
    ``_cols``."""
    with np.errstate(all="ignore"):
        ax, ay = _cols(A, action, exact)
        g = ax * ax + ay * ay - A.k(opd.MAX_SUMMATION)
        k = A.where(A.val(g) > 0 if mask is None else np.asarray(mask), A.k(2.0) * A.inp(np.float32(scale)) * A.inp(np.float32(nu0)), A.k(0.0))
        return dict(dist=A.maximum(g, A.k(0.0)), g0=k * ax, g1=k * ay, margin=g)


def pend_complete_bwd(A, obs, ga, exact=False):
    """d a_y / d a_x = -C_p C_o_inv (pendulum.py:256-262): g0 - g1 (sin (1 / cos)).  ``exact`` (the gradient only): see ``_cols``."""
    with np.errstate(all="ignore"):
        obs = np.asarray(obs, np.float32)
        g0, g1 = _cols(A, ga, exact)
        return g0 - g1 * (A.inp(obs[:, 1]) * (A.k(1.0) / A.inp(obs[:, 0])))


def pend_complete_bwd_fd(obs, ga):
    """The same by differentiating complete_partial (linear in a_x: the central difference is exact) in float64."""
    with np.errstate(all="ignore"):
        e = pend_eq_of_obs(B64, obs)
        one = np.ones(np.asarray(obs).shape[0])
        d = (B64.val(pend_complete(B64, e, V(one))) - B64.val(pend_complete(B64, e, V(-one)))) / 2.0
        ga = np.asarray(ga, np.float32).astype(np.float64)
        return ga[:, 0] + ga[:, 1] * d


def project_b64(env, ap_in, K, lr, corr_eps, momentum, table=None, partial=None, obs=None, exact=False, trace=None, stop_guard=True):
    """The whole per-lane loop in float64 WITH momentum, the running bound carried through every iteration (each adds at most one
    single-step bound: the accumulated m is the K-step tolerance).  Returns (a_p V, a_o V, iters [n], clean [n]): ``clean`` rows met
    no ambiguous mask or stop predicate on the way -- only those say anything about a float32 trajectory.  ``exact``: the float64
    proposal as it is (``project_interval``); ``trace``: a list that receives, per iteration, the decisions of the rows that took
    it as [n, 1 + predicates] booleans (the stop test, then the masks), False where the row had stopped.  ``stop_guard=False``: a stop
    test within its guard does not spoil a row -- the float64 decision stands and a launch that decided otherwise shows as an
    error, not as an exemption.  (SpringPendulum's |h| after Complete is 0 with a magnitude sum of 54: the guard, MARGIN * C_REF =
    2 eps32 m = 1.3e-5, is wider than corr_eps = 1e-5 on EVERY row, while a float32 |h| stays below 0.5 eps32 m = 3.2e-6.)"""
    with np.errstate(all="ignore"):
        eps = float(np.float32(corr_eps))
        if env == "cart":
            c = CartTab(B64, table, partial)
            ap = B64X.inp(ap_in) if exact else B64.inp(ap_in)
            ao = cart_complete(B64, c, ap)
        else:
            e = pend_eq_of_obs(B64, obs)
            ap = B64X.inp(ap_in) if exact else B64.inp(ap_in)
            ao = pend_complete(B64, e, ap)
        n = ap.v.shape[0]
        old = (V(np.zeros(n)), V(np.zeros(n)))
        live, clean, iters = np.ones(n, bool), np.ones(n, bool), np.zeros(n, np.int32)
        for k in range(K):
            if env == "cart":
                a0, a1 = (ap, ao) if partial == 0 else (ao, ap)
                h, g = cart_eq_ineq(B64, c, a0, a1)
                viol = np.abs(h.v) > eps
                amb = ambiguous(V(np.abs(h.v) - eps, h.m), "stop_pred")
                for gj in g:
                    viol |= gj.v > eps
                    amb |= ambiguous(V(gj.v - eps, gj.m), "stop_pred")
                nap, nao, stp, margins = cart_grg_step(B64, c, partial, ap, ao, lr, momentum, old)
                mamb = np.any([ambiguous(mg, "cart_pred") for mg in margins], axis=0)
                on = np.stack([mg.v > 0 for mg in margins], axis=1)
            else:
                h, g = pend_resid(B64, e, ap, ao)
                viol = (np.abs(h.v) > eps) | (g.v > eps)
                amb = ambiguous(V(np.abs(h.v) - eps, h.m), "stop_pred") | ambiguous(V(g.v - eps, g.m), "stop_pred")
                nap, nao, stp, bm = pend_grg_step(B64, e, ap, ao, lr, momentum, old)
                mamb = ambiguous(bm, "pend_pred")
                on = (bm.v > 0)[:, None]
            if k > 0:
                if stop_guard:
                    clean &= ~(live & amb)
                live = live & viol
            clean &= ~(live & mamb)
            if trace is not None:
                trace.append(np.concatenate([live[:, None], on & live[:, None]], axis=1))
            ap, ao = B64.where(live, nap, ap), B64.where(live, nao, ao)
            old = (B64.where(live, stp[0], old[0]), B64.where(live, stp[1], old[1]))
            iters += live
        return ap, ao, iters, clean


def project_interval(env, ap, delta, K, lr, corr_eps, lo, hi, table=None, partial=None, obs=None):
    """Complete + the per-lane loop (corr_momentum = 0) of a float64 proposal ``ap`` that the launch held to within ``delta``:
    the loop in float64 at clip(ap - delta), clip(ap) and clip(ap + delta).  A row whose clip decision, iteration count, stop test or
    any mask differs among the three points, or meets an ambiguous mask at one of them, is AMBIGUOUS: the launch may have taken
    another branch (the stop test is held to the float64 decision at the three points: project_b64, stop_guard).  On every other row the map ap -> a is smooth over the interval (affine for CartSafe, whose masks only pick
    constants; quadratic terms for SpringPendulum), a few float32 ulps wide: the action moves by at most 2 x the larger deviation of
    the end points from the centre (the factor 2 covers the curvature), and the float32 loop adds its own bound, tol_c(<env>_act) *
    eps32 * the magnitude sum carried through the iterations (the convention of check_explore for the budget-0 action).
    Returns (a [n,2] in the action's column order, bound [n,2], ambiguous [n], iters [n], path): ``path`` holds the actions at the
    two end points (``ends``) and the float32 loop's own share of the bound (``own`` [n,2]) -- the proposal is one scalar per row,
    so what follows can be carried along that one-dimensional path."""
    ap, delta = np.asarray(ap, np.float64).reshape(-1), np.asarray(delta, np.float64).reshape(-1)
    lo, hi = float(np.float32(lo)), float(np.float32(hi))
    runs, inside = [], []
    for pt in (ap - delta, ap, ap + delta):
        inside.append(np.stack([pt >= lo, pt <= hi], axis=1))
        tr = []
        p, o, it, clean = project_b64(env, np.clip(pt, lo, hi), K, lr, corr_eps, 0.0, table=table, partial=partial, obs=obs,
                                      exact=True, trace=tr, stop_guard=False)
        runs.append((p, o, it, clean, np.stack(tr, axis=0) if tr else np.zeros((0, ap.size, 1), bool)))
    c = runs[1]
    amb = np.zeros(ap.size, bool)
    for k in (0, 2):
        amb |= (inside[k] != inside[1]).any(axis=1) | (runs[k][2] != c[2]) | (runs[k][4] != c[4]).any(axis=(0, 2))
    for r in runs:
        amb |= ~r[3]
    with np.errstate(all="ignore"):
        dev = [np.maximum(np.abs(runs[0][j].v - c[j].v), np.abs(runs[2][j].v - c[j].v)) for j in (0, 1)]
        own = [tol_c(env + "_act") * EPS32 * B64.mag(c[j]) for j in (0, 1)]
        bp, bo = (2.0 * dev[j] + own[j] + TINY for j in (0, 1))
    join = (lambda p_, o_: cart_join(partial, p_, o_)) if env == "cart" else (lambda p_, o_: np.stack([p_, o_], axis=1))
    path = dict(ends=[join(runs[k][0].v, runs[k][1].v) for k in (0, 2)], own=join(own[0] + TINY, own[1] + TINY))
    return join(c[0].v, c[1].v), join(bp, bo), amb, c[2], path


def batch_project_b64(obs, ap, K, lr, corr_eps, momentum):
    """The whole batch-coupled loop in float64 WITH momentum, the running bound carried through every iteration (the accumulated
    m is at most K single-step bounds).  Returns (a_x V, a_y V, iterations, clean [n], stop_open): ``clean`` rows met no predicate a_x,i dgp_j - bgp_i within K
    single-step guards of 0 along THIS trajectory; ``stop_open``: at some k no row violated surely while one might have."""
    with np.errstate(all="ignore"):
        eps = float(np.float32(corr_eps))
        e = pend_eq_of_obs(B64, obs)
        ax = B64.inp(ap)
        ay = pend_complete(B64, e, ax)
        n = ax.v.shape[0]
        old = (V(np.zeros(n)), V(np.zeros(n)))
        clean, stop_open, k = np.ones(n, bool), False, 0
        for k in range(K + 1):
            if k == K:
                break
            if k > 0:
                h, g = pend_resid(B64, e, ax, ay)
                mh, mg = V(np.abs(h.v) - eps, h.m), V(g.v - eps, g.m)
                ah, ag = ambiguous(mh, "stop_pred"), ambiguous(mg, "stop_pred")
                sure = ((mh.v > 0) & ~ah) | ((mg.v > 0) & ~ag)
                maybe = (mh.v > 0) | (mg.v > 0) | ah | ag
                if not sure.any():
                    stop_open = stop_open or bool(maybe.any())
                    if not ((mh.v > 0) | (mg.v > 0)).any():
                        break
            nx, ny, stp, bm, _ = pend_batch_step(B64, e, ax, ay, lr, momentum, old)
            # a row is clean while every predicate margin stays outside K single-step guards (the margin's bound from exact
            # inputs at this iterate: what K x the single-step tolerance allows the float32 iterate to have drifted)
            _, _, _, bm1, _ = pend_batch_step(B64, e, V(ax.v), V(ay.v), lr)
            clean &= ~ambiguous(V(bm1.v, K * B64.mag(bm1)), "pend_pred").any(axis=1)
            ax, ay, old = nx, ny, stp
        return ax, ay, k, clean, stop_open


def check_batch_momentum(obs, ap, got, K, lr, corr_eps, momentum):
    """rpo_pendulum_project_batchref at the budget K WITH momentum as a whole trajectory: |got - float64 trajectory| per row in
    units of EPS32 * K * the single-step magnitude sum (of the float64 trajectory's last step, taken from exact inputs) -- the
    tolerance is K x the single-step tolerance, NOT the accumulated bound, which the coupling makes hundreds of times wider.
    Returns dict(ratio [n], iters, stop_open, clean [n]: no ambiguous predicate along the float64 momentum trajectory)."""
    got = np.asarray(got, np.float32)
    x, y, it64, clean, stop_open = batch_project_b64(obs, ap, K, lr, corr_eps, momentum)
    with np.errstate(all="ignore"):
        if it64 > 0:
            x9, y9, _, _, _ = batch_project_b64(obs, ap, it64 - 1, lr, corr_eps, momentum)
            e = pend_eq_of_obs(B64, obs)
            sx, sy, _, _, _ = pend_batch_step(B64, e, V(x9.v), V(y9.v), lr)
            mx, my = K * B64.mag(sx), K * B64.mag(sy)
        else:
            mx, my = B64.mag(x), B64.mag(y)
        r = np.maximum(np.abs(got[:, 0] - x.v) / (EPS32 * mx + TINY), np.abs(got[:, 1] - y.v) / (EPS32 * my + TINY))
        r = np.where(np.isfinite(x.v) & np.isfinite(y.v), r, np.where(np.isfinite(got).all(axis=1), np.inf, 0.0))
    return dict(ratio=r, iters=it64, stop_open=stop_open, clean=clean)


# ===================================================================================================== comparison
def ratio(got, ref):
    """|got - ref| / (EPS32 * m) per element for a V ``ref``.  Inf or NaN may come out only where float64 gives them, and must
    come out there: a non-finite value against a finite float64 one, or the reverse, is inf.  An unbounded m (an intermediate
    beyond the float32 range) bounds nothing."""
    got = np.asarray(got, dtype=np.float64)
    r, m = np.broadcast_to(ref.v, got.shape), np.broadcast_to(ref.m, got.shape)
    with np.errstate(all="ignore"):
        out = np.abs(got - r) / (EPS32 * m + TINY)
    # ref finite, bound finite: the ratio, inf if the float32 side is not finite; ref finite, bound unbounded: not judged (0);
    # ref not finite: the float32 side must be non-finite too (0), else inf
    fin = np.isfinite(r)
    same = ~np.isfinite(got)           # (which non-finite value: 0 * inf of a momentum term, inf - inf ... depend on history)
    out = np.where(fin, np.where(np.isfinite(m), np.where(np.isfinite(got), out, np.inf), 0.0), np.where(same, 0.0, np.inf))
    return out


def ambiguous(margin, group):
    """Predicates whose float64 margin lies within GUARD * EPS32 * m of 0 (GUARD = MARGIN * C_REF of the expression)."""
    with np.errstate(all="ignore"):
        m = np.broadcast_to(margin.m, margin.v.shape)
        return (np.abs(margin.v) <= tol_c(group) * EPS32 * m) & (m > 0)        # (m = 0: an exact chain, the float32 margin IS this one)


def check_cart_step(state, action, table, partial, rows, mut=()):
    """Judge the float columns 8..13 and 16..22 of transition rows [n, >= 24] against float64.  Rows whose sign predicate
    n_c x_dot is ambiguous (or could underflow in float32) accept either neighbouring sign.  Returns (dict group -> per-row worst
    ratio [n], ambiguous [n] bool)."""
    rows = np.asarray(rows)
    ref = cart_step(B64, state, action, table, partial)
    prod = ref["prod"]
    # The kernel's sign is that of the FLOAT32 product fl(n_c x_dot) (np.sign in float32): with gradual underflow it is 0 below
    # 2^-150 (|n_c| < 1/2 at the smallest denormal x_dot) although the float64 product keeps its sign -- pinned here as 0.
    mag = np.abs(prod.v)
    flushed = (mag > 0) & (mag < HALF_DENORM * (1 - 1e-3))
    amb = (ambiguous(prod, "sign_pred") | ((mag >= HALF_DENORM * (1 - 1e-3)) & (mag <= HALF_DENORM * (1 + 1e-3)))) \
        & np.isfinite(prod.v) & (prod.v != 0)
    s0 = np.where(flushed, 0.0, B64.val(_sign_of(B64, prod)))
    ref = cart_step(B64, state, action, table, partial, sign=s0)
    cands = [ref]
    if amb.any():
        for alt in (np.where(amb, 0.0, s0), np.where(amb, 1.0, s0), np.where(amb, -1.0, s0)):
            cands.append(cart_step(B64, state, action, table, partial, sign=alt))
    # An ambiguous row is judged against the ONE candidate sign that fits the row as a whole (the largest of its group ratios
    # smallest): the kernel used one sign for every output of the row, so groups may not pick different candidates.
    best = None
    for cd in cands:
        r = dict(cart_viol=np.max([ratio(rows[:, 16], cd["h"])] + [ratio(rows[:, 17 + j], cd["g"][j]) for j in range(6)], axis=0),
                 cart_next=np.max([ratio(rows[:, 8 + j], cd["ns"][j]) for j in (0, 1, 3, 4)], axis=0),
                 cart_acc=np.max([ratio(rows[:, 8 + j], cd["ns"][j]) for j in (2, 5)], axis=0))
        if best is None:
            best = r
        else:                                                        # per row: the candidate that fits the row best as a whole
            tot_new, tot_old = np.max(list(r.values()), axis=0), np.max(list(best.values()), axis=0)
            best = {k: np.where(amb & (tot_new < tot_old), r[k], best[k]) for k in r}
    return best, amb


def check_pend_step(internal, action, rows, nth_stored=None):
    """Judge the float columns of pendulum transition rows [n, 16] (and the stored next theta) against float64."""
    rows = np.asarray(rows)
    ref = pend_step(B64, internal, action)
    out = dict(pend_obs=np.max([ratio(rows[:, j], ref["obs"][j]) for j in range(2)], axis=0),
               pend_viol=np.max([ratio(rows[:, 14], ref["h"]), ratio(rows[:, 15], ref["g"])], axis=0),
               pend_next=np.max([ratio(rows[:, 7 + j], ref["next"][j]) for j in range(5)], axis=0),
               pend_reward=ratio(rows[:, 12], ref["reward"]))
    if nth_stored is not None:
        out["pend_next"] = np.maximum(out["pend_next"], ratio(nth_stored, ref["nth"]))
    return out


def check_profile(env, planes, iters, corr_lr, corr_eps, table=None, partial=None, obs=None):
    """The per-lane loop one iteration at a time (corr_momentum = 0).  planes [K + 1, n, 4], iters [n] from
    rpo_<env>_project_profile or the emulation.  Returns dict:
        grg     [K, n] worst ratio of plane k + 1 against the float64 single step applied to plane k (0 where the row did not step,
                where plane k + 1 must repeat plane k bit for bit: else inf), best over the accepted values of ambiguous predicates
        resid   [K + 1, n] worst ratio of the reported residuals against the float64 residuals of the reported action
        stop_ok [n] bool: stepped at k <=> k == 0 or |eq| > corr_eps or max ineq > corr_eps on the REPORTED residuals, and
                iters == the number of steps taken
        left    [K, n] bool rows left out (more than MAX_ENUM ambiguous predicates), amb [K, n] bool rows with any,
        stop_amb [K + 1, n] bool: the float64 stop margins of the reported iterate lie inside their guard (informative: the stop
                decision itself is held exactly; the momentum trajectory test leaves such rows out)."""
    planes = np.asarray(planes, np.float32)
    K, n = planes.shape[0] - 1, planes.shape[1]
    eps = np.float32(corr_eps)
    grg, left, amb_any = np.zeros((K, n)), np.zeros((K, n), bool), np.zeros((K, n), bool)
    resid = np.zeros((K + 1, n))
    stepped = np.zeros((K, n), bool)
    stop_amb = np.zeros((K + 1, n), bool)        # the float64 stop margins of the reported iterate inside their guard
    if env == "cart":
        c = CartTab(B64, table, partial)
    else:
        e = pend_eq_of_obs(B64, obs)
    with np.errstate(all="ignore"):
        for k in range(K + 1):
            a0, a1 = B64.inp(planes[k, :, 0]), B64.inp(planes[k, :, 1])
            if env == "cart":
                h, g = cart_eq_ineq(B64, c, a0, a1)
                # max_j is 1-Lipschitz in the sup norm: the reported maximum lies within the largest component tolerance of max_j
                gmax = V(np.max([x.v for x in g], axis=0), np.max([B64.mag(x) for x in g], axis=0))
                resid[k] = np.maximum(ratio(planes[k, :, 2], h), ratio(planes[k, :, 3], gmax))
                stop_amb[k] = ambiguous(V(np.abs(h.v) - float(eps), h.m), "stop_pred") | ambiguous(V(gmax.v - float(eps), gmax.m), "stop_pred")
            else:
                h, g = pend_resid(B64, e, a0, a1)
                resid[k] = np.maximum(ratio(planes[k, :, 2], h), ratio(planes[k, :, 3], g))
                stop_amb[k] = ambiguous(V(np.abs(h.v) - float(eps), h.m), "stop_pred") | ambiguous(V(g.v - float(eps), g.m), "stop_pred")
            if k == K:
                break
            want = (np.abs(planes[k, :, 2]) > eps) | (planes[k, :, 3] > eps) if k > 0 else np.ones(n, bool)
            if k > 0:
                want &= stepped[k - 1]
            stepped[k] = want
            same = (planes[k + 1, :, :2].view(np.uint32) == planes[k, :, :2].view(np.uint32)).all(axis=1)
            if env == "cart":
                ap32, ao32 = cart_split(partial, planes[k, :, :2])
                gp32, go32 = cart_split(partial, planes[k + 1, :, :2])
                _, _, _, margins = cart_grg_step(B64, c, partial, ap32, ao32, corr_lr)
                ambm = np.stack([ambiguous(mg, "cart_pred") for mg in margins], axis=1)             # [n, 6]
                base = np.stack([mg.v > 0 for mg in margins], axis=1)
            else:
                _, _, _, bm = pend_grg_step(B64, e, planes[k, :, 0], planes[k, :, 1], corr_lr)
                ambm = ambiguous(bm, "pend_pred")[:, None]
                base = (bm.v > 0)[:, None]
            n_amb = ambm.sum(axis=1)
            amb_any[k] = (n_amb > 0) & want
            left[k] = (n_amb > MAX_ENUM) & want
            best = np.full(n, np.inf)
            for mask in _mask_choices(base, ambm):
                if env == "cart":
                    p1, o1, _, _ = cart_grg_step(B64, c, partial, ap32, ao32, corr_lr, mask=mask)
                    r = np.maximum(ratio(gp32, p1), ratio(go32, o1))
                else:
                    x1, y1, _, _ = pend_grg_step(B64, e, planes[k, :, 0], planes[k, :, 1], corr_lr, mask=mask[:, 0])
                    r = np.maximum(ratio(planes[k + 1, :, 0], x1), ratio(planes[k + 1, :, 1], y1))
                best = np.minimum(best, r)
            grg[k] = np.where(want, np.where(left[k], 0.0, best), np.where(same, 0.0, np.inf))
    took = stepped.sum(axis=0)
    return dict(grg=grg, resid=resid, stop_ok=(took == np.asarray(iters)), stepped=stepped, left=left, amb=amb_any, stop_amb=stop_amb)


def check_batch_budget(obs, prev, cur, took_step, corr_lr, corr_eps, k):
    """Budget k of rpo_pendulum_project_batchref against the float64 coupled step applied to budget k - 1 (``prev`` [n,2] -> ``cur``;
    corr_momentum = 0).  ``took_step``: iters_out said budget k took a k-th step.  Returns dict(ratio [n] with the widened
    tolerance in the denominator, widened [n] bool, stop_ok bool, stop_open bool: every row's stop margin inside its guard)."""
    prev, cur = np.asarray(prev, np.float32), np.asarray(cur, np.float32)
    n = prev.shape[0]
    e = pend_eq_of_obs(B64, obs)
    with np.errstate(all="ignore"):
        h, g = pend_resid(B64, e, B64.inp(prev[:, 0]), B64.inp(prev[:, 1]))
        mh = V(np.abs(h.v) - float(np.float32(corr_eps)), h.m)
        mg = V(g.v - float(np.float32(corr_eps)), g.m)
        sure_viol = ((mh.v > 0) & ~ambiguous(mh, "stop_pred")) | ((mg.v > 0) & ~ambiguous(mg, "stop_pred")) | np.isnan(h.v) | np.isnan(g.v)
        maybe_viol = (mh.v > 0) | (mg.v > 0) | ambiguous(mh, "stop_pred") | ambiguous(mg, "stop_pred")
        if k == 1:
            want, stop_open = True, False
        elif sure_viol.any():
            want, stop_open = True, False
        elif not maybe_viol.any():
            want, stop_open = False, False
        else:
            want, stop_open = bool(took_step), True
        out = dict(stop_ok=bool(took_step) == want, stop_open=stop_open)
        if not took_step:
            out["ratio"] = np.where((prev.view(np.uint32) == cur.view(np.uint32)).all(axis=1), 0.0, np.inf)
            out["widened"] = np.zeros(n, bool)
            return out
        x1, y1, _, bm, dgp = pend_batch_step(B64, e, prev[:, 0], prev[:, 1], corr_lr)
        amb = ambiguous(bm, "pend_pred")                                                     # [n, n]
        lr = float(np.float32(corr_lr))
        extra = lr * (amb * np.abs(dgp.v)[None, :]).sum(axis=1)                              # the row's flipped terms, at most
        tol_x = tol_c("batch_grg") * EPS32 * B64.mag(x1) + extra
        tol_y = tol_c("batch_grg") * EPS32 * B64.mag(y1) + extra * np.abs(e.C_p.v * e.C_o_inv.v) * (1 + 4 * EPS32)
        rx = np.abs(cur[:, 0].astype(np.float64) - x1.v) / (tol_x + TINY)
        ry = np.abs(cur[:, 1].astype(np.float64) - y1.v) / (tol_y + TINY)
        bad = ~np.isfinite(x1.v) | ~np.isfinite(y1.v)
        out["ratio"] = np.where(bad, 0.0, np.maximum(rx, ry)) * tol_c("batch_grg")        # in units of EPS32 * m, as the others
        out["widened"] = amb.any(axis=1)
        return out


def _mask_choices(base, ambm):
    """Every assignment of the (up to MAX_ENUM first) ambiguous predicates of each row: yields masks shaped like ``base``."""
    n_amb = ambm.sum(axis=1)
    order = np.cumsum(ambm, axis=1) - 1
    for flips in itertools.product((False, True), repeat=min(MAX_ENUM, int(n_amb.max()) if len(n_amb) else 0)):
        mask = base.copy()
        for f, flip in enumerate(flips):
            mask ^= (ambm & (order == f)) & flip
        yield mask


def check_ipg(env, step, action, table=None, partial=None, obs=None):
    """rpo_<env>_ineq_partial_grad: per-row worst ratio of step [n,2] against float64, either value of up to MAX_ENUM ambiguous
    predicates accepted.  Returns (ratio [n], left [n] bool: rows with more, not judged)."""
    step, action = np.asarray(step, np.float32), np.asarray(action, np.float32)
    with np.errstate(all="ignore"):
        if env == "cart":
            c = CartTab(B64, table, partial)
            ap = B64.inp(cart_split(partial, action)[0])
            _, margins = cart_reduced_grad(B64, c, ap)
            ambm = np.stack([ambiguous(m, "cart_pred") for m in margins], axis=1)
            base = np.stack([m.v > 0 for m in margins], axis=1)
            got_p, got_o = cart_split(partial, step)
        else:
            e = pend_eq_of_obs(B64, obs)
            _, _, _, bm = pend_grg_step(B64, e, action[:, 0], action[:, 1], 1.0)
            ambm, base = ambiguous(bm, "pend_pred")[:, None], (bm.v > 0)[:, None]
            got_p, got_o = step[:, 0], step[:, 1]
        best = np.full(step.shape[0], np.inf)
        for mask in _mask_choices(base, ambm):
            if env == "cart":
                gp, _ = cart_reduced_grad(B64, c, ap, mask)
                go = -(gp * c.C_p) * c.C_o_inv
            else:
                _, _, (gp, go), _ = pend_grg_step(B64, e, action[:, 0], action[:, 1], 1.0, mask=mask[:, 0])
            best = np.minimum(best, np.maximum(ratio(got_p, gp), ratio(got_o, go)))
        left = ambm.sum(axis=1) > MAX_ENUM
        return np.where(left, 0.0, best), left


def check_lagrangian(env, grad_action, action, nu, scale, table=None, partial=None):
    """d/d action of rpo_<env>_lagrangian [n,2], per-row worst ratio against float64; either value of up to MAX_ENUM ambiguous
    predicates g_j > 0 accepted (margins of exact chains, m = 0, are not ambiguous: 10 * 1 + a1 * 0 - 10 and 16 + 16 - 32 give 0 and
    gradient 0 exactly).  Returns (ratio [n], left [n] bool, exact_zero [n] bool: rows with a margin of exactly 0 and m = 0)."""
    grad_action = np.asarray(grad_action, np.float32)
    with np.errstate(all="ignore"):
        if env == "cart":
            ref = cart_lagrangian(B64, table, partial, action, nu, scale)
            margins = ref["margins"]
        else:
            ref = pend_lagrangian(B64, action, nu, scale)
            margins = [ref["margin"]]
        ambm = np.stack([ambiguous(m, env + "_resid") for m in margins], axis=1)
        base = np.stack([m.v > 0 for m in margins], axis=1)
        zero = np.any([(m.v == 0) & (B64.mag(m) == 0) for m in margins], axis=0)
        best = np.full(grad_action.shape[0], np.inf)
        for mask in _mask_choices(base, ambm):
            l = cart_lagrangian(B64, table, partial, action, nu, scale, mask) if env == "cart" else pend_lagrangian(B64, action, nu, scale, mask[:, 0])
            best = np.minimum(best, np.maximum(ratio(grad_action[:, 0], l["g0"]), ratio(grad_action[:, 1], l["g1"])))
        left = ambm.sum(axis=1) > MAX_ENUM
        return np.where(left, 0.0, best), left, zero


def check_explore(env, action, ap_in, noise, eps_t, lo, hi, table=None, partial=None, obs=None):
    """Exploration + complete_partial (the budget-0 action of rpo_<env>_act_project under RPO_NOISE_EXPLICIT): per-row worst ratio
    of action [n,2] against clip(ap + eps_t noise, lo, hi) and its completion in float64.  The clip is continuous: no seam."""
    action = np.asarray(action, np.float32)
    with np.errstate(all="ignore"):
        ap = explore(B64, ap_in, noise, eps_t, lo, hi)
        if env == "cart":
            ao = cart_complete(B64, CartTab(B64, table, partial), ap)
            gp, go = cart_split(partial, action)
        else:
            ao = pend_complete(B64, pend_eq_of_obs(B64, obs), ap)
            gp, go = action[:, 0], action[:, 1]
        return np.maximum(ratio(gp, ap), ratio(go, ao))


# ===================================================================================================== float32 emulation, rows
def emu_cart_rows(state, action, table, partial, ep_len=0, max_episode_steps=200, mut=()):
    """The transition rows [n,24] of rpo_cartsafe_step from the float32 emulation (no auto-reset)."""
    state, action = np.asarray(state, np.float32), np.asarray(action, np.float32)
    f = cart_step(F32, state, action, table, partial, mut=mut)
    rows = np.zeros((state.shape[0], 24), np.float32)
    rows[:, 0:6], rows[:, 6:8] = state, action
    rows[:, 8:14] = np.stack(f["ns"], axis=1)
    rows[:, 14] = 1.0
    rows[:, 15] = cart_terminated_f32(rows[:, 8:14], mut) | (np.asarray(ep_len) + 1 >= max_episode_steps)
    rows[:, 16] = f["h"]
    rows[:, 17:23] = np.stack(f["g"], axis=1)
    return rows


def emu_pend_rows(internal, action, ep_len=0, max_episode_steps=200, mut=()):
    """(rows [n,16], next internal [n,4]) of rpo_pendulum_step from the float32 emulation (no auto-reset)."""
    internal, action = np.asarray(internal, np.float32), np.asarray(action, np.float32)
    f = pend_step(F32, internal, action, mut=mut)
    rows = np.zeros((internal.shape[0], 16), np.float32)
    rows[:, 0], rows[:, 1] = f["obs"]
    rows[:, 2:5], rows[:, 5:7] = internal[:, 1:4], action
    rows[:, 7:12] = np.stack(f["next"], axis=1)
    rows[:, 12] = f["reward"]
    nint = np.stack([f["nth"], f["next"][2], f["next"][3], f["next"][4]], axis=1).astype(np.float32)
    rows[:, 13] = pend_terminated_f32(nint) | (np.asarray(ep_len) + 1 >= max_episode_steps)
    rows[:, 14], rows[:, 15] = f["h"], f["g"]
    return rows, nint


# ===================================================================================================== inputs
def _nb(v):
    v = np.float32(v)
    return [np.nextafter(v, np.float32(-np.inf)), v, np.nextafter(v, np.float32(np.inf))]


DENORM_MIN = np.float32(1.401298464324817e-45)


def cart_rows(n, seed=0, wide=True):
    """float32 (state [n,6], action [n,2], tag [n]) for the CartSafe step: random rows (reset box for every fourth, else the wide
    box x +-2.5, x_dot +-5, theta +-pi, theta_dot +-10, previous thetaacc +-60; actions uniform +-12) with the edge rows of
    ``cart_edge_rows`` spread over the batch when it has room for them (tag > 0 marks them)."""
    rng = np.random.RandomState(seed)
    st = rng.uniform(-1, 1, (n, 6)) * np.array([2.5, 5.0, 30.0, np.pi, 10.0, 60.0])
    box = np.arange(n) % 4 == 0
    st[box] = rng.uniform(-0.05, 0.05, (int(box.sum()), 6))
    if not wide:
        st = rng.uniform(-0.05, 0.05, (n, 6))
    act = rng.uniform(-12, 12, (n, 2))
    st, act = st.astype(np.float32), act.astype(np.float32)
    tag = np.zeros(n, np.int32)
    es, ea, et = cart_edge_rows()
    m = min(len(et), n // 2)
    if m:
        at = rng.permutation(n)[:m]
        st[at], act[at], tag[at] = es[:m], ea[:m], et[:m]
    return st, act, tag


# tags of the edge rows
T_XDOT0, T_DENORM, T_NC, T_CLIP, T_THRESH, T_DENORM_PIN = 1, 2, 3, 4, 5, 6


def _nc_zero_action(state, f0):
    """f1 such that n_c = f0 sin d0 + f1 sin d1 + m g - ml (thetaacc_prev sin + theta_dot^2 cos) is about 0 (float64)."""
    s = state.astype(np.float64)
    rest = ocs.TOTAL_MASS * ocs.GRAVITY - ocs.POLEMASS_LENGTH * (s[5] * np.sin(s[3]) + s[4] ** 2 * np.cos(s[3]))
    return -(f0 * np.sin(ocs.DELTA[0]) + rest) / np.sin(ocs.DELTA[1])


def cart_edge_rows():
    rng = np.random.RandomState(77)
    S, Aa, T = [], [], []

    def add(s, a, t):
        S.append(np.asarray(s, np.float32)); Aa.append(np.asarray(a, np.float32)); T.append(t)     # noqa: E702
    base = lambda: rng.uniform(-0.05, 0.05, 6).astype(np.float32)                                  # noqa: E731
    for xd in (0.0, -0.0):                                         # sign 0: both friction terms vanish
        for _ in range(3):
            s = base(); s[1] = np.float32(xd); add(s, rng.uniform(-9, 9, 2), T_XDOT0)              # noqa: E702
    for xd in (1e-30, -1e-30, float(DENORM_MIN), -float(DENORM_MIN)):
        for _ in range(2):
            s = base(); s[1] = np.float32(xd); add(s, rng.uniform(-9, 9, 2), T_DENORM)             # noqa: E702
    for off in (-1.0, -0.25, -1e-3, 1e-3, 0.25, 1.0):              # n_c on both sides of 0: f0 in (-10, -6), f1 in (4, 10)
        for xd in (0.7, -0.7):
            s = base(); s[1] = np.float32(xd)                                                      # noqa: E702
            f0 = -8.0 + rng.uniform(-1, 1)
            add(s, [f0, _nc_zero_action(s, f0) - off / abs(np.sin(ocs.DELTA[1]))], T_NC)
    for sgn in (1.0, -1.0):                                        # |n_c| < 1/2 and the smallest denormal: the product rounds to 0
        s = base(); s[1] = sgn * DENORM_MIN                                                        # noqa: E702
        add(s, [-8.0, _nc_zero_action(s, -8.0) - 0.3 / abs(np.sin(ocs.DELTA[1]))], T_DENORM_PIN)
    for v in _nb(10.0) + _nb(-10.0) + [12.0, -12.0, 1e6, -1e6]:     # on and beyond the clip
        add(base(), [v, rng.uniform(-9, 9)], T_CLIP)
        add(base(), [rng.uniform(-9, 9), v], T_CLIP)
    for lim, col in ((X_LIM32, 0), (TH_LIM32, 3)):                 # next x / theta exactly on a threshold and its neighbours
        for sgn in (1.0, -1.0):
            for v in _nb(lim):
                s = base(); s[col] = sgn * v; s[col + 1] = 0.0                                     # noqa: E702
                add(s, rng.uniform(-3, 3, 2), T_THRESH)
    return np.stack(S), np.stack(Aa), np.asarray(T, np.int32)


T_THETA0, T_PI, T_HALFPI, T_SPEED, T_LEN, T_THLIM, T_ACT, T_G32, T_WRAP = 1, 2, 3, 4, 5, 6, 7, 8, 9


def _pend_solve_speed(s, a, target):
    """theta_dot such that the next theta_dot lands on ``target`` (a few float64 fixed-point sweeps; the test then takes what
    the float64 formula gives for the float32 row)."""
    s = s.astype(np.float64).copy()
    for _ in range(30):
        th, thd, l, ld = s
        fth = -np.clip(a[1], -6, 6) * np.sin(th) + np.clip(a[0], -6, 6) * np.cos(th)
        thacc = (fth - opd.M * (opd.G * np.sin(th) + 2 * ld * thd)) / (l * opd.M)
        s[1] = target - thacc * opd.DT
    return s[1]


def pend_edge_rows(half_pi=False):
    rng = np.random.RandomState(78)
    S, Aa, T = [], [], []

    def add(s, a, t):
        S.append(np.asarray(s, np.float32)); Aa.append(np.asarray(a, np.float32)); T.append(t)     # noqa: E702
    lo, hi = opd.RESET_LOW.astype(np.float64), opd.RESET_HIGH.astype(np.float64)
    base = lambda: rng.uniform(lo, hi).astype(np.float32)                                          # noqa: E731
    act = lambda: rng.uniform(-5, 5, 2).astype(np.float32)                                         # noqa: E731
    for _ in range(3):
        s = base(); s[0] = 0.0; add(s, act(), T_THETA0)                                            # noqa: E702
    for v in _nb(np.pi) + _nb(-np.pi):
        s = base(); s[0] = v; add(s, act(), T_PI)                                                  # noqa: E702
    for v in (3 * np.pi, -3 * np.pi, 7.0, -7.0, 3.2, -3.2, 9.0, -9.0):
        s = base(); s[0] = np.float32(v); add(s, act(), T_WRAP)                                    # noqa: E702
    if half_pi:                                                    # cos theta -> 0: C_o_inv of the size of 1e7 (and past a wrap)
        for v in _nb(np.pi / 2) + _nb(-np.pi / 2) + [np.float32(2.5 * np.pi), np.float32(-2.5 * np.pi)]:
            s = base(); s[0] = v; add(s, act(), T_HALFPI)                                          # noqa: E702
    for tgt in (8.0, -8.0, 8.0 + 1e-5, -8.0 - 1e-5, 8.0 - 1e-5, 9.0, -9.0):
        s, a = base(), act()
        s[1] = np.float32(_pend_solve_speed(s, a, tgt)); add(s, a, T_SPEED)                        # noqa: E702
    for l, ld in ((0.75, -5.0), (1.25, 5.0), (0.5, 0.0), (1.5, 0.0), (1.0, 10.0), (1.0, -10.0)):    # l + l_dot dt = 0.5 / 1.5
        s = base(); s[2], s[3] = l, ld; add(s, act(), T_LEN)                                       # noqa: E702
    lim = np.float32(np.pi / 12)
    for sgn in (1.0, -1.0):
        for v in _nb(lim):                                         # next theta near the limit: theta on it, next theta_dot ~ 0
            s, a = base(), act()
            s[0] = sgn * v
            s[1] = np.float32(_pend_solve_speed(s, a, 0.0)); add(s, a, T_THLIM)                    # noqa: E702
    for v in _nb(6.0) + _nb(-6.0) + [7.0, -7.0, 1e6, -1e6]:
        add(base(), [v, rng.uniform(-3, 3)], T_ACT)
        add(base(), [rng.uniform(-3, 3), v], T_ACT)
    for a in pend_g32_actions():
        add(base(), a, T_G32)
    return np.stack(S), np.stack(Aa), np.asarray(T, np.int32)


def pend_g32_actions():
    """Actions with |a|^2 - 32 of both signs within a few ulp, and exactly 0 ((4, 4): 16 + 16 - 32)."""
    out = [np.array([4.0, 4.0], np.float32), np.array([-4.0, 4.0], np.float32)]
    for ax in (3.0, 1.0, 5.5, -2.25):
        ay = np.float32(math.sqrt(32.0 - ax * ax))
        for v in _nb(ay) + [np.nextafter(_nb(ay)[2], np.float32(np.inf))]:
            out.append(np.array([ax, v], np.float32))
    return out


def pend_rows(n, seed=0, half_pi=False, wide=True):
    """float32 (internal [n,4], action [n,2], tag [n]) for the SpringPendulum kernels: random rows (reset box for every fourth,
    else theta +-3 pi for every eighth and +-pi/12 otherwise, theta_dot +-8, l in [0.5, 1.5], l_dot +-2; actions uniform +-7) with the
    edge rows of ``pend_edge_rows`` spread over the batch when it has room for them."""
    rng = np.random.RandomState(seed + 1000)
    st = np.stack([rng.uniform(-np.pi / 12, np.pi / 12, n), rng.uniform(-8, 8, n), rng.uniform(0.5, 1.5, n), rng.uniform(-2, 2, n)], axis=1)
    far = np.arange(n) % 8 == 3
    st[far, 0] = rng.uniform(-3 * np.pi, 3 * np.pi, int(far.sum()))
    box = np.arange(n) % 4 == 0
    lo, hi = opd.RESET_LOW.astype(np.float64), opd.RESET_HIGH.astype(np.float64)
    st[box] = rng.uniform(lo, hi, (int(box.sum()), 4))
    if not wide:
        st = rng.uniform(lo, hi, (n, 4))
    act = rng.uniform(-7, 7, (n, 2))
    st, act = st.astype(np.float32), act.astype(np.float32)
    tag = np.zeros(n, np.int32)
    es, ea, et = pend_edge_rows(half_pi)
    m = min(len(et), n // 2)
    if m:
        at = rng.permutation(n)[:m]
        st[at], act[at], tag[at] = es[:m], ea[:m], et[:m]
    return st, act, tag


def pend_obs32(internal):
    """The float32 observation the kernels read, from numpy's float32 cos / sin (an INPUT of the constraint kernels)."""
    s = np.asarray(internal, np.float32)
    return np.stack([np.cos(s[:, 0]), np.sin(s[:, 0]), s[:, 1], s[:, 2], s[:, 3]], axis=1).astype(np.float32)


def cart_proposals(n, seed=0):
    """Basic actions for the CartSafe projection: uniform [-10, 10] with the box corners +-10 (ON the reduced box rows' thresholds,
    an exact chain: 10 * 1 - 10) and their float32 neighbours, +-0, and values next to the other reduced thresholds (+-6.93, 8)."""
    rng = np.random.RandomState(seed + 5)
    ap = rng.uniform(-10, 10, n).astype(np.float32)
    edge = np.array(_nb(10.0) + _nb(-10.0) + [0.0, -0.0] + _nb(8.0) + [9.9, -9.9, 6.9, -6.9], np.float32)
    m = min(len(edge), n // 2)
    if m:
        ap[rng.permutation(n)[:m]] = edge[:m]
    return ap


def pend_proposals(n, seed=0, half_pi=False):
    """(obs32 [n,5], ap [n]) for the pendulum projection: observations of ``pend_rows`` states (theta within +-pi/12 except the
    wide and edge rows), basic actions uniform [-6, 6] with the box corners and 0."""
    st, act, tag = pend_rows(n, seed, half_pi=half_pi)
    rng = np.random.RandomState(seed + 6)
    ap = rng.uniform(-6, 6, n).astype(np.float32)
    edge = np.array(_nb(6.0) + _nb(-6.0) + [0.0, -0.0, 5.9, -5.9], np.float32)
    m = min(len(edge), n // 4)
    if m:
        ap[rng.permutation(n)[:m]] = edge[:m]
    obs = pend_obs32(st)
    if n >= 8:
        obs[n // 2], ap[n // 2], tag[n // 2] = EXACT_ZERO_OBS, EXACT_ZERO_AP, T_EXACT0
    return obs, ap, tag


# theta = 0, l = 1, l_dot = 1/2: b = 0, so a = (4, 0), dgp = 8, bgp = 32 and the mask's a_x dgp - bgp = 0 EXACTLY, in float32 too
# (m = 0): `>` leaves the row where it is, `>=` would move it by 8 lr.
EXACT_ZERO_OBS, EXACT_ZERO_AP, T_EXACT0 = np.array([1.0, 0.0, 0.0, 1.0, 0.5], np.float32), np.float32(4.0), 10


def batch_inputs(n, kind="random", seed=0):
    """(obs32 [n,5], ap [n]) for the batch-coupled projection.  random: reset-box states with theta_dot +-1, a_x N(0, 1.5) -- about
    a third of the rows infeasible; feasible: theta = 0 rows (C_p = 0, C_o = 1: completion exact, h = 0 exactly) with a_x = 0 and
    b of the size of 5 (|a|^2 < 32 by a wide margin); one_first / one_last: the same with row 0 / n - 1 pushed outside |a|^2 = 32."""
    rng = np.random.RandomState(seed + 11 * n)
    lo, hi = opd.RESET_LOW.astype(np.float64), opd.RESET_HIGH.astype(np.float64)
    st = rng.uniform(lo, hi, (n, 4)).astype(np.float32)
    if kind == "random":
        obs, ap = pend_obs32(st), (1.5 * rng.randn(n)).astype(np.float32)
        if n >= 3:
            obs[1], ap[1] = EXACT_ZERO_OBS, EXACT_ZERO_AP
        return obs, ap
    st[:, 0] = 0.0
    st[:, 1] = 0.0
    st[:, 3] = rng.uniform(-0.05, 0.05, n).astype(np.float32)
    ap = np.zeros(n, np.float32)
    if kind == "one_first":
        ap[0] = 5.0
    elif kind == "one_last":
        ap[n - 1] = 5.0
    else:
        assert kind == "feasible"
    return pend_obs32(st), ap
