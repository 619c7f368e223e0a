"""Float64 restatement of the policy-head and TD kernels (csrc/heads_dev.h: gauss_head_row, gauss_head_bwd_row, tanh_box_bwd_row,
td_*; include/rpo_hip.h: rpo_gauss_head(_bwd), rpo_tanh_box_bwd, rpo_evopf_*, rpo_td_huber), the edge inputs that exercise them and
the yardstick that turns "close to float64" into a number.  Not collected; used by test_heads_f64.py (CPU) and test_heads_gpu.py.

The functions are written from the reference's formulas (model/policy.py:24-33,48-71, agent/sac_pa.py:111, agent/ddpg_pa.py:108-110,
rpo_ddpg.py:331-335, rpo_sac.py:346-353) in torch float64, gradients by autograd:

    ls = clamp(raw_ls - 3, -23, -2),  sd = exp(ls),  x = mean + sd e,  y = tanh(x)
    logp = -e^2/2 - ls - log(2 pi)/2 - log(scale (1 - y^2) + 1e-6)
    ap = clamp(scale y + base, lo, hi)                  (deterministic: y = tanh(mean))

(Normal(mean, sd).log_prob(x) at x = mean + sd e IS -e^2/2 - ls - log(2 pi)/2; the kernels implement this form.  Evaluated literally
as -(x - mean)^2 / (2 sd^2) in float32 the difference x - mean cancels -- see ``module_cancel``.)

Magnitude sums.  Beside every output the same expression is evaluated as a first-order running error bound in units of eps32:
every term enters with its absolute value (its own rounding), and every intermediate with its own magnitude sum times the
derivative of what follows.  With u = one rounding:
    x:        xm  = |mean| + |e| sd
    y:        ym  = (1 - y^2) xm + |y|
    1 - y^2:  omm = 2 |y| ym + 1 + y^2                        (absolute: 1 - y y rounds at the size of 1, however small the result)
    ap:       scale ym + |scale y| + |base| (+ the box's own magnitude sums where the box is computed: EVOPF)
    logp:     e^2/2 + |ls| + log(2 pi)/2 + |log arg| + (scale omm + ...) / arg,   arg = scale (1 - y^2) + 1e-6
so a saturated row (1 - y^2 of the size of eps32, arg -> 1e-6) carries the large bound that the float32 formula -- the reference's
as much as the kernel's -- really has there, and every other row a bound of a few units.  A float32 evaluation of the formula is
expected within a small multiple c of eps32 * magnitude sum on EVERY row; c is measured, per output, as ``C_REF_*`` below.
"""
import math

import numpy as np
import torch

from oracle import evopf as oe

EPS32 = float(torch.finfo(torch.float32).eps)        # 2^-23
TINY = 1e-30                                         # float32 underflow of products far below every value compared here
LS_MIN, LS_MAX = -23.0, -2.0
HALF_LOG_2PI = 0.9189385332046727
YARD_LS = -10.0                                      # rows with raw_ls - 3 below this are left out of the yardstick (only)
MARGIN = 4.0                                         # GPU tolerance = MARGIN * C_REF_* * EPS32 * magnitude sum

# The yardstick: max over the yardstick rows (every edge row and random row with raw_ls - 3 >= -10, three boxes) of
# |float32 - float64| / (EPS32 * magnitude sum), the float32 side being THIS file's functions run by torch on the CPU in float32
# (never a kernel).  Measured by tests/test_heads_f64.py::test_yardstick, which recomputes them and fails on a drift beyond 2x.
C_REF_AP = 0.60          # measured 0.599: ap, stochastic and deterministic mode
C_REF_LOGP = 0.80        # measured 0.794: log-probability per element
C_REF_G_MEAN = 4.1       # measured 4.118: gradient w.r.t. the mean head (dap with dlogp = 0.01, and dap alone); the worst rows are
#                          the half-saturated ones, where 1 - y^2 is a few eps32 and the first-order bound runs out
C_REF_G_LS = 3.75        # measured 3.750: gradient w.r.t. the log-std head, same runs
C_REF_BOX_BWD = 0.30     # measured 0.296: d ap / d o of the deterministic head from o, with and without noise + clip, away from
#                          the clip seam


def f32(v):
    """The float32 value nearest to v, as a Python float (what a ``float`` argument of the C ABI receives)."""
    return float(np.float32(v))


class Box(object):
    """A scalar action box as the stand-alone launches take it: (lo, hi, scale, base), float32-exact."""

    def __init__(self, name, lo, hi, scale=None, base=None):
        self.name, self.lo, self.hi = name, f32(lo), f32(hi)
        self.scale = f32((hi - lo) / 2 if scale is None else scale)
        self.base = f32(lo + (hi - lo) / 2 if base is None else base)

    def __repr__(self):
        return self.name


BOXES = {"wide": Box("wide", -10.0, 10.0), "unit": Box("unit", -1.0, 1.0), "offset": Box("offset", 4.9, 5.1, 0.1, 5.0)}


def _t(v, dtype, like=None):
    t = torch.as_tensor(v)
    if t.dtype not in (torch.float32, torch.float64):
        t = t.to(torch.float64)
    t = t.to(dtype)
    return t if like is None else t.expand_as(like) if t.dim() else t.expand(like.shape)


# ================================================================================================== squashed Gaussian
def gauss_head(mean, raw_ls, e, scale, base, lo, hi, dap=None, dlogp=0.0, deterministic=False, dtype=torch.float64,
               literal=False):
    """Forward and (with ``dap``) backward of the squashed-Gaussian head, elementwise over tensors of one shape; scale, base, lo,
    hi scalars or tensors of that shape.  Returns dict(ap, logp[, g_mean, g_ls]) in ``dtype``; logp per element (EVOPF sums 14).
    ``literal``: log_prob written as Normal.log_prob does, -(x - mean)^2 / (2 sd sd) - ls - log(2 pi)/2 (the torch modules)."""
    mean = _t(mean, dtype).clone().requires_grad_(dap is not None)
    raw_ls = _t(raw_ls, dtype, mean).clone().requires_grad_(dap is not None)
    e, scale, base, lo, hi = (_t(v, dtype, mean) for v in (e, scale, base, lo, hi))
    ls = torch.clamp(raw_ls - 3, min=LS_MIN, max=LS_MAX)
    sd = ls.exp()
    x = mean + e * sd
    y = torch.tanh(x)
    if literal:
        logp = -((x - mean) ** 2) / (2 * sd * sd) - ls - HALF_LOG_2PI
    else:
        logp = -0.5 * e * e - ls - HALF_LOG_2PI
    logp = logp - torch.log(scale * (1 - y * y) + 1e-6)
    a = scale * torch.tanh(mean) + base if deterministic else scale * y + base
    ap = torch.clamp(a, min=lo, max=hi)                          # (tensor bounds: backward passes on lo <= a <= hi, NaN stays NaN)
    out = dict(ap=ap.detach(), logp=logp.detach())
    if dap is not None:
        loss = (_t(dap, dtype, mean) * ap).sum() + (_t(dlogp, dtype, mean) * logp).sum()
        out["g_mean"], out["g_ls"] = torch.autograd.grad(loss, (mean, raw_ls))
    return out


def gauss_mags(mean, raw_ls, e, scale, base, dap=None, dlogp=0.0, deterministic=False, scale_mag=0.0, base_mag=0.0):
    """The magnitude sums of gauss_head's outputs (module docstring), float64.  scale_mag / base_mag: the magnitude sums of a box
    that the kernel computes itself (EVOPF); 0 for a box passed as float32 arguments."""
    d = torch.float64
    mean = _t(mean, d)
    raw_ls, e, scale, base, scale_mag, base_mag = (_t(v, d, mean) for v in (raw_ls, e, scale, base, scale_mag, base_mag))
    ls = torch.clamp(raw_ls - 3, min=LS_MIN, max=LS_MAX)
    sd = ls.exp()
    x = mean + e * sd
    y = torch.tanh(x)
    xm = mean.abs() + e.abs() * sd
    om = 4.0 / (torch.exp(x) + torch.exp(-x)) ** 2               # 1 - tanh^2 without the cancellation
    ym = om * xm + y.abs()
    omm = 2 * y.abs() * ym + 1 + y * y
    arg = scale * om + 1e-6
    if deterministic:
        t = torch.tanh(mean)
        tm = (1 - t * t) * mean.abs() + t.abs()
        ap_mag = scale_mag * t.abs() + scale.abs() * tm + (scale * t).abs() + base_mag + base.abs()
    else:
        ap_mag = scale_mag * y.abs() + scale.abs() * ym + (scale * y).abs() + base_mag + base.abs()
    logp_mag = 0.5 * e * e + ls.abs() + HALF_LOG_2PI + arg.log().abs() + (scale.abs() * omm + (scale_mag + scale.abs()) * om) / arg + 1
    out = dict(ap=ap_mag, logp=logp_mag)
    if dap is not None:
        dap, dlogp = _t(dap, d, mean).abs(), _t(dlogp, d, mean).abs()
        g_ap_mag = dap * (scale.abs() * (omm + 2 * om) + scale_mag * om)
        g_lp_mag = 2 * dlogp * (scale.abs() * (ym * om / arg + y.abs() * omm * 1e-6 / arg ** 2 + 4 * y.abs() * om / arg)
                                + scale_mag * y.abs() * om * 1e-6 / arg ** 2)
        gx_abs = dap * scale.abs() * om + 2 * dlogp * scale.abs() * y.abs() * om / arg
        out["g_mean"] = g_ap_mag + g_lp_mag + gx_abs
        out["g_ls"] = out["g_mean"] * e.abs() * sd + 3 * gx_abs * e.abs() * sd + dlogp
    return out


def module_cancel(mean, raw_ls, e, dlogp=0.0):
    """What the LITERAL float32 form -(x - mean)^2 / (2 sd^2) adds to the bounds, in units of eps32 (first order): x rounds at
    |x|, so x - mean = sd e (1 + delta) with |delta| <= |x| / (|e| sd) u and the term is off by e^2 delta = |e| |x| / sd; in the
    backward the two paths of +-(x - mean) / sd^2 = +-e / sd into the mean meet again and cancel to the rounding of their size,
    and the two of e^2 / sd into sd leave e^2 delta behind (times sd for the log-std head)."""
    d = torch.float64
    mean = _t(mean, d)
    raw_ls, e, dlogp = (_t(v, d, mean) for v in (raw_ls, e, dlogp))
    sd = torch.clamp(raw_ls - 3, min=LS_MIN, max=LS_MAX).exp()
    x = mean + e * sd
    big = e.abs() * (x.abs() + mean.abs()) / sd
    return dict(logp=big + e * e, g_mean=dlogp.abs() * e.abs() / sd, g_ls=dlogp.abs() * (big + e * e))


# ================================================================================================== deterministic tanh box
def tanh_box(o, noise, eps_t, scale, base, lo, hi, dap=None, dtype=torch.float64):
    """ap_det = scale tanh(o) + base; ap = clamp(ap_det + eps_t noise, lo, hi) (noise None: ap = ap_det, no clip); with ``dap``
    g = d (dap . ap) / d o.  Returns dict(ap_det, pre, ap[, g])."""
    o = _t(o, dtype).clone().requires_grad_(dap is not None)
    scale, base, lo, hi = (_t(v, dtype, o) for v in (scale, base, lo, hi))
    ap_det = scale * torch.tanh(o) + base
    pre = ap_det if noise is None else ap_det + _t(eps_t, dtype, o) * _t(noise, dtype, o)
    ap = pre if noise is None else torch.clamp(pre, min=lo, max=hi)
    out = dict(ap_det=ap_det.detach(), pre=pre.detach(), ap=ap.detach())
    if dap is not None:
        out["g"], = torch.autograd.grad((_t(dap, dtype, o) * ap).sum(), (o,))
    return out


def tanh_box_mags(o, scale, dap, scale_mag=0.0):
    """Magnitude sum of tanh_box's g = dap scale (1 - tanh(o)^2) (module docstring; x = o is an input: xm = |o|)."""
    d = torch.float64
    o = _t(o, d)
    scale, dap, scale_mag = (_t(v, d, o) for v in (scale, dap, scale_mag))
    y = torch.tanh(o)
    om = 4.0 / (torch.exp(o) + torch.exp(-o)) ** 2
    ym = om * o.abs() + y.abs()
    omm = 2 * y.abs() * ym + 1 + y * y
    return dap.abs() * (scale.abs() * (omm + 2 * om) + scale_mag * om)


def eps_schedule(eps_start, eps_end, eps_decay, t):
    """PDDDPG_PA.eps_decay (agent/ddpg_pa.py:118-119) at vector step t."""
    return max(eps_end, eps_start - eps_decay * t)


# ================================================================================================== EVOPF box
def evopf_box(state):
    """Per-dimension box of the 14 basic actions from oracle/evopf.py (EVOPFEnv.update) for float32 states, float64:
    (lo, hi, scale, base, scale_mag, base_mag), each [n, 14].  The kernel computes the box in float32 -- table entries rounded
    once; battery limits min(0.2, 0.8 - soc) / 0.9 and 0.9 max(-0.2, 0.1 - soc) -- so lo / hi carry the magnitude sums of those
    expressions, scale = (hi - lo) / 2 and base = lo + scale the sums of theirs."""
    s = np.asarray(state, dtype=np.float64)
    lo, hi = oe.partial_box(s)
    soc = np.abs(s[:, -oe.GRID.ne - oe.NAHEAD:-oe.NAHEAD])
    lo_mag, hi_mag = np.abs(lo), np.abs(hi)
    hi_mag[:, -oe.GRID.ne:] = 2 * (oe.B_HIGH + soc) / oe.ETA_IN
    lo_mag[:, -oe.GRID.ne:] = 2 * oe.ETA_OUT * (oe.B_LOW + soc)
    lo, hi, lo_mag, hi_mag = (torch.from_numpy(np.ascontiguousarray(v)) for v in (lo, hi, lo_mag, hi_mag))
    scale = (hi - lo) * 0.5
    scale_mag = (hi_mag + lo_mag) * 0.5 + scale.abs()
    return lo, hi, scale, lo + scale, scale_mag, lo_mag + scale_mag + (lo + scale).abs()


# ================================================================================================== TD target + smooth-L1
def td_huber(q1, qn1, reward, done, gamma, q2=None, qn2=None, logp=None, alpha=0.0):
    """y = r + gamma (1 - done) (min(qn1, qn2) - alpha logp); per critic d = q - y, dLoss/dq = clamp(d, -1, 1) / n and the mean
    smooth-L1 loss (both critics added), float64 from float32 inputs; gamma / alpha as the kernel's float32 arguments.
    Returns dict(y, d1, g1, loss[, d2, g2])."""
    f = lambda t: None if t is None else torch.as_tensor(t).to(torch.float64).reshape(-1)      # noqa: E731
    q1, qn1, reward, done, q2, qn2, logp = (f(v) for v in (q1, qn1, reward, done, q2, qn2, logp))
    n = q1.numel()
    qn = qn1 if qn2 is None else torch.minimum(qn1, qn2)
    if logp is not None:
        qn = qn - f32(alpha) * logp
    y = reward + f32(gamma) * (1.0 - done) * qn
    out = dict(y=y, loss=0.0)
    for k, q in (("1", q1), ("2", q2)):
        if q is None:
            continue
        d = q - y
        ad = d.abs()
        out["d" + k], out["g" + k] = d, d.clamp(-1.0, 1.0) / n
        out["loss"] += float((torch.where(ad < 1.0, 0.5 * d * d, ad - 0.5)).sum() / n)
    return out


# ================================================================================================== inputs
MEANS = (0.0, 1e-4, -1e-4, 0.5, -0.5, 3.0, -3.0, 9.5, -9.5, 20.0, -20.0, 88.0, -88.0)     # tanhf is exactly 1 from about 9.01 on
DRAWS = (0.0, 1e-3, -1e-3, 1.0, -1.0, 4.0, -4.0, 5.7, -5.7)


def _neighbours(v):
    v = np.float32(v)
    return [np.nextafter(v, np.float32(-np.inf)), np.nextafter(v, np.float32(np.inf))]


def ls_edges():
    """(raw, raw - 3) float32: raw - 3 in {-30, -23 and its two float32 neighbours, -12, -3, -2 and its two neighbours, +5}, every
    raw chosen so that the float32 subtraction raw - 3 is exact."""
    ls = np.array([-30.0, -23.0] + _neighbours(-23.0) + [-12.0, -3.0, -2.0] + _neighbours(-2.0) + [5.0], dtype=np.float32)
    raw = (ls.astype(np.float64) + 3.0).astype(np.float32)
    assert np.array_equal(raw - np.float32(3.0), ls) and np.array_equal(raw.astype(np.float64) - 3.0, ls.astype(np.float64))
    return raw, ls


def edge_grid():
    """The full cross product MEANS x ls_edges x DRAWS: float32 (mean, raw_ls, e), 13 * 10 * 9 = 1170 rows."""
    m, r, e = np.meshgrid(np.array(MEANS, np.float32), ls_edges()[0], np.array(DRAWS, np.float32), indexing="ij")
    return m.reshape(-1), r.reshape(-1), e.reshape(-1)


def random_rows(n, seed):
    """Random rows: means of a trained policy's range with a tail into saturation, raw_ls - 3 in (-9.9, -1) -- both sides of the
    upper clamp, all inside the yardstick -- except every 200th row, which goes down to the lower clamp; draws N(0, 1)."""
    rng = np.random.RandomState(seed)
    mean = np.where(rng.rand(n) < 0.8, 1.5 * rng.randn(n), rng.uniform(-12, 12, n))
    raw = rng.uniform(-6.9, 2.0, n)
    low = np.arange(n) % 200 == 199
    raw[low] = rng.uniform(-22.0, -7.0, int(low.sum()))
    return mean.astype(np.float32), raw.astype(np.float32), rng.randn(n).astype(np.float32)


N_EDGE = 13 * 10 * 9


def rows(n, seed=0):
    """n rows (mean, raw_ls, e, is_edge): the whole edge grid followed by random rows when n allows it, otherwise a fixed random
    choice from the edge grid and as many random rows."""
    em, er, ee = edge_grid()
    if n >= N_EDGE:
        rm, rr, re_ = random_rows(n - N_EDGE, seed) if n > N_EDGE else (np.zeros(0, np.float32),) * 3
        edge = np.arange(n) < N_EDGE
        return np.concatenate([em, rm]), np.concatenate([er, rr]), np.concatenate([ee, re_]), edge
    rm, rr, re_ = random_rows(N_EDGE, seed)
    pick = np.random.RandomState(seed + 1).permutation(2 * N_EDGE)[:n]
    m, r, e = np.concatenate([em, rm])[pick], np.concatenate([er, rr])[pick], np.concatenate([ee, re_])[pick]
    return m, r, e, pick < N_EDGE


def yard_mask(raw_ls):
    return (np.asarray(raw_ls, dtype=np.float64) - 3.0) >= YARD_LS


def gradient_weights(n, seed):
    """dap per row (order 1, both signs, never 0) for the backward tests."""
    rng = np.random.RandomState(seed + 7)
    return (rng.choice([-1.0, 1.0], n) * rng.uniform(0.25, 2.0, n)).astype(np.float32)


def box_rows(box, n, seed=0):
    """Inputs of the deterministic head: raw outputs o over MEANS and N(0, 2) (with a tail into saturation), noise N(0, 1) scaled
    so that a good share of the rows clips on either side; float32 (o, noise)."""
    rng = np.random.RandomState(seed + 3)
    o = np.where(rng.rand(n) < 0.8, 1.5 * rng.randn(n), rng.uniform(-12, 12, n))
    k = min(n, len(MEANS))
    o[:k] = np.array(MEANS)[:k]
    return o.astype(np.float32), rng.randn(n).astype(np.float32)


def clip_mask_rows(box, eps_t):
    """Rows of rpo_tanh_box_bwd that sit on the clip seam: ap_det = base (tanh(o) = 0 exactly) and noise such that ap_det + eps_t *
    noise is exactly lo, hi and their float32 neighbours; eps_t a power of two, every float32 product and sum exact (asserted).
    Returns float32 (ap_det, noise, target) and the bool ``inside`` = lo <= target <= hi."""
    assert math.frexp(eps_t)[0] == 0.5
    lo, hi, base = np.float32(box.lo), np.float32(box.hi), np.float32(box.base)
    target = np.array([lo, hi] + _neighbours(lo) + _neighbours(hi), dtype=np.float32)
    noise = ((target.astype(np.float64) - float(base)) / eps_t).astype(np.float32)
    assert np.array_equal(noise.astype(np.float64) * eps_t + float(base), target.astype(np.float64))      # exact in float64 ...
    assert np.array_equal(base + np.float32(eps_t) * noise, target)                                          # ... and in float32
    return np.full(len(target), base, np.float32), noise, target, (target >= lo) & (target <= hi)


def near_seam(value, lo, hi, rel=8 * EPS32):
    """Rows whose float64 ``value`` lies within a few float32 roundings of lo or hi: there the float32 side may land on the other
    side of the clip mask, and a comparison of gradients says nothing."""
    value, lo, hi = (torch.as_tensor(v, dtype=torch.float64) for v in (value, lo, hi))
    w = rel * torch.maximum(torch.maximum(lo.abs(), hi.abs()), value.abs())
    return ((value - lo).abs() <= w) | ((value - hi).abs() <= w)


def worst(got, ref, mag):
    """max |got - ref| / (EPS32 * mag) over the elements (the quantity C_REF_* bound and the GPU tests limit)."""
    err = (torch.as_tensor(got).to(torch.float64) - ref).abs()
    return float((err / (EPS32 * mag + TINY)).max())


# ============================================================================ the tanh box as the epilogue of rpo_mlp_forward
C_REF_BOX_FWD = 0.40     # measured 0.398 (tests/test_mlp_f64.py::test_box_forward_yardstick): ap = scale tanh(o) + base from o, three boxes


def tanh_box_fwd_mags(o, scale, base):
    """Magnitude sum of ap = scale tanh(o) + base from a given o (module docstring with xm = |o|): scale ym + |scale y| + |base|;
    scale / base Python floats, o on any device."""
    o = o.to(torch.float64)
    y = torch.tanh(o)
    ym = (1 - y * y) * o.abs() + y.abs()
    return abs(scale) * ym + (scale * y).abs() + abs(base)


def box_fwd_rows(seed=0):
    """The o values of the yardstick of the forward map: MEANS, their neighbours, and random rows."""
    g = torch.Generator().manual_seed(seed)
    edge = [float(w) for v in MEANS for w in [np.float32(v)] + _neighbours(v)]
    return torch.cat([torch.tensor(edge, dtype=torch.float64), 3.0 * torch.randn(4096, generator=g, dtype=torch.float64)]).float()
