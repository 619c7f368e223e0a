"""Float64 restatement of the optimiser kernels (rpo_amd/csrc/train_ops.hip: absmax_kernel, adam_body, polyak_kernel,
min_q_bwd_kernel; include/rpo_hip.h: rpo_absmax(_slots), rpo_adam_step(_multi), rpo_polyak, rpo_min_q_bwd), the inputs that
exercise them and the yardstick that turns "close to float64" into a number.  Not collected; used by test_optim_f64.py (CPU) and
test_optim_f64_gpu.py.

One optimiser step, elementwise over float32 tensors taken as exact, in float64 arithmetic (torch.optim.Adam single-tensor path,
clip_grad_norm_(inf), DualAdam's clamp model/dual.py:41-43, soft_update agent/ddpg_pa.py:77-86):

    coef = min(1, thres / (norm + 1e-6))        norm = max |grad_i| over the elements that are not NaN
    g    = coef grad                            (written back; zero_grad: 0 is written back instead)
    g    = -g (maximize);  g += weight_decay w
    m'   = m + (g - m) (1 - beta1)              v' = v beta2 + (1 - beta2) g g
    w'   = w - step_size m' / (sqrt(v') / sqrt(bc2) + eps),   step_size = lr / bc1,  bc_k = 1 - beta_k^step
    w'   = max(w', 0) (clamp_min0);  target' = (1 - tau) target + tau w';  target2' likewise on the first n2 elements

The SCALARS come in two conventions (``scalars=``), the tensors' arithmetic is float64 in both:
    "kernel": what train_ops.hip does with the float arguments of the C ABI: lr, betas, eps, weight_decay, tau, thres rounded to
              float32 first; 1 - beta and 1 - tau formed IN float32 from the rounded value; bc1 and sqrt(bc2) in double from the
              float32 betas; step_size and sqrt(bc2) rounded to float32.  clamp_min0 is fmaxf: a NaN parameter comes out as 0.
    "torch":  what torch.optim.Adam hands the ops of tensors of dtype T (T = the dtype of the state passed in): double betas;
              T(1 - beta1), T(beta2), T(1 - beta2), T(step_size), T(sqrt(bc2)), T(eps), bc from the double betas.  NaN stays NaN.
With float32 betas = (0.9, 0.999) the two disagree on 1 - beta2 by 1.3e-5 relative: float32(1) - float32(0.999) against
float32(1 - 0.999).  One step moves exp_avg_sq by 1.3e-5 (1 - beta2) g^2 = 0.11 eps32 g^2; over thousands of steps it compounds to
1.3e-5 relative (test_optim_f64.py::test_one_minus_beta_deviation).

A float32 result that overflows is inf in the reference as well (v' > FLT_MAX: sqrt(inf) = inf and the update is 0, as in torch).

Magnitude sums (the error of a float32 evaluation is measured in units of eps32 * these):
    exp_avg:     |m| + |g|,  |g| = |coef grad| + weight_decay |w|
    exp_avg_sq:  v + |g|^2
    update:      w'_32 - w_32 formed in float64 from the float32 values, against w' - w, with the sum of three terms:
                 1. |w| + |update before the clamp|.  The new parameter is rounded at its own size, so half an ulp of w is in
                    every update; this term makes that explicit.
                 2. step_size (|m| + |g|) / denom: what exp_avg carries of its own magnitude sum into the update.
                 3. |update| / 2 * (v + |g|^2) / v' * root / denom, root = sqrt(v') / sqrt(bc2): the same for exp_avg_sq.
                 Where g and m cancel in m', the update is small and known no better than m' is.  An eighth of the test parameters
                 are 0 and an eighth tiny; there term 1 alone is no yardstick: the emulation's worst error is C_REF_UPDATE_TERM1_ALL
                 (512) eps32 of it.  Over parameters of ordinary size (|w| >= ORDINARY_W and an update no larger than w) term 1
                 alone does serve: C_REF_UPDATE_TERM1_ORDINARY (1.21, reached under DualAdam's lr = 0.2, where the update is of
                 the parameter's size; 0.50 under lr <= 3e-4, where terms 2 and 3 add under 1 %).
    target:      |target| + |w'|
    gradient written back: |grad|
``C_REF_*``: the worst error of ``emulate_f32`` -- the kernel's formulas line by line in numpy float32, never the reference --
against the "kernel" reference over ``step_cases()``, the very inputs of the GPU tests.
"""
import math

import numpy as np
import torch

EPS32 = float(np.finfo(np.float32).eps)              # 2^-23
FLT_MAX = float(np.finfo(np.float32).max)
TINY = 1e-30                                         # float32 underflow of products far below every value compared here
MARGIN = 4.0                                         # GPU tolerance = MARGIN * C_REF_* * EPS32 * magnitude sum: device sqrtf and
#                                                      division of a few ulp, fused against unfused association
BLOCK, MAX_GRID = 256, 2048                          # RPO_BLOCK, RPO_MAX_GRID (rpo_amd/csrc/common.h)
GRADMAX_LEN, GRADMAX_SLOTS, SLOT_STRIDE = 512, 16, 32
STATE_LEN = 544                                      # RPO_ADAM_STATE_LEN
# words of the state buffer a launch may touch: step, cached step, arrival word (2), two cached doubles (4), 16 sub-counters (2 each)
STATE_WORDS = tuple(range(8)) + tuple(w for k in range(16) for w in (32 + 32 * k, 33 + 32 * k))

# The yardstick: max over step_cases() / polyak_cases() of |emulate_f32 - float64 "kernel" reference| / (EPS32 * magnitude sum).
# Measured by tests/test_optim_f64.py::test_yardstick, which recomputes them and fails when a recorded value is below the
# measurement (or more than twice above it).
C_REF_M = 0.52           # measured 0.515: exp_avg
C_REF_V = 0.99           # measured 0.988: exp_avg_sq
C_REF_UPDATE = 0.84      # measured 0.831: w' - w
C_REF_TARGET = 0.98      # measured 0.977: Polyak target (inside the step and rpo_polyak alone)
C_REF_GRAD = 0.56        # measured 0.555: the clipped gradient written back
# For the record, not used by any tolerance: the update's error in units of eps32 * (|w| + |update|) alone (term 1 of the module
# docstring), over every finite element and over the parameters of ordinary size; test_yardstick recomputes both.
ORDINARY_W = 1e-2
C_REF_UPDATE_TERM1_ALL = 520.0         # measured 512: parameters that are 0 or tiny, where m' cancels
C_REF_UPDATE_TERM1_ORDINARY = 1.25     # measured 1.209


def f32(v):
    """The float32 value nearest to v, as a Python float (what a ``float`` argument of the C ABI receives)."""
    return float(np.float32(v))


class HP(object):
    """Hyper-parameters and flags of one launch; ``tau`` None = no Polyak target.  ``grad_scale``: size of the test's gradients."""

    def __init__(self, name, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, maximize=False, clamp_min0=False, clip_thres=0.0,
                 zero_grad=False, tau=None, grad_scale=1.0):
        self.name, self.lr, self.beta1, self.beta2, self.eps, self.weight_decay = name, lr, betas[0], betas[1], eps, weight_decay
        self.maximize, self.clamp_min0, self.clip_thres, self.zero_grad, self.tau = maximize, clamp_min0, clip_thres, zero_grad, tau
        self.grad_scale = grad_scale

    def __repr__(self):
        return self.name

    def kwargs(self):
        """Keyword arguments of ops.adam_step / entries of ops.adam_step_multi."""
        return dict(lr=self.lr, beta1=self.beta1, beta2=self.beta2, eps=self.eps, weight_decay=self.weight_decay,
                    maximize=self.maximize, clamp_min0=self.clamp_min0, clip_thres=self.clip_thres, zero_grad=self.zero_grad,
                    tau=0.0 if self.tau is None else self.tau)


HP_SETS = dict((h.name, h) for h in (
    HP("critic", 3e-4, clip_thres=0.2, tau=0.005),                                     # the trainers' three sets
    HP("actor", 1e-4, clip_thres=0.2, tau=0.005, zero_grad=True),
    HP("dual", 0.2, maximize=True, clamp_min0=True, zero_grad=True, grad_scale=0.05),
    HP("dual_target", 0.2, maximize=True, clamp_min0=True, tau=0.005, grad_scale=0.05),
    HP("weight_decay", 3e-4, weight_decay=1e-2, clip_thres=0.2, tau=0.005),
    HP("eps", 3e-4, eps=1e-3, clip_thres=0.2, tau=0.005, grad_scale=1e-3),             # sqrt(v) of the size of eps
    HP("betas", 3e-4, betas=(0.5, 0.9), clip_thres=0.2, tau=0.005),
    HP("tau0", 3e-4, clip_thres=0.2, tau=0.0),
    HP("tau1", 3e-4, clip_thres=0.2, tau=1.0),
    HP("maximize_clip", 3e-4, maximize=True, clip_thres=0.2, tau=0.005),
    HP("plain", 3e-4),                                                                 # no clip, no target
    HP("edges", 3e-4, tau=0.005),                                                      # the element edges: no clip (1e30 is in there)
    HP("edges_dual", 0.2, maximize=True, clamp_min0=True, tau=0.005),
))


# ====================================================================================================== float64 reference
def absmax(x, prev=0.0):
    """max(prev, max |x_i|) over the elements that are not NaN (fmaxf drops a NaN operand), float64."""
    a = np.abs(np.asarray(x, dtype=np.float64))
    a = a[~np.isnan(a)]
    return max(float(prev), float(a.max()) if a.size else 0.0)


def clip_coef(norm, thres):
    return min(1.0, thres / (norm + 1e-6))


def _scalars(hp, step, convention, dtype):
    if convention == "kernel":
        b1, b2 = np.float32(hp.beta1), np.float32(hp.beta2)
        tau = np.float32(0.0 if hp.tau is None else hp.tau)
        s = dict(mul2=float(b2), omb1=float(np.float32(1) - b1), omb2=float(np.float32(1) - b2), eps=f32(hp.eps),
                 wd=f32(hp.weight_decay), tau=float(tau), omt=float(np.float32(1) - tau), thres=f32(hp.clip_thres))
        bc1 = 1.0 - math.pow(float(b1), step)
        bc2s = math.sqrt(1.0 - math.pow(float(b2), step))
        s["step_size"], s["bc2s"] = f32(f32(hp.lr) / bc1), f32(bc2s)
        return s
    assert convention == "torch", convention
    r = (lambda x: float(np.float32(x))) if dtype == np.float32 else float
    tau = 0.0 if hp.tau is None else hp.tau
    bc1 = 1.0 - hp.beta1 ** step
    bc2s = math.sqrt(1.0 - hp.beta2 ** step)
    return dict(mul2=r(hp.beta2), omb1=r(1 - hp.beta1), omb2=r(1 - hp.beta2), eps=r(hp.eps), wd=r(hp.weight_decay), tau=r(tau),
                omt=r(1.0 - tau), thres=r(hp.clip_thres), step_size=r(hp.lr / bc1), bc2s=r(bc2s))


def adam(state, grad, hp, scalars="kernel", norm=None, n2=0):
    """One step.  state: dict(param, m, v, step[, target][, target2]) -- ``step`` the count BEFORE this step, the arrays float32
    (or float64: then nothing is rounded to float32 and nothing overflows).  ``norm``: the inf-norm the clip uses (default: of
    ``grad``).  Returns float64 dict(param, m, v, update, update_raw, update_mag, grad, g_mag, coef, step[, target][, target2])."""
    dtype = np.asarray(state["param"]).dtype.type
    w0, m0, v0, g0 = (np.asarray(a, dtype=np.float64) for a in (state["param"], state["m"], state["v"], grad))
    step = int(state["step"]) + 1
    s = _scalars(hp, step, scalars, dtype)
    with np.errstate(all="ignore"):
        coef = 1.0
        if hp.clip_thres > 0.0:
            coef = clip_coef(absmax(g0) if norm is None else float(norm), s["thres"])
        g = g0 * coef
        gout = np.zeros_like(g) if hp.zero_grad else g.copy() if hp.clip_thres > 0.0 else g0.copy()
        g_mag = np.abs(g)
        if hp.maximize:
            g = -g
        if s["wd"] != 0.0:
            g = g + s["wd"] * w0
            g_mag = g_mag + abs(s["wd"]) * np.abs(w0)
        m = m0 + (g - m0) * s["omb1"]
        v = v0 * s["mul2"] + s["omb2"] * g * g
        if dtype == np.float32:
            v = np.where(v > FLT_MAX, np.inf, v)
        root = np.sqrt(v) / s["bc2s"]
        raw = -s["step_size"] * (m / (root + s["eps"]))
        # first-order bound of the update's error: its own roundings and the new parameter's, and what exp_avg / exp_avg_sq carry
        # of theirs into it (d/dm = step_size / denom; d/dv = update / (2 v) * root / denom)
        carried = s["step_size"] * (np.abs(m0) + g_mag) / (root + s["eps"]) \
            + np.where(v > 0, 0.5 * np.abs(raw) * (root / (root + s["eps"])) * (v0 + g_mag ** 2) / v, 0.0)
        update_mag = np.abs(w0) + np.abs(raw) + np.where(np.isfinite(carried), carried, 0.0)
        w = w0 + raw
        if hp.clamp_min0:
            w = np.fmax(w, 0.0) if scalars == "kernel" else np.maximum(w, 0.0)
        out = dict(param=w, m=m, v=v, update=w - w0, update_raw=raw, update_mag=update_mag, grad=gout, g_mag=g_mag, coef=coef, step=step)
        if state.get("target") is not None:
            out["target"] = np.asarray(state["target"], dtype=np.float64) * s["omt"] + w * s["tau"]
        if state.get("target2") is not None:
            t2 = np.asarray(state["target2"], dtype=np.float64).copy()
            t2[:n2] = t2[:n2] * s["omt"] + w[:n2] * s["tau"]
            out["target2"] = t2
    return out


def polyak(param, target, tau, scalars="kernel"):
    """target' = (1 - tau) target + tau param, float64; tau and 1 - tau as the kernel's float32 scalars."""
    p, t = np.asarray(param, dtype=np.float64), np.asarray(target, dtype=np.float64)
    if scalars == "kernel":
        tau32 = np.float32(tau)
        return t * float(np.float32(1) - tau32) + p * float(tau32)
    return t * f32(1.0 - tau) + p * f32(tau)


def min_q_bwd(q1, q2, scale):
    """Gradient of sum(min(q1, q2) * scale) -- with scale = -1 / n the actor loss -mean(min(q1, q2)) of rpo_sac.py:335 -- by
    autograd in float64; ``scale`` as the kernel's float32 argument.  Returns float64 numpy (dq1, dq2)."""
    a = torch.as_tensor(np.asarray(q1)).double().requires_grad_()
    b = torch.as_tensor(np.asarray(q2)).double().requires_grad_()
    (torch.minimum(a, b) * f32(scale)).sum().backward()
    return a.grad.numpy(), b.grad.numpy()


# ====================================================================================================== float32 emulation
MUTATIONS = ("bc_step_minus_1", "eps_dropped", "eps_in_sqrt", "wd_sign", "clamp_after_target", "clip_no_1e6", "n2_inclusive",
             "absmax_tail_skipped", "maximize_before_writeback")


def emulate_absmax(x, prev=0.0, mut=None):
    """absmax_kernel: float4 sweep over the first n / 4 * 4 elements, then the n % 4 tail; fmaxf drops NaN; accumulates on prev."""
    x = np.asarray(x, dtype=np.float32)
    n4 = x.size // 4 * 4
    m = np.float32(0.0)
    if n4:
        m = np.fmax(m, np.fmax.reduce(np.abs(x[:n4])))
    if mut != "absmax_tail_skipped" and x.size > n4:
        m = np.fmax(m, np.fmax.reduce(np.abs(x[n4:])))
    return np.fmax(np.float32(prev), np.float32(m))


def emulate_f32(state, grad, hp, n2=0, norm=None, mut=None, one_minus_beta="kernel"):
    """adam_body line by line in numpy float32 (bias corrections in double, as there).  ``mut``: one of MUTATIONS, a deliberately
    wrong kernel for test_optim_f64.py.  ``one_minus_beta="torch"``: float32(1 - beta) from the double betas instead of the
    kernel's float32(1) - float32(beta) (the size of that deviation).  Returns float32 dict(param, m, v, grad[, target][, target2])."""
    F = np.float32
    w0, m0, v0, g0 = (np.asarray(a, dtype=F) for a in (state["param"], state["m"], state["v"], grad))
    step = int(state["step"]) + 1
    lr, b1, b2, eps, wd, thres = (F(x) for x in (hp.lr, hp.beta1, hp.beta2, hp.eps, hp.weight_decay, hp.clip_thres))
    tau = F(0.0 if hp.tau is None else hp.tau)
    bstep = step - 1 if mut == "bc_step_minus_1" else step
    with np.errstate(all="ignore"):
        bc1 = np.float64(1.0) - math.pow(float(b1), bstep)
        bc2s = math.sqrt(1.0 - math.pow(float(b2), bstep))
        step_size, bc2_sqrt = F(np.float64(lr) / bc1), F(bc2s)
        coef = F(1.0)
        if thres > 0:
            gm = emulate_absmax(g0, mut=mut) if norm is None else F(norm)
            coef = np.fmin(thres / (gm if mut == "clip_no_1e6" else gm + F(1e-6)), F(1.0))
        omb1, omb2 = F(1.0) - b1, F(1.0) - b2
        if one_minus_beta == "torch":
            omb1, omb2 = F(1.0 - hp.beta1), F(1.0 - hp.beta2)
        g = g0 * coef
        gout = np.zeros_like(g) if hp.zero_grad else g.copy() if thres > 0 else g0.copy()
        if hp.maximize:
            g = -g
            if mut == "maximize_before_writeback" and not hp.zero_grad and thres > 0:
                gout = g.copy()
        w = w0
        if wd != 0:
            g = g - wd * w if mut == "wd_sign" else g + wd * w
        m = m0 + (g - m0) * omb1
        v = v0 * b2 + omb2 * g * g
        if mut == "eps_in_sqrt":
            denom = np.sqrt(v + eps) / bc2_sqrt
        elif mut == "eps_dropped":
            denom = np.sqrt(v) / bc2_sqrt
        else:
            denom = np.sqrt(v) / bc2_sqrt + eps
        w = w - step_size * (m / denom)
        wc = np.fmax(w, F(0.0)) if hp.clamp_min0 else w
        src = w if mut == "clamp_after_target" else wc
        out = dict(param=wc.astype(F), m=m.astype(F), v=v.astype(F), grad=gout.astype(F))
        if state.get("target") is not None:
            out["target"] = (np.asarray(state["target"], dtype=F) * (F(1.0) - tau) + src * tau).astype(F)
        if state.get("target2") is not None:
            t2 = np.asarray(state["target2"], dtype=F).copy()
            k = min(n2 + 1, t2.size) if mut == "n2_inclusive" else n2
            t2[:k] = t2[:k] * (F(1.0) - tau) + src[:k] * tau
            out["target2"] = t2
    return out


def emulate_polyak(param, target, tau):
    F = np.float32
    return (np.asarray(target, dtype=F) * (F(1.0) - F(tau)) + np.asarray(param, dtype=F) * F(tau)).astype(F)


# ====================================================================================================== comparison
def worst(got, ref, mag):
    """max |got - ref| / (EPS32 * mag + TINY); equal values (inf included) and NaN against NaN count 0, any other non-finite
    difference inf; 0 for no elements."""
    got, ref, mag = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (got, ref, mag))
    if got.size == 0:
        return 0.0
    with np.errstate(all="ignore"):
        same = (got == ref) | (np.isnan(got) & np.isnan(ref))
        ratio = np.abs(got - ref) / (EPS32 * mag + TINY)
        ratio = np.where(same, 0.0, np.where(np.isnan(ratio), np.inf, ratio))
    return float(ratio.max())


def bitwise(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))


def step_errors(got, state, grad, hp, n2=0, norm=None, scalars="kernel"):
    """The errors of a float32 result ``got`` = dict(param, m, v, grad[, target][, target2]) of one step from ``state`` against
    the float64 reference, each in units of EPS32 * its magnitude sum (module docstring); conditions that are exact (the gradient
    written back under a coefficient of 1, without clip or zeroed; target2 behind n2) give 0.0 or inf."""
    ref = adam(state, grad, hp, scalars=scalars, norm=norm, n2=n2)
    w0, m0, v0 = (np.asarray(state[k], dtype=np.float64) for k in ("param", "m", "v"))
    e = {}
    with np.errstate(all="ignore"):
        e["exp_avg"] = worst(got["m"], ref["m"], np.abs(m0) + ref["g_mag"])
        e["exp_avg_sq"] = worst(got["v"], ref["v"], v0 + ref["g_mag"] ** 2)
        e["update"] = worst(np.asarray(got["param"], dtype=np.float64) - w0, ref["update"], ref["update_mag"])
        if "target" in ref:
            e["target"] = worst(got["target"], ref["target"], np.abs(np.asarray(state["target"], dtype=np.float64)) + np.abs(ref["param"]))
        if "target2" in ref:
            t2 = np.asarray(state["target2"], dtype=np.float64)
            e["target"] = max(e.get("target", 0.0), worst(got["target2"][:n2], ref["target2"][:n2], np.abs(t2[:n2]) + np.abs(ref["param"][:n2])))
            e["target2_tail"] = 0.0 if bitwise(got["target2"][n2:], state["target2"][n2:]) else np.inf
        if hp.zero_grad:
            e["grad_exact"] = 0.0 if bitwise(got["grad"], np.zeros_like(got["grad"])) else np.inf
        elif hp.clip_thres > 0.0 and ref["coef"] < 1.0:
            e["grad"] = worst(got["grad"], ref["grad"], np.abs(np.asarray(grad, dtype=np.float64)))
        else:
            e["grad_exact"] = 0.0 if bitwise(got["grad"], grad) else np.inf
    return e


def update_errors_term1(got, state, grad, hp, n2=0, norm=None):
    """The update's error in units of EPS32 * (|w| + |update before the clamp|) alone: (worst over the finite elements, worst over
    those with |w| >= ORDINARY_W and an update no larger than w).  Recorded as C_REF_UPDATE_TERM1_*; no tolerance uses it."""
    ref = adam(state, grad, hp, norm=norm, n2=n2)
    w0 = np.asarray(state["param"], dtype=np.float64)
    with np.errstate(all="ignore"):
        d = np.asarray(got["param"], dtype=np.float64) - w0
        ok = np.isfinite(d) & np.isfinite(ref["update"]) & np.isfinite(ref["update_raw"])
        mag = np.abs(w0) + np.abs(ref["update_raw"])
        big = ok & (np.abs(w0) >= ORDINARY_W) & (np.abs(ref["update_raw"]) <= np.abs(w0))
    return worst(d[ok], ref["update"][ok], mag[ok]), worst(d[big], ref["update"][big], mag[big])


C_OF = dict(exp_avg="C_REF_M", exp_avg_sq="C_REF_V", update="C_REF_UPDATE", target="C_REF_TARGET", grad="C_REF_GRAD")


def step_ratios(got, state, grad, hp, n2=0, norm=None, scalars="kernel"):
    """step_errors over the tolerance MARGIN * C_REF_*: what the GPU tests assert to be <= 1 (the exact conditions: 0 or inf)."""
    e = step_errors(got, state, grad, hp, n2=n2, norm=norm, scalars=scalars)
    return dict((k, v / (MARGIN * globals()[C_OF[k]]) if k in C_OF else v) for k, v in e.items())


# ====================================================================================================== inputs
SIZES = (1, 3, 255, 256, 257, 4096, 4097, 8449, 2048 * 256 + 517)
STEPS0 = (0, 1, 999, 100000)
ABSMAX_SIZES = (1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 4 * 2048 * 256 + 3, 4 * 2048 * 256 + 7)
# (4 * 2048 * 256 + 3: 2048 workgroups of 256 float4 loads sweep the whole of it in ONE pass and the tail of 3 follows; only from
# + 4 on is there a float4 of the second grid-stride pass: + 7 has one, elements 2097152..2097155, and a tail of 3 behind it)
POLYAK_TAUS = (0.0, 0.25, 1.0)
MIN_Q_SIZES = (1, 257, 2048 * 256 + 5)


def workgroups(n):
    return max(1, min(MAX_GRID, (n + BLOCK - 1) // BLOCK))


def make_state(n, s0, hp, seed=0, with_target2=False):
    """Float32 state of a run in progress and a gradient: parameters N(0, 0.1) -- an eighth exactly 0 and an eighth of the size
    of 1e-6, where w' - w shows the update to its own precision -- m and v >= 0 of the gradient's size."""
    rng = np.random.RandomState(1000 * seed + n % 9973 + 7 * (s0 % 1000))
    gs = hp.grad_scale
    w = 0.1 * rng.randn(n)
    kind = rng.randint(0, 8, n)
    w[kind == 0] = 0.0
    w[kind == 1] *= 1e-5
    if hp.clamp_min0:
        w = np.abs(w)
    st = dict(param=w.astype(np.float32), m=(0.3 * gs * rng.randn(n)).astype(np.float32),
              v=(gs * gs * (0.25 + rng.rand(n))).astype(np.float32), step=s0)
    if hp.tau is not None:
        st["target"] = (0.1 * rng.randn(n)).astype(np.float32)
    if with_target2:
        st["target2"] = (0.1 * rng.randn(n)).astype(np.float32)
    grad = (gs * rng.randn(n) * np.where(rng.rand(n) < 0.5, 1.0, 0.05)).astype(np.float32)
    return st, grad


def with_norm(grad, norm, at=None, negative=False):
    """``grad`` rescaled so that every element is strictly below ``norm`` in size but one, which is float32(norm) exactly."""
    g = np.asarray(grad, dtype=np.float64)
    top = np.float32(norm)
    g = (g * (0.999 * float(top) / max(np.abs(g).max(), 1e-30))).astype(np.float32)
    at = int(np.abs(g).argmax()) if at is None else at
    g[at] = -top if negative else top
    assert np.abs(np.delete(g, at)).max(initial=0.0) < top
    return g


EDGE_N = 257
EDGE_ROWS = dict(zero=0, denormal_v=1, g_1e20=2, g_m1e20=3, g_1e30=4, g_1e_25=5, g_m1e_25=6, stays_zero=64, goes_negative=255, nan=256)


def edge_state(hp):
    """The element edges in one vector of EDGE_N (rows EDGE_ROWS, the rest as make_state)."""
    st, grad = make_state(EDGE_N, 999, hp, seed=3)
    r = EDGE_ROWS

    def put(i, w=None, m=None, v=None, g=None):
        for arr, val in ((st["param"], w), (st["m"], m), (st["v"], v), (grad, g)):
            if val is not None:
                arr[i] = val
    put(r["zero"], m=0.0, v=0.0, g=0.0)                       # 0 / (0 + eps): the update is exactly 0
    put(r["denormal_v"], v=1e-40, g=1e-3, m=1e-4)
    put(r["g_1e20"], g=1e20)                                  # (1 - beta2) g g = 1e37, evaluated left to right: still finite
    put(r["g_m1e20"], g=-1e20)
    put(r["g_1e30"], g=1e30)                                  # (1 - beta2) g g overflows: v = inf, the update is 0
    put(r["g_1e_25"], g=1e-25, m=0.0, v=0.0)                  # g g underflows to 0
    put(r["g_m1e_25"], g=-1e-25, m=0.0, v=0.0)
    put(r["stays_zero"], w=0.0, m=0.0, v=0.0, g=0.0)          # lands exactly on 0
    sign = -1.0 if hp.maximize else 1.0
    put(r["goes_negative"], w=1e-3, m=1.0, v=1.0, g=sign * 1.0)   # one step of lr below 0 without the clamp
    put(r["nan"], g=np.nan)
    assert np.float32(1e-40) != 0 and abs(np.float32(1e-40)) < np.finfo(np.float32).tiny
    return st, grad


class Case(object):
    """One single-step comparison of the GPU tests: state, gradient, hyper-parameters, n2, and which slot holds the norm."""

    def __init__(self, name, state, grad, hp, n2=0, slot=0):
        self.name, self.state, self.grad, self.hp, self.n2, self.slot = name, state, grad, hp, n2, slot
        self.n, self.s0 = grad.size, state["step"]

    def __repr__(self):
        return self.name

    def norm(self):
        return absmax(self.grad) if self.hp.clip_thres > 0.0 else None


def _cases():
    out = []
    crit = HP_SETS["critic"]
    for n in SIZES:                                                          # sizes x steps: state, cache, arrival
        for s0 in STEPS0:
            st, g = make_state(n, s0, crit)
            out.append(Case("size[%d, s0=%d]" % (n, s0), st, g, crit))
    for name in ("actor", "dual", "dual_target", "weight_decay", "eps", "betas", "tau0", "tau1", "maximize_clip", "plain"):
        hp = HP_SETS[name]                                                   # hyper-parameters, one- and two-level arrival
        for n in (6, 257, 8449) if name == "dual" else (257, 8449):              # (6: the multipliers of CartSafe)
            st, g = make_state(n, 999, hp, seed=1)
            out.append(Case("hp[%s, %d]" % (name, n), st, g, hp))
    thres = f32(crit.clip_thres)                                             # clipping
    for tag, norm in (("below", 0.75 * thres), ("at", thres), ("just_above", 1.25 * thres), ("above", None)):
        for k, slot in enumerate((0, 15, 7)):
            st, g = make_state(4097, 999, crit, seed=2 + k)
            if norm is not None:
                g = with_norm(g, norm, negative=bool(k % 2))
            out.append(Case("clip[%s, slot %d]" % (tag, slot), st, g, crit, slot=slot))
    for name in ("edges", "edges_dual"):                                     # element edges
        st, g = edge_state(HP_SETS[name])
        out.append(Case("edges[%s]" % name, st, g, HP_SETS[name]))
    st, g = make_state(257, 999, crit, seed=5)                               # NaN gradient elements under the clip: one in the
    g[100] = g[256] = np.nan                                                 # float4 body of the inf-norm's sweep, one in its tail
    out.append(Case("nan_under_clip", st, g, crit))
    actor = HP("actor_t2", 1e-4, clip_thres=0.2, tau=0.005)                  # target2 over a prefix (rpo_adam_step_multi)
    for n2 in (0, 1, 768, 8449):
        st, g = make_state(8449, 999, actor, seed=6, with_target2=True)
        out.append(Case("target2[n2=%d]" % n2, st, g, actor, n2=n2))
    return out


_CASES = []


def step_cases():
    """Every single-step input of test_optim_f64_gpu.py (built once, read-only): also what C_REF_* is measured over."""
    if not _CASES:
        _CASES.extend(_cases())
        for c in _CASES:
            for a in list(c.state.values()) + [c.grad]:
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
    return _CASES


def case(name):
    for c in step_cases():
        if c.name == name:
            return c
    raise KeyError(name)


_STEADY = {}


def torch_steady_state(n=8449, steps=3000, s0=100000, seed=9):
    """State and gradient of torch.optim.Adam itself (float32, CPU, default betas, lr 3e-4) after ``steps`` steps on gradients
    around a fixed mean: exp_avg / exp_avg_sq carry what torch's own float32(1 - beta) leaves there.  The step count is then set
    to ``s0`` (both bias corrections 1 to double precision at 100000).  Returns (state, grad, torch's own next parameters)."""
    key = (n, steps, s0, seed)
    if key not in _STEADY:
        rng = np.random.RandomState(seed)
        mean = rng.randn(n).astype(np.float32)
        p = torch.nn.Parameter(torch.from_numpy((0.1 * rng.randn(n)).astype(np.float32)))
        opt = torch.optim.Adam([p], lr=3e-4)
        for _ in range(steps):
            p.grad = torch.from_numpy(mean * (1 + 0.1 * rng.randn(n)).astype(np.float32))
            opt.step()
        grad = mean * (1 + 0.1 * rng.randn(n)).astype(np.float32)
        sd = opt.state[p]
        st = dict(param=p.detach().numpy().copy(), m=sd["exp_avg"].numpy().copy(), v=sd["exp_avg_sq"].numpy().copy(), step=s0)
        sd["step"] = torch.tensor(float(s0)) if torch.is_tensor(sd["step"]) else s0
        p.grad = torch.from_numpy(grad.copy())
        opt.step()
        own = dict(param=p.detach().numpy().copy(), m=sd["exp_avg"].numpy().copy(), v=sd["exp_avg_sq"].numpy().copy(), grad=grad)
        _STEADY[key] = (st, grad, own)
    return _STEADY[key]


def absmax_input(n, where, negative, seed=0):
    """n float32 in (-0.5, 0.5) and one element of size 3 at ``where``: first, last, tail (the first element of the n % 4 tail),
    pass2 (the first element of the second grid-stride pass of the float4 sweep); None where n has no such place."""
    at = dict(first=0, last=n - 1, tail=n // 4 * 4 if n % 4 else None,
              pass2=4 * MAX_GRID * BLOCK if n // 4 > MAX_GRID * BLOCK else None)[where]
    if at is None:
        return None, None
    x = (np.random.RandomState(seed + n % 1000).rand(n) - 0.5).astype(np.float32)
    x[at] = -3.0 if negative else 3.0
    return x, at


def absmax_nan_input(n, where, seed=0):
    """n float32 in (-0.5, 0.5) with NaN at ``where`` and -3 in the last element that is not NaN.  body: in the float4 sweep --
    every fifth element (each lane of a float4 in turn) and the whole second float4; tail: the first element of the n % 4 tail
    (the -3 sits beside it where the tail has more); all: every element.  None where n has no such place or nothing else is left."""
    n4 = n // 4 * 4
    nan = np.zeros(n, bool)
    if where == "body":
        nan[:n4][np.arange(n4) % 5 == 1] = True
        nan[4:min(8, n4)] = True
    elif where == "tail":
        nan[n4:n4 + 1] = True
    else:
        assert where == "all", where
        nan[:] = True
    if not nan.any() or (nan.all() and where != "all"):
        return None
    x = (np.random.RandomState(seed + n % 1000 + 17).rand(n) - 0.5).astype(np.float32)
    if not nan.all():
        x[np.flatnonzero(~nan)[-1]] = -3.0
    x[nan] = np.nan
    return x


def polyak_cases():
    for n in SIZES:
        rng = np.random.RandomState(n % 1000 + 11)
        yield n, (0.1 * rng.randn(n)).astype(np.float32), (0.1 * rng.randn(n)).astype(np.float32)


def min_q_input(n, seed=0):
    """q1, q2 float32 with exact ties (a quarter of the rows), +0.0 against -0.0, +-inf on either side and inf against inf."""
    rng = np.random.RandomState(seed + n % 1000)
    q1, q2 = rng.randn(n).astype(np.float32), rng.randn(n).astype(np.float32)
    tie = rng.rand(n) < 0.25
    q2[tie] = q1[tie]
    inf = np.float32(np.inf)
    special = [(0.0, -0.0), (-0.0, 0.0), (inf, 1.0), (1.0, inf), (-inf, 1.0), (1.0, -inf), (inf, inf), (-inf, -inf), (inf, -inf)]
    for k, (a, b) in enumerate(special[:n]):
        i = (n - 1 - k) if n > 300 else k                       # the large size: at the end, in the second grid-stride pass
        q1[i], q2[i] = a, b
    return q1, q2
