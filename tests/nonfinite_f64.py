"""Float64 statement of what a NON-FINITE input does to one vector step and to one evaluation, the case table that plants such
inputs, and the harness that runs a case through a trainer.  Not collected; used by test_nonfinite.py (CPU: the oracle backend)
and test_nonfinite_gpu.py (the HIP launches).

The contract (include/rpo_hip.h: RPO_CTRL_NONFINITE, rpo_cartsafe_step "non-finite", rpo_mlp_forward): a lane that is stepped
with a NaN action, or reaches a non-finite next state or reward, raises ctrl[RPO_CTRL_NONFINITE] = 1 + the vector step, once;
its row's outputs are non-finite where float64 gives that; every other lane keeps its bits.  Nothing here carries a tolerance:
the reference yields MASKS (which elements must be non-finite) and SETS (which lanes are bad), never values to compare with.

One vector step = actor forward (mlp_f64.Mlp64) -> head (heads_f64.tanh_box / gauss_head) -> explore clip -> Complete -> the GRG
loop -> env step (envs_f64.cart_step / pend_step and the projection formulas there), all in float64 from the float32 inputs.
IEEE semantics in everything that carries a NaN towards the failure word: relu is maximum(x, 0) and KEEPS a NaN
(torch.clamp_min), the box clips keep it (torch.clamp), comparisons against it are false (the GRG loop's masks and stop test),
the maximum over violations keeps it.  The env step's OWN clamps come in two statements, because the contract has two readers:

    clips="ieee"   np.clip / np.maximum everywhere: the oracle (oracle/cartsafe.py, oracle/pendulum.py) and the reference code
                   it restates.  A NaN action poisons the next state.
    clips="fmax"   the clamps behind the failure test as fminf / fmaxf, the form include/rpo_hip.h states for the step kernels
                   ("violations ... clamped at 0", the force and speed clips) and tests/test_envs_f64_gpu.py::test_nonfinite_rows
                   pins with envs_f64.B64: a NaN action is flagged and then stepped as the force -10 / -6, relu(NaN violation)
                   is 0 and the clipped NaN speed -8 -- the NEXT state of such a lane is finite.

Both give the same bad lanes and the same word (asserted in test_nonfinite.py); they differ only in which columns behind the
flag hold a NaN.  The CPU test holds "ieee" against the oracle backend, the GPU test holds "fmax" against the kernels.
"""
import numpy as np
import torch

import envs_f64 as ef
import heads_f64 as hf
import mlp_f64 as mf
from oracle import cartsafe as ocs
from oracle import pendulum as opd
from oracle import philox
from rpo_amd._lib import CONST

T_IDX, NF_IDX = CONST["RPO_CTRL_T"], CONST["RPO_CTRL_NONFINITE"]
N = 133                                                  # ragged against the 16- and the 64-lane tile
LANES = (0, 15, 16, 63, 64, N - 1)
QNAN, NEG_QNAN, PINF = 0x7FC00000, 0xFFC00000, 0x7F800000
PLANT_BITS = (QNAN, NEG_QNAN, PINF)                      # as PLANTS of test_mlp_small_f64_gpu.py, by bit pattern
T0 = 5                                                   # the vector step the cases run at: the word is T0 + 1


def f32_of(bits):
    return np.array([bits], dtype=np.uint32).view(np.float32)[0]


def nonfinite(x):
    return ~np.isfinite(np.asarray(x, dtype=np.float64))


def same_bits(a, b):
    """Bit equality of two float32 arrays."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def same_nan_aware(a, b):
    """NaN-aware bit equality: a NaN equals a NaN of any payload and sign, everything else bit for bit."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(np.where(na, 0, a.view(np.uint32)),
                                                                             np.where(nb, 0, b.view(np.uint32)))


# ===================================================================================================== arithmetics
class IEEE(ef.B64):
    """envs_f64.B64 with IEEE 754-2019 maximum / minimum: a NaN operand wins (np.maximum, np.clip, torch.clamp)."""
    name = "ieee"

    @classmethod
    def maximum(cls, a, b):
        a, b = ef.V.of(a), ef.V.of(b)
        return cls.where((a.v >= b.v) | np.isnan(a.v), a, b)

    @classmethod
    def minimum(cls, a, b):
        a, b = ef.V.of(a), ef.V.of(b)
        return cls.where((a.v <= b.v) | np.isnan(a.v), a, b)


ARITH = {"ieee": IEEE, "fmax": ef.B64}


def _v(x):
    return np.asarray(ef.V.of(x).v, dtype=np.float64)


def _nanmax(cols):
    """Maximum over a list of columns that keeps a NaN (torch.max / eval_dev.h nanmax)."""
    return np.max(np.stack([_v(c) for c in cols], axis=0), axis=0)


# ===================================================================================================== the policy
class Spec(object):
    """What one vector step of a trainer depends on, as host values: the actor's float32 parameters, the box, the projection's
    budget, the env's constants."""

    def __init__(self, tr):
        k = tr.kernels
        self.env = "cart" if k.name.startswith("Cart") else "pendulum"
        self.gauss = bool(tr._gauss_policy)
        d = tr.fused.descs["actor"]
        self.tensors = {f: (None if t is None else t.detach().cpu().clone()) for f, t in d.tensors.items()}
        self.S, self.E, self.H, self.n_out = d.S, d.E, d.H, d.n_out
        self.scale, self.base = (hf.f32(v) for v in tr._box_affine)
        self.lo, self.hi = hf.f32(tr._box_lo), hf.f32(tr._box_hi)
        self.K, self.lr = int(tr.max_steps), float(tr.corr_lr)
        self.eval_K, self.eval_lr = int(tr.eval_steps), float(tr.eval_lr)
        self.corr_eps, self.momentum = float(tr.corr_eps), float(tr.corr_momentum)
        self.eps_start, self.eps_end, self.eps_decay = float(tr.eps_start), float(tr.eps), float(tr.decay_value)
        self.partial = int(getattr(k, "partial", 0))
        self.table = ocs.Constants(self.partial).as_array() if self.env == "cart" else None
        self.max_episode_steps = int(tr.vec.max_episode_steps)
        self.viol_thresh = float(tr.vec.viol_thresh)
        self.seed, self.env_id_base = int(tr.seed), int(tr.vec.env_id_base)
        self.cols, self.row_floats = dict(k.cols), int(k.row_floats)

    def with_param(self, field, index, value):
        """A copy whose actor holds ``value`` in element ``index`` of ``field``."""
        import copy
        s = copy.copy(self)
        s.tensors = dict(self.tensors)
        t = self.tensors[field].clone()
        t.view(-1)[index] = float(value)
        s.tensors[field] = t
        return s

    def eps_t(self, t):
        return hf.eps_schedule(self.eps_start, self.eps_end, self.eps_decay, t)

    def rollout_noise(self, n, t, updates=0):
        """The N(0, 1) draw of the rollout at vector step t: RPODDPG's exploration noise (RPO_STREAM_ACT), RPOSAC's rsample
        (RPO_STREAM_POLICY, salt 0, sub-counter ctrl[RPO_CTRL_UPDATES])."""
        ids = np.arange(n) + self.env_id_base
        r = philox.draw(self.seed, ids, t, philox.STREAM_POLICY, updates) if self.gauss else philox.draw(self.seed, ids, t, philox.STREAM_ACT)
        return philox.normal(r[:, 0], r[:, 1]).astype(np.float32)


def policy(spec, obs, noise=None, eps_t=0.0, deterministic=False):
    """The basic action the policy proposes for float32 observations [n, S], float64 [n]: the actor (relu keeps a NaN), then
    RPODDPG's tanh box + clip(ap + eps_t noise) (noise None: no clip, the deterministic policy), or RPOSAC's squashed Gaussian
    (noise = the draw; deterministic: its mean).  Returns (ap, actor output [n, n_out])."""
    net = mf.Mlp64(spec.tensors, spec.S, 0, spec.E, spec.H, n_out=spec.n_out)
    out = net.forward(torch.as_tensor(np.ascontiguousarray(obs, np.float32)))[0]
    if spec.gauss:
        e = torch.zeros(out.shape[0], dtype=torch.float64) if deterministic else torch.as_tensor(noise, dtype=torch.float64)
        ap = hf.gauss_head(out[:, 0], out[:, 1], e, spec.scale, spec.base, spec.lo, spec.hi, deterministic=deterministic)["ap"]
    else:
        nz = None if deterministic or noise is None else torch.as_tensor(noise, dtype=torch.float64)
        ap = hf.tanh_box(out[:, 0], nz, hf.f32(eps_t), spec.scale, spec.base, spec.lo, spec.hi)["ap"]
    return ap.numpy(), out.numpy()


# ===================================================================================================== Complete + GRG
def project(A, spec, ap, obs, K, lr):
    """Complete + the per-lane GRG loop (cartpole.py:369-408 / pendulum.py:256-343 inside rpo_ddpg.py:266-286) from the float32
    rounding of the proposal; the first iteration unconditional, afterwards while |h| > corr_eps or max g > corr_eps -- false
    for a NaN, which therefore leaves the loop after one iteration AS a NaN (x - 0 * ... is NaN).  Returns (action float64
    [n, 2], h [n], g [n, ineq_num]: the signed residuals of the result)."""
    with np.errstate(all="ignore"):
        ap = A.inp(np.asarray(ap, np.float64).astype(np.float32))
        n = ap.v.shape[0]
        if spec.env == "cart":
            c = ef.CartTab(A, spec.table, spec.partial)
            ao = ef.cart_complete(A, c, ap)
        else:
            e = ef.pend_eq_of_obs(A, obs)
            ao = ef.pend_complete(A, e, ap)

        def resid(ap, ao):
            if spec.env == "cart":
                a0, a1 = (ap, ao) if spec.partial == 0 else (ao, ap)
                h, g = ef.cart_eq_ineq(A, c, a0, a1)
                return h, g
            h, g = ef.pend_resid(A, e, ap, ao)
            return h, [g]
        old = (ef.V(np.zeros(n)), ef.V(np.zeros(n)))
        live = np.ones(n, bool)
        eps = float(np.float32(spec.corr_eps))
        for k in range(int(K)):
            h, g = resid(ap, ao)
            if k > 0:
                live = live & ((np.abs(h.v) > eps) | (_nanmax(g) > eps))
                if not live.any():
                    break
            if spec.env == "cart":
                nap, nao, stp, _ = ef.cart_grg_step(A, c, spec.partial, ap, ao, lr, spec.momentum, old)
            else:
                nap, nao, stp, _ = ef.pend_grg_step(A, e, ap, ao, lr, spec.momentum, old)
            ap, ao = A.where(live, nap, ap), A.where(live, nao, ao)
            old = (A.where(live, stp[0], old[0]), A.where(live, stp[1], old[1]))
        h, g = resid(ap, ao)
        if spec.env == "cart":
            action = ef.cart_join(spec.partial, ap.v, ao.v)
        else:
            action = np.stack([ap.v, ao.v], axis=-1)
        return action, _v(h), np.stack([_v(x) for x in g], axis=1)


# ===================================================================================================== env step
def env_step(A, spec, internal, action32, ep_len=None, auto_reset=True):
    """One env step of float32 (internal [n, D], action [n, 2]) in the arithmetic ``A``.  Returns dict: row [n, row_floats]
    float64 (the transition as the ring holds it; done as 0 / 1), bad [n] (NaN action, or a non-finite next state / reward
    BEFORE the speed clip and the reset), next_internal / next_obs float64 (what the lane continues from; NaN-free for a lane
    that was reset: the content of a fresh state is not stated here, only that it is finite), reward, ineq, eq (the step's max
    violation / max |residual|, NaN-keeping), done [n], g [n, ineq_num], h [n]."""
    with np.errstate(all="ignore"):
        internal, action32 = np.asarray(internal, np.float32), np.asarray(action32, np.float32)
        n = internal.shape[0]
        c = spec.cols
        row = np.zeros((n, spec.row_floats))
        if spec.env == "cart":
            o = ef.cart_step(A, internal, action32, spec.table, spec.partial)
            ns = np.stack([_v(x) for x in o["ns"]], axis=1)
            pre_obs, nxt_obs_row, reward = internal.astype(np.float64), ns, np.ones(n)
            g, h = np.stack([_v(x) for x in o["g"]], axis=1), _v(o["h"])
            term = (ns[:, 0] < -ocs.X_THRESHOLD) | (ns[:, 0] > ocs.X_THRESHOLD) | (ns[:, 3] < -ocs.THETA_THRESHOLD) | (ns[:, 3] > ocs.THETA_THRESHOLD)
            state_bad = nonfinite(ns).any(axis=1)
            nxt_int, nxt_obs = ns, ns
        else:
            o = ef.pend_step(A, internal, action32)
            nth = _v(o["nth"])
            nx = [_v(x) for x in o["next"]]                    # cos, sin, theta_dot (clipped), l, l_dot
            pre_obs = np.stack([_v(o["obs"][0]), _v(o["obs"][1])] + [internal[:, i].astype(np.float64) for i in (1, 2, 3)], axis=1)
            nxt_obs_row = np.stack(nx, axis=1)
            reward = _v(o["reward"])
            g, h = _v(o["g"])[:, None], _v(o["h"])
            term = (nx[3] <= 0.5) | (nx[3] >= 1.5) | (nth >= np.pi / 12) | (nth <= -np.pi / 12)
            # the un-clipped next theta_dot is non-finite exactly when the next theta = theta + dt * it is (theta being finite)
            state_bad = nonfinite(nth) | nonfinite(nxt_obs_row).any(axis=1)
            nxt_int, nxt_obs = np.stack([nth, nx[2], nx[3], nx[4]], axis=1), nxt_obs_row
        length = (np.zeros(n, np.int64) if ep_len is None else np.asarray(ep_len, np.int64)) + 1
        done = term | (length >= spec.max_episode_steps)
        row[:, c["state"][0]:c["state"][1]] = pre_obs
        row[:, c["action"][0]:c["action"][1]] = action32
        row[:, c["next_state"][0]:c["next_state"][1]] = nxt_obs_row
        row[:, c["reward"][0]] = reward
        row[:, c["done"][0]] = done
        row[:, c["eq_viol"][0]] = h
        row[:, c["ineq_viol"][0]:c["ineq_viol"][1]] = g
        bad = np.isnan(action32).any(axis=1) | state_bad | nonfinite(reward)
        if auto_reset:                                           # a fresh state is finite
            nxt_int = np.where(done[:, None], 0.0, nxt_int)
            nxt_obs = np.where(done[:, None], 0.0, nxt_obs)
        return dict(row=row, bad=bad, next_internal=nxt_int, next_obs=nxt_obs, reward=reward, ineq=np.max(g, axis=1), eq=np.abs(h),
                    done=done, g=g, h=h)


def vector_step(spec, internal, obs, ep_len, t, clips, has_ctrl=True):
    """One vector step at step counter t: the actor and the projection read ``obs`` [n, S], the step reads ``internal`` (the
    same array on CartSafe).  Returns dict:
        bad [n]             the lanes that must raise the word
        word                t + 1 if any lane is bad and the launch has a ctrl, else 0
        masks               {"row": [n, row_floats], "internal": [n, D], "obs": [n, S], "action": [n, 2]} -- the elements that
                            must be non-finite after the launch (everything else of a bad lane must be finite)"""
    A = ARITH[clips]
    n = internal.shape[0]
    ap, _ = policy(spec, obs, spec.rollout_noise(n, t), spec.eps_t(t))
    action, _, _ = project(A, spec, ap, obs, spec.K, spec.lr)
    a32 = action.astype(np.float32)
    st = env_step(A, spec, internal, a32, ep_len)
    masks = dict(row=nonfinite(st["row"]), internal=nonfinite(st["next_internal"]), obs=nonfinite(st["next_obs"]), action=nonfinite(a32))
    return dict(bad=st["bad"], word=(t + 1 if st["bad"].any() and has_ctrl else 0), masks=masks)


def act(spec, obs, clips="ieee"):
    """policy_act / trainer.act(): the deterministic policy + projection at the evaluation budget + residuals of float32
    observations.  Returns the non-finite masks dict(action [n, 2], proposal [n], eq_resid [n, 1], ineq_resid [n, ineq_num]).
    (No env step: the two statements of its clamps coincide.)"""
    A = ARITH[clips]
    ap, _ = policy(spec, obs, deterministic=True)
    action, h, g = project(A, spec, ap, obs, spec.eval_K, spec.eval_lr)
    return dict(action=nonfinite(action.astype(np.float32)), proposal=nonfinite(ap.astype(np.float32)), eq_resid=nonfinite(h)[:, None],
                ineq_resid=nonfinite(g))


# ===================================================================================================== evaluation
ACC_SLOTS = ("ret", "mean_ineq", "mean_eq", "max_ineq", "max_eq")


def get_obs(spec, internal):
    internal = np.asarray(internal, np.float32)
    if spec.env == "cart":
        return internal
    with np.errstate(all="ignore"):
        return opd.get_obs(internal.astype(np.float64)).astype(np.float32)


def evaluate(spec, init_internal, horizon, clips, obs_of=None):
    """trainer.evaluate(init_states=, horizon=) of the deterministic policy, no auto-reset (RPOTrainerBase.eval()'s loop, eval_dev.h
    rpo_eval_lane_update): per episode
        nonfinite [n]      a LIVE step produced a non-finite reward, max violation or max |residual|
        length [n]         live steps (the one that ended the episode included)
        nan [n, 5]         which of ret, mean_ineq, mean_eq, max_ineq, max_eq are non-finite
        con_ineq [n, NI], con_eq [n, 1]   which cells ineq_max[j] / eq_max[j] of the per-constraint report are non-finite
    A finished lane's row no longer changes, whatever its state becomes.  ``obs_of(step, obs)``: what the policy reads instead
    of the observation (obs_noise=)."""
    A = ARITH[clips]
    state = np.asarray(init_internal, np.float32).copy()
    n = state.shape[0]
    acc = np.zeros((n, 5))
    ni = 6 if spec.env == "cart" else 1
    con_ineq, con_eq = np.zeros((n, ni)), np.zeros((n, 1))
    alive, bad_any, length = np.ones(n, bool), np.zeros(n, bool), np.zeros(n, np.int64)

    def keep_nan_max(a, b):
        return np.where(np.isnan(a), a, np.where(np.isnan(b), b, np.maximum(a, b)))
    with np.errstate(all="ignore"):
        for i in range(int(horizon)):
            obs = get_obs(spec, state)
            seen = obs if obs_of is None else obs_of(i, obs)
            ap, _ = policy(spec, seen, deterministic=True)
            action, _, _ = project(A, spec, ap, seen, spec.eval_K, spec.eval_lr)
            st = env_step(A, spec, state, action.astype(np.float32), np.full(n, i), auto_reset=False)
            new = acc.copy()
            new[:, 0] = acc[:, 0] + st["reward"]
            new[:, 1] = acc[:, 1] + (st["ineq"] - acc[:, 1]) / (i + 1)
            new[:, 2] = acc[:, 2] + (st["eq"] - acc[:, 2]) / (i + 1)
            new[:, 3] = keep_nan_max(acc[:, 3], st["ineq"])
            new[:, 4] = keep_nan_max(acc[:, 4], st["eq"])
            acc = np.where(alive[:, None], new, acc)
            con_ineq = np.where(alive[:, None], keep_nan_max(con_ineq, st["g"]), con_ineq)
            con_eq = np.where(alive[:, None], keep_nan_max(con_eq, np.abs(st["h"])[:, None]), con_eq)
            bad_any |= alive & (nonfinite(st["reward"]) | nonfinite(st["ineq"]) | nonfinite(st["eq"]))
            length += alive
            alive = alive & ~st["done"]
            state = st["next_internal"].astype(np.float32)
    return dict(nonfinite=bad_any, length=length, nan=nonfinite(acc), con_ineq=nonfinite(con_ineq), con_eq=nonfinite(con_eq))


# ===================================================================================================== the case table
INTERNAL_DIM = {"cart": 6, "pendulum": 4}
OBS_DIM = {"cart": 6, "pendulum": 5}


def lane_cases(env, targets=None):
    """[(name, target, [(lane, component, bits), ...])].  target: "state" -- the lane's state, and on SpringPendulum the observation
    rewritten from it, which is the pair every launch leaves behind; "obs" / "internal" (SpringPendulum, launches that read the two
    arrays separately): one of them only.  One component of one lane for every lane of LANES and every value of PLANT_BITS, the
    component walking through the state; then two bad lanes in one launch."""
    out = []
    for target in (targets or (("state",) if env == "cart" else ("state", "obs", "internal"))):
        dim = OBS_DIM[env] if target == "obs" else INTERNAL_DIM[env]
        for b, bits in enumerate(PLANT_BITS):
            for j, lane in enumerate(LANES):
                out.append(("%s-%08X-lane%d" % (target, bits, lane), target, [(lane, (j + b) % dim, bits)]))
        out.append(("%s-two-lanes" % target, target, [(15, 1, NEG_QNAN), (64, 0, QNAN)]))
    return out


PARAM_FIELDS = {False: ("Ws", "bs", "W0", "b0", "W1", "b1"), True: ("Ws", "bs", "W0", "b0", "W1", "b1", "W1b", "b1b")}


def param_cases(gauss):
    """[(name, field, bits)]: one element, either NaN sign, of the first-layer weight and bias, the hidden weight and bias and the
    head weight and bias -- of BOTH heads for RPOSAC.  The element is the middle one of the tensor."""
    return [("%s-%08X" % (f, bits), f, bits) for f in PARAM_FIELDS[bool(gauss)] for bits in (QNAN, NEG_QNAN)]


def param_index(t):
    return t.numel() // 2


def planted_state(env, internal, obs, target, plants):
    """(internal, obs) float32 copies with the plants in; obs is ``internal`` itself on CartSafe."""
    internal = np.array(internal, np.float32, copy=True)
    obs = internal if env == "cart" else np.array(obs, np.float32, copy=True)
    for lane, comp, bits in plants:
        (obs if target == "obs" else internal).view(np.uint32)[lane, comp] = bits      # (by bit pattern: the NaN's sign stays)
        if env == "pendulum" and target == "state":
            # the observation of THAT entry as a step leaves it: cos and sin of a NaN or an infinite angle are NaN, the other
            # entries are copies.  (Every other entry keeps the bits the device's own sincosf wrote.)
            if comp == 0:
                obs[lane, 0] = obs[lane, 1] = np.float32(np.nan)
            else:
                obs.view(np.uint32)[lane, comp + 1] = bits
    return internal, obs


# ===================================================================================================== evaluation cases
def eval_init(h):
    """Initial states of the evaluation cases (``h``: a StepHarness): the reset states, SpringPendulum's angle well inside its
    +-pi/12 (no lane ends on a rounding), and lane 7 one step before the edge, so that it finishes at step 0."""
    init = h.internal0.copy()
    if h.spec.env == "cart":
        init[7, 0], init[7, 1] = 2.39, 2.0                       # x' = 2.39 + 0.02 * 2 > 2.4
    else:
        init[:, 0] = np.clip(init[:, 0], -0.1, 0.1)
        init[7, 2], init[7, 3] = 1.49, 1.0                       # l' = 1.49 + 0.05 * 1 >= 1.5
    return init


def eval_plants(env):
    """The lane plants of the table in the initial state (lane 7 is kept for the episode that ends at once)."""
    return [c for c in lane_cases(env, ("state",)) if all(p[0] != 7 for p in c[2])]


# ===================================================================================================== the harness
class StepHarness(object):
    """One trainer, reset once; every case starts from the same snapshot (state, episode words, ring, statistics, ctrl with the
    step counter at T0 and a clear failure word), runs ONE vector step through ``tr._rollout`` -- the one-launch rollout in the form
    the library's tuning selects, or the single-stage chain -- and returns what it left as numpy."""

    def __init__(self, tr, sync=None):
        self.tr, self.sync = tr, sync or (lambda: None)
        v = tr.vec
        v.reset()
        v.ctrl.zero_()
        v.ctrl[T_IDX] = T0
        self.sync()
        self.names = ("internal", "obs", "action", "ep_len", "ep_ret", "ep_count", "stats", "ctrl")
        self.snap = {k: getattr(v, k).clone() for k in self.names}
        self.rows0 = tr.buffer.rows.clone()
        self.spec = Spec(tr)
        self.internal0 = self.snap["internal"].cpu().numpy()
        self.obs0 = self.snap["obs"].cpu().numpy()
        self.ep_len0 = self.snap["ep_len"].cpu().numpy()

    def restore(self):
        v = self.tr.vec
        for k in self.names:
            getattr(v, k).copy_(self.snap[k])
        self.tr.buffer.rows.copy_(self.rows0)

    def set_state(self, internal, obs):
        v = self.tr.vec
        v.internal.copy_(torch.as_tensor(internal, device=v.internal.device))
        if v.obs is not v.internal:
            v.obs.copy_(torch.as_tensor(obs, device=v.obs.device))

    def step(self):
        self.tr._rollout(False)
        self.sync()
        v = self.tr.vec
        out = {k: getattr(v, k).cpu().numpy() for k in ("internal", "obs", "action", "ep_len", "ep_count", "ctrl")}
        out["rows"] = self.tr.buffer.rows.cpu().numpy()
        return out

    def run(self, internal=None, obs=None):
        self.restore()
        if internal is not None:
            self.set_state(internal, obs)
        return self.step()

    def planted_param(self, field, bits):
        """``with h.planted_param(field, bits) as index:`` -- element ``index`` of the actor's parameter holds the value; put back
        on exit."""
        return planted_param(self.tr, field, bits)


class planted_param(object):
    """One element of a parameter tensor of the trainer's actor holds a value, by bit pattern, inside the ``with`` block."""

    def __init__(self, tr, field, bits):
        self.t = tr.fused.descs["actor"].tensors[field]
        self.i, self.bits = param_index(self.t), bits

    def __enter__(self):
        flat = self.t.detach().view(-1)
        self.old = flat[self.i].clone()
        flat[self.i:self.i + 1].view(torch.int32).fill_(int(np.array([self.bits], np.uint32).view(np.int32)[0]))
        return self.i

    def __exit__(self, *exc):
        self.t.detach().view(-1)[self.i] = self.old
        return False


def check_step(name, out, clean, ref, n, spec, t=T0, word_before=0):
    """One launch's outputs ``out`` against the reference ``ref`` (vector_step) and the launch without the plant ``clean``.
    Returns the list of what is wrong (empty: nothing)."""
    wrong = []
    bad = ref["bad"]
    want = word_before if word_before else ref["word"]
    if int(out["ctrl"][NF_IDX]) != want:
        wrong.append("%s: failure word %d, the reference gives %d (bad lanes %s)" % (name, int(out["ctrl"][NF_IDX]), want, np.flatnonzero(bad)[:8]))
    if int(out["ctrl"][T_IDX]) != t + 1:
        wrong.append("%s: ctrl[T] %d after the step, not %d" % (name, int(out["ctrl"][T_IDX]), t + 1))
    cap = out["rows"].shape[0] // n
    ring = out["rows"].reshape(cap, n, -1)
    ring_clean = clean["rows"].reshape(cap, n, -1)
    slot = t % cap
    got = dict(row=ring[slot][:, :spec.row_floats], internal=out["internal"], obs=out["obs"], action=out["action"])
    for key, mask in ref["masks"].items():
        if key == "obs" and spec.env == "cart":
            continue
        g = nonfinite(got[key])
        if not np.array_equal(g[bad], mask[bad]):
            lane = np.flatnonzero(bad)[np.flatnonzero((g[bad] != mask[bad]).any(axis=1))[0]]
            wrong.append("%s: %s of bad lane %d is non-finite at %s, float64 gives %s" % (name, key, lane, np.flatnonzero(g[lane]), np.flatnonzero(mask[lane])))
    keep = ~bad
    for key, a, b in (("internal", out["internal"], clean["internal"]), ("obs", out["obs"], clean["obs"]), ("action", out["action"], clean["action"]),
                      ("ring row", ring[slot], ring_clean[slot])):
        if not same_bits(a[keep], b[keep]):
            wrong.append("%s: %s of a lane outside the bad set differs from the launch without the plant" % (name, key))
    later = np.arange(cap) != slot
    if not same_bits(ring[later], ring_clean[later]):
        wrong.append("%s: a ring slot other than the step's changed" % name)
    for key in ("ep_len", "ep_count"):
        if not np.array_equal(out[key][keep], clean[key][keep]):
            wrong.append("%s: %s of a lane outside the bad set differs" % (name, key))
    return wrong
