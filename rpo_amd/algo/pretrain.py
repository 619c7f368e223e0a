"""Behaviour cloning of the actor from recorded demonstrations: ``Demonstrations`` and ``trainer.pretrain()``.

The demonstrations are (observation, basic action) pairs -- typically the record of ``trainer.evaluate_opf(record=True)``, the
single-step AC-OPF run as a controller, but any recorded policy serves (a ``BestPolicy`` evaluated with ``record=True``, another
algorithm's actor, or ``Demonstrations.label`` on the states a policy visited: the relabelling step of DAgger).  The target is
always the COMPLETED, PROJECTED action's components at ``env.partial_actions``, in box units -- never the record's ``proposal``,
which on EVOPF-v0 with the fused MLPs is the raw actor output.

The loss (include/rpo_hip.h, rpo_bc_head; csrc/bc.hip) compares tanh(raw actor output) with the target in BOX-NORMALISED
coordinates u = (a - base) / scale, clamped to +-clip: in action units EVOPF's voltage band (+-0.06) would weigh nothing beside pg,
and a target of exactly +-1 -- where nearly every OPF battery component sits -- would drive the raw output to infinity and leave
the actor saturated for the RL phase that follows.

One step is five launches, with no host synchronisation between steps: gather a minibatch from the device-resident table ->
actor forward (raw outputs, activations saved) -> the head -> actor backward (leaves the gradient's inf-norm) -> clip + Adam on
the actor's range of the flat parameter buffer.
"""
import math

import numpy as np
import torch

from .agent.flat import FusedAdam

_SALT_BC = 0x6263                                    # salt of the minibatch draw's Philox index (step + salt)


def _host_f32(x, what):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    try:
        a = np.asarray(x)
        if a.dtype == np.bool_ or a.dtype.kind not in "fiu":
            raise TypeError
        a = np.ascontiguousarray(a, dtype=np.float32)
    except (TypeError, ValueError):
        raise ValueError("Demonstrations: %s must be an array of numbers, got %r" % (what, type(x).__name__))
    return a


class Demonstrations(object):
    """(observation, demonstrated basic action) pairs: ``obs`` float32 [N, obs_dim], ``target`` float32 [N, partial_dim], N >= 1,
    every entry finite (ValueError otherwise).  Host arrays; ``trainer.pretrain`` uploads them once per call.  ``dropped``: the
    rows a constructor left out (``from_trajectory`` / ``label``; 0 otherwise); ``index``: for those two, the positions of the kept
    rows in the flattened input (int64 [N]; None otherwise and after ``extend``)."""

    def __init__(self, obs, target):
        obs, target = _host_f32(obs, "obs"), _host_f32(target, "target")
        if obs.ndim != 2 or target.ndim != 2 or obs.shape[0] != target.shape[0] or obs.shape[0] < 1 or obs.shape[1] < 1 \
                or target.shape[1] < 1:
            raise ValueError("Demonstrations: obs must be [N, obs_dim] and target [N, partial_dim] with N >= 1, got %s and %s"
                             % (obs.shape, target.shape))
        if not (np.isfinite(obs).all() and np.isfinite(target).all()):
            raise ValueError("Demonstrations: obs and target must be finite (from_trajectory / label leave such rows out)")
        self.obs, self.target = obs, target
        self.dropped, self.index = 0, None

    def __len__(self):
        return self.obs.shape[0]

    def __repr__(self):
        return "Demonstrations(rows=%d, obs_dim=%d, partial_dim=%d, dropped=%d)" % (len(self), self.obs.shape[1],
                                                                                   self.target.shape[1], self.dropped)

    @classmethod
    def from_trajectory(cls, t, env, mask=None):
        """The valid steps of an ``EvalTrajectory`` -- and of ``mask`` (bool [episode, step], e.g. ``result.opf_converged``) --
        whose observation and action are finite; target = ``t.action[..., env.partial_actions]``.  ``dropped`` counts the valid
        steps left out."""
        obs, action, valid = np.asarray(t.obs), np.asarray(t.action), np.asarray(t.valid, dtype=bool)
        env = getattr(env, "unwrapped", env)
        O, A = int(env.observation_space.shape[0]), int(env.action_space.shape[0])
        if obs.ndim != 3 or action.ndim != 3 or obs.shape[2] != O or action.shape[2] != A or obs.shape[:2] != valid.shape \
                or action.shape[:2] != valid.shape:
            raise ValueError("Demonstrations.from_trajectory: the trajectory is not one of this env (obs %s, action %s; the env's "
                             "widths are %d and %d)" % (obs.shape, action.shape, O, A))
        keep = valid.copy()
        if mask is not None:
            mask = np.asarray(mask)
            if mask.shape != valid.shape or mask.dtype != np.bool_:
                raise ValueError("Demonstrations.from_trajectory: mask must be bool [episode, step] = %s, got %s %s"
                                 % (valid.shape, mask.dtype, mask.shape))
            keep &= mask
        keep &= np.isfinite(obs).all(axis=2) & np.isfinite(action).all(axis=2)
        if not keep.any():
            raise ValueError("Demonstrations.from_trajectory: no valid, finite step is left")
        pa = np.asarray(env.partial_actions, dtype=np.int64).reshape(-1)
        d = cls(obs[keep], action[keep][:, pa])
        d.dropped, d.index = int(valid.sum() - keep.sum()), np.flatnonzero(keep.reshape(-1))
        return d

    @classmethod
    def label(cls, env, obs, pe="free", pe_cost=None, tol=1e-4, max_iters=40):
        """Expert labels for caller-supplied observations [n, obs_dim]: ``env.opf`` (EVOPF-v0 on a GPU; NotImplementedError
        elsewhere, with the reason) solves every row's single-step AC-OPF -- ``pe="free"`` dispatches the batteries too,
        ``pe="zero"`` leaves them idle -- and the rows that converged to a finite action are kept.  The relabelling step of
        DAgger: ``obs`` are the states a policy visited."""
        env = getattr(env, "unwrapped", env)
        if pe not in ("free", "zero"):
            raise ValueError("Demonstrations.label: pe must be 'free' or 'zero', got %r" % (pe,))
        if not hasattr(env, "opf"):
            raise NotImplementedError("Demonstrations.label: the expert is the single-step AC-OPF of EVOPF-v0 (EVOPFEnv.opf); "
                                      "this env is %s" % type(env).__name__)
        env._opf_free_kernel() if pe == "free" else env._opf_kernel()      # NotImplementedError: oracle backend, CPU device
        o = _host_f32(obs, "obs")
        if o.ndim != 2 or o.shape[0] < 1 or o.shape[1] != env.state_dim:
            raise ValueError("Demonstrations.label: obs must be [n, %d], got %s" % (env.state_dim, o.shape))
        res = env.opf(o, pe="free" if pe == "free" else None, tol=tol, max_iters=max_iters, pe_cost=pe_cost).numpy()
        keep = res["converged"] & np.isfinite(res["action"]).all(axis=1) & np.isfinite(o).all(axis=1)
        if not keep.any():
            raise ValueError("Demonstrations.label: no row converged")
        pa = np.asarray(env.partial_actions, dtype=np.int64).reshape(-1)
        d = cls(o[keep], res["action"][keep][:, pa])
        d.dropped, d.index = int((~keep).sum()), np.flatnonzero(keep)
        return d

    def extend(self, other):
        """Append ``other``'s rows (same widths; ValueError otherwise) in place; returns self."""
        if not isinstance(other, Demonstrations) or other.obs.shape[1] != self.obs.shape[1] \
                or other.target.shape[1] != self.target.shape[1]:
            raise ValueError("Demonstrations.extend: needs Demonstrations of widths (%d, %d), got %r"
                             % (self.obs.shape[1], self.target.shape[1], other))
        self.obs = np.concatenate([self.obs, other.obs])
        self.target = np.concatenate([self.target, other.target])
        self.dropped, self.index = self.dropped + other.dropped, None
        return self

    def save(self, path):
        """One .npz (obs, target, dropped); ``Demonstrations.load`` reads it back."""
        with open(path, "wb") as f:
            np.savez(f, obs=self.obs, target=self.target, dropped=np.int64(self.dropped))

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            d = cls(z["obs"], z["target"])
            d.dropped = int(z["dropped"])
        return d

    def table(self, device):
        """The device-resident table [N, W]: row = (obs | target | zero padding), W a multiple of 4 floats (the gather copies
        16-byte chunks)."""
        O, P = self.obs.shape[1], self.target.shape[1]
        rows = np.zeros((len(self), (O + P + 3) // 4 * 4), dtype=np.float32)
        rows[:, :O], rows[:, O:O + P] = self.obs, self.target
        return torch.from_numpy(rows).to(device)


class PretrainResult(object):
    """What ``trainer.pretrain`` returns.  ``loss``: float32 numpy [steps], L of every step's minibatch BEFORE that step's update,
    read back once after the loop (each value the float32 sum of the head's partials in index order); ``steps``, ``batch_size``,
    ``lr``, ``seed`` (the seed of the minibatch draws; None with ``idx=``), ``rows`` (demonstrations used); ``graph_node_kinds``: with
    ``RPO_GRAPH_AUDIT=1``, {node kind: count} of every captured window, else None."""

    def __init__(self, loss, steps, batch_size, lr, seed, rows, graph_node_kinds=None):
        self.loss, self.steps, self.batch_size, self.lr, self.seed, self.rows = loss, steps, batch_size, lr, seed, rows
        self.graph_node_kinds = graph_node_kinds

    def __repr__(self):
        tail = "" if not self.steps else ", loss %.4g -> %.4g" % (self.loss[0], self.loss[-1])
        return "PretrainResult(steps=%d, batch_size=%d, rows=%d%s)" % (self.steps, self.batch_size, self.rows, tail)


def sum_parts(parts):
    """[steps, G] float32 partials -> [steps] float32: the partials added one after the other in index order."""
    parts = np.asarray(parts, dtype=np.float32)
    if parts.shape[0] == 0:
        return np.zeros(0, dtype=np.float32)
    return np.add.accumulate(parts, axis=1, dtype=np.float32)[:, -1].copy()


# ------------------------------------------------------------------------------------------------ argument checks
def _is_int(v):
    try:
        return not isinstance(v, (bool, np.bool_)) and int(v) == v
    except (TypeError, ValueError, OverflowError):
        return False


def check_steps(steps):
    if not _is_int(steps) or steps < 0:
        raise ValueError("pretrain: steps must be an integer >= 0, got %r" % (steps,))
    return int(steps)


def check_batch_size(tr, batch_size):
    b = tr.batch_size if batch_size is None else batch_size
    if not _is_int(b) or b < 16 or b % 16:
        raise ValueError("pretrain: batch_size must be a positive multiple of 16 (the MLP kernels' row tile), got %r" % (batch_size,))
    return int(b)


def _positive(v, what, given, upper=None):
    try:
        x = float("nan") if isinstance(v, (bool, np.bool_, str, bytes)) else float(v)
    except (TypeError, ValueError):
        x = float("nan")
    if not math.isfinite(x) or not x > 0.0 or (upper is not None and x > upper) or not math.isfinite(float(np.float32(x))) \
            or not float(np.float32(x)) > 0.0:
        raise ValueError("pretrain: %s, got %r" % (what, given))
    return x


def check_weights(weights, P):
    """None, or ``P`` finite numbers >= 0 -> None or the float32 vector."""
    if weights is None:
        return None
    bad = ValueError("pretrain: weights must be None or %d finite numbers >= 0, got %r" % (P, weights))
    if isinstance(weights, torch.Tensor):
        weights = weights.detach().cpu().numpy()
    if isinstance(weights, (bool, np.bool_, str, bytes)):
        raise bad
    try:
        a = np.asarray(weights)
        if a.dtype == np.bool_ or a.dtype.kind not in "fiu":
            raise bad
        a = a.astype(np.float64)
    except (TypeError, ValueError):
        raise bad
    if a.shape != (P,) or not np.all(np.isfinite(a)) or np.any(a < 0):
        raise bad
    with np.errstate(over="ignore"):
        w = a.astype(np.float32)
    if not np.all(np.isfinite(w)):
        raise bad
    return w


def check_idx(idx, steps, batch_size, rows, device):
    """``idx=``: int64 [steps, batch_size] with every entry in [0, rows) -> the tensor on ``device`` (None: None)."""
    if idx is None:
        return None
    t = idx if isinstance(idx, torch.Tensor) else (torch.from_numpy(idx) if isinstance(idx, np.ndarray) else None)
    if t is None or t.dtype != torch.int64 or tuple(t.shape) != (steps, batch_size):
        raise ValueError("pretrain: idx must be int64 [steps, batch_size] = [%d, %d], got %s"
                         % (steps, batch_size, "%s %s" % (t.dtype, tuple(t.shape)) if t is not None else type(idx).__name__))
    if t.numel() and (int(t.min()) < 0 or int(t.max()) >= rows):
        raise ValueError("pretrain: idx has an entry outside [0, %d)" % rows)
    return t.to(device).contiguous()


def fresh_seed(tr):
    """The seed of a ``pretrain()`` call without one: from the trainer seed and a call counter of pretrain's own (host-side
    only; ``evaluate()``'s counter is another)."""
    calls = getattr(tr, "_pretrain_calls", 0)
    tr._pretrain_calls = calls + 1
    return int(((tr.seed ^ 0xBC10BC10) + 0x9E3779B97F4A7C15 * (calls + 1)) & (2 ** 63 - 1))


# ------------------------------------------------------------------------------------------------ the loop
class BCStep(object):
    """The buffers of a cloning run and its step: the five launches, with the arguments ``pretrain`` gives them.  Tests issue the
    same launches by hand through ``trainer.backend`` / ``trainer.fused``."""

    def __init__(self, tr, table, batch_size, lr, seed, weights, clip, window):
        ag, fl, k, dev = tr.agent, tr.agent.flat, tr.kernels, tr.device
        self.tr, self.table, self.B, self.seed, self.weights, self.clip = tr, table, batch_size, seed, weights, float(clip)
        self.O, self.P = k.obs_dim, k.partial_dim
        self.heads = tr.fused.descs["actor"].n_out
        self.evopf = tr._box_affine is None                     # the state-dependent box: the env's own head kernel
        if not self.evopf:
            lo, hi = tr.base_env.box_constraint_partial
            self.lo, self.hi = np.asarray(lo, dtype=np.float32).reshape(-1), np.asarray(hi, dtype=np.float32).reshape(-1)
        self.batch = torch.zeros(batch_size, table.shape[1], device=dev)
        self.raw = torch.zeros(batch_size, self.heads * self.P, device=dev)
        self.draw = torch.zeros_like(self.raw)
        self.G = (batch_size + 15) // 16
        self.parts = torch.zeros(max(1, window), self.G, device=dev)        # one row of partials per step of a window
        self.ctrl = torch.zeros(tr.backend.CTRL_LEN, dtype=torch.int64, device=dev)
        self.ctrl[0] = 1                                        # the table is a ring of one vector step: valid from t = 1 on
        clip_thres = ag.actor_optim.clip_thres
        self.opt = FusedAdam(tr.backend, fl.param(fl.actor_range), fl.gradient(fl.actor_range), lr, ag.reg, clip_thres)
        self.opt.zero_grad_after = True                         # the backward accumulates: every step starts from a zero slice
        self.clipped = bool(clip_thres) and clip_thres != float("inf")

    def step(self, slot, idx=None):
        tr, be, f = self.tr, self.tr.backend, self.tr.fused
        if idx is None:
            be.replay_sample_gather(self.table, 1, self.table.shape[0], self.batch, None, self.seed, _SALT_BC, self.ctrl)
        else:
            be.replay_gather(self.table, idx, self.batch)
        obs, target = self.batch[:, :self.O], self.batch[:, self.O:self.O + self.P]
        f.forward("actor", obs, None, self.raw, save=True)
        if self.evopf:
            be.evopf_bc_head(tr.kernels, obs, self.raw, target, self.weights, self.clip, self.draw, self.parts[slot])
        else:
            be.bc_head(self.raw, target, self.lo, self.hi, self.weights, self.clip, self.draw, self.parts[slot])
        f.backward("actor", obs, None, self.draw, gradmax=self.opt.gradmax if self.clipped else None)
        self.opt.step(gradmax_ready=self.clipped, clock=self.ctrl)


def refuse(tr):
    """NotImplementedError, with the reason, where ``pretrain`` has no kernels to run on."""
    if getattr(tr, "fused", None) is None or "actor" not in tr.fused.descs:
        raise NotImplementedError("pretrain: the cloning step runs the actor through the fused MLP kernels (trainer.fused with an "
                                  "'actor' descriptor); this trainer has none (schedule fused_mlp=0, an unsupported network "
                                  "shape, or a Lagrangian baseline)")
    be = tr.backend
    evopf = tr._box_affine is None
    need = ("evopf_bc_head" if evopf else "bc_head", "replay_sample_gather", "replay_gather", "polyak")
    missing = [n for n in need if not hasattr(be, n)]
    if missing:
        raise NotImplementedError("pretrain: this backend has no %s: the cloning head exists as the HIP kernels rpo_bc_head / "
                                  "rpo_evopf_bc_head only (the CPU oracle backend has none)" % ", ".join(missing))
    if evopf and getattr(tr.kernels, "name", None) != "EVOPF-v0":
        raise NotImplementedError("pretrain: a state-dependent actor box needs the env's own head kernel; only EVOPF-v0 has one")
    if tr.device.type != "cuda":
        raise NotImplementedError("pretrain: the cloning step is HIP kernels and needs a GPU device, got %s: there is no CPU path"
                                  % tr.device)


def pretrain(tr, demos, steps=1000, batch_size=None, lr=None, seed=None, weights=None, clip=0.98, sync_targets=True, idx=None):
    """See ``RPOTrainerBase.pretrain``."""
    from .trainer import _GraphCache
    k, ag = tr.kernels, tr.agent
    steps = check_steps(steps)
    B = check_batch_size(tr, batch_size)
    lr = _positive(ag.lr_actor if lr is None else lr, "lr must be a finite number > 0", lr)
    clip = _positive(clip, "clip must lie in (0, 1]", clip, upper=1.0)
    weights = check_weights(weights, k.partial_dim)
    if not isinstance(demos, Demonstrations) or demos.obs.shape[1] != k.obs_dim or demos.target.shape[1] != k.partial_dim:
        raise ValueError("pretrain: demos must be Demonstrations of widths (obs_dim, partial_dim) = (%d, %d), got %r"
                         % (k.obs_dim, k.partial_dim, demos))
    if not isinstance(sync_targets, (bool, np.bool_)):
        raise ValueError("pretrain: sync_targets must be True or False, got %r" % (sync_targets,))
    N = len(demos)
    idx = check_idx(idx, steps, B, N, tr.device)
    if seed is not None and not _is_int(seed):
        raise ValueError("pretrain: seed must be None or an integer, got %r" % (seed,))
    refuse(tr)
    seed = None if idx is not None else (fresh_seed(tr) if seed is None else int(seed) & (2 ** 64 - 1))
    if steps == 0:
        return PretrainResult(np.zeros(0, dtype=np.float32), 0, B, lr, seed, N)
    fl = ag.flat
    tr._flush_tail()                                            # (a deferred optimiser step of the last iteration comes first)
    if getattr(tr, "_curve", None) is not None:
        tr._curve._order_after_points()                         # (an enqueued evaluation point has taken its snapshot of the actor)
    window = min(steps, max(1, int(tr._cycle)))
    with torch.no_grad():
        run = BCStep(tr, demos.table(tr.device), B, lr, seed, weights, clip, window)
        grad = fl.gradient(fl.actor_range)
        saved = grad.clone()                                    # the slice is handed back as it was found
        grad.zero_()
        log = torch.zeros(steps, run.G, device=tr.device)
        graphs = _GraphCache(bool(tr._graphs.enabled), warm=1)  # the first window runs eagerly (it allocates the scratch)
        done = 0
        while done < steps:
            L = min(window, steps - done)
            if idx is None:
                graphs.run(("bc", L), lambda: [run.step(i) for i in range(L)])
            else:                                               # injected indices: the launches of every step differ, no graph
                for i in range(L):
                    run.step(i, idx[done + i])
            log[done:done + L].copy_(run.parts[:L])
            done += L
        grad.copy_(saved)
        if sync_targets:
            c = fl.actor_range[0]
            sh = fl.critic_range[1] - c if fl.sizes[1] > 0 else 0
            if ag.actor_target_flat is not None:
                tr.backend.polyak(fl.param(fl.actor_range), ag.actor_target_flat, 1.0)
            if sh > 0:
                tr.backend.polyak(fl.param((c, c + sh)), ag.critic_target_flat[c:c + sh], 1.0)
        loss = sum_parts(log.cpu().numpy())
    kinds = [e["node_kinds"] for e in graphs.entries.values() if "node_kinds" in e] if graphs.audit else None
    return PretrainResult(loss, steps, B, lr, seed, N, graph_node_kinds=kinds)
