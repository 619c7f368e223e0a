"""Many-episode policy evaluation: ``RPOTrainerBase.evaluate()``.

``eval()`` is the reference's protocol (rpo_ddpg.py:207-264): 10 episodes, the 10-tuple of (mean, std) pairs, driven from
the host one env step at a time.  ``evaluate()`` runs the same policy, projection and horizon on any number of independent
episodes and returns per-episode arrays (``EvalResult``).  Two paths, chosen from what the trainer can observe:

* **fused** -- RPODDPG / RPOSAC on CartSafe-v0 and SpringPendulum-v0 with the fused MLP kernels: ``rpo_<env>_evaluate``
  (csrc/evaluate.hip) runs actor -> head -> Complete -> GRG -> env step -> per-episode accumulators for up to ``steps`` env
  steps per launch, ``ceil(horizon / steps)`` launches back to back, no host synchronisation in between.
* **stepwise** -- everything else (EVOPF-v0, the Lagrangian baselines, ``fused_mlp=0``, the CPU oracle backend, and
  schedule ``fused_eval=0``): ``_eval_action`` + ``step(auto_reset=False)`` + ``rpo_eval_accumulate`` per env step, or the
  same update in torch ops on a backend without that kernel.

Both paths compute the same bits (``tests/test_evaluate_gpu.py``).  The evaluation owns its vector env, its ``ctrl`` and
its buffers: no trainer state is read-modified-written, so training after an ``evaluate()`` call is the training without it.
Data-parallel runs: ``evaluate()`` runs on the calling rank alone, with no collective (the replicas' networks are
identical, so every rank would compute the same result); call it on one rank.
"""
import numpy as np
import torch

from .. import ops as hip_ops

#: accumulator row layout (include/rpo_hip.h: RPO_EVAL_*)
_RET, _MEAN_INEQ, _MEAN_EQ, _MAX_INEQ, _MAX_EQ, _VIOL, _ITERS, _WORD = range(8)
_ALIVE, _NONFINITE, _LEN_SHIFT = 1, 2, 2
_HORIZON = 500                                                   # eval()'s episode cap


class EvalResult(object):
    """Per-episode results of ``evaluate()``: numpy arrays of length ``episodes``.

    ``ret``, ``length``; ``mean_ineq`` / ``mean_eq``: running means over the episode's steps of the step's max inequality
    violation / max |equality residual| (eval()'s definitions); ``max_ineq`` / ``max_eq``: their maxima; ``viol_steps``: steps
    whose max inequality violation exceeds the vector env's ``viol_thresh``; ``proj_iters``: GRG iterations summed over the
    episode; ``nonfinite``: a live step produced a non-finite reward or violation.  ``path``: "fused" or "stepwise"."""

    FIELDS = ("ret", "length", "mean_ineq", "mean_eq", "max_ineq", "max_eq", "viol_steps", "proj_iters", "nonfinite")

    def __init__(self, acc, path, horizon, seed):
        acc = np.asarray(acc, dtype=np.float32).reshape(-1, 8)
        word = acc[:, _WORD].view(np.int32)
        self.ret = acc[:, _RET].astype(np.float64)
        self.length = (word >> _LEN_SHIFT).astype(np.int64)
        self.mean_ineq = acc[:, _MEAN_INEQ].astype(np.float64)
        self.mean_eq = acc[:, _MEAN_EQ].astype(np.float64)
        self.max_ineq = acc[:, _MAX_INEQ].astype(np.float64)
        self.max_eq = acc[:, _MAX_EQ].astype(np.float64)
        self.viol_steps = acc[:, _VIOL].astype(np.int64)
        self.proj_iters = acc[:, _ITERS].astype(np.int64)
        self.nonfinite = (word & _NONFINITE) != 0
        self.path, self.horizon, self.seed = path, int(horizon), seed

    @property
    def episodes(self):
        return len(self.ret)

    def summary(self):
        """The reference's 10-tuple in eval()'s order: (mean, std) of return, mean ineq, mean eq, max ineq, max eq (numpy's
        population std)."""
        out = []
        for x in (self.ret, self.mean_ineq, self.mean_eq, self.max_ineq, self.max_eq):
            out += [x.mean(), x.std()]
        return tuple(out)

    def violation_rate(self):
        """Fraction of the evaluated env steps whose max inequality violation exceeds ``viol_thresh``."""
        return float(self.viol_steps.sum()) / float(self.length.sum())

    def __repr__(self):
        return "EvalResult(episodes=%d, path=%s, return=%.4f, violation_rate=%.4g)" % (
            self.episodes, self.path, self.ret.mean(), self.violation_rate())


def accumulate_torch(rows, cols, iters, step, viol_thresh, acc):
    """``rpo_eval_accumulate`` in torch ops (backends without the kernel: the CPU oracle), with eval()'s expressions."""
    n = acc.shape[0]
    rows = rows[:n]
    ineq = rows[:, cols["ineq_viol"][0]:cols["ineq_viol"][1]].max(dim=1).values
    eq = rows[:, cols["eq_viol"][0]:cols["eq_viol"][1]].abs().max(dim=1).values
    reward, done = rows[:, cols["reward"][0]], rows[:, cols["done"][0]]
    word = acc[:, _WORD].view(torch.int32)
    if step == 0:
        acc.zero_()
        word.fill_(_ALIVE)
    live = (word & _ALIVE) != 0
    it = iters.to(acc.dtype) if iters is not None else torch.zeros_like(reward)
    a = acc.clone()
    acc[:, _RET] = torch.where(live, a[:, _RET] + reward, a[:, _RET])
    acc[:, _MEAN_INEQ] = torch.where(live, a[:, _MEAN_INEQ] + (ineq - a[:, _MEAN_INEQ]) / (step + 1), a[:, _MEAN_INEQ])
    acc[:, _MEAN_EQ] = torch.where(live, a[:, _MEAN_EQ] + (eq - a[:, _MEAN_EQ]) / (step + 1), a[:, _MEAN_EQ])
    acc[:, _MAX_INEQ] = torch.where(live, torch.maximum(a[:, _MAX_INEQ], ineq), a[:, _MAX_INEQ])
    acc[:, _MAX_EQ] = torch.where(live, torch.maximum(a[:, _MAX_EQ], eq), a[:, _MAX_EQ])
    acc[:, _VIOL] = torch.where(live, a[:, _VIOL] + (ineq > viol_thresh).to(acc.dtype), a[:, _VIOL])
    acc[:, _ITERS] = torch.where(live, a[:, _ITERS] + it, a[:, _ITERS])
    bad = ~(torch.isfinite(reward) & torch.isfinite(ineq) & torch.isfinite(eq))
    w = a[:, _WORD].view(torch.int32)
    nw = (w + (1 << _LEN_SHIFT)) | (bad.to(torch.int32) * _NONFINITE)
    nw = torch.where(done != 0, nw & ~_ALIVE, nw)
    word.copy_(torch.where(live, nw, w))


def default_horizon(tr):
    """eval()'s horizon: min(500, max_episode_steps, the env's episode_steps)."""
    h = _HORIZON
    if tr.max_episode_steps:
        h = min(h, int(tr.max_episode_steps))
    return min(h, getattr(tr.kernels, "episode_steps", h))


def fused_ok(tr):
    """The fused evaluation kernel applies: RPODDPG / RPOSAC with the fused actor (E = 128) on an env whose kernels have it."""
    f = tr.fused
    return bool(tr.schedule.get("fused_eval", 1) and f is not None and "actor" in f.descs and hasattr(tr.kernels, "evaluate")
                and tr._box_affine is not None and f.descs["actor"].E == 128 and tr.device.type == "cuda")


def evaluate(tr, episodes=10, horizon=None, seed=None, init_states=None):
    """See ``RPOTrainerBase.evaluate``."""
    if isinstance(episodes, bool) or int(episodes) != episodes or episodes < 1:
        raise ValueError("evaluate: episodes must be an integer >= 1, got %r" % (episodes,))
    n = int(episodes)
    if horizon is not None and (isinstance(horizon, bool) or int(horizon) != horizon or horizon < 1):
        raise ValueError("evaluate: horizon must be an integer >= 1, got %r" % (horizon,))
    H = int(horizon) if horizon is not None else default_horizon(tr)
    if H >= 1 << 24:
        raise ValueError("evaluate: horizon must be below 2^24 (lengths are counted exactly in float32), got %d" % H)
    k = tr.kernels
    if init_states is not None:
        init_states = torch.as_tensor(init_states, dtype=torch.float32, device=tr.device)
        if tuple(init_states.shape) != (n, k.internal_dim):
            raise ValueError("evaluate: init_states must be [episodes, internal_dim] = [%d, %d], got %s"
                             % (n, k.internal_dim, tuple(init_states.shape)))
    if seed is None:
        # fresh initial states at every call, like eval(): from the trainer seed and a call counter (host-side only)
        calls = getattr(tr, "_evaluate_calls", 0)
        tr._evaluate_calls = calls + 1
        seed = ((tr.seed ^ 0xE7A1E7A1) + 0x9E3779B97F4A7C15 * (calls + 1)) & (2 ** 63 - 1)
    seed = int(seed)
    v = tr.base_env.make_vec(n, seed=seed, env_id_base=0, max_episode_steps=tr.max_episode_steps, device=tr.device,
                             stats_cap=2, viol_thresh=tr.vec.viol_thresh)
    v.reset()
    if init_states is not None:
        v.set_internal(init_states)
    acc = torch.zeros(n, 8, device=tr.device)
    with torch.no_grad():
        if fused_ok(tr):
            path = "fused"
            _run_fused(tr, v, acc, H)
        else:
            path = "stepwise"
            _run_stepwise(tr, v, acc, H)
    return EvalResult(acc.cpu().numpy(), path, H, seed)


def _run_fused(tr, v, acc, H):
    """ceil(H / steps) launches of rpo_<env>_evaluate, enqueued back to back.  steps: RPO_EVAL_LANE_STEPS lane-steps per launch
    (4 steps at 2^20 lanes, one launch for the whole horizon up to ~8000 lanes)."""
    n = v.n
    steps = max(1, min(H, hip_ops.EVAL_LANE_STEPS // n))
    scale, base = tr._box_affine
    desc = tr.fused.descs["actor"]
    for t0 in range(0, H, steps):
        tr.kernels.evaluate(desc, tr._gauss_policy, scale, base, v.internal, None if v.obs is v.internal else v.obs, v.action,
                            v.ep_len, v.ep_ret, v.ep_count, v.ctrl, acc, t0, min(steps, H - t0), tr._box_lo, tr._box_hi,
                            tr.eval_steps, tr.eval_lr, tr.corr_eps, tr.corr_momentum, v.max_episode_steps, v.viol_thresh)


def _run_stepwise(tr, v, acc, H):
    """eval()'s loop: the trainer's deterministic action + projection, one env step without auto-reset, the accumulator
    update.  Finished lanes keep stepping (as in eval()); their rows no longer change."""
    k = tr.kernels
    rows = torch.zeros(v.n, k.ring_floats, device=tr.device)
    iters = torch.zeros(v.n, dtype=torch.int32, device=tr.device)
    update = getattr(tr.backend, "eval_accumulate", None) or accumulate_torch
    for i in range(H):
        tr._eval_action(v, iters=iters)
        v.step(v.action, rows=rows, cap_steps=1, auto_reset=False)
        update(rows, k.cols, iters, i, v.viol_thresh, acc)
