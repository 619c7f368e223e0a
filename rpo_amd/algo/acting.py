"""Projected actions for caller-supplied observations: ``RPOTrainerBase.act()``.

``eval()`` and ``evaluate()`` measure a policy on vector envs the trainer owns and resets itself.  ``act()`` USES it: n
observations of the caller's choosing -> the completed, projected actions ``eval()`` would step in those states, what the
policy proposed, how many GRG iterations every row took and the signed residuals at the result (``ActResult``).  Two paths,
chosen like ``evaluate()``'s:

* **fused** -- RPODDPG / RPOSAC on CartSafe-v0 and SpringPendulum-v0 with the fused 128-wide actor: ONE launch of
  ``rpo_<env>_policy_act`` (csrc/act.hip: the row-tile form, ``form == "tile"``; csrc/act_stream.hip: the LDS-stationary
  streaming form from RPO_ROLLOUT_STREAM_FROM rows, ``form == "stream"``).
* **stepwise** -- everything else (EVOPF-v0, the Lagrangian baselines, 256-wide actors, ``fused_mlp=0``, the CPU oracle
  backend, schedule ``fused_act=0``): the trainer's deterministic proposal, ``act_project(NOISE_NONE, iters)`` and the env's
  residual kernel, launch by launch.

Both paths compute the same bits (``tests/test_act_gpu.py``).  Rows are ALWAYS projected independently with a per-row stop
test -- the B = 1 semantics of the rollout and of ``eval()``; SpringPendulum's batch-coupled reference projection is never
used here, whatever ``batch_reference`` is: ``act(obs)[i]`` is ``act(obs[i:i+1])``.  The call reads the actor's parameters
and writes its result buffers, nothing else: no env lane, control word, replay row, Philox counter or graph is touched, nothing
is drawn from a generator, and nothing waits for the device.  Data-parallel runs: the calling rank acts alone, no collective.
"""
import math

import torch

from .. import ops as hip_ops

_FORMS = {0: None, 1: "tile", 2: "stream", 3: "stream"}


class ActResult(object):
    """What ``act()`` returns: torch tensors on the trainer's device (float32; ``iters`` int32), n rows each.

    ``action`` [n, action_dim]: the completed, projected action (what ``eval()`` would step); ``proposal`` [n, P]: what the
    policy handed to the projection (``EvalTrajectory.proposal``'s definition: after the tanh box or the mean head; EVOPF-v0
    RPODDPG with the fused MLPs: the raw actor output; the Lagrangian baselines have no projection: the proposal IS the action,
    the same tensor); ``iters`` [n]: GRG iterations of the row (0 for the baselines); ``eq_resid`` [n, eq_num] /
    ``ineq_resid`` [n, ineq_num]: the signed residuals at ``action`` (ineq > 0 is a violation; None with ``residuals=False``).
    ``path``: "fused" | "stepwise"; ``form``: "tile" | "stream" on the fused path, else None."""

    FIELDS = ("action", "proposal", "iters", "eq_resid", "ineq_resid")

    def __init__(self, action, proposal, iters, eq_resid=None, ineq_resid=None, path=None, form=None):
        self.action, self.proposal, self.iters, self.eq_resid, self.ineq_resid = action, proposal, iters, eq_resid, ineq_resid
        self.path, self.form = path, form

    @classmethod
    def empty(cls, tr, n, residuals):
        k, dev = tr.kernels, tr.device
        action = torch.zeros(n, k.action_dim, device=dev)
        proposal = action if not _projects(tr) else torch.zeros(n, tr._eval_proposal_dim(), device=dev)
        return cls(action, proposal, torch.zeros(n, dtype=torch.int32, device=dev),
                   torch.zeros(n, k.eq_num, device=dev) if residuals else None,
                   torch.zeros(n, k.ineq_num, device=dev) if residuals else None)

    @property
    def n(self):
        return self.action.shape[0]

    @property
    def residuals(self):
        return self.eq_resid is not None

    def max_ineq(self):
        """[n]: the row's largest signed inequality residual (> 0: violated), NaN-propagating; stays on the device."""
        return self.ineq_resid.max(dim=1).values

    def max_eq(self):
        """[n]: the row's largest |equality residual|; stays on the device."""
        return self.eq_resid.abs().max(dim=1).values

    def numpy(self):
        """The fields as numpy arrays (a dict; waits for the device)."""
        return {f: (None if getattr(self, f) is None else getattr(self, f).detach().cpu().numpy()) for f in self.FIELDS}

    def __repr__(self):
        return "ActResult(n=%d, path=%s, form=%s, residuals=%s)" % (self.n, self.path, self.form, self.residuals)


def _projects(tr):
    """The trainer has a projection (RPODDPG / RPOSAC); the Lagrangian baselines step the actor's output as it is."""
    return not hasattr(tr, "_deterministic")


def fused_ok(tr):
    """``rpo_<env>_policy_act`` applies: ``evaluation.fused_ok``'s conditions, with the schedule key ``fused_act``."""
    f = tr.fused
    return bool(tr.schedule.get("fused_act", 1) and f is not None and "actor" in f.descs and hasattr(tr.kernels, "policy_act")
                and _projects(tr) and tr._box_affine is not None and f.descs["actor"].E == 128 and tr.device.type == "cuda")


def _check(tr, obs, eval_steps, eval_lr, residuals, out, form):
    k = tr.kernels
    obs = torch.as_tensor(obs, dtype=torch.float32, device=tr.device)
    if obs.dim() == 1:
        obs = obs[None, :]
    if obs.dim() != 2 or obs.shape[1] != k.obs_dim or obs.shape[0] == 0:
        raise ValueError("act: obs must be [n, %d] with n >= 1 (or [%d]), got %s" % (k.obs_dim, k.obs_dim, tuple(obs.shape)))
    if obs.stride(1) != 1 or (obs.shape[0] > 1 and obs.stride(0) < k.obs_dim):
        obs = obs.contiguous()
    steps = tr.eval_steps if eval_steps is None else eval_steps
    try:
        ok = not isinstance(steps, bool) and int(steps) == steps and steps >= 0
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("act: eval_steps must be an integer >= 0, got %r" % (eval_steps,))
    lr = tr.eval_lr if eval_lr is None else eval_lr
    try:
        lr = float(lr)
    except (TypeError, ValueError):
        lr = float("nan")
    if not math.isfinite(lr):
        raise ValueError("act: eval_lr must be a finite number, got %r" % (eval_lr,))
    if form not in _FORMS:
        raise ValueError("act: form must be 0 (by size), 1 (row tile), 2 or 3 (streaming, 16- / 64-row groups), got %r" % (form,))
    if out is not None:
        if not isinstance(out, ActResult) or out.n != obs.shape[0] or out.residuals != bool(residuals):
            raise ValueError("act: out must be an ActResult of the same n (%d) and the same residuals (%r), got %r"
                             % (obs.shape[0], bool(residuals), out))
    return obs, int(steps), lr


def act(tr, obs, eval_steps=None, eval_lr=None, residuals=True, out=None, form=0):
    """See ``RPOTrainerBase.act``."""
    obs, steps, lr = _check(tr, obs, eval_steps, eval_lr, residuals, out, form)
    n = obs.shape[0]
    fused = fused_ok(tr)
    if form and not fused:
        raise ValueError("act: form=%r asks for a form of the fused launch; this trainer acts on the stepwise path" % (form,))
    r = out if out is not None else ActResult.empty(tr, n, residuals)
    k = tr.kernels
    with torch.no_grad():
        if fused:
            scale, base = tr._box_affine
            desc = tr.fused.descs["actor"]
            k.policy_act(desc, tr._gauss_policy, scale, base, obs, r.action, r.proposal, r.iters, r.eq_resid, r.ineq_resid,
                         tr._box_lo, tr._box_hi, steps, lr, tr.corr_eps, tr.corr_momentum, form=form)
            stream = n >= hip_ops.CONST["RPO_ROLLOUT_STREAM_FROM"] and desc.tensors["W0"].data_ptr() % 16 == 0
            r.path, r.form = "fused", _FORMS[form] or ("stream" if stream else "tile")
            return r
        obs = obs.contiguous()
        if _projects(tr):
            ap = tr._eval_partial(obs)
            r.proposal.copy_(ap.reshape(r.proposal.shape))
            # (always the per-row kernel: base_env.project(batch_reference=True) would couple SpringPendulum's rows)
            k.act_project(obs, ap, None, r.action, r.iters, hip_ops.NOISE_NONE, 0.0, 0.0, 0.0, tr._box_lo, tr._box_hi, steps, lr,
                          tr.corr_eps, tr.corr_momentum, **tr._act_kw)
        else:
            r.action.copy_(tr._deterministic(obs))
            r.iters.zero_()
        if residuals:
            k.resid(obs, r.action, r.eq_resid, r.ineq_resid)
    r.path, r.form = "stepwise", None
    return r
