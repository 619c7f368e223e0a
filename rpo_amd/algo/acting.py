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

``act(obs, profile=True)`` also returns how the projection CONVERGES (``ActResult.profile``, a ``ProjectionProfile``): for
every budget b = 0..K (K = the call's ``eval_steps``) what ``act(obs, eval_steps=b)`` would return, written down by ONE run at
the budget K -- the loop is deterministic and every row has its own stop test, so a run at K passes through every smaller
budget's result.  Three paths: **fused** (``rpo_<env>_policy_act_profile``, the row tile), **stepwise** (the proposal launches +
``rpo_<env>_project_profile`` + the residual kernel; on EVOPF-v0 opt-in by schedule ``profile_evopf=1``, default 0:
``rpo_evopf_project_profile``, whose planes hold the first two action components and the equality residual of largest magnitude
with its sign) and **sweep** (EVOPF-v0 by default, the oracle backend: K + 1 stepwise ``act()`` calls assembled with torch ops;
correct by construction and slow).

All paths compute the same bits (``tests/test_act_gpu.py``, ``tests/test_act_profile_gpu.py``).  Rows are ALWAYS projected
independently with a per-row stop test -- the B = 1 semantics of the rollout and of ``eval()``; SpringPendulum's batch-coupled reference projection is never
used here, whatever ``batch_reference`` is: ``act(obs)[i]`` is ``act(obs[i:i+1])``.  The call reads the actor's parameters
and writes its result buffers, nothing else: no env lane, control word, replay row, Philox counter or graph is touched, nothing
is drawn from a generator, and nothing waits for the device.  Data-parallel runs: the calling rank acts alone, no collective.
"""
import functools

import numpy as np
import torch

from .. import ops as hip_ops
from .evaluation import check_budget

_FORMS = {0: None, 1: "tile", 2: "stream", 3: "stream"}


class ActResult(object):
    """What ``act()`` returns: torch tensors on the trainer's device (float32; ``iters`` int32), n rows each.

    ``action`` [n, action_dim]: the completed, projected action (what ``eval()`` would step); ``proposal`` [n, P]: what the
    policy handed to the projection (``EvalTrajectory.proposal``'s definition: after the tanh box or the mean head; EVOPF-v0
    RPODDPG with the fused MLPs: the raw actor output; the Lagrangian baselines have no projection: the proposal IS the action,
    the same tensor); ``iters`` [n]: GRG iterations of the row (0 for the baselines); ``eq_resid`` [n, eq_num] /
    ``ineq_resid`` [n, ineq_num]: the signed residuals at ``action`` (ineq > 0 is a violation; None with ``residuals=False``).
    ``path``: "fused" | "stepwise" ("sweep": a profiled call assembled from K + 1 stepwise calls); ``form``: "tile" | "stream" on
    the fused path, else None.  ``profile``: the ``ProjectionProfile`` of a call with ``profile=True``, else None."""

    FIELDS = ("action", "proposal", "iters", "eq_resid", "ineq_resid")

    def __init__(self, action, proposal, iters, eq_resid=None, ineq_resid=None, path=None, form=None):
        self.action, self.proposal, self.iters, self.eq_resid, self.ineq_resid = action, proposal, iters, eq_resid, ineq_resid
        self.path, self.form, self.profile = path, form, None

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


class ProjectionProfile(object):
    """The projection at every budget 0..K of one ``act(obs, profile=True)`` call.

    ``data``: float32 [K + 1, n, 4] on the trainer's device; plane b, row i = (a0, a1, eq_resid, max_j ineq_resid_j) of what
    ``act(obs, eval_steps=b)`` returns for that row (signed residuals; EVOPF-v0, swept or -- schedule ``profile_evopf=1`` -- from
    the one launch of ``rpo_evopf_project_profile``: the first two action components, and ``eq_resid`` is the row's equality
    residual of largest magnitude with its sign, the lowest index among equal magnitudes).  ``iters``:
    int32 [n], the GRG iterations at the budget K.  Plane 0 is Complete alone and plane 1 is always one step further (the
    loop's first iteration is unconditional), even for a row that was already feasible.  The helpers are plain torch ops on
    ``data``; none of them is on ``act()``'s path."""

    def __init__(self, data, iters):
        self.data, self.iters = data, iters

    @property
    def K(self):
        return self.data.shape[0] - 1

    @property
    def n(self):
        return self.data.shape[1]

    def _plane(self, b):
        if isinstance(b, bool) or int(b) != b or not 0 <= b <= self.K:
            raise ValueError("ProjectionProfile: the budget must be an integer in [0, %d], got %r" % (self.K, b))
        return self.data[int(b)]

    def action(self, b):
        """[n, 2]: the action at budget b (a view)."""
        return self._plane(b)[:, 0:2]

    def eq(self, b):
        """[n]: the signed equality residual at budget b (a view)."""
        return self._plane(b)[:, 2]

    def ineq(self, b):
        """[n]: the largest signed inequality residual at budget b (a view; > 0: violated)."""
        return self._plane(b)[:, 3]

    def iters_at(self, b):
        """int32 [n]: the GRG iterations of ``act(obs, eval_steps=b)``: min(b, iters)."""
        self._plane(b)
        return torch.clamp(self.iters, max=int(b))

    def max_violation(self):
        """[K + 1, n]: max(|eq|, relu(ineq)) per budget and row."""
        return torch.maximum(self.data[:, :, 2].abs(), torch.relu(self.data[:, :, 3]))

    def violation_rate(self, thresh):
        """[K + 1]: the share of rows whose ``max_violation`` is above ``thresh``, per budget."""
        return (self.max_violation() > float(thresh)).to(torch.float32).mean(dim=1)

    def budget(self, tol, share=1.0):
        """The smallest budget b at which at least ``share`` of the rows are within ``tol`` (``max_violation <= tol``), or None
        when no budget up to K reaches it (waits for the device)."""
        within = (self.max_violation() <= float(tol)).sum(dim=1).cpu().numpy()
        ok = np.nonzero(within >= float(share) * self.n)[0]
        return int(ok[0]) if ok.size else None

    def numpy(self):
        """``data`` as a numpy array (waits for the device)."""
        return self.data.detach().cpu().numpy()

    def __repr__(self):
        return "ProjectionProfile(K=%d, n=%d)" % (self.K, self.n)


def profile_max_rows(steps):
    """The largest n whose profile of the budget ``steps`` fits RPO_TRACE_MAX_BYTES."""
    return hip_ops.TRACE_MAX_BYTES // (16 * (int(steps) + 1))


def _projects(tr):
    """The trainer has a projection (RPODDPG / RPOSAC); the Lagrangian baselines step the actor's output as it is."""
    return not hasattr(tr, "_deterministic")


def fused_ok(tr):
    """``rpo_<env>_policy_act`` applies: ``evaluation.fused_ok``'s conditions, with the schedule key ``fused_act``."""
    f = tr.fused
    return bool(tr.schedule.get("fused_act", 1) and f is not None and "actor" in f.descs and hasattr(tr.kernels, "policy_act")
                and _projects(tr) and tr._box_affine is not None and f.descs["actor"].E == 128 and tr.device.type == "cuda")


def profile_kernel(tr):
    """The stand-alone profile launch (``rpo_<env>_project_profile``) of a device trainer as a callable with the signature of
    ``project_profile``, or None where the call sweeps: the kernels' own method (CartSafe-v0, SpringPendulum-v0); on EVOPF-v0 the
    backend's ``evopf_project_profile``, and only under the schedule key ``profile_evopf`` (default 0)."""
    k = tr.kernels
    if tr.device.type != "cuda":
        return None
    if hasattr(k, "project_profile"):
        return k.project_profile
    if (tr.schedule.get("profile_evopf", 0) and getattr(k, "name", None) == "EVOPF-v0"
            and hasattr(tr.backend, "evopf_project_profile")):
        return functools.partial(tr.backend.evopf_project_profile, k)
    return None


def _check(tr, obs, eval_steps, eval_lr, residuals, out, form, profile=False):
    k = tr.kernels
    obs = torch.as_tensor(obs, dtype=torch.float32, device=tr.device)
    if obs.dim() == 1:
        obs = obs[None, :]
    if obs.dim() != 2 or obs.shape[1] != k.obs_dim or obs.shape[0] == 0:
        raise ValueError("act: obs must be [n, %d] with n >= 1 (or [%d]), got %s" % (k.obs_dim, k.obs_dim, tuple(obs.shape)))
    steps, lr = check_budget(tr, eval_steps, eval_lr, "act")
    if form not in _FORMS:
        raise ValueError("act: form must be 0 (by size), 1 (row tile), 2 or 3 (streaming, 16- / 64-row groups), got %r" % (form,))
    if out is not None:
        if not isinstance(out, ActResult) or out.n != obs.shape[0] or out.residuals != bool(residuals):
            raise ValueError("act: out must be an ActResult of the same n (%d) and the same residuals (%r), got %r"
                             % (obs.shape[0], bool(residuals), out))
    if profile:
        n, steps = obs.shape[0], int(steps)
        if not _projects(tr):
            raise ValueError("act: profile=True needs a trainer that projects (RPODDPG / RPOSAC); %s has no projection" % type(tr).__name__)
        if form != 0:
            raise ValueError("act: profile=True has the row-tile launch only; form must be 0, got %r" % (form,))
        if 16 * (steps + 1) * n > hip_ops.TRACE_MAX_BYTES:        # (shape arithmetic: nothing has been allocated)
            raise ValueError("act: profile=True needs %d bytes (%d planes x %d rows x 16), above the cap of %d bytes; at most n = %d "
                             "rows fit at eval_steps = %d" % (16 * (steps + 1) * n, steps + 1, n, hip_ops.TRACE_MAX_BYTES,
                                                             profile_max_rows(steps), steps))
        have = None if out is None or out.profile is None else out.profile.data
        if out is not None and (have is None or tuple(have.shape) != (steps + 1, n, 4)):
            raise ValueError("act: profile=True with out= needs an ActResult whose profile is [%d, %d, 4], got %s"
                             % (steps + 1, n, None if have is None else tuple(have.shape)))
    if obs.stride(1) != 1 or (obs.shape[0] > 1 and obs.stride(0) < k.obs_dim):
        obs = obs.contiguous()                                   # (behind the refusals: they allocate nothing)
    return obs, int(steps), lr


def _sweep(tr, obs, steps, lr, residuals, r, data):
    """The profile from K + 1 stepwise calls (EVOPF-v0, backends without the profile kernels): plane b from ``act(eval_steps=b)``;
    the last call, at the budget K, fills ``r``."""
    for b in range(steps + 1):
        last = b == steps
        x = act(tr, obs, eval_steps=b, eval_lr=lr, residuals=True, out=r if last and residuals else None)
        data[b, :, 0:2].copy_(x.action[:, 0:2])
        data[b, :, 2].copy_(x.eq_resid[:, 0] if x.eq_resid.shape[1] == 1 else _signed_absmax(x.eq_resid))
        data[b, :, 3].copy_(x.ineq_resid.max(dim=1).values)
        if last and not residuals:
            for f in ("action", "proposal", "iters"):
                getattr(r, f).copy_(getattr(x, f))
    r.path, r.form = "sweep", None


def _signed_absmax(x):
    """[n, m] -> [n]: the entry of largest magnitude of every row, with its sign (EVOPF-v0 has many equalities)."""
    return x.gather(1, x.abs().argmax(dim=1, keepdim=True))[:, 0]


def _act_profile(tr, obs, steps, lr, residuals, out):
    n, k = obs.shape[0], tr.kernels
    r = out if out is not None else ActResult.empty(tr, n, residuals)
    data = out.profile.data if out is not None else torch.empty(steps + 1, n, 4, device=tr.device)
    project_profile = profile_kernel(tr)
    with torch.no_grad():
        if fused_ok(tr) and hasattr(k, "policy_act_profile"):
            scale, base = tr._box_affine
            k.policy_act_profile(tr.fused.descs["actor"], tr._gauss_policy, scale, base, obs, r.action, r.proposal, r.iters,
                                 r.eq_resid, r.ineq_resid, tr._box_lo, tr._box_hi, steps, lr, tr.corr_eps, tr.corr_momentum, data)
            r.path, r.form = "fused", "tile"
        elif project_profile is not None:
            obs = obs.contiguous()
            ap = tr._eval_partial(obs)
            r.proposal.copy_(ap.reshape(r.proposal.shape))
            # (_act_kw: RPODDPG's ap_is_raw on EVOPF-v0 with the fused MLPs; empty wherever project_profile takes no such keyword)
            project_profile(obs, ap, r.action, r.iters, steps, lr, tr.corr_eps, tr.corr_momentum, data, **tr._act_kw)
            if residuals:
                k.resid(obs, r.action, r.eq_resid, r.ineq_resid)
            r.path, r.form = "stepwise", None
        else:
            _sweep(tr, obs, steps, lr, residuals, r, data)
    r.profile = ProjectionProfile(data, r.iters)
    return r


def act(tr, obs, eval_steps=None, eval_lr=None, residuals=True, out=None, form=0, profile=False):
    """See ``RPOTrainerBase.act``."""
    obs, steps, lr = _check(tr, obs, eval_steps, eval_lr, residuals, out, form, profile)
    if profile:
        return _act_profile(tr, obs, steps, lr, residuals, out)
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
            r.path, r.form, r.profile = "fused", _FORMS[form] or ("stream" if stream else "tile"), None
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
    r.path, r.form, r.profile = "stepwise", None, None
    return r
