"""Many-episode policy evaluation: ``RPOTrainerBase.evaluate()``.

``eval()`` is the reference's protocol (rpo_ddpg.py:207-264): 10 episodes, the 10-tuple of (mean, std) pairs, driven from
the host one env step at a time.  ``evaluate()`` runs the same policy, projection and horizon on any number of independent
episodes and returns per-episode arrays (``EvalResult``).  Two paths, chosen from what the trainer can observe:

* **fused** -- RPODDPG / RPOSAC on CartSafe-v0 and SpringPendulum-v0 with the fused MLP kernels: ``rpo_<env>_evaluate``
  (csrc/evaluate.hip) runs actor -> head -> Complete -> GRG -> env step -> per-episode accumulators for up to ``steps`` env
  steps per launch, ``ceil(horizon / steps)`` launches back to back, no host synchronisation in between.
* **fused, EVOPF-v0** -- opt-in by schedule ``fused_eval_evopf=1`` (default 0): ``rpo_evopf_evaluate`` (csrc/evopf_eval.hip) does
  the same for RPODDPG / RPOSAC with the fused 256-wide actor, four episodes per workgroup (``fused_evopf_ok``); ``record=``,
  ``obs_noise=``, curve mode / ``keep_best``, single-launch sweeps and ``act()`` stay stepwise there.
* **stepwise** -- everything else (EVOPF-v0 by default, the Lagrangian baselines, ``fused_mlp=0``, the CPU oracle backend, and
  schedule ``fused_eval=0``): ``_eval_action`` + ``step(auto_reset=False)`` + ``rpo_eval_accumulate`` per env step, or the
  same update in torch ops on a backend without that kernel.

Both paths compute the same bits (``tests/test_evaluate_gpu.py``).  The evaluation owns its vector env, its ``ctrl`` and
its buffers: no trainer state is read-modified-written, so training after an ``evaluate()`` call is the training without it.
Data-parallel runs: ``evaluate()`` runs on the calling rank alone, with no collective (the replicas' networks are
identical, so every rank would compute the same result); call it on one rank.

Per-step record (``evaluate(record=True | k)``): both paths write one row per live lane and step into a trace buffer
[horizon, k, W] (``RPO_TRACE_*``; the fused kernel's REC instances, ``rpo_eval_record`` or ``record_torch`` on the stepwise
path), returned as ``EvalResult.trajectory`` (``EvalTrajectory``).  The per-episode arrays do not depend on it.

Per-constraint report (``evaluate(constraints=True)``): both paths keep one row per episode on the device (``RPO_CON_*``: the
maximum of every inequality's violation and of every |equality residual| over the episode's live steps, and the number of
live steps on which each inequality exceeds ``viol_thresh``), folded from the values of the step's transition row -- by the
fused kernel's CON instances, ``rpo_eval_constraints`` or ``constraints_torch`` on the stepwise path -- and returned as
``EvalResult.constraints`` (``ConstraintReport``).  Every other result is the same bits with and without it.

Observation noise (``evaluate(obs_noise=sigma)``): at every step the actor and the projection read ``o + sigma * z`` while the
env steps the true state.  ``z(i, s, q)`` for episode i, evaluation step s, column q is the Box-Muller normal of words 0 and 1
of Philox with key = the evaluation's seed and counter (i, s, RPO_STREAM_EVAL_OBS + 0x100 q, 0) -- ``philox_normal(seed,
id_base 0, salt s, that tag)`` of every backend -- and the sum is an f32 multiply, then an f32 add.  The fused kernel's NOISE
instances add it to their staged tile (``rpo_<env>_evaluate_noisy``); the stepwise path fills a buffer of its own per step
(``rpo_eval_obs_noise``, or ``obs_noise_torch``) and hands it to ``_eval_action(obs=)`` and the record.  Both paths compute
the same bits; None, 0 and all-zero run the clean evaluation's launches.  ``eval()``, curve mode and ``act()`` never see noise.

Budget sweeps (``evaluate_budgets(episodes, eval_steps=[...])`` -> ``BudgetSweep``): B projection budgets on the SAME initial
states, group g being bit for bit the ``evaluate()`` call with ``eval_steps[g]`` / ``eval_lr[g]`` and the shared seed.  On the
fused path the B groups run side by side as B x episodes lanes of one launch sequence (``rpo_<env>_evaluate_budgets``: the fused
kernel's BUD instances read the budget and the step size per lane); every other configuration runs the B calls ("sweep").

Policy sweeps (``evaluate_policies([None, p, trainer.best, "b.npz"], episodes)`` -> ``PolicySweep``): P actors on the SAME initial
states, group g being bit for bit the ``evaluate()`` call under ``using_policy(policies[g])`` with the shared seed.  On the fused
path the P actor spans are gathered into one bank [P, span] and the groups run side by side, each padded to whole 64-lane tiles,
as P x padded lanes of one launch sequence (``rpo_<env>_evaluate_policies``: the fused kernel's POL instances take their
group's actor out of the bank); every other configuration runs the P calls ("sweep").  The live actor is never written on the
fused path and is back bit for bit after the sweep path.

Noise sweeps (``evaluate_noise(episodes, obs_noise=[0, 0.01, 0.05, [...]])`` -> ``NoiseSweep``): S sensor-noise levels on the SAME
initial states AND the same draws, group g being bit for bit the ``evaluate()`` call with ``obs_noise=levels[g]`` and the shared
seed -- ``evaluate()`` keys episode i's draw by (seed, i, step, column), so the S calls already share their z.  On the fused path
the groups run side by side, each padded to whole 64-lane tiles, as S x padded lanes of one launch sequence
(``rpo_<env>_evaluate_noise_sweep``: the fused kernel's NSW instances read their group's sigma out of a device table and key the
draw by the episode within the group, not by the lane); every other configuration runs the S calls ("sweep").

The OPF controller (``evaluate_opf(episodes, seed=...)`` -> ``EvalResult`` with ``path`` "opf", EVOPF-v0 on a GPU only): the stepwise
loop on ``evaluate()``'s episodes -- the same ``_initial_env``, so the same days and initial states of charge under the same seed --
with the single-step AC-OPF of the lane's observation in the policy's place (``_run_stepwise(producer=)``: one launch of
``rpo_evopf_opf_free``, or of ``rpo_evopf_opf`` with idle batteries, straight into the env's action rows), a hard-feasible
baseline whose per-episode differences to a policy's result are paired; ``opf_iters`` / ``opf_converged`` [episode, step].

The safety filter (``evaluate_filtered(episodes, seed=...)`` -> ``EvalResult`` with ``path`` "filtered", EVOPF-v0 on a GPU only): the
same loop and episodes with the trainer's own ``_eval_action`` (actor + GRG projection) followed by one launch of
``rpo_evopf_nearest`` on that action -- the feasible dispatch nearest to what the policy asked for -- into the env's action rows;
where the solve did not converge the step takes the policy's own action (``fallback="policy"``, a device select on the converged
flag) or the solver's last iterate (``fallback="last"``); ``filter_iters`` / ``filter_converged`` / ``filter_distance`` [episode,
step].  "policy", "policy + filter" and "OPF" on one seed are paired.

Curve mode (trainer argument ``eval_episodes=N``): the training loop enqueues such an evaluation where it would call
``eval()`` and does not wait for it; ``CurveRunner`` below, results in ``trainer.eval_curve`` (``EvalCurve``).  Curve mode
does not record trajectories and produces no per-constraint reports.  With the trainer argument ``keep_best`` every point's
row is compared with the incumbent's on the device right behind its summary (``rpo_eval_keep_best``, or ``keep_best_torch``)
and the actor's parameters of a winning point are kept: ``trainer.best`` (``BestPolicy``), ``restore_best()``,
``using_best()``.
"""
import collections
import contextlib
import math
import os

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
    episode; ``nonfinite``: a live step produced a non-finite reward or violation.  ``path``: "fused" or "stepwise".
    ``trajectory`` / ``constraints``: the ``EvalTrajectory`` of ``record=`` / the ``ConstraintReport`` of ``constraints=True``,
    else None.  ``obs_noise``: the float32 sigma vector [obs_dim] of ``obs_noise=``, None for a clean evaluation.
    ``evaluate_opf`` (``path`` "opf"; ``proj_iters`` sums the solver's iterations): ``opf_iters`` int32 / ``opf_converged`` bool
    [episode, step], the solver's iteration count and stop flag of every live step (0 / False past the episode's end); None
    otherwise.  ``evaluate_filtered`` (``path`` "filtered"; ``proj_iters`` sums the filter's iterations): ``filter_iters`` int32 /
    ``filter_converged`` bool / ``filter_distance`` float32 [episode, step], the safety filter's iteration count, stop flag and
    objective at exit of every live step (0 / False past the episode's end); None otherwise.  ``days``: int array [episodes], the day of ``scenarios=`` every episode played; None without scenarios."""

    FIELDS = ("ret", "length", "mean_ineq", "mean_eq", "max_ineq", "max_eq", "viol_steps", "proj_iters", "nonfinite")

    def __init__(self, acc, path, horizon, seed, trajectory=None, constraints=None, obs_noise=None):
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
        self.trajectory = trajectory
        self.constraints = constraints
        self.obs_noise = None if obs_noise is None else np.array(obs_noise, dtype=np.float32)
        self.opf_iters = self.opf_converged = None               # evaluate_opf: [episode, step]
        self.filter_iters = self.filter_converged = self.filter_distance = None   # evaluate_filtered: [episode, step]
        self.days = None                                         # scenarios=: int64 [episodes], the day each episode played

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


class EvalTrajectory(object):
    """The per-step record of ``evaluate(record=...)``: numpy arrays indexed [episode, step, ...] over the recorded episodes
    (the first ``episodes`` of the evaluation) and ``horizon`` steps.

    ``obs`` [., ., obs_dim]: the observation the actor and the projection read -- with ``evaluate(obs_noise=)`` the NOISY one,
    what the policy saw, not the state the env stepped (reward, done, ineq and eq are the true state's); ``proposal`` [., ., partial_dim]: the partial
    action the policy handed to the projection, after the tanh box or the mean head (EVOPF-v0 RPODDPG with the fused MLPs hands
    over the raw actor output -- its state-dependent box is applied inside the projection kernel -- and that is what is
    recorded; the Lagrangian baselines have no projection: the proposal is the action); ``action`` [., ., action_dim]: the
    completed, projected action that was stepped; ``reward``; ``done``; ``ineq`` / ``eq``: the step's max inequality violation
    / max |equality residual| as the accumulators received them; ``iters``: GRG iterations of the step (0 without a
    projection); ``valid``: step < length[episode].  Floats are the device's float32 bits; entries of non-valid steps are
    zero.  ``length``: the recorded episodes' lengths; ``viol_thresh``: the threshold of ``EvalResult.viol_steps``."""

    ARRAYS = ("obs", "proposal", "action", "reward", "done", "ineq", "eq", "iters", "valid", "length")

    def __init__(self, viol_thresh, **arrays):
        for name in self.ARRAYS:
            setattr(self, name, np.asarray(arrays[name]))
        self.viol_thresh = float(viol_thresh)

    @classmethod
    def from_trace(cls, trace, dims, length, viol_thresh):
        """trace: the device buffer [T, R, W] as numpy (layout RPO_TRACE_*); dims: (obs_dim, partial_dim, action_dim)."""
        O, P, A = dims
        head, W = hip_ops.trace_layout(O, P, A)
        t = np.ascontiguousarray(np.asarray(trace, dtype=np.float32).reshape(trace.shape[0], -1, W).transpose(1, 0, 2))
        length = np.asarray(length, dtype=np.int64)
        tail = {k: t[:, :, head + c].copy() for k, c in hip_ops.TRACE_SLOT.items()}
        return cls(viol_thresh, obs=t[:, :, :O].copy(), proposal=t[:, :, O:O + P].copy(), action=t[:, :, O + P:O + P + A].copy(),
                   reward=tail["reward"], done=tail["done"] != 0, ineq=tail["ineq"], eq=tail["eq"],
                   iters=t[:, :, O + P + A].astype(np.int32), valid=np.arange(t.shape[1])[None, :] < length[:, None],
                   length=length)

    @property
    def episodes(self):
        return self.obs.shape[0]

    @property
    def horizon(self):
        return self.obs.shape[1]

    def episode(self, i):
        """The arrays of episode i, trimmed to its length: a dict name -> [length[i], ...]."""
        n = int(self.length[i])
        return {name: getattr(self, name)[i, :n] for name in self.ARRAYS if name not in ("valid", "length")}

    def violations(self):
        """The (episode, step) index pairs [m, 2] of the valid steps with ineq > viol_thresh (the steps ``viol_steps`` counts)."""
        return np.argwhere(self.valid & (self.ineq > np.float32(self.viol_thresh)))

    def save(self, path):
        """One .npz with every array (and viol_thresh); ``EvalTrajectory.load`` reads it back."""
        with open(path, "wb") as f:
            np.savez(f, viol_thresh=np.float64(self.viol_thresh), **{name: getattr(self, name) for name in self.ARRAYS})

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            return cls(float(z["viol_thresh"]), **{name: z[name] for name in cls.ARRAYS})

    def opf_gap(self, env, tol=1e-4, max_iters=40, pe="policy"):
        """The optimality gap of every recorded step of an EVOPF-v0 evaluation (``opf_gap`` below) -> ``OpfGap``."""
        return opf_gap(self, env, tol=tol, max_iters=max_iters, pe=pe)

    def __repr__(self):
        return "EvalTrajectory(episodes=%d, horizon=%d, steps=%d)" % (self.episodes, self.horizon, int(self.valid.sum()))


class OpfGap(object):
    """Optimality gaps of a recorded EVOPF-v0 evaluation (``EvalTrajectory.opf_gap``): float64 / bool numpy arrays indexed
    [episode, step].

    ``cost_policy``: ``obj_fn`` of the recorded action (NaN only where the step is not valid); ``cost_opt``: the cost of the
    single-step AC-OPF at that step's observation with the recorded action's battery power pe -- the battery schedule is the
    policy's on both sides, so the reward difference is the cost difference; ``gap`` = (cost_policy - cost_opt) / cost_opt;
    ``converged``: the solver met its stop test (False on non-valid steps).  ``cost_opt`` and ``gap`` are NaN where the solver did
    not converge (infeasible single-step problems exist) or the step is not valid.  ``violation``: the step's max(ineq, eq) of the
    policy's action as recorded.  A NEGATIVE gap is possible and is not clipped: the optimum is taken over feasible dispatches,
    and a policy action that violates a constraint can be cheaper than any of them -- ``feasible_only(viol_thresh)`` masks
    those steps."""

    ARRAYS = ("cost_policy", "cost_opt", "gap", "converged", "valid", "violation")

    def __init__(self, tol, max_iters, **arrays):
        for name in self.ARRAYS:
            setattr(self, name, np.asarray(arrays[name]))
        self.tol, self.max_iters = float(tol), int(max_iters)

    def mean(self):
        """Mean gap over the steps that have one (NaN if none has)."""
        return float(np.nanmean(self.gap)) if np.isfinite(self.gap).any() else float("nan")

    def quantile(self, q):
        return float(np.nanquantile(self.gap, q)) if np.isfinite(self.gap).any() else float("nan")

    def converged_rate(self):
        """Share of the valid steps whose OPF converged."""
        return float(self.converged[self.valid].mean()) if self.valid.any() else float("nan")

    def feasible_only(self, viol_thresh):
        """A copy whose ``gap`` is NaN also where the policy's own action violates a constraint by more than ``viol_thresh``."""
        keep = self.violation <= float(viol_thresh)
        arrays = {name: getattr(self, name).copy() for name in self.ARRAYS}
        arrays["gap"] = np.where(keep, self.gap, np.nan)
        return OpfGap(self.tol, self.max_iters, **arrays)

    def save(self, path):
        with open(path, "wb") as f:
            np.savez(f, tol=np.float64(self.tol), max_iters=np.int64(self.max_iters), **{name: getattr(self, name) for name in self.ARRAYS})

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            return cls(float(z["tol"]), int(z["max_iters"]), **{name: z[name] for name in cls.ARRAYS})

    def __repr__(self):
        return "OpfGap(steps=%d, converged=%.3f, mean gap=%.4g)" % (int(self.valid.sum()), self.converged_rate(), self.mean())


def opf_gap(trajectory, env, tol=1e-4, max_iters=40, pe="policy"):
    """For every valid step of ``trajectory`` (``trainer.evaluate(..., record=...)`` on EVOPF-v0): ``env.opf`` at the step's
    recorded observation with the recorded action's pe, in one launch over all steps, against ``env.obj_fn`` of the recorded
    action -> ``OpfGap``.  ``env``: an EVOPFEnv on a GPU device (NotImplementedError otherwise, with the reason).  With
    ``evaluate(obs_noise=)`` the recorded observation is the noisy one the policy saw.  ``pe="free"``: against the optimum over the
    full action, ``env.opf(obs, pe="free")`` -- ``cost_policy`` and ``cost_opt`` then hold ``obj_fn + pe_cost . pe`` with the
    default ``pe_cost`` ((we / wg) * the step's price: minus the step's reward over wg) of the recorded action and of the free
    optimum in the recorded observation, and ``gap`` is their DIFFERENCE (that objective has no sign to divide by)."""
    if pe not in ("policy", "free"):
        raise ValueError("opf_gap: pe must be 'policy' (the recorded battery power on both sides) or 'free', got %r" % (pe,))
    if not hasattr(env, "opf"):
        raise TypeError("opf_gap: env must be an EVOPFEnv, got %s" % type(env).__name__)
    obs, action, valid = np.asarray(trajectory.obs), np.asarray(trajectory.action), np.asarray(trajectory.valid, dtype=bool)
    if obs.ndim != 3 or obs.shape[2] != env.state_dim or action.shape[2] != env.action_dim:
        raise ValueError("opf_gap: the trajectory is not one of EVOPF-v0 (obs %s, action %s)" % (obs.shape, action.shape))
    shape = valid.shape
    cost_policy, cost_opt = np.full(shape, np.nan), np.full(shape, np.nan)
    converged = np.zeros(shape, dtype=bool)
    if valid.any():
        o = np.ascontiguousarray(obs[valid], dtype=np.float32)
        a = np.ascontiguousarray(action[valid], dtype=np.float32)
        if pe == "free":
            out = env.opf(o, pe="free", tol=tol, max_iters=max_iters)
            res = out.numpy()
            policy = env.obj_fn(a) + (out.pe_cost * env._t(a[:, -env.ne:])).sum(dim=1)
            cost_policy[valid] = policy.detach().cpu().numpy().astype(np.float64)
            res["cost"] = res["objective"]
        else:
            res = env.opf(o, pe=a[:, -env.ne:], tol=tol, max_iters=max_iters).numpy()
            cost_policy[valid] = env.obj_fn(a).detach().cpu().numpy().astype(np.float64)
        converged[valid] = res["converged"]
        cost_opt[valid] = np.where(res["converged"], res["cost"].astype(np.float64), np.nan)
    with np.errstate(all="ignore"):
        # (free pe: the objective carries pe_cost . pe and has no sign; the gap is the difference, in units of obj_fn)
        gap = cost_policy - cost_opt if pe == "free" else (cost_policy - cost_opt) / cost_opt
    violation = np.where(valid, np.maximum(np.asarray(trajectory.ineq, dtype=np.float64), np.asarray(trajectory.eq, dtype=np.float64)), np.nan)
    return OpfGap(tol, max_iters, cost_policy=cost_policy, cost_opt=cost_opt, gap=gap, converged=converged, valid=valid,
                  violation=violation)


class ConstraintReport(object):
    """The per-constraint report of ``evaluate(constraints=True)``: numpy arrays indexed [episode, constraint].

    ``ineq_max`` [n, ineq_num]: the maximum over the episode's live steps of the step's violation of inequality j, as the
    transition row carries it (clamped at 0; a NaN propagates), the device's float32 bits widened; ``ineq_steps``
    [n, ineq_num] int64: the live steps on which that value is > ``viol_thresh`` (the threshold and comparison of
    ``EvalResult.viol_steps``); ``eq_max`` [n, eq_num]: the maximum of |eq_j|.  A step counts exactly when it counts for
    ``EvalResult.length``; ``length``: those lengths.  ``names`` / ``eq_names``: the env's names of the constraints.
    ``ineq_max.max(1)`` is ``max_ineq``, ``eq_max.max(1)`` is ``max_eq`` and
    ``ineq_steps.max(1) <= viol_steps <= ineq_steps.sum(1)`` (while no violation is a NaN)."""

    ARRAYS = ("ineq_max", "ineq_steps", "eq_max", "length")

    def __init__(self, viol_thresh, names, eq_names, **arrays):
        for name in self.ARRAYS:
            setattr(self, name, np.asarray(arrays[name]))
        self.viol_thresh = float(viol_thresh)
        self.names, self.eq_names = tuple(str(x) for x in names), tuple(str(x) for x in eq_names)
        if len(self.names) != self.ineq_max.shape[1] or len(self.eq_names) != self.eq_max.shape[1]:
            raise ValueError("ConstraintReport: %d / %d names for %d inequalities / %d equalities"
                             % (len(self.names), len(self.eq_names), self.ineq_max.shape[1], self.eq_max.shape[1]))

    @classmethod
    def from_rows(cls, con, ineq_num, eq_num, length, viol_thresh, names=None, eq_names=None):
        """con: the device buffer [n, W] as numpy (layout RPO_CON_*)."""
        con = np.asarray(con, dtype=np.float32).reshape(-1, hip_ops.con_width(ineq_num, eq_num))
        names = ["ineq[%d]" % j for j in range(ineq_num)] if names is None else names
        eq_names = ["eq[%d]" % j for j in range(eq_num)] if eq_names is None else eq_names
        return cls(viol_thresh, names, eq_names, ineq_max=con[:, :ineq_num].astype(np.float64),
                   ineq_steps=con[:, ineq_num:2 * ineq_num].astype(np.int64),
                   eq_max=con[:, 2 * ineq_num:2 * ineq_num + eq_num].astype(np.float64), length=np.asarray(length, dtype=np.int64))

    @property
    def episodes(self):
        return self.ineq_max.shape[0]

    def rate(self):
        """Per inequality: the fraction of the evaluated env steps on which it exceeds ``viol_thresh`` [ineq_num]."""
        return self.ineq_steps.sum(0) / float(self.length.sum())

    def worst(self, k=5):
        """The k inequalities with the most violating steps over all episodes (ties: the lower index first), as tuples
        (index, name, steps, max): ``ineq_steps.sum(0)[index]`` and ``ineq_max[:, index].max()``."""
        steps = self.ineq_steps.sum(0)
        order = np.argsort(-steps, kind="stable")[:max(0, int(k))]
        return [(int(j), self.names[j], int(steps[j]), float(self.ineq_max[:, j].max())) for j in order]

    def save(self, path):
        """One .npz with every array, the names and viol_thresh; ``ConstraintReport.load`` reads it back."""
        with open(path, "wb") as f:
            np.savez(f, viol_thresh=np.float64(self.viol_thresh), names=np.array(self.names), eq_names=np.array(self.eq_names),
                     **{name: getattr(self, name) for name in self.ARRAYS})

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            return cls(float(z["viol_thresh"]), [str(x) for x in z["names"]], [str(x) for x in z["eq_names"]],
                       **{name: z[name] for name in cls.ARRAYS})

    def __repr__(self):
        w = self.worst(1)
        return "ConstraintReport(episodes=%d, inequalities=%d, equalities=%d, violated=%d, worst=%s)" % (
            self.episodes, len(self.names), len(self.eq_names), int((self.ineq_steps.sum(0) > 0).sum()),
            "%s: %d steps" % (w[0][1], w[0][2]) if w and w[0][2] else None)


def _nanmax_torch(a, b):
    """rpo_eval_dev::nanmax: torch.maximum's NaN propagation, and the FIRST operand where they compare equal (signed zeros)."""
    return torch.where(a != a, a, torch.where(b != b, b, torch.where(b > a, b, a)))


def constraints_torch(rows, cols, step, viol_thresh, acc, con):
    """``rpo_eval_constraints`` in torch ops (backends without the kernel: the CPU oracle): the step's ineq_viol / eq_viol
    columns into con [n, W] for the lanes that are live BEFORE ``accumulate_torch`` of the same step; step 0 writes every row
    from scratch."""
    n = acc.shape[0]
    rows = rows[:n]
    ineq = rows[:, cols["ineq_viol"][0]:cols["ineq_viol"][1]]
    eq = rows[:, cols["eq_viol"][0]:cols["eq_viol"][1]].abs()
    ni, ne = ineq.shape[1], eq.shape[1]
    if step == 0:
        con.zero_()
    old = con.clone()
    new = torch.zeros_like(con)
    new[:, :ni] = _nanmax_torch(old[:, :ni], ineq)
    new[:, ni:2 * ni] = old[:, ni:2 * ni] + (ineq > viol_thresh).to(con.dtype)
    new[:, 2 * ni:2 * ni + ne] = _nanmax_torch(old[:, 2 * ni:2 * ni + ne], eq)
    if step > 0:
        live = (acc[:, _WORD].view(torch.int32) & _ALIVE) != 0
        new = torch.where(live[:, None], new, old)
    con.copy_(new)


def record_torch(rows, cols, obs, proposal, action, iters, step, acc, trace):
    """``rpo_eval_record`` in torch ops (backends without the kernel: the CPU oracle): row (step, i), i < R, of trace
    [T, R, W] for the lanes that are live BEFORE ``accumulate_torch`` of the same step."""
    n, R = acc.shape[0], trace.shape[1]
    O, A = obs.shape[1], action.shape[1]
    prop = proposal.reshape(n, -1)
    P = prop.shape[1]
    head, _ = hip_ops.trace_layout(O, P, A)
    rows = rows[:R]
    row = torch.zeros_like(trace[step])
    row[:, :O] = obs[:R]
    row[:, O:O + P] = prop[:R]
    row[:, O + P:O + P + A] = action[:R]
    if iters is not None:
        row[:, O + P + A] = iters[:R].to(row.dtype)
    slot = hip_ops.TRACE_SLOT
    row[:, head + slot["reward"]] = rows[:, cols["reward"][0]]
    row[:, head + slot["done"]] = rows[:, cols["done"][0]]
    row[:, head + slot["ineq"]] = rows[:, cols["ineq_viol"][0]:cols["ineq_viol"][1]].max(dim=1).values
    row[:, head + slot["eq"]] = rows[:, cols["eq_viol"][0]:cols["eq_viol"][1]].abs().max(dim=1).values
    if step > 0:
        live = (acc[:R, _WORD].view(torch.int32) & _ALIVE) != 0
        row = torch.where(live[:, None], row, trace[step])
    trace[step] = row


def obs_noise_torch(tr, obs, sigma, seed, step, out):
    """``rpo_eval_obs_noise`` from the backend's ``philox_normal`` and torch ops (backends without the kernel: the CPU oracle):
    out[:, q] = obs[:, q] + sigma[q] * z(., step, q), an unfused multiply and add; a column with sigma[q] == 0 is copied.
    obs, out [n, obs_dim]; sigma: float32 numpy [obs_dim]."""
    n = obs.shape[0]
    out.copy_(obs)
    z = torch.zeros(n, dtype=torch.float32, device=obs.device)
    for q in range(obs.shape[1]):
        if sigma[q] == 0:
            continue
        tr.backend.philox_normal(z, seed, 0, int(step), hip_ops.STREAM_EVAL_OBS + 0x100 * q)
        out[:, q] = obs[:, q] + z * float(sigma[q])


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


#: episodes up to which FusedNets.forward runs a wide network layer by layer (csrc/mlp_gemm.h: gemm_path_ok)
_GEMM_PATH_ROWS = 16384


def fused_evopf_ok(tr, episodes, record=0, sigma=None):
    """The fused EVOPF-v0 evaluation kernel (``rpo_evopf_evaluate``) applies to this ``evaluate()`` call: schedule
    ``fused_eval_evopf`` (default 0) and ``fused_eval``, RPODDPG / RPOSAC with the fused 256-wide actor on an env with a
    state-dependent box whose backend has ``evopf_evaluate`` for it, no record, no observation noise -- and the stepwise path's actor
    forward being the layer-by-layer launches whose summation order the kernel reproduces: at most 16384 episodes and the
    tunings ``mlp_gemm`` / ``gemm_ksplit`` at their defaults.  ``CurveRunner`` keeps ``fused_ok``: curve mode stays stepwise."""
    f = tr.fused
    if not (tr.schedule.get("fused_eval_evopf", 0) and tr.schedule.get("fused_eval", 1)) or tr.device.type != "cuda":
        return False
    if f is None or "actor" not in f.descs or hasattr(tr, "_deterministic"):
        return False
    if not hasattr(tr.backend, "evopf_evaluate") or getattr(tr.kernels, "name", None) != "EVOPF-v0":
        return False
    d = f.descs["actor"]
    if tr._box_affine is not None or d.E != 256 or d.H != 256 or episodes > _GEMM_PATH_ROWS or record or sigma is not None:
        return False
    return hip_ops.tuning.get("mlp_gemm") == 1 and hip_ops.tuning.get("gemm_ksplit") == 1


def check_episodes(episodes, what="evaluate: episodes"):
    try:
        ok = not isinstance(episodes, bool) and int(episodes) == episodes and episodes >= 1
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("%s must be an integer >= 1, got %r" % (what, episodes))
    return int(episodes)


def check_record(record, episodes):
    """``record`` of evaluate() -> the number of recorded episodes: True: all; an integer 1 <= k <= episodes: k; False / 0: 0."""
    if record is True:
        return episodes
    if record is False:
        return 0
    try:
        ok = int(record) == record and 0 <= record <= episodes
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("evaluate: record must be True, False or an integer in [0, episodes = %d], got %r" % (episodes, record))
    return int(record)


def check_constraints(constraints):
    """``constraints`` of evaluate(): a bool (ValueError otherwise)."""
    if not isinstance(constraints, (bool, np.bool_)):
        raise ValueError("evaluate: constraints must be True or False, got %r" % (constraints,))
    return bool(constraints)


def check_obs_noise(obs_noise, obs_dim):
    """``obs_noise`` of evaluate() -> None (None) or the float32 sigma vector [obs_dim]: a number >= 0 is broadcast, a sequence
    of ``obs_dim`` numbers >= 0 is taken as it is.  ValueError for a negative or non-finite entry, a bool (alone or as an
    entry), another length or anything that is no number."""
    if obs_noise is None:
        return None
    bad = ValueError("evaluate: obs_noise must be None, a number >= 0 or %d numbers >= 0, got %r" % (obs_dim, obs_noise))
    if isinstance(obs_noise, (bool, np.bool_, str, bytes)):
        raise bad
    if isinstance(obs_noise, torch.Tensor):
        obs_noise = obs_noise.detach().cpu().numpy()
    try:
        if np.ndim(obs_noise) and any(isinstance(x, (bool, np.bool_)) for x in np.asarray(obs_noise, dtype=object).reshape(-1)):
            raise bad
        a = np.asarray(obs_noise)
        if a.dtype == np.bool_ or a.dtype.kind not in "fiu":
            raise bad
        a = a.astype(np.float64)
    except (TypeError, ValueError):
        raise bad
    if a.ndim == 0:
        a = np.full(obs_dim, float(a))
    if a.shape != (obs_dim,) or not np.all(np.isfinite(a)) or np.any(a < 0):
        raise bad
    with np.errstate(over="ignore"):
        sigma = a.astype(np.float32)
    if not np.all(np.isfinite(sigma)):                           # (a float64 above the float32 range)
        raise bad
    return sigma


def check_budget(tr, eval_steps, eval_lr, what="evaluate"):
    """The per-call projection overrides of ``evaluate()`` / ``act()`` -> (eval_steps, eval_lr) with None replaced by the
    trainer's: ``eval_steps`` an integer >= 0, ``eval_lr`` a finite number (ValueError otherwise)."""
    steps = tr.eval_steps if eval_steps is None else eval_steps
    try:
        ok = not isinstance(steps, bool) and int(steps) == steps and steps >= 0
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("%s: eval_steps must be an integer >= 0, got %r" % (what, eval_steps))
    lr = tr.eval_lr if eval_lr is None else eval_lr
    try:
        lr = float(lr)
    except (TypeError, ValueError):
        lr = float("nan")
    if not math.isfinite(lr):
        raise ValueError("%s: eval_lr must be a finite number, got %r" % (what, eval_lr))
    return int(steps), lr


def fresh_seed(tr):
    """The seed of an ``evaluate()`` / ``evaluate_budgets()`` call without one: fresh initial states at every call, like eval(),
    from the trainer seed and a call counter (host-side only), which it advances."""
    calls = getattr(tr, "_evaluate_calls", 0)
    tr._evaluate_calls = calls + 1
    return int(((tr.seed ^ 0xE7A1E7A1) + 0x9E3779B97F4A7C15 * (calls + 1)) & (2 ** 63 - 1))


def check_horizon(tr, horizon, what="evaluate"):
    """``horizon`` of the evaluate*() calls -> the number of env steps (None: ``default_horizon``); ValueError otherwise."""
    if horizon is not None and (isinstance(horizon, bool) or int(horizon) != horizon or horizon < 1):
        raise ValueError("%s: horizon must be an integer >= 1, got %r" % (what, horizon))
    H = int(horizon) if horizon is not None else default_horizon(tr)
    if H >= 1 << 24:
        raise ValueError("%s: horizon must be below 2^24 (lengths are counted exactly in float32), got %d" % (what, H))
    return H


def check_init_states(tr, init_states, n, what="evaluate"):
    """``init_states`` of the evaluate*() calls -> None or the float32 tensor [n, internal_dim] on the trainer's device."""
    if init_states is None:
        return None
    init_states = torch.as_tensor(init_states, dtype=torch.float32, device=tr.device)
    if tuple(init_states.shape) != (n, tr.kernels.internal_dim):
        raise ValueError("%s: init_states must be [episodes, internal_dim] = [%d, %d], got %s"
                         % (what, n, tr.kernels.internal_dim, tuple(init_states.shape)))
    return init_states


def check_scenarios(tr, scenarios, n, what="evaluate"):
    """``scenarios`` of evaluate() / evaluate_opf() -> (None, None), or ((table, day) on the trainer's device: the vector env's
    ``scenario``, days int64 numpy [n]): episode e plays day e % len(scenarios).  NotImplementedError naming EVOPF-v0 on another
    env, backend or device; TypeError for anything but a ``Scenarios``."""
    if scenarios is None:
        return None, None
    if getattr(tr.kernels, "name", None) != "EVOPF-v0" or not isinstance(tr.kernels, hip_ops.EvopfKernels) \
            or tr.device.type != "cuda":
        raise NotImplementedError("%s: scenarios are played by the HIP step kernel of EVOPF-v0 on a GPU (rpo_evopf_step_scenario) "
                                  "only; this trainer's env is %s (%s) on %s"
                                  % (what, getattr(tr.kernels, "name", "?"), type(tr.kernels).__name__, tr.device))
    from ..env.electrical_grid.scenarios import Scenarios
    if not isinstance(scenarios, Scenarios):
        raise TypeError("%s: scenarios must be a Scenarios, got %s" % (what, type(scenarios).__name__))
    days = np.arange(n, dtype=np.int64) % len(scenarios)
    return (scenarios.table(tr.device), torch.as_tensor(days.astype(np.int32), device=tr.device)), days


def _make_vec(tr, n, seed, scenario=None):
    kw = {} if scenario is None else dict(scenario=scenario)
    return tr.base_env.make_vec(n, seed=seed, env_id_base=0, max_episode_steps=tr.max_episode_steps, device=tr.device,
                                stats_cap=2, viol_thresh=tr.vec.viol_thresh, **kw)


def _initial_env(tr, n, seed, init_states, scenario=None):
    """The initial env of ``evaluate()``: n lanes reset under ``seed`` -- or to hour 0 of their day of ``scenario`` -- then the
    injection of ``init_states``."""
    v = _make_vec(tr, n, seed, scenario)
    v.reset()
    if init_states is not None:
        v.set_internal(init_states)
    return v


def _constraint_report(tr, con, length, viol_thresh):
    """``ConstraintReport`` of the rows ``con`` (numpy, [n, W]) with the env's names of the constraints."""
    return ConstraintReport.from_rows(con, tr.kernels.ineq_num, tr.kernels.eq_num, length, viol_thresh,
                                      getattr(tr.base_env, "ineq_names", None), getattr(tr.base_env, "eq_names", None))


def evaluate(tr, episodes=10, horizon=None, seed=None, init_states=None, record=False, eval_steps=None, eval_lr=None,
             constraints=False, obs_noise=None, scenarios=None):
    """See ``RPOTrainerBase.evaluate``."""
    n = check_episodes(episodes)
    scenario, days = check_scenarios(tr, scenarios, n)
    want_con = check_constraints(constraints)
    sigma = check_obs_noise(obs_noise, tr.kernels.obs_dim)
    if sigma is not None and not sigma.any():                    # 0 and all-zero: the clean evaluation, nothing new runs
        sigma = None
    budget = (None, None) if eval_steps is None and eval_lr is None else check_budget(tr, eval_steps, eval_lr)
    R = check_record(record, n)
    H = check_horizon(tr, horizon)
    k = tr.kernels
    fused = fused_ok(tr)
    fused_evopf = not fused and scenario is None and fused_evopf_ok(tr, n, R, sigma)   # (the fused kernel has no table-fed instance)
    dims = (k.obs_dim, k.partial_dim if fused else tr._eval_proposal_dim(), k.action_dim)
    if R:
        nbytes = 4 * H * R * hip_ops.trace_layout(*dims)[1]
        if nbytes > hip_ops.TRACE_MAX_BYTES:
            raise ValueError("evaluate: record=%r needs a trace buffer of %d bytes (horizon %d x %d episodes x %d floats), above "
                             "the cap of %d bytes; record fewer episodes (record=k)"
                             % (record, nbytes, H, R, hip_ops.trace_layout(*dims)[1], hip_ops.TRACE_MAX_BYTES))
    init_states = check_init_states(tr, init_states, n)
    seed = fresh_seed(tr) if seed is None else int(seed)
    v = _initial_env(tr, n, seed, init_states, scenario)
    acc = torch.zeros(n, 8, device=tr.device)
    # the record: zeroed here (the kernels write live lanes' rows only and never clear it), [step, episode, W]
    trace = torch.zeros(H, R, hip_ops.trace_layout(*dims)[1], device=tr.device) if R else None
    # the per-constraint report: step 0 writes every row from scratch, nothing to clear
    con = torch.empty(n, hip_ops.con_width(k.ineq_num, k.eq_num), device=tr.device) if want_con else None
    noise = {} if sigma is None else dict(noise=(sigma, seed))   # keyed by the evaluation's seed, like the reset stream
    path, run = ("fused", _run_fused) if fused else ("fused", _run_fused_evopf) if fused_evopf else ("stepwise", _run_stepwise)
    with torch.no_grad():
        run(tr, v, acc, H, trace=trace, budget=budget, con=con, **noise)
    res = EvalResult(acc.cpu().numpy(), path, H, seed, obs_noise=sigma)
    res.days = days
    if want_con:
        res.constraints = _constraint_report(tr, con.cpu().numpy(), res.length, v.viol_thresh)
    if R:
        res.trajectory = EvalTrajectory.from_trace(trace.cpu().numpy(), dims, res.length[:R], v.viol_thresh)
    return res


def evaluate_opf(tr, episodes=10, seed=None, horizon=None, init_states=None, record=False, constraints=False, pe="free",
                 pe_cost=None, tol=1e-4, max_iters=40, scenarios=None):
    """See ``RPOTrainerBase.evaluate_opf``, whose parameters these are; ``scenarios`` (here only: the method's parameter list is
    fixed) is ``evaluate()``'s -- a ``Scenarios``, episode e plays day e % len(scenarios), ``result.days`` records it."""
    if pe not in ("free", "zero"):
        raise ValueError("evaluate_opf: pe must be 'free' (the battery power is dispatched too) or 'zero' (idle batteries), got %r"
                         % (pe,))
    if pe_cost is not None and pe != "free":
        raise ValueError("evaluate_opf: pe_cost is the linear cost of the free battery power: pass pe='free' with it")
    env = tr.base_env
    if getattr(tr.kernels, "name", None) != "EVOPF-v0" or not hasattr(env, "opf"):
        raise NotImplementedError("evaluate_opf: the OPF controller is the single-step AC-OPF of EVOPF-v0; this trainer's env is %s"
                                  % getattr(tr.kernels, "name", type(env).__name__))
    fn = env._opf_free_kernel() if pe == "free" else env._opf_kernel()          # NotImplementedError: oracle backend, CPU device
    tol, iters_cap = float(tol), int(max_iters)
    if not tol > 0.0 or iters_cap != max_iters or iters_cap < 0:
        raise ValueError("evaluate_opf: tol must be > 0 and max_iters an integer >= 0, got %r and %r" % (tol, max_iters))
    n = check_episodes(episodes)
    scenario, days = check_scenarios(tr, scenarios, n, "evaluate_opf")
    want_con = check_constraints(constraints)
    R = check_record(record, n)
    H = check_horizon(tr, horizon, "evaluate_opf")
    k = tr.kernels
    idx = torch.as_tensor(np.asarray(env.partial_actions), dtype=torch.int64, device=tr.device)
    dims = (k.obs_dim, int(idx.numel()), k.action_dim)
    if R:
        nbytes = 4 * H * R * hip_ops.trace_layout(*dims)[1]
        if nbytes > hip_ops.TRACE_MAX_BYTES:
            raise ValueError("evaluate_opf: record=%r needs a trace buffer of %d bytes, above the cap of %d bytes; record fewer "
                             "episodes (record=k)" % (record, nbytes, hip_ops.TRACE_MAX_BYTES))
    if pe_cost is not None:
        pe_cost = torch.as_tensor(pe_cost, dtype=torch.float32, device=tr.device)
        if pe_cost.dim() == 0 or (pe_cost.dim() == 1 and pe_cost.shape[0] == env.ne):
            pe_cost = pe_cost.expand(n, env.ne)
        if tuple(pe_cost.shape) != (n, env.ne):
            raise ValueError("evaluate_opf: pe_cost must be None, a number, [%d] or [episodes, %d], got %s"
                             % (env.ne, env.ne, tuple(pe_cost.shape)))
        pe_cost = pe_cost.contiguous()
    init_states = check_init_states(tr, init_states, n, "evaluate_opf")
    seed = fresh_seed(tr) if seed is None else int(seed)
    v = _initial_env(tr, n, seed, init_states, scenario)
    acc = torch.zeros(n, 8, device=tr.device)
    trace = torch.zeros(H, R, hip_ops.trace_layout(*dims)[1], device=tr.device) if R else None
    con = torch.empty(n, hip_ops.con_width(k.ineq_num, k.eq_num), device=tr.device) if want_con else None
    info = torch.empty(n, 4, device=tr.device)
    log = torch.zeros(H, n, 2, device=tr.device)                 # (iterations, converged) of every step's launch

    def producer(v, iters, step):
        # one launch on the observation, straight into the env's action rows (pe = None: zeros, the idle battery)
        fn(k, v.obs, pe_cost, v.action, info, tol, iters_cap)
        iters.copy_(info[:, 2])
        log[step].copy_(info[:, 2:])
        return v.action.index_select(1, idx) if R else None      # (the proposal is read by the record alone)

    with torch.no_grad():
        _run_stepwise(tr, v, acc, H, trace=trace, con=con, producer=producer)
    res = EvalResult(acc.cpu().numpy(), "opf", H, seed)
    res.days = days
    live = np.arange(H)[None, :] < res.length[:, None]           # filled while the episode is live
    log = log.cpu().numpy().transpose(1, 0, 2)
    res.opf_iters = np.where(live, log[:, :, 0], 0).astype(np.int32)
    res.opf_converged = live & (log[:, :, 1] > 0.5)
    if want_con:
        res.constraints = _constraint_report(tr, con.cpu().numpy(), res.length, v.viol_thresh)
    if R:
        res.trajectory = EvalTrajectory.from_trace(trace.cpu().numpy(), dims, res.length[:R], v.viol_thresh)
    return res


def evaluate_filtered(tr, episodes=10, seed=None, horizon=None, init_states=None, record=False, constraints=False, weight=None,
                      tol=1e-4, max_iters=40, fallback="policy", eval_steps=None, eval_lr=None, scenarios=None):
    """See ``RPOTrainerBase.evaluate_filtered``."""
    if fallback not in ("policy", "last"):
        raise ValueError("evaluate_filtered: fallback must be 'policy' (a step whose solve did not converge takes the policy's own "
                         "action) or 'last' (the solver's last iterate), got %r" % (fallback,))
    env = tr.base_env
    if getattr(tr.kernels, "name", None) != "EVOPF-v0" or not hasattr(env, "nearest_feasible"):
        raise NotImplementedError("evaluate_filtered: the safety filter is the nearest-feasible solve of EVOPF-v0; this trainer's "
                                  "env is %s" % getattr(tr.kernels, "name", type(env).__name__))
    fn = env._nearest_kernel()                                   # NotImplementedError: oracle backend, CPU device
    tol, iters_cap = float(tol), int(max_iters)
    if not tol > 0.0 or iters_cap != max_iters or iters_cap < 0:
        raise ValueError("evaluate_filtered: tol must be > 0 and max_iters an integer >= 0, got %r and %r" % (tol, max_iters))
    n = check_episodes(episodes)
    scenario, days = check_scenarios(tr, scenarios, n, "evaluate_filtered")
    want_con = check_constraints(constraints)
    kw = {}
    if eval_steps is not None or eval_lr is not None:
        kw["eval_steps"], kw["eval_lr"] = check_budget(tr, eval_steps, eval_lr, "evaluate_filtered")
    R = check_record(record, n)
    H = check_horizon(tr, horizon, "evaluate_filtered")
    k = tr.kernels
    idx = torch.as_tensor(np.asarray(env.partial_actions), dtype=torch.int64, device=tr.device)
    dims = (k.obs_dim, int(idx.numel()), k.action_dim)
    if R:
        nbytes = 4 * H * R * hip_ops.trace_layout(*dims)[1]
        if nbytes > hip_ops.TRACE_MAX_BYTES:
            raise ValueError("evaluate_filtered: record=%r needs a trace buffer of %d bytes, above the cap of %d bytes; record "
                             "fewer episodes (record=k)" % (record, nbytes, hip_ops.TRACE_MAX_BYTES))
    weight = env._check_weight(weight, n, "evaluate_filtered")
    init_states = check_init_states(tr, init_states, n, "evaluate_filtered")
    seed = fresh_seed(tr) if seed is None else int(seed)
    v = _initial_env(tr, n, seed, init_states, scenario)
    acc = torch.zeros(n, 8, device=tr.device)
    trace = torch.zeros(H, R, hip_ops.trace_layout(*dims)[1], device=tr.device) if R else None
    con = torch.empty(n, hip_ops.con_width(k.ineq_num, k.eq_num), device=tr.device) if want_con else None
    info = torch.empty(n, 4, device=tr.device)
    policy = torch.empty_like(v.action)                          # the policy's own action of the step: the filter's target
    log = torch.zeros(H, n, 4, device=tr.device)                 # the filter's info row of every step's launch

    def producer(v, iters, step):
        # the trainer's deterministic action + GRG projection, then one launch that moves it to the nearest feasible dispatch
        tr._eval_action(v, iters=iters, **kw)
        policy.copy_(v.action)
        fn(k, v.obs, policy, weight, v.action, info, tol, iters_cap)
        if fallback == "policy":                                 # a select on the device: no host decision
            v.action.copy_(torch.where(info[:, 3:4] > 0.5, v.action, policy))
        iters.copy_(info[:, 2])
        log[step].copy_(info)
        return policy.index_select(1, idx) if R else None        # (the proposal is read by the record alone)

    with torch.no_grad():
        _run_stepwise(tr, v, acc, H, trace=trace, con=con, producer=producer)
    res = EvalResult(acc.cpu().numpy(), "filtered", H, seed)
    res.days = days
    live = np.arange(H)[None, :] < res.length[:, None]           # filled while the episode is live
    log = log.cpu().numpy().transpose(1, 0, 2)
    res.filter_iters = np.where(live, log[:, :, 2], 0).astype(np.int32)
    res.filter_converged = live & (log[:, :, 3] > 0.5)
    res.filter_distance = np.where(live, log[:, :, 0], 0).astype(np.float32)
    if want_con:
        res.constraints = _constraint_report(tr, con.cpu().numpy(), res.length, v.viol_thresh)
    if R:
        res.trajectory = EvalTrajectory.from_trace(trace.cpu().numpy(), dims, res.length[:R], v.viol_thresh)
    return res


#: the env kernels' method of a ``variant`` of _run_fused -> what is said to a record or a noise next to it
_VARIANT_REFUSALS = {"evaluate_budgets": "per-lane budgets run without a record and without observation noise",
                     "evaluate_policies": "policy groups run without a record and without observation noise",
                     "evaluate_noise_sweep": "noise levels per group run without a record and without a sigma of the whole launch"}


def _run_fused(tr, v, acc, H, desc=None, trace=None, budget=(None, None), con=None, noise=None, variant=None):
    """ceil(H / steps) launches of rpo_<env>_evaluate, enqueued back to back.  steps: RPO_EVAL_LANE_STEPS lane-steps per launch
    (4 steps at 2^20 lanes, one launch for the whole horizon up to ~8000 lanes).  ``desc``: another actor descriptor than the
    trainer's (the curve's parameter snapshot).  ``trace``: the zeroed record [H, R, W] every launch continues
    (rpo_<env>_evaluate_record).  ``budget``: evaluate()'s per-call (eval_steps, eval_lr), None: the trainer's.  ``con``: the
    per-constraint report [n, W] every launch continues (rpo_<env>_evaluate_constraints).  ``noise``: (sigma float32 numpy
    [obs_dim], seed) of ``obs_noise=`` (rpo_<env>_evaluate_noisy; the draw is keyed by the absolute step t0 + s); None: the
    kernels' ``evaluate`` gets no such keyword.  ``variant``: (the env kernels' method, its arguments behind viol_thresh...) of a
    sweep in place of ``evaluate`` -- one at most by construction, con only, neither trace nor noise:
    ("evaluate_budgets",) with ``budget`` = (eval_steps int32 [n], eval_lr float32 [n]) on the device, the budget and step size
    of every lane (rpo_<env>_evaluate_budgets); ("evaluate_policies", bank [P, span], group_lanes, episodes) with ``desc`` over
    bank[0]: an actor per group of lanes (rpo_<env>_evaluate_policies); ("evaluate_noise_sweep", sigma_table [S, 8] on the
    device, seed, group_lanes, episodes): a noise level per group of lanes (rpo_<env>_evaluate_noise_sweep)."""
    n = v.n
    eval_steps = tr.eval_steps if budget[0] is None else budget[0]
    eval_lr = tr.eval_lr if budget[1] is None else budget[1]
    steps = max(1, min(H, hip_ops.EVAL_LANE_STEPS // n))
    scale, base = tr._box_affine
    desc = tr.fused.descs["actor"] if desc is None else desc
    kw = {} if trace is None else dict(trace=trace)
    if con is not None:
        kw["con"] = con
    if noise is not None:
        kw["noise"] = noise
    method, *tail = ("evaluate",) if variant is None else variant
    if variant is not None and (trace is not None or noise is not None):
        raise ValueError(_VARIANT_REFUSALS[method])
    for t0 in range(0, H, steps):                                # (the method is looked up at every launch)
        getattr(tr.kernels, method)(desc, tr._gauss_policy, scale, base, v.internal, None if v.obs is v.internal else v.obs,
                                    v.action, v.ep_len, v.ep_ret, v.ep_count, v.ctrl, acc, t0, min(steps, H - t0), tr._box_lo,
                                    tr._box_hi, eval_steps, eval_lr, tr.corr_eps, tr.corr_momentum, v.max_episode_steps,
                                    v.viol_thresh, *tail, **kw)


def _run_fused_evopf(tr, v, acc, H, trace=None, budget=(None, None), con=None, noise=None):
    """_run_fused on EVOPF-v0 (``fused_evopf_ok``: neither trace nor noise): ceil(H / steps) launches of rpo_evopf_evaluate back to
    back, EVOPF_EVAL_LANE_STEPS lane-steps per launch -- a lane-step is a power-flow solve there, not a row of a tile.  The box
    depends on the state, so there is no (scale, base): the kernel applies it like rpo_evopf_act_project / rpo_evopf_gauss_head."""
    assert trace is None and noise is None
    eval_steps = tr.eval_steps if budget[0] is None else budget[0]
    eval_lr = tr.eval_lr if budget[1] is None else budget[1]
    steps = max(1, min(H, hip_ops.EVOPF_EVAL_LANE_STEPS // v.n))
    for t0 in range(0, H, steps):
        tr.backend.evopf_evaluate(tr.kernels, tr.fused.descs["actor"], tr._gauss_policy, v.internal, v.action, v.ep_len, v.ep_ret,
                                  v.ep_count, v.ctrl, acc, t0, min(steps, H - t0), eval_steps, eval_lr, tr.corr_eps,
                                  tr.corr_momentum, v.max_episode_steps, v.viol_thresh, v.seed, v.env_id_base, con=con)


def _run_stepwise(tr, v, acc, H, trace=None, budget=(None, None), con=None, noise=None, producer=None):
    """eval()'s loop: the trainer's deterministic action + projection, one env step without auto-reset, the accumulator
    update.  Finished lanes keep stepping (as in eval()); their rows no longer change.  ``trace``: the zeroed record
    [H, R, W]; the step's row goes in before the accumulator update (which ends the lanes the step finished), from a copy
    of the observation the policy read (the step overwrites it).  ``con``: the per-constraint report [n, W], updated before
    the accumulators for the same reason.  ``noise``: (sigma, seed) of ``obs_noise=``: step i's noisy observation goes into a
    buffer of its own (never into the env's rows: CartSafe-v0's observation IS its state), which the policy, the projection
    and the record read; the env steps what it holds.  ``producer``: ``producer(v, iters, step)`` in the place of the
    trainer's ``_eval_action`` -- it writes v.action from v.obs and ``iters``, and returns the proposal to record
    (``evaluate_opf``: the OPF controller); without it nothing here differs."""
    k = tr.kernels
    rows = torch.zeros(v.n, k.ring_floats, device=tr.device)
    iters = torch.zeros(v.n, dtype=torch.int32, device=tr.device)
    update = getattr(tr.backend, "eval_accumulate", None) or accumulate_torch
    record = getattr(tr.backend, "eval_record", None) or record_torch
    report = getattr(tr.backend, "eval_constraints", None) or constraints_torch
    obs_in = torch.zeros_like(v.obs) if trace is not None or noise is not None else None
    kw = {} if budget == (None, None) else dict(eval_steps=budget[0], eval_lr=budget[1])
    if noise is not None:
        sigma, seed = noise
        perturb = getattr(tr.backend, "eval_obs_noise", None)
        sigma_dev = torch.as_tensor(sigma, device=tr.device)
        kw["obs"] = obs_in
    for i in range(H):
        if noise is not None:
            if perturb is not None:
                perturb(v.obs, sigma_dev, seed, i, obs_in)
            else:
                obs_noise_torch(tr, v.obs, sigma, seed, i, obs_in)
        elif trace is not None:
            obs_in.copy_(v.obs)
        proposal = tr._eval_action(v, iters=iters, **kw) if producer is None else producer(v, iters, i)
        v.step(v.action, rows=rows, cap_steps=1, auto_reset=False)
        if trace is not None:
            record(rows, k.cols, obs_in, proposal, v.action, iters, i, acc, trace)
        if con is not None:
            report(rows, k.cols, i, v.viol_thresh, acc, con)
        update(rows, k.cols, iters, i, v.viol_thresh, acc)


# ------------------------------------------------------------------------------------------------ sweeps: shared
def _padded(n):
    """n episodes of a group padded to whole 64-lane tiles."""
    return (n + hip_ops.POLICY_GROUP_ALIGN - 1) // hip_ops.POLICY_GROUP_ALIGN * hip_ops.POLICY_GROUP_ALIGN


def _tile_groups(tr, v, seed, G, want_con, GL=None):
    """(env, acc, con) of G copies of the initial env ``v``, group-major: lane g * GL + e is episode e of group g.  internal AND
    obs are tiled (SpringPendulum's injected observation comes from torch's cos / sin: recomputing it here would not be
    evaluate()'s bits); the bookkeeping of the new env is zero, like the reset one's.  GL None: the groups are not padded and
    con is left to step 0, which writes every row; else every group has GL >= n lanes, the padding lanes keep the new env's rows
    (the kernel neither steps nor writes them) and con is zeroed."""
    n = v.n
    lanes = n if GL is None else GL
    big = _make_vec(tr, G * lanes, seed)
    big.internal.view(G, lanes, -1)[:, :n].copy_(v.internal)
    if big.obs is not big.internal:
        big.obs.view(G, lanes, -1)[:, :n].copy_(v.obs)
    acc = torch.zeros(G * lanes, 8, device=tr.device)
    con = None
    if want_con:
        con = (torch.empty if GL is None else torch.zeros)(G * lanes, hip_ops.con_width(tr.kernels.ineq_num, tr.kernels.eq_num),
                                                           device=tr.device)
    return big, acc, con


def _group_results(tr, acc, con, G, n, H, seed, viol_thresh):
    """The G ``EvalResult``s (path "fused") of the first n lanes of every group of acc [G * GL, 8] / con [G * GL, W] or None."""
    acc_host = acc.cpu().numpy().reshape(G, -1, 8)
    con_host = None if con is None else con.cpu().numpy().reshape(G, acc_host.shape[1], -1)
    results = []
    for g in range(G):
        res = EvalResult(acc_host[g, :n], "fused", H, seed)
        if con is not None:
            res.constraints = _constraint_report(tr, con_host[g, :n], res.length, viol_thresh)
        results.append(res)
    return results


# ------------------------------------------------------------------------------------------------ budget sweeps
MAX_BUDGETS = 64
Paired = collections.namedtuple("Paired", "mean stderr n")
_FUSED_BUDGET_LANES = 1 << 24                                    # B x episodes lanes of one fused launch; beyond: "sweep"


class ResultSweep(object):
    """What ``BudgetSweep``, ``PolicySweep`` and ``NoiseSweep`` share: G ``EvalResult``s of the same episodes (``sweep[g]`` is ``results[g]``)
    and their fields stacked into [G, episodes] arrays whose rows ARE the results' arrays (one memory)."""

    def _stack(self, results, path):
        self.results, self.path = list(results), path
        if not self.results:
            raise ValueError("%s: no results" % type(self).__name__)
        if len(set(r.episodes for r in self.results)) != 1:
            raise ValueError("%s: the results have different numbers of episodes" % type(self).__name__)
        self.seed, self.horizon = self.results[0].seed, self.results[0].horizon
        for f in EvalResult.FIELDS:
            rows = np.stack([getattr(r, f) for r in self.results])
            setattr(self, f, rows)
            for g, r in enumerate(self.results):                 # the result's array becomes row g of the stack
                setattr(r, f, rows[g])
        self.iters = self.proj_iters

    def __len__(self):
        return len(self.results)

    def __getitem__(self, g):
        return self.results[g]

    @property
    def episodes(self):
        return self.ret.shape[1]

    def violation_rate(self):
        """Per group: the fraction of its evaluated env steps whose max inequality violation exceeds ``viol_thresh`` [G]."""
        return self.viol_steps.sum(axis=1).astype(np.float64) / self.length.sum(axis=1).astype(np.float64)

    def ret_mean(self):
        """Per group: the mean return over the episodes [G]."""
        return self.ret.mean(axis=1)

    def paired(self, a, b):
        """The paired comparison of groups a and b: ``Paired(mean, stderr, n)`` of the per-episode return difference
        ``ret[a] - ret[b]`` (episode e of both started from the same state); stderr: the sample standard deviation (n - 1)
        over sqrt(n), NaN for n = 1."""
        d = self.ret[a] - self.ret[b]
        n = d.shape[0]
        return Paired(float(d.mean()), float(d.std(ddof=1) / math.sqrt(n)) if n > 1 else float("nan"), n)


class BudgetSweep(ResultSweep):
    """The result of ``evaluate_budgets()``: B projection budgets evaluated on the same initial states.

    ``eval_steps`` int64 [B] / ``eval_lr`` float32 [B]: the budgets in the caller's order; ``results``: B ``EvalResult``s
    (``sweep[g]`` is ``results[g]``), each what ``evaluate(eval_steps=eval_steps[g], eval_lr=eval_lr[g])`` with the shared seed
    returns.  ``ret``, ``length``, ``mean_ineq``, ``mean_eq``, ``max_ineq``, ``max_eq``, ``viol_steps``, ``proj_iters`` (also
    ``iters``), ``nonfinite``: [B, episodes] arrays whose rows ARE the results' arrays (one memory).  ``path``: "fused" (one
    launch sequence over B x episodes lanes) or "sweep" (B ``evaluate()`` calls).  ``seed``, ``horizon``: the shared ones."""

    def __init__(self, results, eval_steps, eval_lr, path):
        results = list(results)
        self.eval_steps = np.array(eval_steps, dtype=np.int64).reshape(-1)
        self.eval_lr = np.array(eval_lr, dtype=np.float32).reshape(-1)
        if not results or not len(results) == len(self.eval_steps) == len(self.eval_lr):
            raise ValueError("BudgetSweep: %d results for %d budgets and %d step sizes"
                             % (len(results), len(self.eval_steps), len(self.eval_lr)))
        self._stack(results, path)

    def budget(self, max_rate=0.0):
        """The smallest ``eval_steps[g]`` whose ``violation_rate()[g]`` is <= ``max_rate``; None if no budget of the sweep is."""
        ok = self.violation_rate() <= max_rate
        return int(self.eval_steps[ok].min()) if ok.any() else None

    def __repr__(self):
        return "BudgetSweep(budgets=%s, episodes=%d, path=%s, violation_rate=%s)" % (
            self.eval_steps.tolist(), self.episodes, self.path, np.array2string(self.violation_rate(), precision=4))


def check_budgets(tr, eval_steps, eval_lr):
    """``eval_steps`` / ``eval_lr`` of evaluate_budgets() -> (list of B ints, list of B floats): a non-empty sequence of at most
    ``MAX_BUDGETS`` integers >= 0 (duplicates allowed, order kept); ``eval_lr`` None (the trainer's), one finite number or B finite
    numbers (ValueError otherwise)."""
    what = "evaluate_budgets"
    if eval_steps is None or isinstance(eval_steps, (str, bytes)) or np.ndim(eval_steps) != 1:
        raise ValueError("%s: eval_steps must be a non-empty sequence of integers >= 0, got %r" % (what, eval_steps))
    steps = list(eval_steps)
    if not 1 <= len(steps) <= MAX_BUDGETS:
        raise ValueError("%s: eval_steps must hold 1 to %d budgets, got %d" % (what, MAX_BUDGETS, len(steps)))
    if eval_lr is None or (np.ndim(eval_lr) == 0 and not isinstance(eval_lr, (str, bytes))):
        lrs = [eval_lr] * len(steps)
    elif isinstance(eval_lr, (str, bytes)) or np.ndim(eval_lr) != 1 or len(eval_lr) != len(steps):
        raise ValueError("%s: eval_lr must be None, one finite number or %d finite numbers, got %r" % (what, len(steps), eval_lr))
    else:
        lrs = list(eval_lr)
    out = []
    for b, lr in zip(steps, lrs):
        if b is None or isinstance(b, (bool, np.bool_)) or isinstance(lr, (bool, np.bool_)):
            raise ValueError("%s: eval_steps must be integers >= 0 and eval_lr finite numbers, got %r / %r" % (what, b, lr))
        out.append(check_budget(tr, b, lr, what))
    return [b for b, _ in out], [lr for _, lr in out]


def evaluate_budgets(tr, episodes=10, eval_steps=None, eval_lr=None, horizon=None, seed=None, init_states=None, constraints=False):
    """See ``RPOTrainerBase.evaluate_budgets``."""
    from .acting import _projects
    n = check_episodes(episodes, "evaluate_budgets: episodes")
    want_con = check_constraints(constraints)
    if not _projects(tr):
        raise ValueError("evaluate_budgets needs a trainer that projects (RPODDPG / RPOSAC); %s has no projection" % type(tr).__name__)
    steps, lrs = check_budgets(tr, eval_steps, eval_lr)
    B = len(steps)
    H = check_horizon(tr, horizon, "evaluate_budgets")
    init_states = check_init_states(tr, init_states, n, "evaluate_budgets")
    seed = fresh_seed(tr) if seed is None else int(seed)         # ONE seed (and one tick of the call counter) for all budgets
    fused = bool(fused_ok(tr) and hasattr(tr.kernels, "evaluate_budgets") and tr.schedule.get("fused_budgets", 1)
                 and B * n <= _FUSED_BUDGET_LANES)
    if not fused:
        results = [evaluate(tr, episodes=n, horizon=H, seed=seed, init_states=init_states, eval_steps=b, eval_lr=lr,
                            constraints=want_con) for b, lr in zip(steps, lrs)]
        return BudgetSweep(results, steps, lrs, "sweep")
    # B unpadded groups: lane g * n + e is episode e under budget g
    big, acc, con = _tile_groups(tr, _initial_env(tr, n, seed, init_states), seed, B, want_con)
    lanes = (torch.tensor(steps, dtype=torch.int32, device=tr.device).repeat_interleave(n),
             torch.tensor(lrs, dtype=torch.float32, device=tr.device).repeat_interleave(n))
    with torch.no_grad():
        _run_fused(tr, big, acc, H, budget=lanes, con=con, variant=("evaluate_budgets",))
    return BudgetSweep(_group_results(tr, acc, con, B, n, H, seed, big.viol_thresh), steps, lrs, "fused")


# ------------------------------------------------------------------------------------------------ policy sweeps
MAX_POLICIES = 64
_FUSED_POLICY_LANES = 1 << 24                                    # P x padded lanes of one fused launch; beyond: "sweep"


class PolicySweep(ResultSweep):
    """The result of ``evaluate_policies()``: P actors evaluated on the same initial states.

    ``names``: P strings in the caller's order; ``results``: P ``EvalResult``s (``sweep[g]`` is ``results[g]``), each what
    ``evaluate()`` under ``using_policy(policies[g])`` with the shared seed returns.  ``ret``, ``length``, ``mean_ineq``,
    ``mean_eq``, ``max_ineq``, ``max_eq``, ``viol_steps``, ``proj_iters`` (also ``iters``), ``nonfinite``: [P, episodes] arrays
    whose rows ARE the results' arrays (one memory).  ``path``: "fused" (one launch sequence over P x padded lanes) or "sweep"
    (P ``evaluate()`` calls).  ``seed``, ``horizon``: the shared ones."""

    def __init__(self, results, names, path):
        results, self.names = list(results), tuple(str(x) for x in names)
        if not results or len(results) != len(self.names):
            raise ValueError("PolicySweep: %d results for %d names" % (len(results), len(self.names)))
        self._stack(results, path)

    def best(self, max_rate=0.0):
        """The index ``keep_best`` would hold after seeing the groups in order (``keep_best_wins`` of csrc/eval_dev.h on the
        groups' summaries): a group is safe when its violation rate is <= ``max_rate``; safe beats unsafe; among safe groups
        the strictly higher mean return wins; among unsafe ones the strictly lower rate, then the higher return; ties keep the
        earlier group; a group with a non-finite episode or a NaN mean return is never taken.  None: no group is eligible."""
        length, viol, ret = self.length.sum(axis=1), self.viol_steps.sum(axis=1), self.ret_mean()
        held = held_rate = None
        for g in range(len(self)):
            if self.nonfinite[g].any() or ret[g] != ret[g]:
                continue
            rate = float("inf") if length[g] == 0 else float(viol[g]) / float(length[g])
            if held is not None:
                safe, held_safe = rate <= max_rate, held_rate <= max_rate
                if safe != held_safe:
                    wins = safe
                elif safe:
                    wins = ret[g] > ret[held]
                else:
                    wins = rate < held_rate or (rate == held_rate and ret[g] > ret[held])
                if not wins:
                    continue
            held, held_rate = g, rate
        return held

    def __repr__(self):
        return "PolicySweep(policies=%s, episodes=%d, path=%s, return=%s, violation_rate=%s)" % (
            list(self.names), self.episodes, self.path, np.array2string(self.ret_mean(), precision=4),
            np.array2string(self.violation_rate(), precision=4))


def actor_span(tr, what):
    """(flat buffer, actor_range) of a trainer whose actor lives in the flat parameter buffer (ValueError otherwise)."""
    flat = getattr(tr.agent, "flat", None)
    if getattr(flat, "actor_range", None) is None:
        raise ValueError("%s needs the actor in the flat parameter buffer (agent.flat.actor_range): %s has none"
                         % (what, type(tr.agent).__name__))
    return flat, flat.actor_range


def check_policy(entry, size, what):
    """One policy of ``using_policy()`` / ``evaluate_policies()`` -> None (the live actor) or a flat float32 tensor of ``size``
    floats: None; a float32 tensor or numpy array of exactly ``size`` floats; a ``BestPolicy``; a path ``BestPolicy.load`` reads
    (ValueError for anything else, another length, another dtype, a file that does not load)."""
    if entry is None:
        return None
    if isinstance(entry, (str, bytes, os.PathLike)):
        if not os.path.isfile(entry):
            raise ValueError("%s: %r is not a file" % (what, entry))
        try:
            entry = BestPolicy.load(entry)
        except Exception as e:                                   # noqa: BLE001 (np.load's own errors, a missing key)
            raise ValueError("%s: BestPolicy.load cannot read %r (%s)" % (what, entry, e))
    if isinstance(entry, BestPolicy):
        entry = entry.params
    if isinstance(entry, np.ndarray) and entry.dtype == np.float32:
        entry = torch.from_numpy(np.ascontiguousarray(entry))
    if not isinstance(entry, torch.Tensor) or entry.dtype != torch.float32:
        raise ValueError("%s: a policy is None, a float32 tensor / array of %d floats, a BestPolicy or a path, got %s"
                         % (what, size, type(entry).__name__ if not hasattr(entry, "dtype") else entry.dtype))
    if entry.numel() != size:
        raise ValueError("%s: the actor's span of the flat parameter buffer has %d floats, the policy has %d"
                         % (what, size, entry.numel()))
    return entry.detach().reshape(-1)


def policy_params(tr):
    """See ``RPOTrainerBase.policy_params``."""
    flat, rng = actor_span(tr, "policy_params()")
    with torch.no_grad():
        return flat.param(rng).clone()


@contextlib.contextmanager
def using_policy(tr, policy):
    """See ``RPOTrainerBase.using_policy``."""
    flat, rng = actor_span(tr, "using_policy()")
    src = check_policy(policy, rng[1] - rng[0], "using_policy()")
    if src is None:                                              # the live actor is the live actor
        yield tr
        return
    live = flat.param(rng)
    with torch.no_grad():
        stash = live.clone()
        live.copy_(src)
    try:
        yield tr
    finally:
        with torch.no_grad():
            live.copy_(stash)


def _policy_name(entry, g):
    if entry is None:
        return "live"
    if isinstance(entry, (str, bytes, os.PathLike)):
        return os.fspath(entry) if not isinstance(entry, bytes) else os.fsdecode(entry)
    return "best[%d]" % entry.point if isinstance(entry, BestPolicy) else "policy[%d]" % g


def check_policies(tr, policies, names):
    """``policies`` / ``names`` of evaluate_policies() -> (flat, actor_range, list of P spans (None: the live actor), P names): a
    sequence of 1 to ``MAX_POLICIES`` entries ``check_policy`` takes; ``names`` None or P strings (ValueError otherwise)."""
    what = "evaluate_policies"
    flat, rng = actor_span(tr, what + "()")
    if policies is None or isinstance(policies, (str, bytes, torch.Tensor, np.ndarray, BestPolicy)) or not hasattr(policies, "__len__"):
        raise ValueError("%s: policies must be a sequence of 1 to %d policies, got %r" % (what, MAX_POLICIES, type(policies).__name__))
    entries = list(policies)
    if not 1 <= len(entries) <= MAX_POLICIES:
        raise ValueError("%s: policies must hold 1 to %d policies, got %d" % (what, MAX_POLICIES, len(entries)))
    spans = [check_policy(e, rng[1] - rng[0], "%s: policies[%d]" % (what, g)) for g, e in enumerate(entries)]
    if names is None:
        names = [_policy_name(e, g) for g, e in enumerate(entries)]
    elif isinstance(names, (str, bytes)) or not hasattr(names, "__len__") or len(names) != len(entries) or \
            not all(isinstance(x, str) for x in names):
        raise ValueError("%s: names must be None or %d strings, got %r" % (what, len(entries), names))
    return flat, rng, spans, list(names)


def actor_desc_over(tr, buf):
    """The fused actor's ``MlpDesc`` over ``buf``: a float32 vector laid out like the actor's span of the flat parameter buffer
    (every tensor at its offset in the span)."""
    flat, d = tr.agent.flat, tr.fused.descs["actor"]
    tensors = {}
    for key, p in d.tensors.items():
        if p is not None:
            off = flat.offset[id(p)] - flat.actor_range[0]
            tensors[key] = buf[off:off + p.numel()].view(p.shape)
    return tr.backend.MlpDesc(tensors, d.S, d.A, d.E, d.H, d.n_out, d.cat, head_dim=d.head_dim)


def policy_bank(tr, spans):
    """(bank, descriptor) of the fused path: the P spans (None: the live actor's) side by side in one device tensor
    [P, span] -- the span is a multiple of 4 floats by FlatParams' padding, so every policy's tensors keep the alignment of
    the live ones -- and ONE ``MlpDesc`` over policy 0 (``actor_desc_over``)."""
    flat, (lo, hi) = actor_span(tr, "evaluate_policies()")
    live = flat.param((lo, hi))
    bank = torch.empty(len(spans), hi - lo, device=tr.device)
    for g, src in enumerate(spans):
        bank[g].copy_(live if src is None else src)
    return bank, actor_desc_over(tr, bank[0])


def evaluate_policies(tr, policies, episodes=10, seed=None, horizon=None, init_states=None, constraints=False, names=None):
    """See ``RPOTrainerBase.evaluate_policies``."""
    _, _, spans, names = check_policies(tr, policies, names)
    n = check_episodes(episodes, "evaluate_policies: episodes")
    want_con = check_constraints(constraints)
    P = len(spans)
    H = check_horizon(tr, horizon, "evaluate_policies")
    init_states = check_init_states(tr, init_states, n, "evaluate_policies")
    seed = fresh_seed(tr) if seed is None else int(seed)         # ONE seed (and one tick of the call counter) for all policies
    GL = _padded(n)
    fused = bool(fused_ok(tr) and hasattr(tr.kernels, "evaluate_policies") and tr.schedule.get("fused_policies", 1)
                 and P * GL <= _FUSED_POLICY_LANES)
    if not fused:
        results = []
        for src in spans:
            with using_policy(tr, src):
                results.append(evaluate(tr, episodes=n, horizon=H, seed=seed, init_states=init_states, constraints=want_con))
        return PolicySweep(results, names, "sweep")
    v = _initial_env(tr, n, seed, init_states)
    with torch.no_grad():
        bank, desc = policy_bank(tr, spans)
        # P groups padded to GL lanes: lane g * GL + e is episode e under policy g
        big, acc, con = _tile_groups(tr, v, seed, P, want_con, GL)
        _run_fused(tr, big, acc, H, desc=desc, con=con, variant=("evaluate_policies", bank, GL, n))
    return PolicySweep(_group_results(tr, acc, con, P, n, H, seed, big.viol_thresh), names, "fused")


# ------------------------------------------------------------------------------------------------ noise sweeps
MAX_NOISE_LEVELS = 64
_FUSED_NOISE_LANES = 1 << 24                                     # S x padded lanes of one fused launch; beyond: "sweep"


class NoiseSweep(ResultSweep):
    """The result of ``evaluate_noise()``: S sensor-noise levels evaluated on the same initial states and the same draws.

    ``levels``: float32 [S, obs_dim], the sigma vector of every level in the caller's order (None: zeros; a number: broadcast);
    ``results``: S ``EvalResult``s (``sweep[g]`` is ``results[g]``), each what ``evaluate(obs_noise=levels[g])`` with the shared
    seed returns, with ``obs_noise = levels[g]``.  ``ret``, ``length``, ``mean_ineq``, ``mean_eq``, ``max_ineq``, ``max_eq``,
    ``viol_steps``, ``proj_iters`` (also ``iters``), ``nonfinite``: [S, episodes] arrays whose rows ARE the results' arrays (one
    memory).  ``path``: "fused" (one launch sequence over S x padded lanes) or "sweep" (S ``evaluate()`` calls).  ``seed``,
    ``horizon``: the shared ones."""

    def __init__(self, results, levels, path):
        results = list(results)
        self.levels = np.array(levels, dtype=np.float32)
        if not results or self.levels.ndim != 2 or len(results) != self.levels.shape[0]:
            raise ValueError("NoiseSweep: %d results for levels of shape %s" % (len(results), self.levels.shape))
        self._stack(results, path)
        for g, r in enumerate(self.results):
            r.obs_noise = self.levels[g]

    def tolerance(self, max_rate=0.0):
        """The index of the last level, in the order given, of the longest prefix of levels whose ``violation_rate()`` are all
        <= ``max_rate`` (with increasing levels: the largest noise the policy is still safe under); -1 if level 0 already
        exceeds it.  A level behind the first failing one does not count, whatever its rate."""
        bad = np.flatnonzero(~(self.violation_rate() <= max_rate))
        return (int(bad[0]) if bad.size else len(self)) - 1

    def __repr__(self):
        return "NoiseSweep(levels=%s, episodes=%d, path=%s, return=%s, violation_rate=%s)" % (
            np.array2string(self.levels.max(axis=1), precision=4), self.episodes, self.path,
            np.array2string(self.ret_mean(), precision=4), np.array2string(self.violation_rate(), precision=4))


def check_noise_levels(obs_noise, obs_dim):
    """``obs_noise`` of evaluate_noise() -> the float32 levels [S, obs_dim]: a non-empty sequence of at most
    ``MAX_NOISE_LEVELS`` entries, each what ``check_obs_noise`` takes (None: zeros); ValueError otherwise, naming the index of an
    offending entry."""
    what = "evaluate_noise"
    if obs_noise is None or isinstance(obs_noise, (str, bytes)) or not hasattr(obs_noise, "__len__") or \
            (isinstance(obs_noise, (np.ndarray, torch.Tensor)) and obs_noise.ndim == 0):
        raise ValueError("%s: obs_noise must be a sequence of 1 to %d noise levels, got %r" % (what, MAX_NOISE_LEVELS, obs_noise))
    entries = list(obs_noise)
    if not 1 <= len(entries) <= MAX_NOISE_LEVELS:
        raise ValueError("%s: obs_noise must hold 1 to %d noise levels, got %d" % (what, MAX_NOISE_LEVELS, len(entries)))
    levels = np.zeros((len(entries), obs_dim), dtype=np.float32)
    for g, entry in enumerate(entries):
        try:
            sigma = check_obs_noise(entry, obs_dim)
        except ValueError as e:
            raise ValueError("%s: obs_noise[%d]: %s" % (what, g, e))
        if sigma is not None:
            levels[g] = sigma
    return levels


def evaluate_noise(tr, episodes=10, obs_noise=None, horizon=None, seed=None, init_states=None, constraints=False):
    """See ``RPOTrainerBase.evaluate_noise``."""
    k = tr.kernels
    levels = check_noise_levels(obs_noise, k.obs_dim)
    n = check_episodes(episodes, "evaluate_noise: episodes")
    want_con = check_constraints(constraints)
    S = levels.shape[0]
    H = check_horizon(tr, horizon, "evaluate_noise")
    init_states = check_init_states(tr, init_states, n, "evaluate_noise")
    seed = fresh_seed(tr) if seed is None else int(seed)         # ONE seed (and one tick of the call counter) for all levels
    GL = _padded(n)
    fused = bool(fused_ok(tr) and hasattr(k, "evaluate_noise_sweep") and tr.schedule.get("fused_noise_sweep", 1)
                 and S * GL <= _FUSED_NOISE_LANES)
    if not fused:
        results = [evaluate(tr, episodes=n, horizon=H, seed=seed, init_states=init_states, constraints=want_con,
                            obs_noise=levels[g]) for g in range(S)]
        return NoiseSweep(results, levels, "sweep")
    v = _initial_env(tr, n, seed, init_states)
    with torch.no_grad():
        # S groups padded to GL lanes: lane g * GL + e is episode e under level g
        big, acc, con = _tile_groups(tr, v, seed, S, want_con, GL)
        table = np.zeros((S, 8), dtype=np.float32)               # sigma[S, 8], zero beyond obs_dim
        table[:, :k.obs_dim] = levels
        table = torch.from_numpy(table).to(tr.device)
        _run_fused(tr, big, acc, H, con=con, variant=("evaluate_noise_sweep", table, seed, GL, n))
    return NoiseSweep(_group_results(tr, acc, con, S, n, H, seed, big.viol_thresh), levels, "fused")


# ------------------------------------------------------------------------------------------------ evaluation curves
#: curve row layout (include/rpo_hip.h: RPO_CURVE_*)
CURVE_LEN = 16
_C_STEP, _C_EPISODES, _C_STATS, _C_LENGTH, _C_VIOL, _C_NONFINITE = 0, 1, 2, 12, 13, 14
_CURVE_WS = 4096
_CURVE_RING = 64                                                 # device rows between two harvests
_STATS = ("ret", "mean_ineq", "mean_eq", "max_ineq", "max_eq")   # eval()'s order


def curve_seed(trainer_seed, k):
    """Seed of the vector env of evaluation point k (k = 0, 1, ... over the life of a trainer) of a curve-mode run:
    ((trainer_seed ^ 0xC0A7C0A7) + 0x9E3779B97F4A7C15 * (k + 1)) mod 2^63.  Independent of ``evaluate()``'s call counter."""
    return ((int(trainer_seed) ^ 0xC0A7C0A7) + 0x9E3779B97F4A7C15 * (int(k) + 1)) & (2 ** 63 - 1)


class EvalCurve(object):
    """The learning curve of a curve-mode run (``eval_episodes=N``): numpy arrays with one entry per harvested point.

    ``step`` (vector steps done when the point was taken), ``episodes``, the ten columns of eval()'s tuple (``ret_mean``,
    ``ret_std``, ``mean_ineq_mean``, ``mean_ineq_std``, ``mean_eq_mean``, ``mean_eq_std``, ``max_ineq_mean``, ``max_ineq_std``,
    ``max_eq_mean``, ``max_eq_std``), ``length_mean``, ``violation_rate`` (``EvalResult.violation_rate()``) and ``nonfinite``
    (episodes with the non-finite bit).  ``rows``: the raw [points, 16] float64 rows (RPO_CURVE_* layout)."""

    COLUMNS = ("step", "episodes") + tuple("%s_%s" % (s, m) for s in _STATS for m in ("mean", "std")) + \
        ("length_mean", "violation_rate", "nonfinite")

    def __init__(self, rows=None):
        self.rows = np.zeros((0, CURVE_LEN)) if rows is None else np.array(rows, dtype=np.float64).reshape(-1, CURVE_LEN)

    def __len__(self):
        return self.rows.shape[0]

    @property
    def step(self):
        return self.rows[:, _C_STEP].astype(np.int64)

    @property
    def episodes(self):
        return self.rows[:, _C_EPISODES].astype(np.int64)

    @property
    def length_mean(self):
        return self.rows[:, _C_LENGTH] / self.rows[:, _C_EPISODES]

    @property
    def violation_rate(self):
        return self.rows[:, _C_VIOL] / self.rows[:, _C_LENGTH]

    @property
    def nonfinite(self):
        return self.rows[:, _C_NONFINITE].astype(np.int64)

    def summary(self, k):
        """Point k as eval()'s 10-tuple."""
        return tuple(float(x) for x in self.rows[k, _C_STATS:_C_STATS + 10])

    def __repr__(self):
        return "EvalCurve(points=%d)" % len(self)


for _i, _s in enumerate(_STATS):
    for _j, _m in enumerate(("mean", "std")):
        setattr(EvalCurve, "%s_%s" % (_s, _m), property(lambda self, c=_C_STATS + 2 * _i + _j: self.rows[:, c].copy()))


def summarize_torch(acc, ctrl, row_out):
    """``rpo_eval_summarize`` in torch ops (backends without the kernel: the CPU oracle): the accumulator rows acc [n, 8] ->
    one curve row row_out [16] float64, nothing read back to the host.  Means and population standard deviations of the
    float32 columns widened to float64, the deviations taken about the mean."""
    n = acc.shape[0]
    x = acc[:, :5].to(torch.float64)
    word = acc[:, _WORD].contiguous().view(torch.int32)
    mean = x.sum(dim=0) / n
    d = x - mean
    std = torch.sqrt((d * d).sum(dim=0) / n)
    row_out[_C_STEP] = ctrl[0].to(torch.float64)
    row_out[_C_EPISODES] = float(n)
    row_out[_C_STATS:_C_STATS + 10:2] = mean
    row_out[_C_STATS + 1:_C_STATS + 10:2] = std
    row_out[_C_LENGTH] = (word >> _LEN_SHIFT).to(torch.float64).sum()
    row_out[_C_VIOL] = acc[:, _VIOL].to(torch.float64).sum()
    row_out[_C_NONFINITE] = ((word & _NONFINITE) != 0).to(torch.float64).sum()
    row_out[CURVE_LEN - 1] = 0.0


def _rate_torch(row):
    length = row[_C_LENGTH]
    return torch.where(length == 0, torch.full_like(length, float("inf")), row[_C_VIOL] / length)


def keep_best_torch(src, best, row, best_row, best_point, point, max_violation_rate):
    """``rpo_eval_keep_best`` in torch ops (backends without the kernel: the CPU oracle), nothing read on the host: the
    criterion of include/rpo_hip.h as a 0-dim bool, then the three predicated writes."""
    ret, best_ret = row[_C_STATS], best_row[_C_STATS]
    rate, best_rate = _rate_torch(row), _rate_torch(best_row)
    safe, best_safe = rate <= max_violation_rate, best_rate <= max_violation_rate
    eligible = ~(row[_C_NONFINITE] > 0) & (ret == ret)
    wins = (best_point[0] < 0) | (safe & ~best_safe) | (safe & best_safe & (ret > best_ret)) | \
        (~safe & ~best_safe & ((rate < best_rate) | ((rate == best_rate) & (ret > best_ret))))
    take = eligible & wins
    best.copy_(torch.where(take, src, best))
    best_row.copy_(torch.where(take, row, best_row))
    best_point.copy_(torch.where(take, torch.full_like(best_point, int(point)), best_point))


def check_keep_best(keep_best):
    """The trainers' ``keep_best`` -> None (off: False / None) or ``max_violation_rate`` as a float (True: 0.0; a number
    >= 0, inf allowed).  ValueError for a negative or NaN rate and for anything that is no number."""
    if keep_best is None or keep_best is False:
        return None
    if keep_best is True:
        return 0.0
    if isinstance(keep_best, (str, bytes)) or not isinstance(keep_best, (int, float, np.integer, np.floating)):
        raise ValueError("keep_best must be False, True or a violation rate >= 0, got %r" % (keep_best,))
    rate = float(keep_best)
    if not rate >= 0.0:
        raise ValueError("keep_best: the violation rate must be >= 0, got %r" % (keep_best,))
    return rate


def keep_best_from_env(text):
    """``RPO_KEEP_BEST``: unset / "" / "0" / "false" / "off": off; "1" / "true" / "on": True; anything else: the rate."""
    t = (text or "").strip().lower()
    if t in ("", "0", "false", "off"):
        return False
    if t in ("1", "true", "on"):
        return True
    try:
        return float(t)
    except ValueError:
        raise ValueError("RPO_KEEP_BEST must be 0, 1 or a violation rate >= 0, got %r" % (text,))


class BestPolicy(object):
    """The policy a ``keep_best`` run holds: the evaluation point that won on the device (``rpo_eval_keep_best``).

    ``point``: its index (``curve_seed(seed, point)`` seeded it); ``step``: the vector steps done when it was taken;
    ``row``: its curve row as a one-point ``EvalCurve`` (``row.ret_mean[0]``, ``row.violation_rate[0]``, ...); ``params``:
    a clone of the actor's span of the flat parameter buffer at that point, float32, on the trainer's device (on the CPU
    after ``load``); ``max_violation_rate``: the rate up to which a point counted as safe."""

    def __init__(self, point, row, params, max_violation_rate):
        self.point = int(point)
        self.row = EvalCurve(row)
        self.step = int(self.row.rows[0, _C_STEP])
        self.params = params
        self.max_violation_rate = float(max_violation_rate)

    def save(self, path):
        """One .npz (point, the raw row, the parameters, the rate); ``BestPolicy.load`` reads it back."""
        with open(path, "wb") as f:
            np.savez(f, point=np.int64(self.point), row=self.row.rows[0], params=self.params.detach().cpu().numpy(),
                     max_violation_rate=np.float64(self.max_violation_rate))

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            return cls(int(z["point"]), z["row"], torch.from_numpy(np.array(z["params"], dtype=np.float32)),
                       float(z["max_violation_rate"]))

    def __repr__(self):
        return "BestPolicy(point=%d, step=%d, return=%.4f, violation_rate=%.4g)" % (
            self.point, self.step, self.row.ret_mean[0], self.row.violation_rate[0])


class CurveRunner(object):
    """The evaluation points of a curve-mode trainer (``eval_episodes=N``): enqueued by the training loop, never waited for.

    Point k is what a blocking ``trainer.evaluate(episodes=N, seed=curve_seed(trainer.seed, k))`` at the same place returns,
    reduced on the device (``rpo_eval_summarize``, or ``summarize_torch``) into row ``k mod 64`` of a device ring; the rows
    are read by ``harvest()`` (the trainer's statistics harvest, ``save()``, the ``eval_curve`` property) -- the only place
    that waits for the device.  The evaluation env, the accumulators and the ring are allocated once.

    * fused path (``fused_ok``), schedule ``eval_overlap=1``: the actor's span of the flat parameter buffer and the training
      env's step counter are copied (eager torch copies on the training stream, outside any captured window) into a snapshot;
      an event hands over to a dedicated evaluation stream, which runs reset, the evaluate launches on the SNAPSHOT and the
      summary, and records the point's event.  The training stream goes on with the update at once; the next point, the
      harvest and ``save()`` wait for that event, so two points never share the snapshot or the accumulators.
    * everything else (stepwise path; ``eval_overlap=0``): the same launches in order on the training stream.

    ``keep_best`` (None: off; else the violation rate up to which a point is safe): behind the summary, on the same stream,
    ``rpo_eval_keep_best`` compares the point's row with the incumbent's (``best_row``, ``best_point``: -1 for none) and
    copies the snapshot (overlapped) or the live actor span (in order) into ``best`` if the point wins.  No host read, no
    launch inside a captured window; off, the launches are those without it."""

    def __init__(self, tr, episodes, keep_best=None):
        self.tr, self.n = tr, check_episodes(episodes, "eval_episodes")
        self.rows = np.zeros((0, CURVE_LEN))                     # harvested
        self.points = self.done = 0                              # enqueued / harvested over the life of the trainer
        self.v = self.event = self.last_seed = None
        self.keep_rate = keep_best                               # None: off; else max_violation_rate (check_keep_best)
        self.best = self._best_pending = None
        if keep_best is not None and getattr(getattr(tr.agent, "flat", None), "actor_range", None) is None:
            raise ValueError("keep_best needs the actor in the flat parameter buffer (agent.flat.actor_range): %s has none"
                             % type(tr.agent).__name__)

    def _alloc(self):
        tr, dev = self.tr, self.tr.device
        self.v = _make_vec(tr, self.n, 0)
        self.acc = torch.zeros(self.n, 8, device=dev)
        self.ring = torch.zeros(_CURVE_RING, CURVE_LEN, dtype=torch.float64, device=dev)
        self.ws = torch.zeros(_CURVE_WS, dtype=torch.float64, device=dev)
        self.H = default_horizon(tr)
        self.fused = fused_ok(tr)
        self.overlap = bool(self.fused and tr.schedule.get("eval_overlap", 1))
        if self.overlap:
            flat = tr.agent.flat
            lo, hi = flat.actor_range
            self.src, self.snap = flat.param(flat.actor_range), torch.zeros(hi - lo, device=dev)
            self.desc = actor_desc_over(tr, self.snap)
            self.step_word = torch.zeros(1, dtype=torch.int64, device=dev)
            self.stream = torch.cuda.Stream()
        if self.keep_rate is not None:
            self._alloc_best()

    def _alloc_best(self):
        """The incumbent: the actor's span, its curve row and the index of its point (-1: none), filled outside any window."""
        if self.best is not None:
            return
        flat, dev = self.tr.agent.flat, self.tr.device
        self.live = flat.param(flat.actor_range)
        self.best = torch.zeros_like(self.live)
        self.best_row = torch.zeros(CURVE_LEN, dtype=torch.float64, device=dev)
        self.best_point = torch.full((1,), -1, dtype=torch.int64, device=dev)
        if self._best_pending is not None:
            self._load_best(self._best_pending)
            self._best_pending = None

    def enqueue(self):
        """One evaluation point with the parameters as they are now on the current (training) stream."""
        tr = self.tr
        if tr.dist.rank != 0:                                    # rank 0 evaluates, no collective (as evaluate())
            return
        if self.v is None:
            self._alloc()
        k = self.points
        if k - self.done >= _CURVE_RING:                         # the ring is harvested before it wraps
            self.harvest()
        self.v.seed = self.last_seed = curve_seed(tr.seed, k)
        row = self.ring[k % _CURVE_RING]
        with torch.no_grad():
            if self.overlap:
                main = torch.cuda.current_stream()
                if self.event is not None:
                    main.wait_event(self.event)                  # the previous point has read the snapshot
                self.snap.copy_(self.src)
                self.step_word.copy_(tr.vec.ctrl[0:1])
                ready = torch.cuda.Event()
                ready.record(main)
                self.stream.wait_event(ready)
                with torch.cuda.stream(self.stream):
                    self._point(row, self.desc, self.step_word, k, self.snap)
                    self.event = torch.cuda.Event()
                    self.event.record(self.stream)
            else:
                self._point(row, None, tr.vec.ctrl, k, self.live if self.keep_rate is not None else None)
        self.points = k + 1

    def _point(self, row, desc, ctrl, k, src):
        tr, v = self.tr, self.v
        v.ep_count.zero_()                                       # a fresh vector env: episode 0 of every lane's reset stream
        v.ctrl.zero_()
        v.reset()
        if self.fused:
            _run_fused(tr, v, self.acc, self.H, desc)
        else:
            _run_stepwise(tr, v, self.acc, self.H)
        summarize = getattr(tr.backend, "eval_summarize", None)
        if summarize is not None:
            summarize(self.acc, ctrl, row, self.ws)
        else:
            summarize_torch(self.acc, ctrl, row)
        if self.keep_rate is not None:
            # the decision and the predicated copy, behind the summary on its stream: src is the snapshot (overlapped: the
            # point's event keeps the next point from overwriting it) or the live span (in order), read before the update
            keep = getattr(tr.backend, "eval_keep_best", None) or keep_best_torch
            keep(src, self.best, row, self.best_row, self.best_point, k, self.keep_rate)

    def wait(self):
        if self.event is not None:
            self.event.synchronize()

    def harvest(self):
        """Read the outstanding rows (waits for the device) and print their ``Eval:`` lines."""
        if self.points == self.done:
            return
        self.wait()
        idx = torch.as_tensor([k % _CURVE_RING for k in range(self.done, self.points)], device=self.ring.device)
        new = self.ring[idx].cpu().numpy()
        self.rows = np.concatenate([self.rows, new], 0)
        self.done = self.points
        for r in new:
            self.tr._print_eval(int(r[_C_STEP]), tuple(float(x) for x in r[_C_STATS:_C_STATS + 10]), multipliers=False)

    def last(self):
        """The per-episode results of the last enqueued point (its accumulator rows stay on the device until the next one)."""
        if self.points == 0:
            return None
        self.wait()
        return EvalResult(self.acc.cpu().numpy(), "fused" if self.fused else "stepwise", self.H, self.last_seed)

    def state(self):
        self.harvest()
        st = dict(rows=self.rows.copy(), points=self.points, episodes=self.n)
        if self.keep_rate is not None:                           # (additional entries: a checkpoint without them has no incumbent)
            self._alloc_best()
            self.wait()
            st.update(best=self.best.clone(), best_row=self.best_row.clone(), best_point=self.best_point.clone(),
                      keep_rate=self.keep_rate)
        return st

    def load_state(self, st):
        """``st``: ``state()`` of a checkpoint, or None (a checkpoint written without curve mode: an empty curve).  The
        incumbent of a ``keep_best`` run comes back with it; a checkpoint that holds none leaves none."""
        self.wait()
        self.rows = np.zeros((0, CURVE_LEN)) if st is None else np.array(st["rows"], dtype=np.float64).reshape(-1, CURVE_LEN)
        self.points = self.done = 0 if st is None else int(st["points"])
        if self.keep_rate is not None:
            held = st if st is not None and st.get("best") is not None else None
            if self.best is None:                                # (nothing allocated yet: applied by _alloc_best)
                self._best_pending = held
            else:
                self._load_best(held)

    def _load_best(self, st):
        if st is None:
            self.best.zero_()
            self.best_row.zero_()
            self.best_point.fill_(-1)
            return
        if st["best"].numel() != self.best.numel():
            raise ValueError("checkpoint holds a best policy of %d parameters, this trainer's actor has %d"
                             % (st["best"].numel(), self.best.numel()))
        self.best.copy_(st["best"])
        self.best_row.copy_(st["best_row"])
        self.best_point.copy_(st["best_point"])

    # -------------------------------------------------------------------------------------------- the kept policy
    def _order_after_points(self):
        """The current stream waits (on the device) for the last enqueued point: its decision and copy have landed."""
        if self.event is not None:
            torch.cuda.current_stream().wait_event(self.event)

    def best_policy(self):
        """``BestPolicy`` of the incumbent, or None (no eligible point yet).  Waits for the last point's event."""
        if self.keep_rate is None or (self.best is None and self._best_pending is None):
            return None
        self._alloc_best()
        self.wait()
        point = int(self.best_point.cpu()[0])
        if point < 0:
            return None
        return BestPolicy(point, self.best_row.cpu().numpy(), self.best.clone(), self.keep_rate)

    def restore_best(self):
        """live actor span <- the kept span where a point is held, as device copies on the current stream: no host read."""
        self._alloc_best()
        self._order_after_points()
        with torch.no_grad():
            self.live.copy_(torch.where(self.best_point[0] >= 0, self.best, self.live))
