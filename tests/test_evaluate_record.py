"""trainer.evaluate(record=...) on the CPU: the stepwise path driven by the oracle backend (``record_torch``).

Three checks recur here and in test_evaluate_record_gpu.py (which imports the helpers below):

* **arrays-equal** -- every ``EvalResult`` array of a recording evaluation is bit-equal to the same call without it.
* **replay** -- each recorded episode's valid steps, folded in numpy float32 and in step order through the arithmetic of
  ``rpo_eval_lane_update`` (sequential reward sum, running means with the float32 reciprocal of step + 1, NaN-propagating
  maxima, threshold count, iteration sum), give ``ret``, ``mean_ineq``, ``mean_eq``, ``max_ineq``, ``max_eq``, ``viol_steps``,
  ``proj_iters`` and ``length`` bit for bit; no step before the last valid one is done, and an episode shorter than the
  horizon ends on a done step.  (The converse does not hold: an episode may terminate, or meet the TimeLimit, on the very
  step that is also the horizon's last -- length == horizon with done set, e.g. every 200-step episode at the default
  horizon of 200.)
* **dynamics** -- ``obs[e, t]`` and ``action[e, t]`` go through the CPU oracle env (oracle/cartsafe.py, oracle/pendulum.py);
  its next observation, reward and violations are ``obs[e, t + 1]``, ``reward[e, t]``, ``ineq[e, t]`` and ``eq[e, t]``.  This
  pins the record to something other than the code under test.

Dynamics tolerances.  CartSafe-v0: the observation is the state, so the oracle sees exactly what the backend saw; on the
oracle backend (which rounds the oracle's float64 step to float32) the match is exact, and asserted as such.
SpringPendulum-v0: the observation carries (cos, sin) of the angle, not the angle; the helper recovers it with arctan2 from
the float32 pair (|theta| < pi / 12 on a live step, error below 1e-7), so the match is to round-off: float32 quantities at
test_oracle_golden.py's F32_TOL, the violations at test_pendulum_step's tolerance there.  The GPU file passes the
tolerances of the step-kernel-vs-fixture tests of test_kernels_gpu.py.
"""
import numpy as np
import pytest
import torch

import oracle_backend as ob
from oracle import cartsafe as cs
from oracle import pendulum as pd
from test_eval_golden import CASES
from test_train_step_golden import build_trainer

F32 = np.float32
RESULT_ARRAYS = ("ret", "length", "mean_ineq", "mean_eq", "max_ineq", "max_eq", "viol_steps", "proj_iters", "nonfinite")

# (next-observation columns, rtol, atol) groups, reward, ineq, eq tolerances; None = exact
EXACT = dict(next_obs=None, reward=None, ineq=None, eq=None)
PEND_CPU_TOL = dict(next_obs=[(slice(None), 2e-6, 2e-6)], reward=(2e-6, 2e-6), ineq=(2e-6, 1e-5), eq=(2e-6, 1e-5))


# ------------------------------------------------------------------------------------------------ shared helpers
def assert_arrays_equal(a, b):
    for f in RESULT_ARRAYS:
        np.testing.assert_array_equal(getattr(a, f), getattr(b, f), err_msg=f)
    assert a.path == b.path and a.horizon == b.horizon


def _nanmax(a, b):
    """rpo_eval_dev::nanmax"""
    return a if a != a else (b if b != b else (b if b > a else a))


def replay_episode(tj, e, divide=False):
    """The valid steps of episode e through rpo_eval_lane_update's arithmetic, float32 -> the accumulator's fields.
    ``divide``: the running means as ``accumulate_torch`` computes them on the CPU (see the CPU suite below)."""
    ret = mi = me = xi = xe = F32(0)
    viol = iters = n = 0
    thresh = F32(tj.viol_thresh)
    for t in range(tj.horizon):
        if not tj.valid[e, t]:
            continue
        assert n == t, "valid steps are a prefix"
        reward, ineq, eq = tj.reward[e, t], tj.ineq[e, t], tj.eq[e, t]
        inv = F32(1) / F32(t + 1)
        with np.errstate(invalid="ignore", over="ignore"):
            ret = F32(ret + reward)
            if divide:
                mi = F32(mi + F32(F32(ineq - mi) / F32(t + 1)))
                me = F32(me + F32(F32(eq - me) / F32(t + 1)))
            else:
                mi = F32(mi + F32(F32(ineq - mi) * inv))
                me = F32(me + F32(F32(eq - me) * inv))
        xi, xe = _nanmax(xi, ineq), _nanmax(xe, eq)
        viol += int(ineq > thresh)
        iters += int(tj.iters[e, t])
        n += 1
    return dict(ret=ret, mean_ineq=mi, mean_eq=me, max_ineq=xi, max_eq=xe, viol_steps=viol, proj_iters=iters, length=n)


def assert_replay(r, episodes=None, divide=False):
    tj = r.trajectory
    for e in (range(tj.episodes) if episodes is None else episodes):
        got = replay_episode(tj, e, divide)
        for f in ("ret", "mean_ineq", "mean_eq", "max_ineq", "max_eq"):
            want = F32(getattr(r, f)[e])
            assert got[f].tobytes() == want.tobytes(), (e, f, got[f], want)
        for f in ("viol_steps", "proj_iters", "length"):
            assert got[f] == int(getattr(r, f)[e]), (e, f, got[f], getattr(r, f)[e])
        n = got["length"]
        assert n >= 1 and (bool(tj.done[e, n - 1]) or n == r.horizon), (e, n)
        assert not tj.done[e, :n - 1].any(), e


def assert_zero_outside_valid(tj):
    inv = ~tj.valid
    for name in ("obs", "proposal", "action", "reward", "ineq", "eq", "iters", "done"):
        assert not np.any(getattr(tj, name)[inv]), name


def _close(got, want, tol, what):
    if tol is None:
        np.testing.assert_array_equal(got, want, err_msg=what)
    else:
        np.testing.assert_allclose(got, want, rtol=tol[0], atol=tol[1], err_msg=what)


def assert_dynamics(r, envname, tol, max_episode_steps=200, episodes=None):
    """Every valid step of the recorded episodes through the oracle env, all steps of all episodes in one batch."""
    tj = r.trajectory
    E = np.arange(tj.episodes) if episodes is None else np.asarray(episodes)
    valid = tj.valid[E]
    e_idx, t_idx = np.nonzero(valid)
    obs, action = tj.obs[E][e_idx, t_idx], tj.action[E][e_idx, t_idx]
    if envname == "cart":
        nxt, reward, term, ineq, eq = cs.step(obs.astype(np.float64), action, cs.Constants(1))
    else:
        internal = np.stack([np.arctan2(obs[:, 1].astype(np.float64), obs[:, 0].astype(np.float64)), obs[:, 2], obs[:, 3],
                             obs[:, 4]], axis=1).astype(np.float64)
        _, nxt, reward, term, ineq, eq = pd.step(internal, action)
    _close(tj.reward[E][e_idx, t_idx], reward.astype(F32), tol["reward"], "reward")
    _close(tj.ineq[E][e_idx, t_idx], ineq.max(axis=1), tol["ineq"], "ineq")
    _close(tj.eq[E][e_idx, t_idx], np.abs(eq).max(axis=1), tol["eq"], "eq")
    # the next observation, where the episode went on
    has_next = np.zeros_like(valid)
    has_next[:, :-1] = valid[:, 1:]
    sel = has_next[e_idx, t_idx]
    nobs = tj.obs[E][e_idx[sel], t_idx[sel] + 1]
    if tol["next_obs"] is None:
        np.testing.assert_array_equal(nobs, nxt[sel].astype(F32), err_msg="next obs")
    else:
        for cols, rtol, atol in tol["next_obs"]:
            np.testing.assert_allclose(nobs[:, cols], nxt[sel][:, cols], rtol=rtol, atol=atol, err_msg="next obs")
    assert sel.sum() > 0
    # done = the env's own termination or the TimeLimit; exact only where the dynamics are (a state within round-off of a
    # threshold may end an episode a step earlier or later in float32)
    if tol["next_obs"] is None:
        np.testing.assert_array_equal(tj.done[E][e_idx, t_idx], term | (t_idx + 1 >= max_episode_steps), err_msg="done")


# ------------------------------------------------------------------------------------------------ the CPU suite
def _trainer(golden, algo, envname, tag):
    g = golden("eval_%s_%s%s" % (algo, envname, tag))
    torch.manual_seed(1)
    tr = build_trainer(algo, envname, ob, torch.device("cpu"), num_envs=1, use_graph=False)
    sd = {k[len("actor."):]: torch.tensor(g[k]) for k in g.files if k.startswith("actor.")}
    tr.agent.actor.load_state_dict(sd)
    return g, tr


# Replay on this backend.  rpo_eval_lane_update does not run here: the accumulators are ``accumulate_torch``'s, whose running
# means are eval()'s ``(x - m) / (i + 1)`` -- on the CPU a true float32 division (test_evaluate.py pins
# ``summary() == eval()`` to the bit), on the GPU torch's ``x * (1 / b)``, which is what the kernel spells out.  A replay
# with the reciprocal differs from the CPU accumulators in the last bit (measured: sac-pendulum, episode 2, mean_eq
# 2.3841858e-07 against 2.3841856e-07), so the CPU replay divides, and everything else is the kernel's arithmetic; the
# GPU suite replays with the reciprocal.
CPU = dict(divide=True)


@pytest.mark.parametrize("algo,envname,tag", CASES)
def test_recording_changes_no_result_and_replays(golden, algo, envname, tag):
    """Arrays-equal, eval()'s 10-tuple, replay and dynamics on the reference-trained policies of tests/golden/eval_*.npz."""
    torch.set_num_threads(1)
    g, tr = _trainer(golden, algo, envname, tag)
    init = torch.tensor(g["init"], dtype=torch.float32)
    plain = tr.evaluate(10, init_states=init)
    r = tr.evaluate(10, init_states=init, record=True)
    assert plain.trajectory is None and r.path == "stepwise"
    assert_arrays_equal(r, plain)
    tr._eval_init_inject = init
    assert r.summary() == tuple(tr.eval())                    # the golden cases' 10-tuple, with recording on
    tj = r.trajectory
    k = tr.kernels
    assert tj.episodes == 10 and tj.horizon == r.horizon
    assert tj.obs.shape == (10, r.horizon, k.obs_dim) and tj.proposal.shape == (10, r.horizon, k.partial_dim)
    assert tj.action.shape == (10, r.horizon, k.action_dim) and tj.iters.shape == tj.valid.shape == (10, r.horizon)
    np.testing.assert_array_equal(tj.length, r.length)
    np.testing.assert_array_equal(tj.valid.sum(axis=1), r.length)
    assert_zero_outside_valid(tj)
    assert_replay(r, **CPU)
    assert_dynamics(r, envname, EXACT if envname == "cart" else PEND_CPU_TOL)
    # the proposal is the action's basic coordinate before the projection moved it
    p = 1 if envname == "cart" else 0
    moved = np.abs(tj.action[..., p] - tj.proposal[..., 0])[tj.valid]
    assert np.isfinite(moved).all()
    if tag:
        assert moved.max() > 0 and tj.iters.max() > 0


@pytest.mark.parametrize("algo,envname", [("ddpg", "cart"), ("sac", "pendulum")])
def test_record_k_records_the_first_k_episodes(algo, envname):
    torch.set_num_threads(1)
    torch.manual_seed(5)
    tr = build_trainer(algo, envname, ob, torch.device("cpu"), num_envs=4, use_graph=False, capacity=8)
    full = tr.evaluate(6, seed=3, horizon=9, record=True)
    part = tr.evaluate(6, seed=3, horizon=9, record=2)
    none = tr.evaluate(6, seed=3, horizon=9, record=0)
    assert none.trajectory is None and tr.evaluate(6, seed=3, horizon=9, record=False).trajectory is None
    assert_arrays_equal(full, part)
    assert_arrays_equal(full, none)
    assert full.trajectory.episodes == 6 and part.trajectory.episodes == 2 and part.trajectory.horizon == 9
    for name in part.trajectory.ARRAYS:
        np.testing.assert_array_equal(getattr(part.trajectory, name), getattr(full.trajectory, name)[:2], err_msg=name)
    assert_replay(part, **CPU)
    ep = full.trajectory.episode(4)
    n = int(full.length[4])
    assert set(ep) == {"obs", "proposal", "action", "reward", "done", "ineq", "eq", "iters"}
    assert all(len(x) == n for x in ep.values())
    np.testing.assert_array_equal(ep["obs"], full.trajectory.obs[4, :n])


def test_record_validates_its_argument(golden):
    _, tr = _trainer(golden, "ddpg", "cart", "")
    for bad in (-1, 5, 1.5, "all", None, [1]):
        with pytest.raises(ValueError, match="record"):
            tr.evaluate(4, horizon=3, record=bad)
    assert tr.evaluate(4, horizon=3, record=4).trajectory.episodes == 4
    # 20000 episodes x 1000 steps x 16 floats = 1.28e9 bytes: above the 2^30 cap, refused before anything is allocated
    with pytest.raises(ValueError, match=r"record.*1280000000"):
        tr.evaluate(20000, horizon=1000, record=True)
    assert tr.evaluate(20000, horizon=1, record=3).trajectory.episodes == 3


def test_violations_and_save_load(golden, tmp_path):
    torch.set_num_threads(1)
    g, tr = _trainer(golden, "ddpg", "cart", "_sat")          # the shifted actor leaves violations behind the projection
    r = tr.evaluate(10, init_states=torch.tensor(g["init"], dtype=torch.float32), record=7)
    tj = r.trajectory
    v = tj.violations()
    assert v.shape == (int(r.viol_steps[:7].sum()), 2) and len(v) > 0
    np.testing.assert_array_equal(np.bincount(v[:, 0], minlength=7), r.viol_steps[:7])
    assert (tj.ineq[v[:, 0], v[:, 1]] > tj.viol_thresh).all() and tj.valid[v[:, 0], v[:, 1]].all()
    path = str(tmp_path / "traj.npz")
    tj.save(path)
    from rpo_amd.algo import EvalTrajectory
    back = EvalTrajectory.load(path)
    for name in tj.ARRAYS:
        a, b = getattr(tj, name), getattr(back, name)
        assert a.dtype == b.dtype and a.shape == b.shape, name
        np.testing.assert_array_equal(a, b, err_msg=name)
    assert back.viol_thresh == tj.viol_thresh
    np.testing.assert_array_equal(back.violations(), v)


@pytest.mark.parametrize("algo,envname", [("ddpg", "cart"), ("sac", "pendulum")])
def test_recording_evaluate_leaves_the_trainer_untouched(algo, envname):
    """test_evaluate_leaves_the_trainer_untouched with recording on."""
    torch.set_num_threads(1)
    dev = torch.device("cpu")

    def fresh():
        torch.manual_seed(5)
        tr = build_trainer(algo, envname, ob, dev, num_envs=4, use_graph=False, capacity=8)
        tr.vec.reset()
        return tr
    a = fresh()
    a.run_steps(10)
    b = fresh()
    b.run_steps(5)
    r = b.evaluate(5, horizon=20, record=True)
    assert r.trajectory.episodes == 5 and r.length.min() >= 1
    b.run_steps(5)
    for name in ("internal", "obs", "action", "ep_len", "ep_ret", "ep_count", "ctrl", "stats"):
        assert torch.equal(getattr(a.vec, name), getattr(b.vec, name)), name
    assert torch.equal(a.buffer.rows, b.buffer.rows)
    assert torch.equal(a.agent.flat.data, b.agent.flat.data)
    assert torch.equal(a.agent.critic_target_flat, b.agent.critic_target_flat)
    assert torch.equal(a.agent.nju.weight, b.agent.nju.weight)
    assert a._t == b._t == 10


def test_lagrangian_baseline_records_its_action_as_the_proposal():
    torch.set_num_threads(1)
    torch.manual_seed(5)
    tr = build_trainer("ddpgla", "cart", ob, torch.device("cpu"), num_envs=4, fused=False)
    r = tr.evaluate(3, seed=2, horizon=6, record=True)
    tj = r.trajectory
    assert r.path == "stepwise" and tj.proposal.shape == tj.action.shape == (3, 6, 2)
    np.testing.assert_array_equal(tj.proposal, tj.action)
    assert not tj.iters.any()
    assert_arrays_equal(r, tr.evaluate(3, seed=2, horizon=6))
    assert_replay(r, **CPU)
