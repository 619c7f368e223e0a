"""Scenarios of EVOPF-v0 on the MI355X: the table the device deals (rpo_evopf_scenario_table) against the oracle, the table-fed
reset and step (rpo_evopf_reset_scenario / rpo_evopf_step_scenario) against the Philox-dealt ones bit for bit, whole evaluations
on the dealt days bit for bit, and a caller's days (tests/golden/evopf_days.npz through ``Scenarios.from_system_days``) through
``trainer.evaluate`` / ``rpo_amd.algo.evaluate_opf``.  5 lanes throughout the kernel tests: one full four-wave workgroup and a ragged one.
The host side: tests/test_scenarios.py."""
import functools

import numpy as np
import pytest
import torch

from oracle import evopf as oe
from rpo_amd import _lib
from rpo_amd.algo import evaluate_opf
from rpo_amd.algo.evaluation import EvalTrajectory
from rpo_amd.env.electrical_grid.scenarios import Scenarios
from test_scenarios import fixture_days
from test_train_step_golden import build_trainer

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
N = 5
SEED = 77


@functools.lru_cache(maxsize=None)
def _env():
    from rpo_amd.env import EVOPFEnv
    assert torch.cuda.is_available()
    return EVOPFEnv(device=DEV)


@functools.lru_cache(maxsize=None)
def _trainer():
    """RPODDPG with the fused 256-wide actor and schedule fused_eval_evopf = 1 (a call without a record, a noise or scenarios
    takes the fused evaluation kernel), a few updates off its initialisation; shared by the tests, which change nothing in it."""
    from rpo_amd import ops
    torch.manual_seed(5)
    tr = build_trainer("ddpg", "evopf256", ops, DEV, num_envs=16, use_graph=False, schedule=dict(fused_eval_evopf=1))
    tr.vec.reset()
    tr.run_steps(8)
    return tr


@functools.lru_cache(maxsize=None)
def _days():
    """Three of the fixture's days (the negative-price one among them), demand up by 10 %."""
    z = fixture_days()
    S = Scenarios.from_system_days(_env(), z["load"], z["price"], seed=0)[2:5].scale_demand(1.1)
    assert S.price.min() < 0 and (S.price[:, 24:] != 0).all()
    return S


def bits(x):
    x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return x.view(np.int32) if x.dtype == np.float32 else x


def same(a, b):
    """bitwise, NaNs included"""
    a, b = bits(a), bits(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def assert_same_result(a, b, fields=None):
    for f in fields or a.FIELDS:
        assert same(getattr(a, f), getattr(b, f)), f
    if a.trajectory is not None or b.trajectory is not None:
        for name in EvalTrajectory.ARRAYS:
            assert same(getattr(a.trajectory, name), getattr(b.trajectory, name)), name


# ------------------------------------------------------------------------------------------------ 1. the table
@pytest.mark.parametrize("episode", [0, 3])
def test_table_matches_the_oracle(episode):
    S = _env().scenarios(N, SEED, env_id_base=5, episode=episode)
    assert len(S) == N
    ids = 5 + np.arange(N)
    for t in range(24):                                          # test_evopf_gpu.py::test_reset_matches_oracle's tolerance
        np.testing.assert_allclose(S.demand[:, t], oe.episode_demand(SEED, ids, episode, t), rtol=1e-5, atol=2e-5, err_msg=str(t))
    np.testing.assert_allclose(S.price[:, :24], oe.episode_price(SEED, ids, episode, 0), rtol=1e-5, atol=2e-5)
    assert same(S.price[:, 24:], np.zeros((N, 24), dtype=np.float32))
    # another episode, another lane block: other days
    other = _env().scenarios(N, SEED, env_id_base=5, episode=episode + 1)
    assert not np.array_equal(other.demand, S.demand) and not np.array_equal(other.price, S.price)


# ------------------------------------------------------------------------------------------------ 2. reset and step
def _actions(steps):
    """One action sequence [steps, N, 43] for both envs: in the neighbourhood of a dispatch (|v| near 1, small angles, some
    generation and battery power), nothing either env could tell apart."""
    g = torch.Generator().manual_seed(3)
    a = torch.zeros(steps, N, 43)
    a[:, :, 0:10] = torch.rand(steps, N, 10, generator=g) * 0.6
    a[:, :, 10:24] = 1.0 + 0.05 * (torch.rand(steps, N, 14, generator=g) - 0.5)
    a[:, :, 24:38] = 0.2 * (torch.rand(steps, N, 14, generator=g) - 0.5)
    a[:, :, 38:43] = 0.4 * (torch.rand(steps, N, 5, generator=g) - 0.5)
    return a.to(DEV)


def test_table_fed_equals_philox_dealt_bit_for_bit():
    env = _env()
    S = env.scenarios(N, SEED)
    plain = env.make_vec(N, seed=SEED)
    fed = env.make_vec(N, seed=SEED, scenario=(S.table(DEV), torch.arange(N, dtype=torch.int32, device=DEV)))
    rows_a, rows_b = (torch.full((N, env.kernels.ring_floats), 7.0, device=DEV) for _ in range(2))

    def compare(what):
        for name in ("internal", "ep_len", "ep_ret"):
            assert same(getattr(plain, name), getattr(fed, name)), (what, name)
        assert same(rows_a, rows_b), (what, "row")

    plain.reset()
    fed.reset()
    compare("reset")
    assert float(plain.internal.abs().sum()) > 0
    steps = 25                                                   # the 25th step runs past the end of the day
    actions = _actions(steps)
    for t in range(steps):
        plain.step(actions[t], rows=rows_a, cap_steps=1, auto_reset=False)
        fed.step(actions[t], rows=rows_b, cap_steps=1, auto_reset=False)
        compare(t)
    obs = fed.internal.cpu().numpy()
    assert (obs[:, :28] == 0).all() and (obs[:, 33:] == 0).all() and int(fed.ep_len[0]) == steps
    assert same(plain.ctrl, fed.ctrl) and int(fed.ctrl[_lib.CONST["RPO_CTRL_T"]]) == steps
    # the statistics: the four waves of a workgroup add into one address in the order they arrive (float32 atomics), so two runs
    # of ONE kernel agree to the reassociation of four terms only: 3 roundings of 2^-24 relative to the largest partial sum
    np.testing.assert_allclose(fed.stats.cpu().numpy(), plain.stats.cpu().numpy(), rtol=1e-6, atol=1e-6 * float(plain.stats.abs().max()))
    assert float(plain.stats.abs().sum()) > 0
    with pytest.raises(ValueError):
        fed.step(actions[0], rows=rows_b, cap_steps=1)           # never auto-resets


def test_a_day_outside_the_table_is_never_read():
    """day[i] outside [0, days): the lane's observation is NaN and the failure word is set; its neighbours play their days."""
    env = _env()
    S = env.scenarios(3, SEED)
    day = torch.tensor([1, -1, 3, 2 ** 31 - 1, 0], dtype=torch.int32, device=DEV)
    v = env.make_vec(N, seed=SEED, scenario=(S.table(DEV), day))
    v.reset()
    obs = v.internal.cpu().numpy()
    data = np.r_[0:28, 33:57]
    for lane, d in ((0, 1), (4, 0)):
        assert same(obs[lane, :28], S.demand[d, 0]) and same(obs[lane, 33:], S.price[d, :24])
    assert np.isnan(obs[[1, 2, 3]][:, data]).all() and (obs[:, 28:33] == np.float32(0.2)).all()
    rows = torch.zeros(N, env.kernels.ring_floats, device=DEV)
    assert int(v.ctrl[_lib.CONST["RPO_CTRL_NONFINITE"]]) == 0
    v.step(_actions(1)[0], rows=rows, cap_steps=1, auto_reset=False)
    obs = v.internal.cpu().numpy()
    assert same(obs[0, :28], S.demand[1, 1]) and same(obs[4, 33:], S.price[0, 1:25])
    assert np.isnan(obs[[1, 2, 3]][:, data]).all() and int(v.ctrl[_lib.CONST["RPO_CTRL_NONFINITE"]]) != 0


# ------------------------------------------------------------------------------------------------ 3. whole evaluations
def test_evaluations_on_the_dealt_days_are_the_philox_evaluations():
    tr = _trainer()
    s = 11
    S = tr.base_env.scenarios(8, seed=s)
    base = tr.evaluate(8, seed=s, record=True)
    fed = tr.evaluate(8, seed=s, record=True, scenarios=S)
    assert base.path == fed.path == "stepwise" and base.days is None and np.array_equal(fed.days, np.arange(8))
    assert (base.length == 24).all() and base.proj_iters.sum() > 0
    assert_same_result(base, fed)
    # the fused kernel has no table-fed instance: a call with scenarios steps, and gives the fused call's bits
    fused = tr.evaluate(8, seed=s)
    fed_plain = tr.evaluate(8, seed=s, scenarios=S)
    assert fused.path == "fused" and fed_plain.path == "stepwise" and fed_plain.trajectory is None
    assert_same_result(fused, fed_plain)
    for f in fused.FIELDS:                                       # ... which are the recorded call's too
        assert same(getattr(fused, f), getattr(fed, f)), f


def test_opf_evaluations_on_the_dealt_days_are_the_philox_evaluations():
    tr = _trainer()
    s = 12
    S = tr.base_env.scenarios(4, seed=s)
    base = tr.evaluate_opf(4, seed=s, record=True)
    fed = evaluate_opf(tr, 4, seed=s, record=True, scenarios=S)   # (the method's parameter list is fixed)
    assert base.path == fed.path == "opf" and np.array_equal(fed.days, np.arange(4)) and base.opf_converged.any()
    assert_same_result(base, fed)
    assert same(base.opf_iters, fed.opf_iters) and same(base.opf_converged, fed.opf_converged)


# ------------------------------------------------------------------------------------------------ 4. the caller's days
@functools.lru_cache(maxsize=None)
def _caller_run():
    return _trainer().evaluate(7, record=True, scenarios=_days(), seed=1)


def test_the_callers_days_are_what_the_policy_sees():
    tr, S, res = _trainer(), _days(), _caller_run()
    tj = res.trajectory
    assert res.path == "stepwise" and np.array_equal(res.days, np.arange(7) % 3) and (res.length == 24).all()
    for e in range(7):
        d = e % 3
        for t in range(24):
            assert same(tj.obs[e, t, 0:28], S.demand[d, t]), (e, t)
            assert same(tj.obs[e, t, 33:57], S.price[d, t:t + 24]), (e, t)     # the look-ahead runs past midnight
    assert (tj.obs[:, 1:, 56] != 0).all()
    # episodes 0 and 3: the same day, a deterministic policy, the same start -- rows do not depend on their neighbours
    for f in res.FIELDS:
        assert same(getattr(res, f)[0], getattr(res, f)[3]), f
    for name in EvalTrajectory.ARRAYS:
        assert same(getattr(tj, name)[0], getattr(tj, name)[3]), name
    assert not same(tj.obs[0], tj.obs[1])
    # the reward is the env's formula on what was recorded (tests/test_evopf_opf_free.py's tolerance for reward_fn)
    assert not res.nonfinite.any()
    reward = tr.base_env.reward_fn(tj.obs.reshape(-1, 57).astype(np.float64), tj.action.reshape(-1, 43).astype(np.float64))
    assert np.allclose(tj.reward.reshape(-1), reward, rtol=1e-5, atol=1e-5), np.abs(tj.reward.reshape(-1) - reward).max()
    # init_states still override hour 0: the day goes on from the injected state of charge
    init = torch.tensor(tj.obs[:, 0], device=DEV)
    init[:, 28:33] = 0.5
    inj = tr.evaluate(7, record=True, scenarios=S, seed=1, init_states=init).trajectory
    assert (inj.obs[:, 0, 28:33] == 0.5).all() and same(inj.obs[:, :, :28], tj.obs[:, :, :28]) and same(inj.obs[:, :, 33:], tj.obs[:, :, 33:])


def test_obs_noise_on_the_callers_days_is_keyed_by_the_seed():
    tr, S = _trainer(), _days()
    a = tr.evaluate(7, record=True, scenarios=S, seed=1, obs_noise=0.05)
    b = tr.evaluate(7, record=True, scenarios=S, seed=1, obs_noise=0.05)
    c = tr.evaluate(7, record=True, scenarios=S, seed=2, obs_noise=0.05)
    assert_same_result(a, b)
    assert not same(a.trajectory.obs, c.trajectory.obs) and not same(a.trajectory.obs, _caller_run().trajectory.obs)
    assert np.array_equal(a.days, c.days) and np.array_equal(a.days, np.arange(7) % 3)
    # the env steps the true days: without noise the seed keys nothing
    d, e = tr.evaluate(7, scenarios=S, seed=1), tr.evaluate(7, scenarios=S, seed=2)
    assert_same_result(d, e)


def test_budget_and_constraints_work_as_on_the_stepwise_path():
    tr, S = _trainer(), _days()
    res = tr.evaluate(7, scenarios=S, seed=1, eval_steps=0, constraints=True, record=2)
    assert res.path == "stepwise" and (res.proj_iters == 0).all() and res.trajectory.episodes == 2
    assert np.array_equal(res.constraints.eq_max.max(axis=1), res.max_eq)
    full = _caller_run()
    assert same(res.trajectory.obs[:, 0], full.trajectory.obs[:2, 0]) and full.proj_iters.sum() > 0


# ------------------------------------------------------------------------------------------------ 5. the paired comparison
def test_policy_and_opf_controller_play_the_same_days():
    tr, S = _trainer(), _days()
    policy = _caller_run()
    opf = evaluate_opf(tr, 7, record=True, scenarios=S, seed=1)
    assert opf.path == "opf" and np.array_equal(opf.days, policy.days)
    assert same(opf.trajectory.obs[:, 0], policy.trajectory.obs[:, 0])
    assert same(opf.trajectory.obs[:, :, :28], policy.trajectory.obs[:, :, :28])
    assert same(opf.trajectory.obs[:, :, 33:], policy.trajectory.obs[:, :, 33:])
    assert opf.opf_converged.any()
