"""trainer.evaluate() on EVOPF-v0 under schedule ``fused_eval_evopf=1``: ``rpo_evopf_evaluate`` (csrc/evopf_eval.hip) against the
stepwise path of the same build, bit for bit on every field of ``EvalResult`` and of the ``ConstraintReport``.

The shapes are the smallest that can still go wrong: a 16-lane trainer with the fused 256-wide MLPs, 3 episodes (one ragged
workgroup of four waves), 5 (a full and a ragged one) and 37 (nine full, one ragged), whole 24-step days unless a test cuts them.
The trainers are built once per algorithm; every test leaves the switch on."""
import numpy as np
import pytest
import torch

from test_train_step_golden import build_trainer

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
DAY = 24
SOC = slice(28, 33)                                              # the five state-of-charge columns of the EVOPF state


@pytest.fixture(scope="module")
def hip():
    from rpo_amd import ops
    assert torch.cuda.is_available()
    return ops


@pytest.fixture(scope="module")
def trainers(hip):
    made = {}

    def get(algo):
        if algo not in made:
            torch.manual_seed(5)
            tr = build_trainer(algo, "evopf256", hip, DEV, num_envs=16, use_graph=False, schedule=dict(fused_eval_evopf=1))
            tr.vec.reset()
            tr.run_steps(8)                                      # a policy that has moved off its initialisation
            made[algo] = tr
        return made[algo]
    return get


def _on_off(tr, **kw):
    tr.schedule["fused_eval_evopf"] = 1
    a = tr.evaluate(**kw)
    tr.schedule["fused_eval_evopf"] = 0
    b = tr.evaluate(**kw)
    tr.schedule["fused_eval_evopf"] = 1
    assert a.path == "fused" and b.path == "stepwise"
    return a, b


def _equal(a, b, sl=slice(None)):
    for f in a.FIELDS:
        np.testing.assert_array_equal(getattr(a, f)[sl], getattr(b, f), err_msg=f)


@pytest.mark.parametrize("episodes", [3, 37])
@pytest.mark.parametrize("algo", ["ddpg", "sac"])
def test_fused_equals_stepwise_bit_for_bit(trainers, algo, episodes):
    a, b = _on_off(trainers(algo), episodes=episodes, seed=11)
    _equal(a, b)
    assert (a.length == DAY).all() and a.proj_iters.sum() > 0


@pytest.mark.parametrize("algo", ["ddpg", "sac"])
def test_lanes_are_independent_of_n(trainers, algo):
    tr = trainers(algo)
    big, small = tr.evaluate(37, seed=21), tr.evaluate(5, seed=21)
    assert big.path == small.path == "fused"
    _equal(big, small, slice(0, 5))


def test_launch_split_changes_no_bit(trainers, hip, monkeypatch):
    tr = trainers("ddpg")
    whole = tr.evaluate(5, seed=31, constraints=True)
    launches = []
    inner = hip.evopf_evaluate
    monkeypatch.setattr(hip, "evopf_evaluate", lambda *a, **k: (launches.append((a[10], a[11])), inner(*a, **k))[1])
    monkeypatch.setattr(hip, "EVOPF_EVAL_LANE_STEPS", 15)        # 3 steps per launch at n = 5
    split = tr.evaluate(5, seed=31, constraints=True)
    assert launches == [(t0, 3) for t0 in range(0, DAY, 3)]
    assert whole.path == split.path == "fused"
    _equal(whole, split)
    for f in ("ineq_max", "ineq_steps", "eq_max"):
        np.testing.assert_array_equal(getattr(whole.constraints, f), getattr(split.constraints, f), err_msg=f)


@pytest.mark.parametrize("horizon,length", [(26, DAY), (5, 5)])
def test_horizons(trainers, horizon, length):
    a, b = _on_off(trainers("sac"), episodes=5, seed=41, horizon=horizon)
    _equal(a, b)
    assert (a.length == length).all()


@pytest.mark.parametrize("budget", [dict(eval_steps=0), dict(eval_steps=3, eval_lr=None)])
def test_budget_per_call(trainers, budget):
    tr = trainers("ddpg")
    if "eval_lr" in budget:
        budget = dict(budget, eval_lr=2 * tr.eval_lr)
    a, b = _on_off(tr, episodes=5, seed=51, **budget)
    _equal(a, b)
    assert a.proj_iters.max() <= budget["eval_steps"] * DAY


@pytest.mark.parametrize("algo", ["ddpg", "sac"])
def test_constraint_report(trainers, algo):
    a, b = _on_off(trainers(algo), episodes=5, seed=61, constraints=True)
    _equal(a, b)
    ca, cb = a.constraints, b.constraints
    assert ca.ineq_max.shape == ca.ineq_steps.shape == (5, 58) and ca.eq_max.shape == (5, 28)
    for f in ("ineq_max", "ineq_steps", "eq_max", "length"):
        np.testing.assert_array_equal(getattr(ca, f), getattr(cb, f), err_msg=f)
    np.testing.assert_array_equal(ca.ineq_max.max(1), a.max_ineq)
    np.testing.assert_array_equal(ca.eq_max.max(1), a.max_eq)


def test_init_states(trainers):
    tr = trainers("ddpg")
    v = tr.base_env.make_vec(5, seed=71, max_episode_steps=tr.max_episode_steps, device=DEV, stats_cap=2)
    v.reset()
    init = v.internal.clone()
    init[:, SOC] = 0.5
    a, b = _on_off(tr, episodes=5, seed=71, init_states=init)
    _equal(a, b)
    plain = tr.evaluate(5, seed=71)
    assert not np.array_equal(plain.ret, a.ret)                  # the injected charge is what the episodes started from


@pytest.mark.parametrize("algo", ["ddpg", "sac"])
def test_summary_equals_eval(trainers, algo):
    """The arrangement of test_stepwise_only_configurations: eval() gets the evaluation's own vector env, its episode counter set
    so that its reset draws episode 0."""
    tr = trainers(algo)
    r = tr.evaluate(10, seed=4)
    assert r.path == "fused"
    tr._vec_eval = tr.base_env.make_vec(10, seed=4, max_episode_steps=tr.max_episode_steps, device=DEV, stats_cap=2)
    tr._vec_eval.ep_count.fill_(-1)
    tr._eval_rows = torch.zeros(10, tr.kernels.ring_floats, device=DEV)
    assert r.summary() == tuple(tr.eval())


def test_no_side_effects_on_the_device(trainers, hip):
    tr = trainers("sac")
    torch.cuda.synchronize()
    snap = {k: getattr(tr.vec, k).clone() for k in ("internal", "ep_len", "ep_ret", "ep_count", "ctrl", "stats")}
    rows, flat = tr.buffer.rows.clone(), tr.agent.flat.data.clone()
    r = tr.evaluate(37, constraints=True)
    assert r.path == "fused"
    torch.cuda.synchronize()
    for k, x in snap.items():
        assert torch.equal(getattr(tr.vec, k), x), k
    assert int(tr.vec.ctrl[hip.CONST["RPO_CTRL_NONFINITE"]]) == 0
    assert torch.equal(tr.buffer.rows, rows) and torch.equal(tr.agent.flat.data, flat)


@pytest.mark.parametrize("kw", [dict(record=2), dict(obs_noise=1e-3)])
def test_record_and_noise_decline(trainers, kw):
    tr = trainers("ddpg")
    a = tr.evaluate(5, seed=81, **kw)
    tr.schedule["fused_eval_evopf"] = 0
    b = tr.evaluate(5, seed=81, **kw)
    tr.schedule["fused_eval_evopf"] = 1
    assert a.path == b.path == "stepwise"
    _equal(a, b)


@pytest.mark.parametrize("key", ["mlp_gemm", "gemm_ksplit"])
def test_other_forward_kernels_decline(trainers, hip, key):
    """With another kernel behind the stepwise path's actor forward the fused kernel's summation order is not the path's."""
    tr = trainers("ddpg")
    t = hip.tuning(**{key: 0})
    try:
        assert tr.evaluate(3, seed=91, horizon=2).path == "stepwise"
    finally:
        t.__exit__()
    assert hip.tuning.get(key) == 1
    assert tr.evaluate(3, seed=91, horizon=2).path == "fused"


def test_budget_sweep_inherits(trainers):
    tr = trainers("ddpg")
    on = tr.evaluate_budgets(5, eval_steps=[0, 3], seed=101)
    tr.schedule["fused_eval_evopf"] = 0
    off = tr.evaluate_budgets(5, eval_steps=[0, 3], seed=101)
    tr.schedule["fused_eval_evopf"] = 1
    assert len(on) == len(off) == 2
    for g in range(2):
        assert on[g].path == "fused" and off[g].path == "stepwise"
        _equal(on[g], off[g])
