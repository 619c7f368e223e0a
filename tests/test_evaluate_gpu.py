"""trainer.evaluate() on the MI355X: the fused evaluation kernel (rpo_<env>_evaluate) against the stepwise path, eval(), the
reference's recorded episodes, and the training it must not disturb.

Bit equality.  The fused kernel is built from the rollout's pieces (mlp_tile_forward, gauss_head_row, *_explore_project,
cart_lane / pend_lane) and the stepwise path's launches run the same per-row functions; both update the accumulators through
rpo_eval_lane_update.  So every per-episode array is EQUAL between the paths, and summary() equals eval()'s 10-tuple.
"""
import numpy as np
import pytest
import torch

from test_eval_golden import CASES
from test_train_step_golden import build_trainer

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")


@pytest.fixture(scope="module")
def hip():
    from rpo_amd import ops
    assert torch.cuda.is_available()
    return ops


def _fixture_trainer(golden, hip, algo, envname, tag):
    g = golden("eval_%s_%s%s" % (algo, envname, tag))
    torch.manual_seed(1)
    tr = build_trainer(algo, envname, hip, DEV, num_envs=1, use_graph=False)
    sd = {k[len("actor."):]: torch.tensor(g[k]) for k in g.files if k.startswith("actor.")}
    tr.agent.actor.load_state_dict(sd)
    return g, tr, torch.tensor(g["init"], dtype=torch.float32, device=DEV)


def _both(tr, **kw):
    tr.schedule["fused_eval"] = 1
    a = tr.evaluate(**kw)
    tr.schedule["fused_eval"] = 0
    b = tr.evaluate(**kw)
    tr.schedule["fused_eval"] = 1
    return a, b


def _equal(a, b, sl=slice(None)):
    for f in a.FIELDS:
        np.testing.assert_array_equal(getattr(a, f)[sl], getattr(b, f), err_msg=f)


@pytest.mark.parametrize("algo,envname,tag", CASES)
def test_fused_evaluate_matches_the_reference_episodes(golden, hip, algo, envname, tag):
    """The tolerances of test_eval_matches_reference_on_gpu (float32 dynamics): one step of one episode for the lengths."""
    g, tr, init = _fixture_trainer(golden, hip, algo, envname, tag)
    r = tr.evaluate(10, init_states=init)
    assert r.path == "fused"
    assert np.abs(r.length - g["ep_length"]).sum() <= 1
    step = 1.0 if envname == "cart" else float(np.max(np.abs(g["ep_return"] / np.maximum(g["ep_length"], 1))))
    np.testing.assert_allclose(r.ret, g["ep_return"], rtol=0, atol=step + 1e-4)
    np.testing.assert_allclose(r.max_ineq, g["ep_max_ineq"], rtol=2e-2 if tag else 2e-5, atol=2e-6)
    assert np.abs(r.max_eq).max() < 2e-5
    assert not r.nonfinite.any()


@pytest.mark.parametrize("episodes", [10, 1000, 4096])
@pytest.mark.parametrize("algo,envname", [("ddpg", "cart"), ("sac", "cart"), ("ddpg", "pendulum"), ("sac", "pendulum")])
def test_fused_equals_stepwise_bit_for_bit(hip, algo, envname, episodes):
    torch.manual_seed(5)
    tr = build_trainer(algo, envname, hip, DEV, num_envs=64, use_graph=False)
    tr.vec.reset()
    tr.run_steps(8)                                            # a policy that has moved off its initialisation
    a, b = _both(tr, episodes=episodes, seed=11)
    assert a.path == "fused" and b.path == "stepwise"
    _equal(a, b)
    assert a.length.min() >= 1 and a.proj_iters.sum() > 0


@pytest.mark.parametrize("algo,envname,tag", CASES)
def test_summary_equals_eval(golden, hip, algo, envname, tag):
    """10 injected initial states: evaluate(10).summary() is eval()'s 10-tuple, bit for bit, on both paths."""
    g, tr, init = _fixture_trainer(golden, hip, algo, envname, tag)
    a, b = _both(tr, episodes=10, init_states=init)
    tr._eval_init_inject = init
    ref = tuple(tr.eval())
    assert a.summary() == ref
    assert b.summary() == ref


@pytest.mark.parametrize("algo,envname", [("ddpg", "cart"), ("sac", "pendulum")])
def test_lanes_are_independent(hip, algo, envname):
    torch.manual_seed(5)
    tr = build_trainer(algo, envname, hip, DEV, num_envs=64, use_graph=False)
    small = tr.evaluate(16, seed=21)
    for n in (4096, 16384):                                    # 16- and 64-lane workgroups
        _equal(tr.evaluate(n, seed=21), small, slice(0, 16))
    if envname == "cart":                                      # (the observation IS the injected state)
        v = tr.base_env.make_vec(16, seed=21, max_episode_steps=tr.max_episode_steps, device=DEV, stats_cap=2)
        v.reset()
        _equal(tr.evaluate(16, init_states=v.internal.clone()), small)


@pytest.mark.parametrize("algo,envname", [("ddpg", "evopf256"), ("ddpgla", "cart"), ("sacla", "cart")])
def test_stepwise_only_configurations(hip, algo, envname):
    torch.manual_seed(5)
    la = algo.endswith("la")
    tr = build_trainer(algo, envname, hip, DEV, num_envs=16, use_graph=False, fused=not la)    # (EVOPF: the fused 256-wide MLPs)
    if envname.startswith("evopf"):
        # an EVOPF episode is not defined by its initial state alone (the day's demand is drawn from the lane's reset
        # stream): eval() gets the evaluation's own vector env, its episode counter set so that its reset draws episode 0
        r = tr.evaluate(10, seed=4)
        tr._vec_eval = tr.base_env.make_vec(10, seed=4, max_episode_steps=tr.max_episode_steps, device=DEV, stats_cap=2)
        tr._vec_eval.ep_count.fill_(-1)
        tr._eval_rows = torch.zeros(10, tr.kernels.ring_floats, device=DEV)
        assert r.length.max() <= 24
    else:
        v = tr.base_env.make_vec(10, seed=4, max_episode_steps=tr.max_episode_steps, device=DEV, stats_cap=2)
        v.reset()
        init = v.internal.clone()
        r = tr.evaluate(10, init_states=init)
        tr._eval_init_inject = init
    assert r.path == "stepwise"
    assert r.summary() == tuple(tr.eval())


def test_no_side_effects_on_the_device(hip, monkeypatch):
    monkeypatch.setenv("RPO_GRAPH_CYCLE", "4")

    def fresh():
        torch.manual_seed(5)
        tr = build_trainer("ddpg", "cart", hip, DEV, num_envs=512, use_graph=True)
        tr.vec.reset()
        return tr
    a = fresh()
    a.run_steps(16)
    b = fresh()
    b.run_steps(8)
    torch.cuda.synchronize()
    snap = {k: getattr(b.vec, k).clone() for k in ("internal", "ep_len", "ep_ret", "ep_count", "ctrl", "stats")}
    rows, flat = b.buffer.rows.clone(), b.agent.flat.data.clone()
    r = b.evaluate(4096)
    assert r.path == "fused"
    torch.cuda.synchronize()
    for k, x in snap.items():
        assert torch.equal(getattr(b.vec, k), x), k
    assert int(b.vec.ctrl[hip.CONST["RPO_CTRL_NONFINITE"]]) == 0
    assert torch.equal(b.buffer.rows, rows) and torch.equal(b.agent.flat.data, flat)
    b.run_steps(8)
    torch.cuda.synchronize()
    assert any(e["graph"] is not None for e in b._graphs.entries.values())
    for k in ("internal", "ep_len", "ep_ret", "ep_count", "ctrl"):
        assert torch.equal(getattr(a.vec, k), getattr(b.vec, k)), k
    assert torch.equal(a.buffer.rows, b.buffer.rows)
    assert torch.equal(a.agent.flat.data, b.agent.flat.data)
    assert torch.equal(a.agent.critic_target_flat, b.agent.critic_target_flat)


@pytest.mark.parametrize("algo,envname", [("ddpg", "cart"), ("sac", "pendulum")])
def test_steps_boundary(hip, algo, envname, monkeypatch):
    """Several launches per evaluation with a last partial one (steps = 7, horizon 50), and horizon 1."""
    from rpo_amd import ops
    torch.manual_seed(5)
    tr = build_trainer(algo, envname, hip, DEV, num_envs=64, use_graph=False)
    monkeypatch.setattr(ops, "EVAL_LANE_STEPS", 1000 * 7)
    a, b = _both(tr, episodes=1000, seed=2, horizon=50)
    _equal(a, b)
    assert a.length.max() > 7                                # (episodes ran across launches)
    a, b = _both(tr, episodes=1000, seed=2, horizon=1)
    _equal(a, b)
    assert (a.length == 1).all()
