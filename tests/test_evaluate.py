"""trainer.evaluate() on the CPU: the stepwise path driven by the oracle backend (float64 dynamics, torch-op accumulators).

* The reference-trained policies of ``tests/golden/eval_*.npz`` (see test_eval_golden.py) with their injected initial
  states: the per-episode returns, lengths and maximal violations the reference recorded, with the tolerances of
  ``test_eval_matches_reference_on_oracle_backend``; ``summary()`` is ``eval()``'s 10-tuple exactly.
* Argument validation, the non-finite flag, and the absence of side effects on the trainer.
"""
import numpy as np
import pytest
import torch

import oracle_backend as ob
from test_eval_golden import CASES
from test_train_step_golden import build_trainer


def _trainer(golden, algo, envname, tag):
    g = golden("eval_%s_%s%s" % (algo, envname, tag))
    torch.manual_seed(1)
    tr = build_trainer(algo, envname, ob, torch.device("cpu"), num_envs=1, use_graph=False)
    sd = {k[len("actor."):]: torch.tensor(g[k]) for k in g.files if k.startswith("actor.")}
    tr.agent.actor.load_state_dict(sd)
    return g, tr


@pytest.mark.parametrize("algo,envname,tag", CASES)
def test_evaluate_reproduces_the_reference_episodes(golden, algo, envname, tag):
    torch.set_num_threads(1)
    g, tr = _trainer(golden, algo, envname, tag)
    init = torch.tensor(g["init"], dtype=torch.float32)
    r = tr.evaluate(10, init_states=init)
    assert r.path == "stepwise" and r.episodes == 10
    np.testing.assert_allclose(r.ret, g["ep_return"], rtol=0, atol=1e-4)
    np.testing.assert_array_equal(r.length, g["ep_length"])
    np.testing.assert_allclose(r.max_ineq, g["ep_max_ineq"], rtol=2e-5, atol=2e-6)
    assert np.abs(r.max_eq).max() < 2e-5 and np.abs(g["ep_max_eq"]).max() < 2e-5
    assert not r.nonfinite.any()
    assert (r.proj_iters >= 0).all() and (r.viol_steps <= r.length).all()
    if tag:                                                  # the shifted actors leave violations behind the projection
        assert r.viol_steps.sum() > 0 and 0 < r.violation_rate() <= 1
    # the same trainer and initial states through eval(): the same 10 numbers, exactly
    tr._eval_init_inject = init
    assert r.summary() == tuple(tr.eval())


def test_evaluate_validates_its_arguments(golden):
    _, tr = _trainer(golden, "ddpg", "cart", "")
    with pytest.raises(ValueError):
        tr.evaluate(0)
    with pytest.raises(ValueError):
        tr.evaluate(4, horizon=0)
    with pytest.raises(ValueError):
        tr.evaluate(4, init_states=torch.zeros(3, 6))
    with pytest.raises(ValueError):
        tr.evaluate(4, init_states=torch.zeros(4, 5))


def test_seeds_and_horizon(golden):
    torch.set_num_threads(1)
    _, tr = _trainer(golden, "ddpg", "cart", "")
    a, b = tr.evaluate(6, seed=3, horizon=7), tr.evaluate(6, seed=3, horizon=7)
    for f in a.FIELDS:
        np.testing.assert_array_equal(getattr(a, f), getattr(b, f))
    assert a.horizon == 7 and a.length.max() <= 7
    c, d = tr.evaluate(6, horizon=7), tr.evaluate(6, horizon=7)     # seed=None: fresh initial states per call
    assert c.seed != d.seed
    # lane independence: the first episodes of a larger evaluation are the smaller evaluation (round-off residuals aside: the
    # oracle's CPU matmuls round with the batch size; the GPU suite checks the bits)
    e = tr.evaluate(3, seed=3, horizon=7)
    np.testing.assert_array_equal(a.length[:3], e.length)
    np.testing.assert_array_equal(a.ret[:3], e.ret)
    np.testing.assert_allclose(a.mean_eq[:3], e.mean_eq, rtol=0, atol=1e-6)


def test_nonfinite_flag_and_frozen_rows():
    """The stepwise accumulator update on hand-made transition rows: a live step with a non-finite reward sets the flag; a
    finished episode's row no longer changes, whatever its lane produces."""
    from rpo_amd.algo.evaluation import EvalResult, accumulate_torch
    from rpo_amd.ops import CartSafeKernels
    cols = CartSafeKernels.cols
    rows = torch.zeros(3, 32)
    rows[:, cols["reward"][0]] = 1.0
    rows[:, cols["ineq_viol"][0] + 2] = torch.tensor([0.5, 0.0, 2e-3])
    rows[:, cols["eq_viol"][0]] = torch.tensor([-1e-6, 0.0, 0.0])
    rows[1, cols["done"][0]] = 1.0                            # lane 1 ends at step 0
    acc = torch.zeros(3, 8)
    iters = torch.tensor([3, 1, 2], dtype=torch.int32)
    accumulate_torch(rows, cols, iters, 0, 1e-3, acc)
    before = acc[1].clone()
    rows[:, cols["reward"][0]] = float("nan")                 # step 1: every lane's reward is NaN
    rows[1, cols["ineq_viol"][0]] = float("inf")
    accumulate_torch(rows, cols, iters, 1, 1e-3, acc)
    r = EvalResult(acc.numpy(), "stepwise", 2, 0)
    np.testing.assert_array_equal(r.nonfinite, [True, False, True])
    np.testing.assert_array_equal(r.length, [2, 1, 2])
    assert torch.equal(acc[1], before)                        # frozen: the finished lane's NaN / inf did not reach its row
    assert r.ret[1] == 1.0 and np.isnan(r.ret[0]) and np.isnan(r.ret[2])
    np.testing.assert_array_equal(r.viol_steps, [2, 0, 2])
    np.testing.assert_array_equal(r.proj_iters, [6, 1, 4])
    np.testing.assert_allclose(r.max_ineq, [0.5, 0.0, 2e-3], rtol=1e-7)
    np.testing.assert_allclose(r.mean_eq, [1e-6, 0.0, 0.0], rtol=1e-6)


@pytest.mark.parametrize("algo,envname", [("ddpg", "cart"), ("sac", "pendulum")])
def test_evaluate_leaves_the_trainer_untouched(algo, envname):
    """run_steps(k) -> evaluate() -> run_steps(k) equals run_steps(2k) bit for bit: parameters, env lanes, ctrl, replay."""
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
    r = b.evaluate(5, horizon=20)
    assert r.length.min() >= 1
    b.run_steps(5)
    for name in ("internal", "obs", "action", "ep_len", "ep_ret", "ep_count", "ctrl", "stats"):
        assert torch.equal(getattr(a.vec, name), getattr(b.vec, name)), name
    assert torch.equal(a.buffer.rows, b.buffer.rows)
    assert torch.equal(a.agent.flat.data, b.agent.flat.data)
    assert torch.equal(a.agent.critic_target_flat, b.agent.critic_target_flat)
    assert torch.equal(a.agent.nju.weight, b.agent.nju.weight)
    assert a._t == b._t == 10
