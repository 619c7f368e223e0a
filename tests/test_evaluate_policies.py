"""trainer.evaluate_policies() on the CPU: the "sweep" path driven by the oracle backend, ``policy_params()`` /
``using_policy()``, the host side of ``PolicySweep`` on synthetic accumulator rows, and the refusals.

The definition is the yardstick: group g of a sweep is ``evaluate()`` under ``using_policy(policies[g])`` with the shared seed,
bit for bit -- accumulator rows (every ``EvalResult`` field) and the ``ConstraintReport``.  The candidates are the live actor,
the live actor with its last bias shifted (``_shifted`` / ``SHIFT`` of test_act.py: the projection iterates and steps are
violated) and the span of a second trainer built with another seed.  Every bit-for-bit test first asserts that the policies
matter (``assert_policies_matter``): with the group ignored all groups would be equal and the comparison vacuous.
test_evaluate_policies_gpu.py imports the helpers below."""
import functools

import numpy as np
import pytest
import torch

import oracle_backend as ob
from rpo_amd.algo.evaluation import (CURVE_LEN, MAX_POLICIES, BestPolicy, EvalResult, PolicySweep, keep_best_torch)
from test_act import SHIFT, _shifted
from test_evaluate_budgets import _Allocations, _rows, assert_group_is
from test_evaluate_constraints import _cpu_trainer, initial_obs
from test_train_step_golden import build_trainer

H = 12
CASES = [("ddpg", "cart"), ("sac", "pendulum")]


# ------------------------------------------------------------------------------------------------ shared helpers
def shifted_span(tr, delta):
    """The live actor's span with the last bias moved by ``delta``; the live actor is left as it was."""
    with _shifted(tr, delta):
        return tr.policy_params()


def definition(tr, policy, **kw):
    """The ``evaluate()`` call a group of ``evaluate_policies([.., policy, ..], **kw)`` is defined by."""
    with tr.using_policy(policy):
        return tr.evaluate(**kw)


def assert_policies_matter(s):
    """The precondition of every bit-for-bit comparison: the groups differ (returns or iteration counts) and a step of some
    group was violated."""
    assert len({s.ret[g].tobytes() + s.iters[g].tobytes() for g in range(len(s))}) >= 2, "every group has the same results"
    assert int(s.viol_steps.max()) > 0, "no group has a violating step"


def assert_sweep_is_the_definition(tr, s, policies, **kw):
    assert len(s) == len(policies) == len(s.names)
    for g, p in enumerate(policies):
        assert_group_is(s[g], definition(tr, p, **kw))


def flat_bits(tr):
    return tr.agent.flat.data.detach().cpu().numpy().tobytes()


@functools.lru_cache(maxsize=None)
def _trainers(algo, envname):
    """(the trainer of the CPU evaluation tests, a second one built with another seed): shared and left unchanged."""
    tr = _cpu_trainer(algo, envname)
    torch.manual_seed(6)
    other = build_trainer(algo, envname, ob, torch.device("cpu"), num_envs=64, use_graph=False, seed=12)
    other.vec.reset()
    other.run_steps(8)
    return tr, other


def candidates(tr, other, envname):
    """[the live actor, the live actor with its last bias shifted, the span of a trainer with another seed]"""
    return [None, shifted_span(tr, SHIFT[envname]), other.policy_params()]


# ------------------------------------------------------------------------------------------------ the sweep path
@pytest.mark.parametrize("algo,envname", CASES)
def test_sweep_equals_the_calls_under_using_policy(algo, envname):
    tr, other = _trainers(algo, envname)
    policies = candidates(tr, other, envname)
    before = flat_bits(tr)
    for constraints in (False, True):
        kw = dict(episodes=7, horizon=H, seed=21, constraints=constraints)
        s = tr.evaluate_policies(policies, **kw)
        assert isinstance(s, PolicySweep) and s.path == "sweep" and s.seed == 21 and s.horizon == H and s.episodes == 7
        assert s.names == ("live", "policy[1]", "policy[2]") and all(r.path == "stepwise" for r in s.results)
        assert_policies_matter(s)
        assert_sweep_is_the_definition(tr, s, policies, **kw)
        assert_group_is(s[0], tr.evaluate(**kw))                 # None: the live actor, no context at all
    if envname == "cart":                                        # init_states are shared by all policies
        kw = dict(episodes=7, horizon=H, seed=21, init_states=initial_obs(tr, 7, 5))
        s = tr.evaluate_policies(policies, names=["a", "b", "c"], **kw)
        assert s.names == ("a", "b", "c")
        assert_policies_matter(s)
        assert_sweep_is_the_definition(tr, s, policies, **kw)
    assert flat_bits(tr) == before


def test_sweep_equals_the_calls_on_evopf():
    tr = _cpu_trainer("ddpg", "evopf")
    torch.manual_seed(6)
    other = build_trainer("ddpg", "evopf", ob, torch.device("cpu"), num_envs=4, fused=False, use_graph=False, seed=12)
    policies = [None, other.policy_params(), tr.policy_params() * 2.0]
    before = flat_bits(tr)
    kw = dict(episodes=2, horizon=2, seed=3, constraints=True)
    s = tr.evaluate_policies(policies, **kw)
    assert s.path == "sweep" and s[0].path == "stepwise"
    assert_policies_matter(s)
    assert_sweep_is_the_definition(tr, s, policies, **kw)
    assert flat_bits(tr) == before


def test_one_seed_and_one_tick_of_the_call_counter():
    tr, other = _trainers("ddpg", "cart")
    calls = getattr(tr, "_evaluate_calls", 0)
    try:
        s = tr.evaluate_policies([None, other.policy_params(), None], 3, horizon=2)
        assert tr._evaluate_calls == calls + 1 and s.seed == s[0].seed == s[1].seed == s[2].seed
        tr._evaluate_calls = calls                               # the seed is the one evaluate() draws at the same count
        assert tr.evaluate(3, horizon=2).seed == s.seed
        tr.evaluate_policies([None], 3, horizon=2, seed=1)
        assert tr._evaluate_calls == calls + 1                   # (an explicit seed: no tick)
    finally:
        tr._evaluate_calls = calls


# ------------------------------------------------------------------------------------------------ policy_params / using_policy
def test_using_policy_restores_the_live_span_bit_for_bit():
    tr, other = _trainers("ddpg", "cart")
    lo, hi = tr.agent.flat.actor_range
    p = other.policy_params()
    assert p.dtype == torch.float32 and p.shape == (hi - lo,) and p.device == tr.device
    before, live = flat_bits(tr), tr.agent.flat.param(tr.agent.flat.actor_range)
    assert not torch.equal(live, p)
    with tr.using_policy(p) as inside:
        assert inside is tr and torch.equal(live, p)             # the live actor IS p ...
        assert tr.agent.flat.data[:lo].numpy().tobytes() == np.frombuffer(before, np.float32)[:lo].tobytes()   # ... nothing else moved
        r = tr.evaluate(5, horizon=H, seed=2)
    assert flat_bits(tr) == before
    assert_group_is(r, other.evaluate(5, horizon=H, seed=2))     # the same env and projection: the other trainer's policy
    with pytest.raises(RuntimeError, match="inside"):
        with tr.using_policy(p):
            assert torch.equal(live, p)
            raise RuntimeError("inside")
    assert flat_bits(tr) == before
    with tr.using_policy(None):                                  # None: the live policy stays
        assert flat_bits(tr) == before
    assert flat_bits(tr) == before
    for bad in (p[:-1], p.double(), p.long(), [0.0] * (hi - lo), 3, "no/such/file.npz", torch.zeros(hi - lo + 4)):
        with pytest.raises(ValueError):
            with tr.using_policy(bad):
                pass
        assert flat_bits(tr) == before


def test_using_best_is_unchanged():
    """A trainer without keep_best still refuses using_best() / restore_best(); using_policy() needs no keep_best."""
    tr, other = _trainers("ddpg", "cart")
    with pytest.raises(ValueError, match="keep_best"):
        with tr.using_best():
            pass
    with pytest.raises(ValueError, match="keep_best"):
        tr.restore_best()
    with tr.using_policy(other.policy_params()):
        pass


def test_policy_params_is_a_clone():
    torch.manual_seed(5)
    tr = build_trainer("ddpg", "cart", ob, torch.device("cpu"), num_envs=64, use_graph=False)
    tr.vec.reset()
    tr.run_steps(4)
    p = tr.policy_params()
    live = tr.agent.flat.param(tr.agent.flat.actor_range)
    assert torch.equal(p, live) and p.data_ptr() != live.data_ptr()
    keep = p.clone()
    tr.run_steps(8)
    assert torch.equal(p, keep) and not torch.equal(p, live)     # training moved the live span, not the clone
    p += 1.0
    assert not torch.equal(live, p)                              # and the other way round


def test_best_policies_and_paths_are_accepted(tmp_path):
    tr, other = _trainers("ddpg", "cart")
    p = shifted_span(tr, SHIFT["cart"])
    best = BestPolicy(4, np.zeros(CURVE_LEN), p.clone(), 0.0)
    path = str(tmp_path / "b.npz")
    best.save(path)
    kw = dict(episodes=5, horizon=H, seed=9, constraints=True)
    s = tr.evaluate_policies([None, p, best, path, p.numpy(), tmp_path / "b.npz"], **kw)
    assert s.names == ("live", "policy[1]", "best[4]", path, "policy[4]", path)
    assert_policies_matter(s)
    for g in (2, 3, 4, 5):
        assert_group_is(s[g], s[1])
    assert_group_is(s[1], definition(tr, p, **kw))
    assert_group_is(definition(tr, best, **kw), s[1])
    assert_group_is(definition(tr, path, **kw), s[1])


# ------------------------------------------------------------------------------------------------ PolicySweep on synthetic rows
def _sweep(viols, rets=None, nonfinite=(), lengths=None, n=5, seed=0):
    """A PolicySweep over made-up accumulator rows: ``viols[g]`` violating steps per episode, ``rets[g]`` a constant return
    (None: random), ``lengths[g]`` a constant length (None: random), groups in ``nonfinite`` with the non-finite bit set."""
    rng = np.random.RandomState(seed)
    results = []
    for g, v in enumerate(viols):
        acc, length = _rows(rng, n, v)
        if rets is not None and rets[g] is not None:
            acc[:, 0] = rets[g]
        if lengths is not None:
            acc[:, 7] = (np.full(n, lengths[g], np.int32) << 2).view(np.float32)
        if g in nonfinite:
            acc[0, 7] = (acc[0, 7:8].view(np.int32) | 2).view(np.float32)[0]
        results.append(EvalResult(acc, "fused", 10, 42))
    return PolicySweep(results, ["p%d" % g for g in range(len(viols))], "fused")


def test_policy_sweep_arrays_and_paired():
    s = _sweep([[0, 0, 0, 0, 0], [2, 1, 0, 3, 1], [0, 1, 0, 0, 0]])
    assert len(s) == 3 and s.episodes == 5 and s.path == "fused" and s.seed == 42 and s.horizon == 10 and s.names == ("p0", "p1", "p2")
    for f in EvalResult.FIELDS + ("iters",):
        x = getattr(s, f)
        assert x.shape == (3, 5), f
        for g in range(3):
            row = getattr(s[g], "proj_iters" if f == "iters" else f)
            assert s[g] is s.results[g] and np.shares_memory(x[g], row) and x[g].tobytes() == row.tobytes(), f
    np.testing.assert_array_equal(s.violation_rate(), [r.violation_rate() for r in s.results])
    np.testing.assert_array_equal(s.ret_mean(), [r.ret.mean() for r in s.results])
    assert s.violation_rate().shape == s.ret_mean().shape == (3,)
    for a, b in ((0, 1), (1, 0), (2, 2), (0, 2)):
        d = s.ret[a] - s.ret[b]
        got = s.paired(a, b)
        assert got == (got.mean, got.stderr, got.n) == (d.mean(), d.std(ddof=1) / np.sqrt(5), 5)
    assert s.paired(0, 1).mean == -s.paired(1, 0).mean and s.paired(2, 2) == (0.0, 0.0, 5)
    one = _sweep([[0], [1]], n=1)
    got = one.paired(0, 1)
    assert got.n == 1 and got.mean == float(one.ret[0, 0] - one.ret[1, 0]) and np.isnan(got.stderr)
    assert "PolicySweep" in repr(s)
    with pytest.raises(ValueError):
        PolicySweep(s.results, ["a", "b"], "fused")
    with pytest.raises(ValueError):
        PolicySweep([], [], "fused")


def _keep_best_order(s, max_rate):
    """The point ``keep_best_torch`` holds after the groups' curve rows went by in order (None: none was taken)."""
    best, best_row = torch.zeros(1), torch.zeros(CURVE_LEN, dtype=torch.float64)
    best_point = torch.full((1,), -1, dtype=torch.int64)
    for g in range(len(s)):
        row = torch.zeros(CURVE_LEN, dtype=torch.float64)
        row[1], row[2] = s.episodes, float(s.ret_mean()[g])      # RPO_CURVE_EPISODES, RPO_CURVE_STATS (the mean return)
        row[12], row[13], row[14] = float(s.length[g].sum()), float(s.viol_steps[g].sum()), float(s.nonfinite[g].sum())
        keep_best_torch(torch.full((1,), float(g)), best, row, best_row, best_point, g, max_rate)
    return None if int(best_point[0]) < 0 else int(best_point[0])


@pytest.mark.parametrize("name,kw,max_rate,want", [
    ("safe beats unsafe, whatever the return", dict(viols=[[1] * 5, [0] * 5, [2] * 5], rets=[9.0, 1.0, 8.0]), 0.0, 1),
    ("among safe groups the higher return", dict(viols=[[0] * 5] * 3, rets=[2.0, 5.0, 3.0]), 0.0, 1),
    ("a return tie keeps the earlier group", dict(viols=[[0] * 5] * 3, rets=[5.0, 5.0, 4.0]), 0.0, 0),
    ("all unsafe: the lower rate", dict(viols=[[3] * 5, [1] * 5, [2] * 5], rets=[9.0, 1.0, 5.0], lengths=[8] * 3), 0.0, 1),
    ("all unsafe, a rate tie: the higher return", dict(viols=[[1] * 5] * 3, rets=[2.0, 6.0, 4.0], lengths=[8] * 3), 0.0, 1),
    ("all unsafe, rate and return tie: the earlier", dict(viols=[[1] * 5] * 3, rets=[2.0, 6.0, 6.0], lengths=[8] * 3), 0.0, 1),
    ("a non-finite group is never taken", dict(viols=[[0] * 5] * 3, rets=[2.0, 9.0, 3.0], nonfinite=(1,)), 0.0, 2),
    ("a NaN return is never taken", dict(viols=[[0] * 5] * 3, rets=[float("nan"), 1.0, 0.5]), 0.0, 1),
    ("every group non-finite", dict(viols=[[0] * 5] * 2, rets=[1.0, 2.0], nonfinite=(0, 1)), 0.0, None),
    ("max_rate makes a violating group safe", dict(viols=[[0] * 5, [1] * 5], rets=[1.0, 2.0], lengths=[8] * 2), 0.2, 1),
    ("the unsafe incumbent loses to a later safe one", dict(viols=[[1] * 5, [4] * 5, [0] * 5], rets=[9.0, 9.5, 0.0]), 0.0, 2),
])
def test_best_is_keep_bests_order(name, kw, max_rate, want):
    s = _sweep(**kw)
    assert s.best(max_rate) == want == _keep_best_order(s, max_rate), name
    if max_rate == 0.0:
        assert s.best() == want


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_allocate_nothing(monkeypatch, tmp_path):
    tr, other = _trainers("ddpg", "cart")
    lo, hi = tr.agent.flat.actor_range
    p = other.policy_params()
    calls, before = getattr(tr, "_evaluate_calls", 0), flat_bits(tr)
    not_a_policy = str(tmp_path / "x.npz")
    np.savez(not_a_policy, a=np.zeros(3))
    bad_calls = [dict(policies=[]), dict(policies=()), dict(policies=None), dict(policies=[None] * (MAX_POLICIES + 1)),
                 dict(policies=p), dict(policies="b.npz"), dict(policies=3),
                 dict(policies=[p[:-1]]), dict(policies=[None, torch.zeros(hi - lo + 4)]), dict(policies=[p.double()]),
                 dict(policies=[p.long()]), dict(policies=[p.numpy().astype(np.float64)]), dict(policies=[[0.0] * (hi - lo)]),
                 dict(policies=[None, 3]), dict(policies=[True]), dict(policies=[str(tmp_path / "missing.npz")]),
                 dict(policies=["not a file"]), dict(policies=[str(tmp_path)]), dict(policies=[not_a_policy]),
                 dict(policies=[None, p], names=["a"]), dict(policies=[None, p], names="ab"), dict(policies=[p], names=[1]),
                 dict(policies=[p], episodes=0), dict(policies=[p], episodes=True), dict(policies=[p], episodes=2.5),
                 dict(policies=[p], horizon=0), dict(policies=[p], horizon=1 << 24), dict(policies=[p], constraints=1),
                 dict(policies=[p], episodes=3, init_states=np.zeros((2, 6), np.float32)),
                 dict(policies=[p], episodes=3, init_states=np.zeros((3, 5), np.float32))]
    with _Allocations(tr, monkeypatch) as spy:
        for kw in bad_calls:
            with pytest.raises(ValueError):
                tr.evaluate_policies(**kw)
        for kw in (dict(record=True), dict(obs_noise=0.1), dict(eval_steps=3), dict(eval_lr=0.1)):   # not part of this entry point
            with pytest.raises(TypeError):
                tr.evaluate_policies([p], 2, **kw)
        monkeypatch.setattr(tr.agent.flat, "actor_range", None)  # an agent whose actor is not in the flat buffer
        for call in (lambda: tr.evaluate_policies([None]), tr.policy_params, lambda: tr.using_policy(None).__enter__()):
            with pytest.raises(ValueError, match="actor_range"):
                call()
        assert spy.seen == []
    assert getattr(tr, "_evaluate_calls", 0) == calls and flat_bits(tr) == before    # a refused call draws no seed
    assert tr.agent.flat.actor_range == (lo, hi)
    assert len(tr.evaluate_policies([None] * MAX_POLICIES, 2, horizon=1, seed=1)) == MAX_POLICIES    # P = 64 is allowed
