"""trainer.evaluate_budgets() on the CPU: the "sweep" path driven by the oracle backend, the host side of ``BudgetSweep`` on
synthetic accumulator rows, and the refusals.

The definition is the yardstick: group g of a sweep is ``evaluate()`` with ``eval_steps[g]`` / ``eval_lr[g]`` and the shared
seed, bit for bit -- accumulator rows (every ``EvalResult`` field) and the ``ConstraintReport``.  The actor's last bias is
shifted (``_shifted`` of test_act.py) so that the projection iterates and the budget matters.
test_evaluate_budgets_gpu.py imports the helpers below."""
import numpy as np
import pytest
import torch

from rpo_amd.algo.evaluation import MAX_BUDGETS, BudgetSweep, EvalResult
from test_act import SHIFT, _shifted
from test_evaluate_constraints import _cpu_trainer, assert_reports_equal, initial_obs

H = 12


# ------------------------------------------------------------------------------------------------ shared helpers
def definition(tr, g, steps, lrs, **kw):
    """The ``evaluate()`` call group g of ``evaluate_budgets(eval_steps=steps, eval_lr=lrs, **kw)`` is defined by."""
    return tr.evaluate(eval_steps=steps[g], eval_lr=lrs[g], **kw)


def assert_group_is(res, want):
    """Every EvalResult field and the report of one group against the definition's, bit for bit (NaN-safe)."""
    for f in EvalResult.FIELDS:
        x, y = getattr(res, f), getattr(want, f)
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), f
    assert res.seed == want.seed and res.horizon == want.horizon
    assert (res.constraints is None) == (want.constraints is None) and res.trajectory is None and res.obs_noise is None
    if want.constraints is not None:
        assert_reports_equal(res.constraints, want.constraints)


def assert_budgets_matter(s):
    """The precondition of every bit-for-bit comparison: the groups did iterate differently and something was violated."""
    assert len({s.iters[g].tobytes() for g in range(len(s))}) >= 2, "proj_iters is the same in every group"
    assert int(s.viol_steps.max()) > 0, "no group has a violating step"


def assert_sweep_is_the_definition(tr, s, steps, lrs, **kw):
    assert len(s) == len(steps) and s.eval_steps.tolist() == list(steps)
    assert s.eval_lr.dtype == np.float32 and s.eval_lr.tobytes() == np.asarray(lrs, dtype=np.float32).tobytes()
    for g in range(len(steps)):
        assert_group_is(s[g], definition(tr, g, steps, lrs, **kw))


def lr_list(tr, B):
    """B different step sizes around the trainer's."""
    return [tr.eval_lr * f for f in (1.0, 0.5, 2.0, 1.5, 0.75, 3.0)[:B]]


# ------------------------------------------------------------------------------------------------ the sweep path
@pytest.mark.parametrize("algo,envname", [("ddpg", "cart"), ("sac", "pendulum")])
def test_sweep_equals_the_calls(algo, envname):
    tr = _cpu_trainer(algo, envname)
    steps = [0, 1, 3, tr.eval_steps]
    lrs = lr_list(tr, 4)
    with _shifted(tr, SHIFT[envname]):
        for constraints in (False, True):
            kw = dict(episodes=7, horizon=H, seed=21, constraints=constraints)
            s = tr.evaluate_budgets(eval_steps=steps, eval_lr=lrs, **kw)
            assert isinstance(s, BudgetSweep) and s.path == "sweep" and s.seed == 21 and s.horizon == H and s.episodes == 7
            assert_budgets_matter(s)
            assert_sweep_is_the_definition(tr, s, steps, lrs, **kw)
        # init_states are shared by all budgets; one eval_lr is broadcast, None is the trainer's
        init = initial_obs(tr, 7, 5) if envname == "cart" else None
        kw = dict(episodes=7, horizon=H, seed=21, init_states=init)
        s = tr.evaluate_budgets(eval_steps=[2, 0, 2], eval_lr=0.5 * tr.eval_lr, **kw)
        assert_sweep_is_the_definition(tr, s, [2, 0, 2], [0.5 * tr.eval_lr] * 3, **kw)
        assert_group_is(s[0], s[2])                              # duplicates are allowed and give equal groups
        s = tr.evaluate_budgets(eval_steps=(1,), **kw)
        assert_group_is(s[0], tr.evaluate(eval_steps=1, **kw))
        assert s.eval_lr.tobytes() == np.float32(tr.eval_lr).tobytes()


def test_sweep_equals_the_calls_on_evopf():
    tr = _cpu_trainer("ddpg", "evopf")
    kw = dict(episodes=2, horizon=2, seed=3, constraints=True)
    steps, lrs = [0, 2], [tr.eval_lr, 2.0 * tr.eval_lr]
    s = tr.evaluate_budgets(eval_steps=steps, eval_lr=lrs, **kw)
    assert s.path == "sweep" and s[0].path == "stepwise"
    assert_sweep_is_the_definition(tr, s, steps, lrs, **kw)
    assert int(s.iters[0].max()) == 0 and int(s.iters[1].max()) > 0


def test_one_seed_and_one_tick_of_the_call_counter():
    tr = _cpu_trainer("ddpg", "cart")
    calls = getattr(tr, "_evaluate_calls", 0)
    s = tr.evaluate_budgets(3, eval_steps=[0, 1, 2], horizon=2)
    assert tr._evaluate_calls == calls + 1 and s.seed == s[0].seed == s[1].seed == s[2].seed
    tr._evaluate_calls = calls                                   # the seed is the one evaluate() draws at the same count
    assert tr.evaluate(3, horizon=2).seed == s.seed
    keep = tr.eval_steps, tr.eval_lr
    tr.evaluate_budgets(3, eval_steps=[4], eval_lr=[0.1], horizon=2, seed=1)
    assert (tr.eval_steps, tr.eval_lr) == keep and tr._evaluate_calls == calls + 1   # (an explicit seed: no tick)


# ------------------------------------------------------------------------------------------------ BudgetSweep on synthetic rows
def _rows(rng, n, viol):
    """Accumulator rows (RPO_EVAL_* layout) of n finished episodes; ``viol``: violating steps per episode."""
    acc = np.zeros((n, 8), dtype=np.float32)
    acc[:, 0] = rng.uniform(1, 9, n)
    acc[:, 1:5] = rng.uniform(0, 1, (n, 4))
    acc[:, 5] = viol
    acc[:, 6] = rng.randint(0, 30, n)
    length = rng.randint(3, 10, n)
    acc[:, 7] = (length.astype(np.int32) << 2).view(np.float32)
    return acc, length


def test_budget_sweep_helpers():
    rng = np.random.RandomState(0)
    n, steps = 5, [7, 0, 3, 3]
    viols = [[0, 0, 0, 0, 0], [2, 1, 0, 3, 1], [0, 1, 0, 0, 0], [0, 0, 0, 0, 0]]
    accs, lens = zip(*[_rows(rng, n, v) for v in viols])
    results = [EvalResult(a, "fused", 10, 42) for a in accs]
    s = BudgetSweep(results, steps, [0.1, 0.2, 0.3, 0.4], "fused")
    assert len(s) == 4 and s.episodes == n and s.path == "fused" and s.seed == 42 and s.horizon == 10
    assert s.eval_steps.dtype.kind == "i" and s.eval_steps.tolist() == steps and s.eval_lr.dtype == np.float32
    assert all(s[g] is s.results[g] is results[g] for g in range(4))
    for f in EvalResult.FIELDS + ("iters",):
        x = getattr(s, f)
        assert x.shape == (4, n), f
        for g in range(4):
            row = getattr(s[g], "proj_iters" if f == "iters" else f)
            assert np.shares_memory(x[g], row) and x[g].tobytes() == row.tobytes(), f
    for g in range(4):
        np.testing.assert_array_equal(s.ret[g], accs[g][:, 0].astype(np.float64))
        np.testing.assert_array_equal(s.length[g], lens[g])
        np.testing.assert_array_equal(s.viol_steps[g], viols[g])
        np.testing.assert_array_equal(s.max_ineq[g], accs[g][:, 3].astype(np.float64))
        np.testing.assert_array_equal(s.max_eq[g], accs[g][:, 4].astype(np.float64))
        np.testing.assert_array_equal(s.iters[g], accs[g][:, 6].astype(np.int64))
    rate = s.violation_rate()
    assert rate.shape == (4,) and rate.dtype == np.float64
    np.testing.assert_array_equal(rate, [float(np.sum(viols[g])) / float(lens[g].sum()) for g in range(4)])
    np.testing.assert_array_equal(rate, [r.violation_rate() for r in results])
    np.testing.assert_array_equal(s.ret_mean(), [r.ret.mean() for r in results])
    assert s.ret_mean().shape == (4,)
    # the smallest budget that is safe enough, not the first in the list
    assert s.budget() == 3 and s.budget(0.0) == 3 and isinstance(s.budget(), int)
    assert s.budget(max_rate=rate[2]) == 3 and s.budget(max_rate=rate[1]) == 0 and s.budget(1.0) == 0
    assert BudgetSweep(results[1:3], [0, 3], [0.1, 0.1], "sweep").budget() is None
    assert BudgetSweep(results[1:3], [0, 3], [0.1, 0.1], "sweep").budget(rate[2]) == 3
    assert "BudgetSweep" in repr(s)
    with pytest.raises(ValueError):
        BudgetSweep(results, steps[:3], [0.1] * 4, "fused")
    with pytest.raises(ValueError):
        BudgetSweep([], [], [], "fused")


# ------------------------------------------------------------------------------------------------ refusals
class _Allocations(object):
    """Inside the block no vector env is made and ``evaluate()`` is not entered."""

    def __init__(self, tr, monkeypatch):
        self.tr, self.mp, self.seen = tr, monkeypatch, []

    def __enter__(self):
        from rpo_amd.algo import evaluation
        self.mp.setattr(self.tr.base_env, "make_vec", lambda *a, **k: self.seen.append("make_vec"))
        self.mp.setattr(evaluation, "evaluate", lambda *a, **k: self.seen.append("evaluate"))
        return self

    def __exit__(self, *exc):
        self.mp.undo()
        return False


def test_refusals_allocate_nothing(monkeypatch):
    tr = _cpu_trainer("ddpg", "cart")
    calls = getattr(tr, "_evaluate_calls", 0)
    nan, inf = float("nan"), float("inf")
    bad_calls = [dict(eval_steps=[]), dict(eval_steps=()), dict(eval_steps=None), dict(), dict(eval_steps=3),
                 dict(eval_steps=list(range(MAX_BUDGETS + 1))), dict(eval_steps=[[1, 2]]), dict(eval_steps="12"),
                 dict(eval_steps=[1, True]), dict(eval_steps=[False]), dict(eval_steps=[-1]), dict(eval_steps=[2, 2.5]),
                 dict(eval_steps=[1, "3"]), dict(eval_steps=[1, None]),
                 dict(eval_steps=[1, 2], eval_lr=[0.1]), dict(eval_steps=[1, 2], eval_lr=[0.1, 0.2, 0.3]),
                 dict(eval_steps=[1, 2], eval_lr=[]), dict(eval_steps=[1, 2], eval_lr=nan), dict(eval_steps=[1, 2], eval_lr=inf),
                 dict(eval_steps=[1, 2], eval_lr=[0.1, nan]), dict(eval_steps=[1, 2], eval_lr=[0.1, -inf]),
                 dict(eval_steps=[1, 2], eval_lr="0.1"), dict(eval_steps=[1, 2], eval_lr=[0.1, True]),
                 dict(eval_steps=[1], episodes=0), dict(eval_steps=[1], episodes=True), dict(eval_steps=[1], episodes=2.5),
                 dict(eval_steps=[1], horizon=0), dict(eval_steps=[1], horizon=1 << 24), dict(eval_steps=[1], constraints=1),
                 dict(eval_steps=[1], episodes=3, init_states=np.zeros((2, 6), np.float32)),
                 dict(eval_steps=[1], episodes=3, init_states=np.zeros((3, 5), np.float32))]
    with _Allocations(tr, monkeypatch) as spy:
        for kw in bad_calls:
            with pytest.raises(ValueError):
                tr.evaluate_budgets(**kw)
        for kw in (dict(record=True), dict(obs_noise=0.1)):      # not part of this entry point
            with pytest.raises(TypeError):
                tr.evaluate_budgets(2, eval_steps=[1], **kw)
        assert spy.seen == []
    assert getattr(tr, "_evaluate_calls", 0) == calls            # a refused call draws no seed
    assert len(tr.evaluate_budgets(2, eval_steps=list(range(MAX_BUDGETS)), horizon=1, seed=1)) == MAX_BUDGETS   # B = 64 is allowed


def test_a_trainer_without_a_projection_is_refused(monkeypatch):
    from test_train_step_golden import build_trainer
    import oracle_backend as ob
    torch.manual_seed(5)
    tr = build_trainer("ddpgla", "cart", ob, torch.device("cpu"), fused=False, num_envs=8)
    assert tr.evaluate(2, horizon=2).path == "stepwise"          # (evaluate() itself serves the baselines)
    with _Allocations(tr, monkeypatch) as spy:
        with pytest.raises(ValueError, match="projection"):
            tr.evaluate_budgets(2, eval_steps=[0, 1])
        assert spy.seen == []
