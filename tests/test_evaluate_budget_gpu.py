"""trainer.evaluate(eval_steps=, eval_lr=) on the MI355X: the per-call projection budget reaches the fused launch and the stepwise
loop, and leaves the trainer's attributes alone.  Trainers are tests/test_act_gpu.py's; the actor's last bias is shifted
(``SHIFT``) so that the projection has work to do and the budget matters."""
import numpy as np
import pytest
import torch

from test_act_gpu import SHIFT, _setup, _shifted

pytestmark = pytest.mark.gpu

EPISODES = 64


def _same(a, b):
    for f in a.FIELDS:
        assert np.array_equal(getattr(a, f), getattr(b, f)), f


@pytest.mark.parametrize("algo,envname", [("ddpg", "cart"), ("sac", "pendulum")])
def test_evaluate_takes_a_budget_per_call(algo, envname):
    assert torch.cuda.is_available()
    tr, _, _ = _setup(algo, envname)
    keep = tr.eval_steps, tr.eval_lr
    kw = dict(episodes=EPISODES, seed=21)
    with _shifted(tr, SHIFT[envname]):
        base = tr.evaluate(**kw)
        assert base.path == "fused" and int(base.proj_iters.max()) >= 2
        _same(tr.evaluate(eval_steps=tr.eval_steps, eval_lr=tr.eval_lr, **kw), base)
        # Complete only: no iteration anywhere, and what a trainer with eval_steps = 0 evaluates
        zero = tr.evaluate(eval_steps=0, **kw)
        assert int(np.abs(zero.proj_iters).max()) == 0
        tr.eval_steps = 0
        try:
            attr = tr.evaluate(**kw)
        finally:
            tr.eval_steps = keep[0]
        _same(zero, attr)
        # the fused launch and the stepwise loop get the same override
        over = dict(eval_steps=7, eval_lr=3.0 * tr.eval_lr)
        fused = tr.evaluate(**over, **kw)
        tr.schedule["fused_eval"] = 0
        try:
            step = tr.evaluate(**over, **kw)
        finally:
            tr.schedule["fused_eval"] = 1
        assert fused.path == "fused" and step.path == "stepwise"
        _same(fused, step)
        assert not np.array_equal(fused.proj_iters, base.proj_iters)
        _same(tr.evaluate(**kw), base)                           # ... for that call only
    assert (tr.eval_steps, tr.eval_lr) == keep
    for bad in (-1, 2.5, True, "3"):
        with pytest.raises(ValueError):
            tr.evaluate(episodes=2, eval_steps=bad)
