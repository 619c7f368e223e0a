"""``keep_best`` on the CPU: the host logic of the kept policy driven by the oracle backend, with ``keep_best_torch`` standing
in for ``rpo_eval_keep_best``.  The criterion's yardstick is the numpy restatement of tests/test_keep_best_gpu.py, on the same
hand-written row sequences."""
import numpy as np
import pytest
import torch

import oracle_backend as ob
from rpo_amd.algo import BestPolicy
from rpo_amd.algo import evaluation as ev
from test_eval_curve import _fresh
from test_keep_best_gpu import CURVE_LEN, SEQUENCES, choose_numpy, pattern, wins_numpy
from test_train_step_golden import build_trainer

CPU = torch.device("cpu")


def test_the_sequences_walk_every_branch():
    """The hand-written expectation against the numpy criterion, so that neither drifts alone."""
    for max_rate, rows, want in SEQUENCES:
        held, taken = choose_numpy(rows, max_rate)
        assert [int(t) for t in taken] == want and held == max(k for k, t in enumerate(want) if t)
    assert ev.CURVE_LEN == CURVE_LEN


@pytest.mark.parametrize("n", [1, 5, 1027])
def test_keep_best_torch_equals_the_numpy_criterion(n):
    call = 0
    for max_rate, rows, _ in SEQUENCES:
        best = torch.full((n,), -7, dtype=torch.int32).view(torch.float32)
        best_row = torch.zeros(CURVE_LEN, dtype=torch.float64)
        best_point = torch.full((1,), -1, dtype=torch.int64)
        want_best, want_row, held = best.clone(), np.zeros(CURVE_LEN), -1
        for k, row in enumerate(rows):
            src = torch.from_numpy(pattern(n, call)).view(torch.float32)
            call += 1
            before = src.clone()
            ev.keep_best_torch(src, best, torch.tensor(row), best_row, best_point, k, max_rate)
            if wins_numpy(row, want_row, held, max_rate):
                want_row, held, want_best = row.copy(), k, before.clone()
            assert int(best_point[0]) == held, (max_rate, k)
            assert best_row.numpy().tobytes() == want_row.tobytes(), (max_rate, k)
            assert best.numpy().tobytes() == want_best.numpy().tobytes(), (max_rate, k)
            assert src.numpy().tobytes() == before.numpy().tobytes()


def test_constructor_refusals(monkeypatch):
    kw = dict(num_envs=2, use_graph=False)
    with pytest.raises(ValueError, match="eval_episodes"):
        build_trainer("ddpg", "cart", ob, CPU, keep_best=True, **kw)
    for bad in (-0.1, float("nan"), "often", [0.1], np.True_):
        with pytest.raises(ValueError):
            build_trainer("ddpg", "cart", ob, CPU, eval_episodes=3, keep_best=bad, **kw)
    tr = build_trainer("ddpg", "cart", ob, CPU, eval_episodes=3, **kw)
    assert tr.keep_best is False and tr.best is None and tr._curve.keep_rate is None
    with pytest.raises(ValueError, match="keep_best"):
        tr.restore_best()
    assert build_trainer("ddpg", "cart", ob, CPU, eval_episodes=3, keep_best=True, **kw).keep_best == 0.0
    assert build_trainer("sacla", "cart", ob, CPU, eval_episodes=3, keep_best=0.125, fused=False, **kw).keep_best == 0.125
    assert build_trainer("ddpg", "cart", ob, CPU, eval_episodes=3, keep_best=False, **kw).keep_best is False
    monkeypatch.setenv("RPO_KEEP_BEST", "0.25")
    assert build_trainer("sac", "pendulum", ob, CPU, eval_episodes=3, **kw).keep_best == 0.25
    assert build_trainer("sac", "pendulum", ob, CPU, eval_episodes=3, keep_best=False, **kw).keep_best is False
    monkeypatch.setenv("RPO_KEEP_BEST", "1")
    assert build_trainer("ddpg", "cart", ob, CPU, eval_episodes=3, **kw).keep_best == 0.0
    with pytest.raises(ValueError, match="eval_episodes"):
        build_trainer("ddpg", "cart", ob, CPU, **kw)
    monkeypatch.setenv("RPO_KEEP_BEST", "sometimes")
    with pytest.raises(ValueError):
        build_trainer("ddpg", "cart", ob, CPU, eval_episodes=3, **kw)
    monkeypatch.setenv("RPO_KEEP_BEST", "0")
    assert build_trainer("ddpg", "cart", ob, CPU, **kw).keep_best is False


def test_best_policy_round_trip(tmp_path):
    row = SEQUENCES[0][1][8].copy()
    row[0] = 1500.0
    b = BestPolicy(4, row, torch.arange(37, dtype=torch.float32) * 0.5, 0.25)
    assert b.point == 4 and b.step == 1500 and b.row.ret_mean[0] == -10.0 and b.row.violation_rate[0] == 0.25
    b.save(str(tmp_path / "best.npz"))
    c = BestPolicy.load(str(tmp_path / "best.npz"))
    assert c.point == 4 and c.step == 1500 and c.max_violation_rate == 0.25
    assert c.row.rows.tobytes() == b.row.rows.tobytes() and torch.equal(c.params, b.params)
    assert "point=4" in repr(c)


def test_run_on_the_oracle_backend(tmp_path, monkeypatch):
    """None before any point; then the numpy criterion on the harvested rows names the held point, its row and -- against a
    second run that copies the actor's span where the loop evaluates -- its parameters; using_best / restore_best; the
    checkpoint."""
    torch.set_num_threads(1)
    monkeypatch.setenv("RPO_VERBOSE", "0")
    kw = dict(use_graph=False, capacity=16, eval_fre=2)

    def fresh(**more):
        tr = _fresh("ddpg", "cart", ob, CPU, 4, **dict(kw, **more))
        tr.max_episode_steps = 6                               # (a short horizon: the oracle steps the lanes from Python)
        tr.work_dir = str(tmp_path / "ckpt")
        return tr
    a = fresh(eval_episodes=3, keep_best=0.5)
    assert a.best is None
    a.run_steps(9, eval=True)
    rows = a.eval_curve.rows
    kstar, taken = choose_numpy(rows, 0.5)
    assert len(rows) == 4 and kstar >= 0
    best = a.best
    assert best.point == kstar and best.row.rows[0].tobytes() == rows[kstar].tobytes() and best.step == 2 * (kstar + 1)
    b = fresh()
    spans = []
    flat = b.agent.flat
    b.eval = lambda rendering=False: spans.append(flat.param(flat.actor_range).clone()) or (0.0,) * 10
    b.run_steps(9, eval=True)
    assert len(spans) == 4 and torch.equal(best.params, spans[kstar])
    assert torch.equal(a.agent.flat.data, b.agent.flat.data)   # the same training
    live = a.agent.flat.data.clone()
    with pytest.raises(KeyError):
        with a.using_best():
            assert torch.equal(a.agent.flat.param(a.agent.flat.actor_range), best.params)
            raise KeyError("x")
    assert torch.equal(a.agent.flat.data, live)
    # the checkpoint carries the incumbent; one without it leaves none
    a.save()
    c = fresh(eval_episodes=3, keep_best=0.5)
    c.load()
    got = c.best
    assert got.point == kstar and got.row.rows.tobytes() == best.row.rows.tobytes() and torch.equal(got.params, best.params)
    a.restore_best()
    assert torch.equal(a.agent.flat.param(a.agent.flat.actor_range), best.params)
    d = fresh(eval_episodes=3)
    d.run_steps(5, eval=True)
    d.save()
    e = fresh(eval_episodes=3, keep_best=True)
    e.run_steps(3, eval=True)
    e.load()
    assert e.best is None and len(e.eval_curve) == 2
