"""Curve mode (``eval_episodes=N``) on the CPU: the host logic of the enqueued evaluation points driven by the oracle backend,
with ``summarize_torch`` standing in for ``rpo_eval_summarize``.

* Point k of a curve-mode run is the blocking ``evaluate(episodes=N, seed=curve_seed(seed, k))`` of the same run without curve
  mode, called where the loop calls ``eval()``: same steps, same per-episode accumulator rows, and every curve column within
  the summation bound below.
* The summary alone, on synthetic accumulator rows.
* The device ring wrapping, checkpoints, argument validation, the printed lines.

The bound (``check_row``).  A float64 sum of n terms in ANY order differs from the exact sum by at most (n - 1) u sum|x|,
u = 2^-53; dividing by n adds one rounding.  So |mean - x.mean()| <= n u mean|x| against numpy's own float64 result, and the
same bound relative to the variance for the mean of the squared deviations.
"""
import numpy as np
import pytest
import torch

import oracle_backend as ob
from rpo_amd.algo import EvalCurve, curve_seed
from rpo_amd.algo import evaluation as ev
from rpo_amd.algo.evaluation import EvalResult
from test_train_step_golden import build_trainer

U = 2.0 ** -53
STATS = ("ret", "mean_ineq", "mean_eq", "max_ineq", "max_eq")
CPU = torch.device("cpu")


def check_row(row, r, step=None):
    """One curve row [16] against the numpy values of an EvalResult (float32 accumulators widened to float64)."""
    c = EvalCurve(row)
    n = r.episodes
    assert len(c) == 1 and c.episodes[0] == n
    if step is not None:
        assert c.step[0] == step
    for name in STATS:
        x = getattr(r, name)
        m, s = getattr(c, name + "_mean")[0], getattr(c, name + "_std")[0]
        print("%s n=%d: mean %.17g numpy %.17g | var %.17g numpy %.17g" % (name, n, m, x.mean(), s * s, x.var()))
        if not np.isfinite(x).all():
            continue
        assert abs(m - x.mean()) <= n * U * np.abs(x).mean(), name
        assert abs(s * s - x.var()) <= n * U * x.var(), name
    assert c.rows[0, 12] == r.length.sum() and c.rows[0, 13] == r.viol_steps.sum()
    assert c.nonfinite[0] == r.nonfinite.sum()
    assert c.length_mean[0] == r.length.sum() / n and c.violation_rate[0] == r.violation_rate()
    assert c.summary(0) == tuple(c.rows[0, 2:12])


def synthetic_acc(n, kind, seed=0):
    """Accumulator rows [n, 8] float32 in the RPO_EVAL_* layout."""
    rng = np.random.default_rng(seed)
    acc = np.zeros((n, 8), dtype=np.float32)
    acc[:, :5] = rng.normal(size=(n, 5)) * np.array([100.0, 1e-3, 1e-6, 1e-2, 1e-5]) + np.array([-250.0, 2e-3, 0.0, 5e-2, 1e-5])
    if kind == "constant":
        acc[:, :5] = np.array([3.25, 0.1, 1e-7, 7.0, 0.0], dtype=np.float32)
    if kind == "outlier":
        acc[n // 2, 0] = 1e30
    length = rng.integers(1, 200, size=n)
    acc[:, 5] = rng.integers(0, length + 1)
    acc[:, 6] = rng.integers(0, 50 * length)
    word = (length << 2).astype(np.int32)
    if kind == "nonfinite":
        word[::3] |= 2
    acc[:, 7] = word.view(np.float32)
    return acc


SYNTHETIC = [(n, kind) for n in (1, 17, 256, 4097, 65536) for kind in ("random", "constant", "outlier", "nonfinite")]


@pytest.mark.parametrize("n,kind", SYNTHETIC)
def test_summarize_torch_meets_the_summation_bound(n, kind):
    acc = torch.tensor(synthetic_acc(n, kind, seed=n))
    ctrl = torch.zeros(8, dtype=torch.int64)
    ctrl[0] = 1234
    a, b = torch.zeros(16, dtype=torch.float64), torch.full((16,), 7.0, dtype=torch.float64)
    ev.summarize_torch(acc, ctrl, a)
    ev.summarize_torch(acc, ctrl, b)
    assert a.numpy().tobytes() == b.numpy().tobytes()
    r = EvalResult(acc.numpy(), "stepwise", 200, 0)
    check_row(a.numpy(), r, step=1234)
    if n == 1:
        assert (a[3:12:2] == 0).all()
    if kind == "nonfinite":
        assert a[14] == len(range(0, n, 3))


def _fresh(algo, envname, backend, dev, n_envs, **kw):
    torch.manual_seed(5)
    tr = build_trainer(algo, envname, backend, dev, num_envs=n_envs, **kw)
    tr.vec.reset()
    return tr


def blocking_twin(tr, episodes):
    """Replace tr.eval by the EXISTING blocking evaluate() with the curve's seeds; returns the list the results go to."""
    results = []

    def fake_eval(rendering=False):
        r = tr.evaluate(episodes=episodes, seed=curve_seed(tr.seed, len(results)))
        results.append((tr._t, r))
        return r.summary()
    tr.eval = fake_eval
    return results


def check_points_equal_blocking(a, results):
    curve = a.eval_curve
    assert len(curve) == len(results) >= 3
    np.testing.assert_array_equal(curve.step, [t for t, _ in results])
    for k, (t, r) in enumerate(results):
        check_row(curve.rows[k], r, step=t)
    last = a.eval_curve_last
    for f in last.FIELDS:
        np.testing.assert_array_equal(getattr(last, f), getattr(results[-1][1], f), err_msg=f)
    assert last.seed == results[-1][1].seed and last.horizon == results[-1][1].horizon


@pytest.mark.parametrize("algo,envname", [("ddpg", "cart"), ("sac", "pendulum")])
def test_points_equal_blocking_evaluations_on_oracle_backend(algo, envname, monkeypatch):
    torch.set_num_threads(1)
    monkeypatch.setenv("RPO_VERBOSE", "0")
    kw = dict(use_graph=False, capacity=16, eval_fre=3)
    a = _fresh(algo, envname, ob, CPU, 4, eval_episodes=48, **kw)
    a.max_episode_steps = 12                                   # (a short horizon: the oracle steps 48 lanes from Python)
    a.run_steps(10, eval=True)
    b = _fresh(algo, envname, ob, CPU, 4, **kw)
    b.max_episode_steps = 12
    results = blocking_twin(b, 48)
    b.run_steps(10, eval=True)
    check_points_equal_blocking(a, results)
    assert a.eval_curve_last.path == "stepwise"
    # ... and the training beside them is the same training
    assert torch.equal(a.agent.flat.data, b.agent.flat.data) and torch.equal(a.buffer.rows, b.buffer.rows)
    assert torch.equal(a.vec.ctrl, b.vec.ctrl) and torch.equal(a.vec.internal, b.vec.internal)


def test_more_points_than_ring_rows(monkeypatch):
    torch.set_num_threads(1)
    monkeypatch.setenv("RPO_VERBOSE", "0")
    monkeypatch.setattr(ev, "_CURVE_RING", 4)
    a = _fresh("ddpg", "cart", ob, CPU, 4, use_graph=False, capacity=16, eval_fre=1, eval_episodes=3)
    a.max_episode_steps = 4
    a.run_steps(11, eval=True)
    assert a._curve.points == 11 and a._curve.ring.shape[0] == 4
    c = a.eval_curve
    np.testing.assert_array_equal(c.step, np.arange(1, 12))
    b = _fresh("ddpg", "cart", ob, CPU, 4, use_graph=False, capacity=16, eval_fre=1, eval_episodes=3)
    b.max_episode_steps = 4
    for _ in range(11):                                        # read after every point: the ring never wraps
        b.run_steps(1, eval=True)
        b.eval_curve
    assert c.rows.tobytes() == b.eval_curve.rows.tobytes()


def resume_roundtrip(backend, dev, tmp_path, n_envs, **kw):
    """save() after point 2, load() into a fresh trainer, continue: the curve of the uninterrupted run, bit for bit."""
    def fresh(**more):
        tr = _fresh("ddpg", "cart", backend, dev, n_envs, eval_fre=3, **dict(kw, **more))
        tr.work_dir = str(tmp_path / "ckpt")
        return tr
    a = fresh(eval_episodes=16)
    a.run_steps(19, eval=True)
    b = fresh(eval_episodes=16)
    b.run_steps(10, eval=True)                                 # points 0, 1, 2 (steps 3, 6, 9)
    b.save()
    c = fresh(eval_episodes=16)
    c.load()
    assert len(c.eval_curve) == 3 and c._curve.points == 3
    c.run_steps(9, eval=True)
    ca, cc = a.eval_curve, c.eval_curve
    np.testing.assert_array_equal(ca.step, [3, 6, 9, 12, 15, 18])
    assert ca.rows.tobytes() == cc.rows.tobytes()
    # a checkpoint of a trainer without curve mode loads into one with it: an empty curve, the same training
    d = fresh()
    d.run_steps(4)
    d.save()
    e = fresh(eval_episodes=16)
    e.run_steps(7, eval=True)
    assert len(e.eval_curve) == 2
    e.load()
    assert len(e.eval_curve) == 0 and e._curve.points == 0 and e._t == 4
    # ... and the other way round
    b.save()
    f = fresh()
    f.load()
    assert len(f.eval_curve) == 0 and f._t == 10


def test_curve_travels_with_the_checkpoint(tmp_path, monkeypatch):
    torch.set_num_threads(1)
    monkeypatch.setenv("RPO_VERBOSE", "0")
    resume_roundtrip(ob, CPU, tmp_path, 4, use_graph=False, capacity=32)


def test_arguments_and_defaults(monkeypatch):
    for bad in (0, -3, 2.5, True, "many"):
        with pytest.raises(ValueError):
            build_trainer("ddpg", "cart", ob, CPU, num_envs=2, use_graph=False, eval_episodes=bad)
    tr = build_trainer("ddpg", "cart", ob, CPU, num_envs=2, use_graph=False)
    assert tr.eval_episodes is None and tr._curve is None and len(tr.eval_curve) == 0 and tr.eval_curve_last is None
    assert tr.schedule["eval_overlap"] == 1
    monkeypatch.setenv("RPO_EVAL_EPISODES", "7")
    tr = build_trainer("sacla", "cart", ob, CPU, num_envs=2, use_graph=False, fused=False)
    assert tr.eval_episodes == 7 and tr._curve.n == 7
    monkeypatch.setenv("RPO_EVAL_EPISODES", "0")
    with pytest.raises(ValueError):
        build_trainer("ddpg", "cart", ob, CPU, num_envs=2, use_graph=False)
    # documented formula, independent of evaluate()'s call counter
    assert curve_seed(11, 0) == ((11 ^ 0xC0A7C0A7) + 0x9E3779B97F4A7C15) & (2 ** 63 - 1)
    assert len({curve_seed(11, k) for k in range(100)}) == 100 and curve_seed(11, 3) != curve_seed(12, 3)
    assert EvalCurve.COLUMNS[2:12] == tuple(s + m for s in STATS for m in ("_mean", "_std"))


def test_lines_are_printed_at_the_harvest(monkeypatch, capsys):
    torch.set_num_threads(1)
    monkeypatch.setenv("RPO_VERBOSE", "1")
    a = _fresh("ddpg", "cart", ob, CPU, 4, use_graph=False, capacity=16, eval_fre=2, eval_episodes=3)
    a.max_episode_steps = 4
    a.run_steps(5, eval=True)
    assert "Eval: epoch" not in capsys.readouterr().out       # enqueued, not read
    curve = a.eval_curve
    out = capsys.readouterr().out
    assert out.count("Eval: epoch") == 2 and "Eval: epoch 2," in out and "Eval: epoch 4," in out and "lambda" not in out
    assert f"rewards: {curve.ret_mean[0]:.4f}({curve.ret_std[0]:.4f})" in out
    a.eval_curve
    assert "Eval" not in capsys.readouterr().out               # each row once
