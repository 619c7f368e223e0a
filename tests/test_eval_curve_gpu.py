"""Curve mode (``eval_episodes=N``) on the MI355X: evaluation points enqueued beside the training (a side stream on a snapshot
of the actor, or in order), reduced by ``rpo_eval_summarize``.  The yardstick of every point is the existing blocking
``trainer.evaluate()``; the bound of every curve column is the float64 summation bound of tests/test_eval_curve.py."""
import numpy as np
import pytest
import torch

from rpo_amd.algo import curve_seed
from rpo_amd.algo.evaluation import EvalResult
from test_eval_curve import (SYNTHETIC, _fresh, blocking_twin, check_points_equal_blocking, check_row, resume_roundtrip,
                             synthetic_acc)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")


@pytest.fixture(scope="module")
def hip():
    from rpo_amd import ops
    assert torch.cuda.is_available()
    return ops


def _pair(hip, algo, envname, n_envs, iters, monkeypatch, fused=True, **kw):
    monkeypatch.setenv("RPO_VERBOSE", "0")
    a = _fresh(algo, envname, hip, DEV, n_envs, fused=fused, eval_episodes=48, **kw)
    a.run_steps(iters, eval=True)
    b = _fresh(algo, envname, hip, DEV, n_envs, fused=fused, **kw)
    results = blocking_twin(b, 48)
    b.run_steps(iters, eval=True)
    torch.cuda.synchronize()
    check_points_equal_blocking(a, results)
    assert torch.equal(a.agent.flat.data, b.agent.flat.data) and torch.equal(a.vec.internal, b.vec.internal)
    return a, b


@pytest.mark.parametrize("overlap", [1, 0])
@pytest.mark.parametrize("algo,envname", [("ddpg", "cart"), ("sac", "cart"), ("ddpg", "pendulum"), ("sac", "pendulum")])
def test_points_equal_blocking_evaluations_fused(hip, algo, envname, overlap, monkeypatch):
    """eval_fre 7 with 16-iteration windows: points inside and across the windows' span, training on."""
    a, _ = _pair(hip, algo, envname, 256, 40, monkeypatch, use_graph=True, capacity=64, eval_fre=7,
                 schedule=dict(eval_overlap=overlap))
    assert a.eval_curve_last.path == "fused" and a._curve.overlap == bool(overlap)
    assert any(e["graph"] is not None for e in a._graphs.entries.values())


@pytest.mark.parametrize("algo,envname,fused", [("ddpg", "evopf256", True), ("ddpgla", "cart", False)])
def test_points_equal_blocking_evaluations_stepwise(hip, algo, envname, fused, monkeypatch):
    a, _ = _pair(hip, algo, envname, 16, 24, monkeypatch, fused=fused, use_graph=True, capacity=32, eval_fre=7)
    assert a.eval_curve_last.path == "stepwise" and not a._curve.overlap


@pytest.mark.parametrize("algo,envname", [("ddpg", "cart"), ("sac", "pendulum")])
def test_the_update_behind_a_point_steps_the_actor(hip, algo, envname, monkeypatch):
    """policy_fre = 1: the update right behind every point writes the actor's parameters while the evaluation may still be
    running -- it reads the snapshot taken on the training stream in front of that update."""
    a, _ = _pair(hip, algo, envname, 256, 24, monkeypatch, use_graph=True, capacity=64, eval_fre=5, policy_fre=1)
    assert a._curve.overlap and a.eval_curve_last.path == "fused"


def _acc_of(r):
    acc = np.zeros((r.episodes, 8), dtype=np.float32)
    for j, f in enumerate(("ret", "mean_ineq", "mean_eq", "max_ineq", "max_eq", "viol_steps", "proj_iters")):
        acc[:, j] = getattr(r, f)
    acc[:, 7] = ((r.length << 2) | (r.nonfinite.astype(np.int64) << 1)).astype(np.int32).view(np.float32)
    return acc


def _summarize(hip, acc, step):
    dacc = torch.tensor(acc, device=DEV)
    ctrl = torch.zeros(hip.CTRL_LEN, dtype=torch.int64, device=DEV)
    ctrl[0] = step
    ws = torch.full((hip.CURVE_WS,), float("nan"), dtype=torch.float64, device=DEV)     # (nothing of it is read before written)
    rows = torch.full((2, hip.CURVE_LEN), -1.0, dtype=torch.float64, device=DEV)
    hip.eval_summarize(dacc, ctrl, rows[0], ws)
    ws.fill_(float("nan"))
    hip.eval_summarize(dacc, ctrl, rows[1], ws)
    out = rows.cpu().numpy()
    assert out[0].tobytes() == out[1].tobytes()
    return out[0]


@pytest.mark.parametrize("n,kind", SYNTHETIC + [(1 << 20, "random")])
def test_summarize_kernel_on_synthetic_rows(hip, n, kind):
    acc = synthetic_acc(n, kind, seed=n)
    row = _summarize(hip, acc, 77)
    check_row(row, EvalResult(acc, "fused", 200, 0), step=77)
    if n == 1:
        assert (row[3:12:2] == 0).all()
    if kind == "nonfinite":
        assert row[14] == len(range(0, n, 3))


@pytest.mark.parametrize("episodes", [48, 1024, 1025, 5000])
def test_summarize_kernel_on_evaluate_rows(hip, episodes):
    tr = _fresh("ddpg", "cart", hip, DEV, 64, use_graph=False)
    tr.run_steps(8)
    r = tr.evaluate(episodes=episodes, seed=3)
    acc = _acc_of(r)
    for f in r.FIELDS:                                          # (the rebuilt rows are the evaluation's rows)
        np.testing.assert_array_equal(getattr(EvalResult(acc, r.path, r.horizon, r.seed), f), getattr(r, f))
    check_row(_summarize(hip, acc, 8), r, step=8)


def test_summarize_refuses_bad_arguments(hip):
    from rpo_amd import _lib
    lib = _lib.load()
    assert lib.rpo_eval_summarize(0, None, None, None, None, None) == _lib.CONST["RPO_ERR_ARG"]
    assert lib.rpo_eval_summarize((1 << 20) + 1, None, None, None, None, None) == _lib.CONST["RPO_ERR_ARG"]
    assert lib.rpo_eval_summarize(4, None, None, None, None, None) == _lib.CONST["RPO_ERR_NULL"]


def _state(tr):
    ag, v = tr.agent, tr.vec
    out = dict(flat=ag.flat.data, critic_target=ag.critic_target_flat, nju=ag.nju.weight, rows=tr.buffer.rows,
               internal=v.internal, obs=v.obs, ep_len=v.ep_len, ep_ret=v.ep_ret, ep_count=v.ep_count, ctrl=v.ctrl)
    if ag.actor_target_flat is not None:
        out["actor_target"] = ag.actor_target_flat
    for name in ("critic_optim", "actor_optim", "nju_optim"):
        opt = getattr(ag, name, None)
        if opt is not None and hasattr(opt, "exp_avg"):
            out[name + ".m"], out[name + ".v"], out[name + ".step"] = opt.exp_avg, opt.exp_avg_sq, opt.step_dev[0:1]
    return out


@pytest.mark.parametrize("algo,envname", [("ddpg", "cart"), ("sac", "cart"), ("sac", "pendulum")])
def test_training_is_untouched(hip, algo, envname, monkeypatch):
    """3 x eval_fre iterations without evaluation, with overlapped points and with in-order points: the same bits everywhere,
    no hand-over or non-finite flag raised.  4096 episodes per point: 256 workgroups resident beside the update's launches."""
    monkeypatch.setenv("RPO_VERBOSE", "0")
    kw = dict(use_graph=True, capacity=64, eval_fre=20)
    ref = _fresh(algo, envname, hip, DEV, 512, **kw)
    ref.run_steps(60, eval=False)
    torch.cuda.synchronize()
    want = _state(ref)
    for overlap in (1, 0):
        tr = _fresh(algo, envname, hip, DEV, 512, eval_episodes=4096, schedule=dict(eval_overlap=overlap), **kw)
        tr.run_steps(60, eval=True)
        torch.cuda.synchronize()
        assert tr._curve.points == 3 and tr._curve.overlap == bool(overlap)
        for k, x in _state(tr).items():
            assert torch.equal(x, want[k]), (overlap, k)
        assert [(k, int(x[0])) for k, x in tr._device_flags() if int(x[0])] == []
        curve = tr.eval_curve
        np.testing.assert_array_equal(curve.step, [20, 40, 60])
        assert (curve.episodes == 4096).all() and (curve.nonfinite == 0).all()
        if overlap:
            first = curve.rows.copy()
        else:
            assert first.tobytes() == curve.rows.tobytes()        # identical either way


def test_more_points_than_ring_rows_and_resume(hip, tmp_path, monkeypatch):
    monkeypatch.setenv("RPO_VERBOSE", "0")
    kw = dict(use_graph=True, capacity=64, eval_fre=1, eval_episodes=16)
    a = _fresh("ddpg", "cart", hip, DEV, 64, **kw)
    a.run_steps(70, eval=True)                                  # 70 points through a ring of 64 rows, never read in between
    assert a._curve.points == 70 and a._curve.ring.shape[0] == 64
    b = _fresh("ddpg", "cart", hip, DEV, 64, **kw)
    for _ in range(7):
        b.run_steps(10, eval=True)
        b.eval_curve
    ca, cb = a.eval_curve, b.eval_curve
    np.testing.assert_array_equal(ca.step, np.arange(1, 71))
    assert ca.rows.tobytes() == cb.rows.tobytes()
    resume_roundtrip(hip, DEV, tmp_path, 64, use_graph=True, capacity=32)


@pytest.mark.parametrize("algo,envname,n", [("ddpg", "cart", 512), ("sac", "pendulum", 512), ("ddpg", "evopf256", 16)])
def test_the_evaluation_stays_outside_the_windows(hip, algo, envname, n, monkeypatch):
    """RPO_GRAPH_AUDIT=1: every captured graph of a curve-mode run holds kernel nodes only, the same graphs are captured as
    without curve mode, and the windows hold as many nodes.  (Only the windows are compared by count: EVOPF-v0's
    single-iteration graph is captured before the first evaluation point, after the same iterations in both runs, and was
    seen with 23 kernel nodes in one run and 21 in the next of the same process, and with 23 in both in another process --
    a property of that capture, not of the evaluation.)"""
    monkeypatch.setenv("RPO_GRAPH_AUDIT", "1")
    monkeypatch.setenv("RPO_VERBOSE", "0")
    kinds = []
    for extra in ({}, dict(eval_episodes=48)):
        tr = _fresh(algo, envname, hip, DEV, n, use_graph=True, capacity=64, eval_fre=40, **extra)
        tr.run_steps(96, eval=True)
        torch.cuda.synchronize()
        assert not tr._graphs.capture_failed
        kinds.append({k: e.get("node_kinds") for k, e in tr._graphs.entries.items() if e["graph"] is not None})
        print(envname, extra, kinds[-1])
    plain, curve = kinds
    assert curve and set(curve) == set(plain)
    windows = [k for k in curve if k[0] == "cycle"]
    assert windows and all(curve[k] == plain[k] for k in windows)
    for k in curve.values():
        assert set(k) == {"kernel"}, k
