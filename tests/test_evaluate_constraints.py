"""trainer.evaluate(constraints=True) on the CPU: the stepwise path driven by the oracle backend (``constraints_torch``).

The yardstick is the project's own transition rows: the stepwise loop is driven by hand (``_eval_action`` +
``step(auto_reset=False)``), every step's rows are kept on the host, and numpy reduces them with the definitions of
``ConstraintReport`` -- maxima started at 0 with rpo_eval_dev::nanmax, counts of ``> float32(viol_thresh)``, over the steps
``t < length[episode]``.  The report must equal that reduction on the float32 bits and on the counts.
test_evaluate_constraints_gpu.py imports the helpers below.

Inputs.  A policy a few training steps old violates nothing, and a constant shift of the actor's last bias (``_shifted`` of
test_act.py) pushes CartSafe-v0 against ONE of its two net-force limits only.  ``two_sided`` therefore replaces the actor's
last layer by 30 x a seeded random vector with no bias: the proposal saturates at +-10 (of the box of 10) with a sign that
depends on the state, Complete leaves |net horizontal force| = 10 cos(pi/6) + 10 tan(pi/6) cos(pi/3) = 11.5 > 8, and with
``eval_steps=0`` nothing repairs it -- ``hforce_max`` is violated where the proposal is positive, ``hforce_min`` where it is
negative.  The weight seed is the first one whose proposals on the evaluation's own initial observations have both signs
(a property of the inputs, not of the report); the saturated forces also end episodes before the horizon of 12.
"""
import numpy as np
import pytest
import torch

import oracle_backend as ob
from rpo_amd.algo import ConstraintReport
from rpo_amd.algo.evaluation import EvalResult
from test_act import SHIFT, _shifted
from test_train_step_golden import build_trainer

F32 = np.float32
H = 12


# ------------------------------------------------------------------------------------------------ shared helpers
def initial_obs(tr, n, seed):
    """The observations evaluate(n, seed=seed) starts from."""
    v = tr.base_env.make_vec(n, seed=seed, env_id_base=0, max_episode_steps=tr.max_episode_steps, device=tr.device, stats_cap=2,
                             viol_thresh=tr.vec.viol_thresh)
    v.reset()
    return v.obs.clone()


class two_sided(object):
    """Inside the block the actor's last layer is 30 x randn(weight seed) without bias, the weight seed being the first of
    0..31 for which the proposals at the initial observations of evaluate(n, seed=seed) saturate with both signs."""

    def __init__(self, tr, n, seed):
        t = tr.fused.descs["actor"].tensors
        self.tr, self.w, self.b, self.obs = tr, t["W1"], t["b1"], initial_obs(tr, n, seed)

    def __enter__(self):
        with torch.no_grad():
            self.old = self.w.detach().clone(), self.b.detach().clone()
            self.b.zero_()
            for ws in range(32):
                w = torch.randn(self.w.shape, generator=torch.Generator().manual_seed(ws))
                self.w.copy_(30.0 * w.to(self.w.device))
                ap = self.tr._eval_partial(self.obs).reshape(-1)
                if int((ap > 9.0).sum()) >= 2 and int((ap < -9.0).sum()) >= 2:
                    return self
        self.__exit__()
        raise AssertionError("no weight seed gives proposals of both signs")

    def __exit__(self, *exc):
        with torch.no_grad():
            self.w.copy_(self.old[0])
            self.b.copy_(self.old[1])
        return False


def rows_by_hand(tr, n, seed, horizon, eval_steps=None):
    """evaluate()'s stepwise loop without its statistics -> the transition rows of every step, numpy [horizon, n, ring]."""
    k = tr.kernels
    v = tr.base_env.make_vec(n, seed=seed, env_id_base=0, max_episode_steps=tr.max_episode_steps, device=tr.device, stats_cap=2,
                             viol_thresh=tr.vec.viol_thresh)
    v.reset()
    rows = torch.zeros(n, k.ring_floats, device=tr.device)
    iters = torch.zeros(n, dtype=torch.int32, device=tr.device)
    out = []
    with torch.no_grad():
        for _ in range(horizon):
            if eval_steps is None:
                tr._eval_action(v, iters=iters)
            else:
                tr._eval_action(v, iters=iters, eval_steps=eval_steps, eval_lr=tr.eval_lr)
            v.step(v.action, rows=rows, cap_steps=1, auto_reset=False)
            out.append(rows.cpu().numpy().copy())
    return np.stack(out), float(v.viol_thresh)


def _nanmax(a, b):
    """rpo_eval_dev::nanmax, elementwise"""
    return np.where(a != a, a, np.where(b != b, b, np.where(b > a, b, a)))


def reduce_rows(rows, cols, length, viol_thresh):
    """The definitions of ConstraintReport on the host: (ineq_max, ineq_steps, eq_max) of the steps t < length[episode]."""
    (e0, e1), (i0, i1) = cols["eq_viol"], cols["ineq_viol"]
    n = rows.shape[1]
    imax, emax = np.zeros((n, i1 - i0), F32), np.zeros((n, e1 - e0), F32)
    steps = np.zeros((n, i1 - i0), np.int64)
    for t in range(rows.shape[0]):
        live = (t < np.asarray(length))[:, None]
        ineq, eq = rows[t, :, i0:i1], np.abs(rows[t, :, e0:e1])
        imax = np.where(live, _nanmax(imax, ineq), imax)
        emax = np.where(live, _nanmax(emax, eq), emax)
        steps += live & (ineq > F32(viol_thresh))
    return imax, steps, emax


def assert_report_equals_rows(r, rows, cols, viol_thresh):
    c = r.constraints
    imax, steps, emax = reduce_rows(rows, cols, r.length, viol_thresh)
    assert c.ineq_max.dtype == np.float64 and c.eq_max.dtype == np.float64 and c.ineq_steps.dtype == np.int64
    assert c.ineq_max.shape == imax.shape and c.eq_max.shape == emax.shape
    for name, got, want in (("ineq_max", c.ineq_max, imax), ("eq_max", c.eq_max, emax)):
        got = got.astype(F32)
        assert np.array_equal(got.astype(np.float64), getattr(c, name), equal_nan=True), name   # widened float32 bits
        print(name, "cells that differ:", int((got.view(np.int32) != want.view(np.int32)).sum()), "of", got.size)
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), name
    print("ineq_steps cells that differ:", int((c.ineq_steps != steps).sum()), "of", steps.size)
    np.testing.assert_array_equal(c.ineq_steps, steps)
    np.testing.assert_array_equal(c.length, r.length)
    assert c.viol_thresh == viol_thresh


def assert_consistent(r):
    """The report against the scalar accumulators, exact."""
    c = r.constraints
    np.testing.assert_array_equal(c.ineq_max.max(1), r.max_ineq)
    np.testing.assert_array_equal(c.eq_max.max(1), r.max_eq)
    assert (c.ineq_steps.max(1) <= r.viol_steps).all() and (r.viol_steps <= c.ineq_steps.sum(1)).all()
    assert (c.ineq_steps <= r.length[:, None]).all() and (c.ineq_steps >= 0).all()


def assert_not_vacuous(r):
    """Two different inequalities were violated and an episode ended before the horizon."""
    assert int((r.constraints.ineq_steps.sum(0) > 0).sum()) >= 2, r.constraints.ineq_steps.sum(0)
    assert (r.length < r.horizon).any() and r.length.min() >= 1


def assert_results_equal(a, b):
    for f in EvalResult.FIELDS:
        np.testing.assert_array_equal(getattr(a, f), getattr(b, f), err_msg=f)
    assert a.path == b.path and a.horizon == b.horizon and a.seed == b.seed


def assert_reports_equal(a, b):
    for name in ConstraintReport.ARRAYS:
        x, y = getattr(a, name), getattr(b, name)
        assert x.dtype == y.dtype and x.shape == y.shape, name
        assert x.tobytes() == y.tobytes(), name              # bit for bit (NaN-safe)
    assert a.names == b.names and a.eq_names == b.eq_names and a.viol_thresh == b.viol_thresh


# ------------------------------------------------------------------------------------------------ the CPU suite
def _cpu_trainer(algo, envname):
    torch.set_num_threads(1)
    torch.manual_seed(5)
    if envname == "evopf":                                       # a Newton solve per row and step on this backend
        return build_trainer(algo, envname, ob, torch.device("cpu"), num_envs=4, fused=False, use_graph=False)
    tr = build_trainer(algo, envname, ob, torch.device("cpu"), num_envs=64, use_graph=False)
    tr.vec.reset()
    tr.run_steps(8)
    return tr


@pytest.fixture(scope="module")
def cart():
    """(trainer, evaluate(17, seed=3, horizon=12, eval_steps=0, constraints=True) under two_sided, the rows by hand)."""
    tr = _cpu_trainer("ddpg", "cart")
    with two_sided(tr, 17, 3):
        r = tr.evaluate(17, seed=3, horizon=H, eval_steps=0, constraints=True)
        rows, thresh = rows_by_hand(tr, 17, 3, H, eval_steps=0)
    return tr, r, rows, thresh


def test_cart_report_equals_the_rows_and_is_not_vacuous(cart):
    tr, r, rows, thresh = cart
    assert r.path == "stepwise" and isinstance(r.constraints, ConstraintReport)
    assert r.constraints.ineq_max.shape == (17, 6) and r.constraints.eq_max.shape == (17, 1)
    assert_report_equals_rows(r, rows, tr.kernels.cols, thresh)
    assert_consistent(r)
    assert_not_vacuous(r)


@pytest.mark.parametrize("algo,envname,n,horizon", [("sac", "pendulum", 17, H), ("ddpg", "evopf", 2, 3)])
def test_report_equals_the_rows(algo, envname, n, horizon):
    tr = _cpu_trainer(algo, envname)
    if envname == "evopf":
        r = tr.evaluate(n, seed=3, horizon=horizon, constraints=True)
        rows, thresh = rows_by_hand(tr, n, 3, horizon)
    else:
        with _shifted(tr, SHIFT[envname]):                       # violations behind the projection
            r = tr.evaluate(n, seed=3, horizon=horizon, constraints=True)
            rows, thresh = rows_by_hand(tr, n, 3, horizon)
    k = tr.kernels
    assert r.path == "stepwise" and r.constraints.ineq_max.shape == (n, k.ineq_num) and r.constraints.eq_max.shape == (n, k.eq_num)
    assert_report_equals_rows(r, rows, k.cols, thresh)
    assert_consistent(r)
    if envname == "pendulum":
        assert r.constraints.ineq_steps.sum() > 0 and (r.length < horizon).any()
    else:
        assert r.constraints.eq_max.max() > 0                    # (the Newton solve's residual)


@pytest.mark.parametrize("algo,envname", [("ddpg", "cart"), ("sac", "pendulum")])
def test_the_report_changes_no_other_result(algo, envname):
    tr = _cpu_trainer(algo, envname)
    kw = dict(episodes=9, seed=4, horizon=H)
    with _shifted(tr, SHIFT[envname]):
        plain, con = tr.evaluate(**kw), tr.evaluate(constraints=True, **kw)
        rec, both = tr.evaluate(record=5, **kw), tr.evaluate(record=5, constraints=True, **kw)
        over = tr.evaluate(constraints=True, eval_steps=0, eval_lr=2.0 * tr.eval_lr, **kw)
        init = tr.evaluate(constraints=True, init_states=initial_obs(tr, 9, 4) if envname == "cart" else None, **kw)
    assert plain.constraints is None and rec.constraints is None and con.trajectory is None
    assert_results_equal(con, plain)
    assert_results_equal(both, plain)
    assert_reports_equal(both.constraints, con.constraints)
    for name in rec.trajectory.ARRAYS:
        assert getattr(both.trajectory, name).tobytes() == getattr(rec.trajectory, name).tobytes(), name
    # the recorded steps carry the same maxima
    tj = both.trajectory
    want = np.where(tj.valid, tj.ineq, 0).max(1).astype(np.float64)
    np.testing.assert_array_equal(both.constraints.ineq_max[:5].max(1), want)
    assert int(np.abs(over.proj_iters).max()) == 0 and over.constraints.ineq_steps.sum() >= con.constraints.ineq_steps.sum()
    assert_reports_equal(init.constraints, con.constraints)     # (cart: the observation IS the injected state)


def test_host_helpers(cart, tmp_path):
    tr, r, _, _ = cart
    c = r.constraints
    assert c.names == tr.base_env.ineq_names and c.eq_names == tr.base_env.eq_names and c.episodes == 17
    total = c.ineq_steps.sum(0)
    np.testing.assert_array_equal(c.rate(), total / float(r.length.sum()))
    assert c.rate().shape == (6,) and 0 < c.rate().max() <= 1
    w = c.worst()
    assert len(w) == 5 and len(c.worst(2)) == 2 and len(c.worst(100)) == 6 and c.worst(0) == []
    assert [x[2] for x in w] == sorted(total.tolist(), reverse=True)[:5]
    j, name, steps, mx = w[0]
    assert name == c.names[j] and steps == total[j] == total.max() and mx == c.ineq_max[:, j].max() > c.viol_thresh
    assert {w[0][1], w[1][1]} == {"hforce_max", "hforce_min"}
    assert "ConstraintReport(episodes=17" in repr(c) and name in repr(c)
    path = str(tmp_path / "con.npz")
    c.save(path)
    assert_reports_equal(ConstraintReport.load(path), c)
    # a hand-made report: counts, ties and names
    h = ConstraintReport.from_rows(np.array([[0.5, 0.0, 2.0, 3, 0, 3, 0.25, 0], [0.1, 0.0, 1.0, 1, 0, 1, 0.5, 0]], F32), 3, 1,
                                   [4, 4], 0.05)
    assert h.names == ("ineq[0]", "ineq[1]", "ineq[2]") and h.eq_names == ("eq[0]",)
    assert h.worst(2) == [(0, "ineq[0]", 4, 0.5), (2, "ineq[2]", 4, 2.0)] and h.rate().tolist() == [0.5, 0.0, 0.5]
    assert h.eq_max.tolist() == [[0.25], [0.5]] and h.ineq_steps.tolist() == [[3, 0, 3], [1, 0, 1]]
    with pytest.raises(ValueError):
        ConstraintReport(0.05, ("a",), ("b",), ineq_max=h.ineq_max, ineq_steps=h.ineq_steps, eq_max=h.eq_max, length=h.length)


@pytest.mark.parametrize("envname,ineq,eq", [("cart", 6, 1), ("pendulum", 1, 1), ("evopf", 58, 28)])
def test_names_of_the_three_envs(envname, ineq, eq):
    tr = _cpu_trainer("ddpg", envname)
    env = tr.base_env
    assert len(env.ineq_names) == ineq == tr.kernels.ineq_num and len(env.eq_names) == eq == tr.kernels.eq_num
    assert len(set(env.ineq_names)) == ineq and len(set(env.eq_names)) == eq
    if envname == "evopf":                                       # the blocks of oracle/evopf.py's ineq_resid, in its order
        assert env.ineq_names[0] == "pgmax[0]" and env.ineq_names[9] == "pgmin[4]" and env.ineq_names[20] == "vmax[0]"
        assert env.ineq_names[47] == "vmin[13]" and env.ineq_names[48] == "pemax[0]" and env.ineq_names[57] == "pemin[4]"
        assert env.eq_names[0] == "pbal[0]" and env.eq_names[27] == "qbal[13]"


def test_constraints_validates_its_argument_and_curve_mode_has_no_report():
    tr = _cpu_trainer("ddpg", "cart")
    calls = getattr(tr, "_evaluate_calls", 0)
    for bad in (1, 0, None, "yes", [True], 1.0):
        with pytest.raises(ValueError, match="constraints"):
            tr.evaluate(4, horizon=3, constraints=bad)
    assert getattr(tr, "_evaluate_calls", 0) == calls            # refused before anything was drawn or allocated
    assert tr.evaluate(4, horizon=3).constraints is None and tr.evaluate(4, horizon=3, constraints=False).constraints is None
    torch.manual_seed(5)
    cv = build_trainer("ddpg", "cart", ob, torch.device("cpu"), num_envs=4, use_graph=False, capacity=8, eval_episodes=3)
    assert cv.eval_curve_last is None
    cv._curve.enqueue()
    assert cv.eval_curve_last.constraints is None and cv.eval_curve_last.episodes == 3
