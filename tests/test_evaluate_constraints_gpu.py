"""trainer.evaluate(constraints=True) on the MI355X: the fused kernel's CON instances (rpo_<env>_evaluate_constraints)
against the stepwise path's rpo_eval_constraints, that kernel against a numpy reduction of the transition rows copied off the
device, the scalar accumulators, the per-step record, and the training and the default call they must not disturb.  Helpers
and inputs are those of test_evaluate_constraints.py (``two_sided``: a CartSafe-v0 actor that violates both net-force limits;
``_shifted``: SpringPendulum-v0 behind its force limit).
"""
import subprocess

import numpy as np
import pytest
import torch

from rpo_amd.algo.evaluation import EvalResult
from test_act import SHIFT, _shifted
from test_evaluate_constraints import (H, assert_consistent, assert_not_vacuous, assert_report_equals_rows, assert_reports_equal,
                                       rows_by_hand, two_sided)
from test_train_step_golden import build_trainer

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")


@pytest.fixture(scope="module")
def hip():
    from rpo_amd import ops
    assert torch.cuda.is_available()
    return ops


_TRAINED = {}


def _trained(hip, algo, envname):
    """One trainer per case for the module (the tests leave it as they found it)."""
    if (algo, envname) not in _TRAINED:
        torch.manual_seed(5)
        tr = build_trainer(algo, envname, hip, DEV, num_envs=64, use_graph=False)
        tr.vec.reset()
        tr.run_steps(8)                                        # a policy that has moved off its initialisation
        _TRAINED[(algo, envname)] = tr
    return _TRAINED[(algo, envname)]


def _policy(tr, envname, n, seed):
    return two_sided(tr, n, seed) if envname == "cart" else _shifted(tr, SHIFT[envname])


def _both(tr, **kw):
    tr.schedule["fused_eval"] = 1
    try:
        a = tr.evaluate(**kw)
        tr.schedule["fused_eval"] = 0
        b = tr.evaluate(**kw)
    finally:
        tr.schedule["fused_eval"] = 1
    assert a.path == "fused" and b.path == "stepwise"
    return a, b


def _fields_equal(a, b):
    for f in EvalResult.FIELDS:
        np.testing.assert_array_equal(getattr(a, f), getattr(b, f), err_msg=f)


# 17: a partly filled 16-lane workgroup; 100: several of them; 12288 = 64 * 192: the smallest episode count at which eval_kernel
# runs its 64-lane workgroups.  eval_steps=0 is the case whose violations are known in advance (test_evaluate_constraints.py).
@pytest.mark.parametrize("algo,envname,episodes,eval_steps", [("ddpg", "cart", 17, 0), ("ddpg", "cart", 100, None),
                                                              ("sac", "pendulum", 17, 0), ("sac", "pendulum", 100, None),
                                                              ("ddpg", "cart", 12288, None), ("sac", "pendulum", 12288, 0)])
def test_fused_report_equals_stepwise_report_bit_for_bit(hip, algo, envname, episodes, eval_steps):
    tr = _trained(hip, algo, envname)
    with _policy(tr, envname, episodes, 3):
        a, b = _both(tr, episodes=episodes, seed=3, horizon=H, eval_steps=eval_steps, constraints=True)
    _fields_equal(a, b)
    assert_reports_equal(a.constraints, b.constraints)
    k = tr.kernels
    assert a.constraints.ineq_max.shape == (episodes, k.ineq_num) and a.constraints.eq_max.shape == (episodes, k.eq_num)
    for r in (a, b):
        assert_consistent(r)
    assert a.length.max() > 1
    if eval_steps == 0:                                        # (infeasible after Complete, and nothing repairs it)
        assert a.constraints.ineq_steps.sum() > 0 and (a.length < H).any()
    if envname == "cart" and eval_steps == 0:
        assert_not_vacuous(a)
        assert_not_vacuous(b)


@pytest.mark.parametrize("algo,envname", [("ddpg", "cart"), ("sac", "pendulum")])
def test_report_continues_across_launches(hip, algo, envname, monkeypatch):
    """steps = 5 of a horizon of 12: three launches, t0 = 0, 5, 10, the last one partial."""
    tr = _trained(hip, algo, envname)
    with _policy(tr, envname, 100, 3):
        whole = tr.evaluate(100, seed=3, horizon=H, constraints=True)
        monkeypatch.setattr(hip, "EVAL_LANE_STEPS", 100 * 5)
        a, b = _both(tr, episodes=100, seed=3, horizon=H, constraints=True)
    assert a.length.max() > 5                                 # (episodes ran on into a launch with t0 > 0)
    _fields_equal(a, b)
    _fields_equal(a, whole)
    assert_reports_equal(a.constraints, b.constraints)
    assert_reports_equal(a.constraints, whole.constraints)
    assert_consistent(a)


def test_stepwise_kernel_against_the_rows_cart(hip):
    tr = _trained(hip, "ddpg", "cart")
    tr.schedule["fused_eval"] = 0
    try:
        with two_sided(tr, 100, 3):
            r = tr.evaluate(100, seed=3, horizon=H, eval_steps=0, constraints=True)
            rows, thresh = rows_by_hand(tr, 100, 3, H, eval_steps=0)
    finally:
        tr.schedule["fused_eval"] = 1
    assert r.path == "stepwise"
    assert_report_equals_rows(r, rows, tr.kernels.cols, thresh)
    assert_consistent(r)
    assert_not_vacuous(r)


def test_stepwise_kernel_against_the_rows_evopf(hip):
    torch.manual_seed(5)
    tr = build_trainer("ddpg", "evopf256", hip, DEV, num_envs=16, use_graph=False)
    r = tr.evaluate(16, seed=3, horizon=4, constraints=True)
    rows, thresh = rows_by_hand(tr, 16, 3, 4)
    k = tr.kernels
    assert r.path == "stepwise" and r.constraints.ineq_max.shape == (16, 58) and r.constraints.eq_max.shape == (16, 28)
    assert hip.con_width(k.ineq_num, k.eq_num) == 144
    assert_report_equals_rows(r, rows, k.cols, thresh)
    assert_consistent(r)
    assert r.constraints.names[20] == "vmax[0]" and len(r.constraints.worst()) == 5
    assert (r.length == 4).all() and r.constraints.eq_max.max() > 0
    plain = tr.evaluate(16, seed=3, horizon=4)
    _fields_equal(r, plain)
    assert plain.constraints is None


@pytest.mark.parametrize("algo,envname", [("ddpg", "cart"), ("sac", "pendulum")])
def test_report_with_a_record(hip, algo, envname):
    """constraints=True, record=8 in one call: trace, accumulators and report are those of the separate calls, on both paths."""
    tr = _trained(hip, algo, envname)
    kw = dict(episodes=100, seed=3, horizon=H)
    with _policy(tr, envname, 100, 3):
        both = _both(tr, record=8, constraints=True, **kw)
        rec = _both(tr, record=8, **kw)
        con = _both(tr, constraints=True, **kw)
        plain = tr.evaluate(**kw)
    for x, r, c in zip(both, rec, con):
        assert r.constraints is None and c.trajectory is None and x.trajectory.episodes == 8
        _fields_equal(x, plain)
        _fields_equal(r, plain)
        _fields_equal(c, plain)
        assert_reports_equal(x.constraints, c.constraints)
        for name in r.trajectory.ARRAYS:
            assert getattr(x.trajectory, name).tobytes() == getattr(r.trajectory, name).tobytes(), name
        tj = x.trajectory
        assert tj.valid.sum() == x.length[:8].sum() > 8
        np.testing.assert_array_equal(np.where(tj.valid, tj.ineq, 0).max(1).astype(np.float64), x.constraints.ineq_max[:8].max(1))
        np.testing.assert_array_equal(np.where(tj.valid, tj.eq, 0).max(1).astype(np.float64), x.constraints.eq_max[:8].max(1))
    assert_reports_equal(both[0].constraints, both[1].constraints)


def test_the_default_call_is_unchanged(hip):
    """evaluate() without the argument: no report, and the accumulator bits of the launches without one -- the bindings called
    directly with and without con agree too."""
    tr = _trained(hip, "ddpg", "cart")
    with two_sided(tr, 1000, 3):
        plain = tr.evaluate(1000, seed=3)
        off = tr.evaluate(1000, seed=3, constraints=False)
        on = tr.evaluate(1000, seed=3, constraints=True)

        def direct(con):
            v = tr.base_env.make_vec(48, seed=9, max_episode_steps=tr.max_episode_steps, device=DEV, stats_cap=2)
            v.reset()
            acc = torch.zeros(48, 8, device=DEV)
            scale, base = tr._box_affine
            for t0 in (0, 6):
                tr.kernels.evaluate(tr.fused.descs["actor"], tr._gauss_policy, scale, base, v.internal, None, v.action, v.ep_len,
                                    v.ep_ret, v.ep_count, v.ctrl, acc, t0, 6, tr._box_lo, tr._box_hi, tr.eval_steps, tr.eval_lr,
                                    tr.corr_eps, tr.corr_momentum, v.max_episode_steps, v.viol_thresh,
                                    **({} if con is None else dict(con=con)))
            return acc
        a0 = direct(None)
        con = torch.full((48, 16), float("nan"), device=DEV)    # (step 0 writes every cell, padding included)
        a1 = direct(con)
        for bad in (torch.zeros(48, 12, device=DEV), torch.zeros(47, 16, device=DEV), torch.zeros(48 * 16, device=DEV)):
            with pytest.raises(hip.RpoHipError):
                direct(bad)
        with pytest.raises(hip.RpoHipError, match="invalid argument"):
            direct(torch.zeros(48 * 16 + 4, device=DEV)[1:-3].view(48, 16))       # 4-byte aligned only
    assert plain.path == "fused" and plain.constraints is None and off.constraints is None
    _fields_equal(plain, off)
    _fields_equal(plain, on)
    assert torch.equal(a0, a1)
    con = con.cpu().numpy()
    assert np.isfinite(con).all() and not con[:, 13:].any() and con[:, :6].max() > 0


def test_constraints_have_no_side_effects_on_the_device(hip, monkeypatch):
    """test_no_side_effects_on_the_device with the report on: training after evaluate(constraints=True) is the training without."""
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
    r = b.evaluate(4096, constraints=True, record=8)
    assert r.path == "fused" and r.constraints.episodes == 4096
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


def test_abi_exports_the_constraint_entry_points(hip):
    from rpo_amd import _lib
    new = {"rpo_cartsafe_evaluate_constraints", "rpo_pendulum_evaluate_constraints", "rpo_eval_constraints"}
    assert new <= set(_lib.PROTOTYPES)
    syms = subprocess.run(["nm", "-D", "--defined-only", _lib.LIBRARY], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in syms.splitlines() if " T " in line}
    assert new <= exported and exported == set(_lib.PROTOTYPES)
    assert hip.con_width(6, 1) == 16 and hip.con_width(1, 1) == 4 and hip.con_width(58, 28) == 144
