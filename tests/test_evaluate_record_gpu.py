"""trainer.evaluate(record=...) on the MI355X: the fused kernel's REC instances (rpo_<env>_evaluate_record) against the
stepwise path's rpo_eval_record, the accumulators they must not change, the oracle env, and the training they must not
disturb.  The checks (arrays-equal, replay, dynamics) and their helpers are those of test_evaluate_record.py; the replay
here is rpo_eval_lane_update's arithmetic to the letter (float32 reciprocal), the dynamics tolerances are those of
test_cart_step_matches_reference / test_pendulum_step_matches_reference (test_kernels_gpu.py: float32 dynamics on the
device against the float64 oracle).
"""
import subprocess

import numpy as np
import pytest
import torch

from test_evaluate_record import (assert_arrays_equal, assert_dynamics, assert_replay, assert_zero_outside_valid)
from test_train_step_golden import build_trainer

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
COMBOS = [("ddpg", "cart"), ("sac", "cart"), ("ddpg", "pendulum"), ("sac", "pendulum")]
# test_kernels_gpu.py: cart next state (positions / velocities 1e-5, accelerations 1e-4), eq 2e-6, ineq 2e-6 / 4e-6, reward
# exact (1 per step); pendulum next obs 2e-5, reward 2e-5 / 1e-6, violations 1e-5 / 1e-4
CART_TOL = dict(next_obs=[([0, 1, 3, 4], 1e-5, 1e-5), ([2, 5], 1e-4, 1e-4)], reward=None, ineq=(2e-6, 4e-6), eq=(2e-6, 2e-6))
PEND_TOL = dict(next_obs=[(slice(None), 2e-5, 2e-5)], reward=(2e-5, 1e-6), ineq=(1e-5, 1e-4), eq=(1e-5, 1e-4))


@pytest.fixture(scope="module")
def hip():
    from rpo_amd import ops
    assert torch.cuda.is_available()
    return ops


def _trained(hip, algo, envname, **kw):
    torch.manual_seed(5)
    tr = build_trainer(algo, envname, hip, DEV, num_envs=64, use_graph=False, **kw)
    tr.vec.reset()
    tr.run_steps(8)                                            # a policy that has moved off its initialisation
    return tr


def _both(tr, **kw):
    tr.schedule["fused_eval"] = 1
    a = tr.evaluate(**kw)
    tr.schedule["fused_eval"] = 0
    b = tr.evaluate(**kw)
    tr.schedule["fused_eval"] = 1
    assert a.path == "fused" and b.path == "stepwise"
    return a, b


def _traces_equal(a, b):
    ta, tb = a.trajectory, b.trajectory
    for name in ta.ARRAYS:
        x, y = getattr(ta, name), getattr(tb, name)
        assert x.dtype == y.dtype and x.shape == y.shape, name
        assert x.tobytes() == y.tobytes(), name              # bit for bit (NaN-safe)


# 1000: not a multiple of 16 (a partly filled 16-lane workgroup), the whole horizon in one launch; 12288 = 64 * 192: the 64-lane
# instance; 524288: RPO_EVAL_LANE_STEPS / n = 8 < the horizon of 32, so the trace spans four launches (t0 = 0, 8, 16, 24) -- the
# policies' episodes are short (cart ~11 steps), so only a launch this short is continued by live recorded lanes
@pytest.mark.parametrize("episodes,record,horizon", [(1000, True, None), (12288, 64, None), (524288, 64, 32)])
@pytest.mark.parametrize("algo,envname", COMBOS)
def test_fused_trace_equals_stepwise_trace_bit_for_bit(hip, algo, envname, episodes, record, horizon):
    tr = _trained(hip, algo, envname)
    a, b = _both(tr, episodes=episodes, seed=11, record=record, horizon=horizon)
    per_launch = hip.EVAL_LANE_STEPS // episodes
    assert a.horizon == (horizon or 200) and (horizon is None or per_launch < a.horizon)
    assert a.trajectory.episodes == (episodes if record is True else record)
    assert_arrays_equal(a, tr.evaluate(episodes=episodes, seed=11, horizon=horizon))
    for f in ("ret", "length", "mean_ineq", "mean_eq", "max_ineq", "max_eq", "viol_steps", "proj_iters", "nonfinite"):
        np.testing.assert_array_equal(getattr(a, f), getattr(b, f), err_msg=f)
    _traces_equal(a, b)
    assert a.trajectory.valid.sum() == a.length[:a.trajectory.episodes].sum() > 0
    assert_replay(a)
    if horizon is not None:
        assert a.length[:64].max() > per_launch              # (recorded episodes ran on into a later launch)


@pytest.mark.parametrize("algo,envname", COMBOS)
def test_fused_record_arrays_equal_replay_and_dynamics(hip, algo, envname):
    tr = _trained(hip, algo, envname)
    plain = tr.evaluate(episodes=1000, seed=7)
    r = tr.evaluate(episodes=1000, seed=7, record=True)
    assert r.path == "fused" and plain.trajectory is None
    assert_arrays_equal(r, plain)
    tj = r.trajectory
    assert tj.obs.shape == (1000, 200, tr.kernels.obs_dim) and tj.proposal.shape == (1000, 200, 1)
    assert tj.action.shape == (1000, 200, 2)
    np.testing.assert_array_equal(tj.length, r.length)
    assert_zero_outside_valid(tj)
    assert_replay(r)
    assert_dynamics(r, envname, CART_TOL if envname == "cart" else PEND_TOL)
    assert len(tj.violations()) == r.viol_steps.sum()
    assert tj.iters.sum() == r.proj_iters.sum() > 0


def test_fused_record_with_injected_initial_states(hip, golden):
    """The reference-trained, bias-shifted pendulum actor (violations behind the projection) from injected initial states:
    the recorded observation is the one the actor read (torch's cos / sin of the injected angle at step 0)."""
    g = golden("eval_ddpg_pendulum_sat")
    torch.manual_seed(1)
    tr = build_trainer("ddpg", "pendulum", hip, DEV, num_envs=1, use_graph=False)
    tr.agent.actor.load_state_dict({k[len("actor."):]: torch.tensor(g[k]) for k in g.files if k.startswith("actor.")})
    init = torch.tensor(g["init"], dtype=torch.float32, device=DEV)
    a, b = _both(tr, episodes=10, init_states=init, record=True)
    _traces_equal(a, b)
    assert_replay(a)
    assert_dynamics(a, "pendulum", PEND_TOL)
    v = a.trajectory.violations()
    assert len(v) == a.viol_steps.sum() > 0


@pytest.mark.parametrize("algo,envname", [("ddpg", "evopf256"), ("ddpgla", "cart")])
def test_stepwise_only_configurations_record(hip, algo, envname):
    torch.manual_seed(5)
    la = algo.endswith("la")
    tr = build_trainer(algo, envname, hip, DEV, num_envs=16, use_graph=False, fused=not la)
    k = tr.kernels
    plain = tr.evaluate(10, seed=4)
    r = tr.evaluate(10, seed=4, record=True)
    assert r.path == "stepwise"
    assert_arrays_equal(r, plain)
    tj = r.trajectory
    H = r.horizon
    P = k.action_dim if la else k.partial_dim
    assert tj.obs.shape == (10, H, k.obs_dim) and tj.proposal.shape == (10, H, P) and tj.action.shape == (10, H, k.action_dim)
    assert tj.reward.shape == tj.done.shape == tj.ineq.shape == tj.eq.shape == tj.iters.shape == tj.valid.shape == (10, H)
    assert_zero_outside_valid(tj)
    assert_replay(r)
    assert len(tj.violations()) == r.viol_steps.sum()
    if la:
        np.testing.assert_array_equal(tj.proposal, tj.action)
        assert not tj.iters.any()
    part = tr.evaluate(10, seed=4, record=3)
    for name in tj.ARRAYS:
        np.testing.assert_array_equal(getattr(part.trajectory, name), getattr(tj, name)[:3], err_msg=name)


def test_recording_has_no_side_effects_on_the_device(hip, monkeypatch):
    """test_no_side_effects_on_the_device with recording on: training after evaluate(record=True) is the training without."""
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
    r = b.evaluate(4096, record=True)
    assert r.path == "fused" and r.trajectory.episodes == 4096
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


def test_trace_arguments_are_validated(hip):
    """The wrappers refuse a trace of another width or with more rows than lanes; the entry points a short or misaligned one."""
    tr = _trained(hip, "ddpg", "cart")
    v = tr.base_env.make_vec(32, seed=1, max_episode_steps=tr.max_episode_steps, device=DEV, stats_cap=2)
    v.reset()
    acc = torch.zeros(32, 8, device=DEV)
    scale, base = tr._box_affine

    def run(trace, steps=4):
        tr.kernels.evaluate(tr.fused.descs["actor"], tr._gauss_policy, scale, base, v.internal, None, v.action, v.ep_len, v.ep_ret,
                            v.ep_count, v.ctrl, acc, 0, steps, tr._box_lo, tr._box_hi, tr.eval_steps, tr.eval_lr, tr.corr_eps,
                            tr.corr_momentum, v.max_episode_steps, v.viol_thresh, trace=trace)
    for shape in ((4, 32, 12), (4, 33, 16), (4, 0, 16)):
        with pytest.raises(hip.RpoHipError):
            run(torch.zeros(*shape, device=DEV))
    with pytest.raises(hip.RpoHipError, match="invalid argument"):
        run(torch.zeros(3, 32, 16, device=DEV))                # steps [0, 4) do not fit 3 trace steps
    with pytest.raises(hip.RpoHipError, match="invalid argument"):
        run(torch.zeros(4 * 32 * 16 + 4, device=DEV)[1:-3].view(4, 32, 16))      # 4-byte aligned only
    run(torch.zeros(4, 32, 16, device=DEV))
    torch.cuda.synchronize()


def test_abi_exports_the_record_entry_points(hip):
    from rpo_amd import _lib
    new = {"rpo_cartsafe_evaluate_record", "rpo_pendulum_evaluate_record", "rpo_eval_record"}
    assert new <= set(_lib.PROTOTYPES)
    syms = subprocess.run(["nm", "-D", "--defined-only", _lib.LIBRARY], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in syms.splitlines() if " T " in line}
    assert new <= exported and exported == set(_lib.PROTOTYPES)
    assert _lib.CONST["RPO_ABI_VERSION"] == 6 == _lib.load().rpo_abi_version()
    assert hip.trace_layout(6, 1, 2) == (12, 16) and hip.trace_layout(5, 1, 2) == (12, 16)
