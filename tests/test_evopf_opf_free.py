"""The single-step AC-OPF of EVOPF-v0 with the battery power free, without a GPU: the float64 yardstick
(tests/evopf_opf_free_f64.py) against central differences, against scipy's SLSQP answers in tests/golden/evopf_opf_free.npz and
against the fixed-pe yardstick (tests/evopf_opf_f64.py); the public surface (``EVOPFEnv.opf(pe="free")``, ``OpfResult.objective``,
``reward_fn``, ``opf_gap(pe="free")``, ``trainer.evaluate_opf``) over stand-ins for the backend functions; the C-ABI entry point
``rpo_evopf_opf_free`` and its refusals.  The kernel itself: tests/test_evopf_opf_free_gpu.py."""
import ctypes
import functools
import inspect
import os
import types

import numpy as np
import pytest
import torch

import evopf_opf_f64 as opf64
import evopf_opf_free_f64 as free64
import oracle_backend as ob
from oracle import evopf as ev
from rpo_amd import _lib, ops
from rpo_amd.algo import EvalTrajectory, OpfGap, opf_gap
from rpo_amd.algo.evaluation import evaluate_opf
from rpo_amd.env.electrical_grid.evopf import EVOPFEnv, OpfResult
from test_evopf_opf import AMBIG_CAP, FakeOpf, states, trajectory
from test_train_step_golden import build_trainer

ARG, NULL = _lib.CONST["RPO_ERR_ARG"], _lib.CONST["RPO_ERR_NULL"]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "evopf_opf_free.npz")
TOL = 1e-4


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def classes(z):
    """(feasible, infeasible, left out) masks from SLSQP's final equality residual, and the cap on the third
    (test_evopf_opf.classes on this fixture)."""
    eq = z["slsqp_eq_resid"]
    feas, infeas = eq < 1e-6, eq > 1e-3
    other = ~(feas | infeas)
    assert other.mean() <= AMBIG_CAP, "left out: %d of %d" % (other.sum(), len(eq))
    return feas, infeas, other


@functools.lru_cache(maxsize=None)
def helper_on_feasible():
    z = golden()
    feas, _, _ = classes(z)
    return feas, free64.solve_free_many(z["obs"][feas], tol=TOL, max_iters=25)


# ------------------------------------------------------------------------------------------------ the yardstick
def test_battery_columns_have_the_sign_of_eq_resid():
    """``jac_free`` against central differences of ``eq_resid`` in every column of x, the battery columns above all: +1 in the
    real-power equation of bus spv[j], where ``eq_jac`` itself has the reference's -1."""
    rng = np.random.default_rng(0)
    for _ in range(3):
        a = np.zeros(43)
        a[:10] = rng.uniform(-0.2, 0.8, 10)
        a[ev.GRID.vm0:ev.GRID.va0] = rng.uniform(0.94, 1.06, 14)
        a[ev.GRID.va0:ev.GRID.pe0] = rng.uniform(-0.3, 0.3, 14)
        a[ev.GRID.pe0:] = rng.uniform(-0.18, 0.2, 5)
        s = rng.uniform(0.0, 0.5, size=(1, 57))
        J = free64.jac_free(a)
        fd = np.zeros_like(J)
        for c, j in enumerate(free64.XIDX):
            e = np.zeros(43)
            e[j] = 1e-6
            fd[:, c] = (ev.eq_resid(s, (a + e)[None])[0] - ev.eq_resid(s, (a - e)[None])[0]) / 2e-6
        assert np.abs(J - fd).max() <= 1e-7 * max(1.0, np.abs(J).max())
        pe_cols = J[:, -5:]
        assert np.array_equal(pe_cols[np.asarray(ev.GRID.spv), np.arange(5)], np.ones(5)) and pe_cols.sum() == 5.0
        assert np.array_equal(ev.eq_jac(a[None])[0][:, ev.GRID.pe0:], -pe_cols)          # hazard E1: the literal sign, untouched


def test_fixture_holds_the_stated_observations():
    z = golden()
    obs = free64.fixture_obs()
    demand, _ = opf64.fixture_states()
    assert z["obs"].shape == (384, 57) and np.array_equal(z["obs"], obs) and np.array_equal(obs[:, :28], demand)
    assert np.array_equal(obs[24, 33:], ev.episode_price(11, np.array([0]), 1, 0)[0])
    soc = obs[:, 28:33]
    init = (soc == ev.B_INIT).all(axis=1)
    ends = np.isin(soc, [ev.B_LOW, ev.B_HIGH]).all(axis=1)
    assert init.sum() == 96 and ends.sum() == 96 and (~init & ~ends).sum() == 192
    assert soc.min() >= ev.B_LOW and soc.max() <= ev.B_HIGH
    assert os.path.getsize(GOLDEN) < 512 * 1024


def test_helper_against_slsqp_on_all_states():
    z = golden()
    feas, infeas, other = classes(z)
    print("feasible %d, infeasible %d, left out %d" % (feas.sum(), infeas.sum(), other.sum()))
    _, r = helper_on_feasible()
    assert r["converged"].all() and r["iters"].max() <= 25
    infeasibility = free64.infeasibility(z["obs"][feas], r["action"])
    dev = r["objective"] - z["slsqp_objective"][feas]
    pe = r["action"][:, 38:]
    hi, lo = ev.battery_bounds(z["obs"][feas][:, 28:33])
    at_bound = (np.minimum(hi - pe, pe - lo) <= 1e-3).mean()
    print("iterations %d..%d, infeasibility <= %.3g, objective - SLSQP in [%.3g, %.3g], pe at a bound: %.3f"
          % (r["iters"].min(), r["iters"].max(), infeasibility.max(), dev.min(), dev.max(), at_bound))
    assert infeasibility.max() <= TOL
    assert np.abs(dev).max() <= 1e-4
    assert np.allclose(r["objective"], free64.objective(z["obs"][feas], r["action"]), rtol=0, atol=1e-12)
    bad = free64.solve_free_many(z["obs"][infeas], tol=TOL, max_iters=80)
    assert infeas.sum() == 5 and not bad["converged"].any() and (bad["iters"] == 80).all()


def test_helper_against_the_fixed_pe_yardstick():
    z = golden()
    feas, r = helper_on_feasible()
    pick = np.arange(0, feas.sum(), 6)                            # 64 of the feasible observations
    obs = z["obs"][feas][pick]
    worst_fixed, worst_zero, compared = 0.0, -np.inf, 0
    for k, row in enumerate(pick):
        fixed = opf64.solve(obs[k, :28], pe=r["action"][row, 38:], tol=TOL, max_iters=40)
        assert fixed["converged"]
        worst_fixed = max(worst_fixed, abs(fixed["cost"] - r["cost"][row]))
        hi, lo = ev.battery_bounds(obs[k, 28:33])
        zero = opf64.solve(obs[k, :28], pe=None, tol=TOL, max_iters=40)
        if zero["converged"] and (lo <= 0).all() and (hi >= 0).all():
            worst_zero = max(worst_zero, r["objective"][row] - zero["cost"])
            compared += 1
    print("|fixed-pe cost at pe* - free cost| <= %.3g; free objective - objective at pe = 0 <= %.3g on %d states"
          % (worst_fixed, worst_zero, compared))
    assert worst_fixed <= 1e-4
    assert compared >= 60 and worst_zero <= 1e-4


def test_helper_without_iterations_is_the_flat_start():
    obs = golden()["obs"][50]
    r = free64.solve_free(obs, max_iters=0)
    hi, lo = ev.battery_bounds(obs[28:33])
    assert not r["converged"] and r["iters"] == 0 and np.array_equal(r["action"], free64.flat_start(obs))
    assert np.array_equal(r["action"][38:], 0.5 * (hi + lo)) and np.array_equal(r["action"][:38], opf64.flat_start(0.0)[:38])


# ------------------------------------------------------------------------------------------------ surface over a stand-in
class FakeOpfFree(object):
    """Stands in for ``ops.evopf_opf_free`` on CPU tensors: cost = 1 + pd[0], converged iff qd[0] >= 0, action = (pd[:5] in pg, pe
    = -0.01 * the pe_cost it used, zeros elsewhere), 7 iterations, residual 5e-5 -- and keeps what it was called with."""

    def __init__(self):
        self.calls = []

    def __call__(self, kernels, obs, pe_cost, action, info, tol, max_iters):
        self.calls.append(dict(obs=obs.clone(), pe_cost=None if pe_cost is None else pe_cost.clone(), tol=tol, max_iters=max_iters,
                               action=action, info=info))
        used = (5.0 * obs[:, 33:34]).expand(-1, 5) if pe_cost is None else pe_cost
        action.zero_()
        action[:, :5] = obs[:, :5]
        action[:, 38:] = -0.01 * used
        info[:, 0] = 1.0 + obs[:, 0]
        info[:, 1] = 5e-5
        info[:, 2] = 7.0
        info[:, 3] = (obs[:, 14] >= 0).float()


@pytest.fixture
def fake_env(monkeypatch):
    env = EVOPFEnv(backend=ob, device="cpu")
    fixed, fake = FakeOpf(), FakeOpfFree()
    monkeypatch.setattr(env, "_opf_kernel", lambda: fixed, raising=True)
    monkeypatch.setattr(env, "_opf_free_kernel", lambda: fake, raising=True)
    return env, fake, fixed


def test_opf_free_result_objective_and_pe_cost(fake_env):
    env, fake, fixed = fake_env
    s = states(5)
    a = env.opf(s, pe="free")
    assert isinstance(a, OpfResult) and len(fake.calls) == 1 and not fixed.calls and fake.calls[0]["pe_cost"] is None
    assert (fake.calls[0]["tol"], fake.calls[0]["max_iters"]) == (1e-4, 40) and fake.calls[0]["obs"].shape == (5, 57)
    want = np.repeat(np.float32(5.0) * s[:, 33:34], 5, axis=1)
    assert a.pe_cost.shape == (5, 5) and np.array_equal(a.pe_cost.numpy(), want) and a.pe_cost.is_contiguous()
    assert torch.equal(a.objective, a.cost + (a.pe_cost * a.action[:, 38:]).sum(1)) and not torch.equal(a.objective, a.cost)
    host = a.numpy()
    assert set(host) == {"action", "cost", "residual", "iters", "converged", "pe_cost", "objective"}
    assert np.array_equal(host["pe_cost"], want) and np.array_equal(host["objective"], a.objective.numpy())
    assert a.converged.tolist() == [False, True, True, False, True] and a.iters.tolist() == [7] * 5
    # pe_cost: a number, [5], [n, 5]
    for given, full in ((0.25, np.full((5, 5), 0.25, np.float32)), (np.arange(5.0), np.tile(np.arange(5.0, dtype=np.float32), (5, 1))),
                        (s[:, 40:45], s[:, 40:45])):
        b = env.opf(s, pe="free", pe_cost=given, tol=1e-3, max_iters=9)
        assert np.array_equal(fake.calls[-1]["pe_cost"].numpy(), full) and fake.calls[-1]["pe_cost"].is_contiguous()
        assert np.array_equal(b.pe_cost.numpy(), full) and (fake.calls[-1]["tol"], fake.calls[-1]["max_iters"]) == (1e-3, 9)
        assert np.allclose(b.objective.numpy(), b.cost.numpy() + (full * b.action.numpy()[:, 38:]).sum(1))
    one = env.opf(s[0], pe="free")
    assert one.action.shape == (1, 43) and one.pe_cost.shape == (1, 5)
    # fixed-pe results: pe_cost None, objective is cost, numpy() as it was
    f = env.opf(s, pe=np.full((5, 5), 0.1, np.float32))
    assert f.pe_cost is None and f.objective is not None and torch.equal(f.objective, f.cost)
    assert set(f.numpy()) == {"action", "cost", "residual", "iters", "converged"} and len(fixed.calls) == 1


def test_opf_free_argument_checks_and_out_reuse(fake_env):
    env, fake, fixed = fake_env
    s = states(4)
    with pytest.raises(ValueError, match="state of charge"):
        env.opf(s[:, :28], pe="free")                             # demands alone carry no soc and no price
    for kw in (dict(pe="Free"), dict(pe="zero"), dict(pe="free", state_in=torch.zeros(4, 168)),
               dict(pe="free", state_out=torch.zeros(4, 168)), dict(pe="free", tol=0.0), dict(pe="free", max_iters=-1),
               dict(pe="free", pe_cost=np.zeros(4)), dict(pe="free", pe_cost=np.zeros((3, 5))), dict(pe="free", pe_cost=np.zeros((4, 4))),
               dict(pe=None, pe_cost=1.0), dict(pe=np.zeros((4, 5), np.float32), pe_cost=1.0)):
        with pytest.raises(ValueError):
            env.opf(s, **kw)
    assert not fake.calls and not fixed.calls
    first = env.opf(s, pe="free")
    again = env.opf(states(4, seed=1), pe="free", pe_cost=2.0, out=first)
    assert again is first and fake.calls[-1]["action"] is first.action and fake.calls[-1]["info"] is first.info
    assert np.array_equal(first.pe_cost.numpy(), np.full((4, 5), 2.0, np.float32))
    back = env.opf(s, out=first)                                  # the same buffers for a fixed-pe call: pe_cost is reset
    assert back is first and first.pe_cost is None and torch.equal(first.objective, first.cost)
    with pytest.raises(ValueError):
        env.opf(s, pe="free", out=env.opf(states(3), pe="free"))


def test_reward_fn_is_the_step_reward():
    env = EVOPFEnv(backend=ob, device="cpu")
    rng = np.random.default_rng(3)
    n = 6
    state = ev.reset(11, np.arange(n), 0)
    action = rng.uniform(0.0, 0.5, size=(n, 43))
    action[:, 38:] = rng.uniform(-0.18, 0.2, size=(n, 5))
    want = ev.step(state, action, np.zeros(n, np.int64), np.zeros(n, np.int64), 11, np.arange(n), auto_reset=False)["reward"]
    got = env.reward_fn(state, action)
    assert isinstance(got, np.ndarray) and got.shape == (n,) and np.allclose(got, want, rtol=1e-12, atol=1e-12)
    t = env.reward_fn(torch.tensor(state, dtype=torch.float32), torch.tensor(action, dtype=torch.float32))
    assert isinstance(t, torch.Tensor) and t.shape == (n,) and np.allclose(t.numpy(), want, rtol=1e-5, atol=1e-5)
    assert env.reward_fn(state[0], action[0]).shape == (1,)
    # an objective in reward units: reward = -wg * (obj_fn + (we / wg) price sum(pe))
    assert np.allclose(got, -env.wg * free64.objective(state, action), rtol=1e-12, atol=1e-12)


def test_opf_gap_free_places_nans_and_round_trips(fake_env, tmp_path):
    env, fake, fixed = fake_env
    tj = trajectory()
    gap = tj.opf_gap(env, tol=1e-3, max_iters=30, pe="free")
    assert isinstance(gap, OpfGap) and len(fake.calls) == 1 and not fixed.calls and fake.calls[0]["obs"].shape == (6, 57)
    assert (fake.calls[0]["tol"], fake.calls[0]["max_iters"]) == (1e-3, 30) and fake.calls[0]["pe_cost"] is None
    conv = tj.valid & (tj.obs[:, :, 14] >= 0)
    assert np.array_equal(gap.converged, conv) and np.array_equal(gap.valid, tj.valid)
    assert np.array_equal(np.isnan(gap.cost_policy), ~tj.valid)
    assert np.array_equal(np.isnan(gap.cost_opt), ~conv) and np.array_equal(np.isnan(gap.gap), ~conv)
    o, a = tj.obs[tj.valid].astype(np.float64), tj.action[tj.valid].astype(np.float64)
    assert np.allclose(gap.cost_policy[tj.valid], free64.objective(o, a), rtol=1e-5)
    price = tj.obs[:, :, 33].astype(np.float64)
    opt = 1.0 + tj.obs[:, :, 0] + 5 * (5.0 * price) * (-0.01 * 5.0 * price)      # the stand-in's cost + pe_cost . pe
    assert np.allclose(gap.cost_opt[conv], opt[conv], rtol=1e-5)
    assert np.array_equal(gap.gap[conv], gap.cost_policy[conv] - gap.cost_opt[conv])          # the difference, not a ratio
    path = str(tmp_path / "gap.npz")
    gap.save(path)
    back = OpfGap.load(path)
    for name in OpfGap.ARRAYS:
        assert np.array_equal(getattr(back, name), getattr(gap, name), equal_nan=True), name
    assert np.array_equal(opf_gap(tj, env, tol=1e-3, max_iters=30, pe="free").gap, gap.gap, equal_nan=True)
    # the default stays the policy's pe on both sides
    tj.opf_gap(env)
    assert len(fixed.calls) == 1 and np.array_equal(fixed.calls[0]["pe"].numpy(), tj.action[tj.valid][:, 38:])
    assert list(inspect.signature(opf_gap).parameters)[-1] == "pe" and inspect.signature(opf_gap).parameters["pe"].default == "policy"
    with pytest.raises(ValueError):
        tj.opf_gap(env, pe="zero")


def test_not_implemented_with_a_reason_without_the_kernel():
    env = EVOPFEnv(backend=ob, device="cpu")
    s = states(2)
    for call in (lambda: env.opf(s, pe="free"), lambda: trajectory().opf_gap(env, pe="free")):
        with pytest.raises(NotImplementedError, match="evopf_opf"):
            call()
    hip_on_cpu = EVOPFEnv(device="cpu")
    with pytest.raises(NotImplementedError, match="GPU"):
        hip_on_cpu.opf(s, pe="free")
    for e in (env, hip_on_cpu):                                   # evaluate_opf: the same reasons, before anything is built
        tr = types.SimpleNamespace(base_env=e, kernels=types.SimpleNamespace(name="EVOPF-v0"))
        for pe in ("free", "zero"):
            with pytest.raises(NotImplementedError, match="evopf_opf" if e is env else "GPU"):
                evaluate_opf(tr, pe=pe)
    cart = types.SimpleNamespace(base_env=object(), kernels=types.SimpleNamespace(name="CartSafe-v0"))
    with pytest.raises(NotImplementedError, match="EVOPF-v0"):
        evaluate_opf(cart)


@functools.lru_cache(maxsize=None)
def _cpu_evopf_trainer():
    torch.manual_seed(4)
    tr = build_trainer("ddpg", "evopf", ob, torch.device("cpu"), fused=False, num_envs=2, use_graph=False, capacity=32)
    tr.vec.reset()
    return tr


def test_evaluate_opf_refusals(monkeypatch):
    tr = _cpu_evopf_trainer()
    assert callable(tr.evaluate_opf)
    sig = inspect.signature(tr.evaluate_opf).parameters
    assert list(sig) == ["episodes", "seed", "horizon", "init_states", "record", "constraints", "pe", "pe_cost", "tol", "max_iters"]
    assert (sig["pe"].default, sig["tol"].default, sig["max_iters"].default, sig["episodes"].default) == ("free", 1e-4, 40, 10)
    with pytest.raises(NotImplementedError, match="evopf_opf"):   # the oracle backend has no solver
        tr.evaluate_opf(2)
    for kw in (dict(pe="policy"), dict(pe=None), dict(pe="zero", pe_cost=1.0)):
        with pytest.raises(ValueError):
            tr.evaluate_opf(2, **kw)
    fake = FakeOpfFree()
    monkeypatch.setattr(tr.base_env, "_opf_free_kernel", lambda: fake, raising=True)
    for kw in (dict(tol=0.0), dict(max_iters=-1), dict(max_iters=1.5), dict(episodes=0), dict(horizon=0), dict(record=5),
               dict(constraints=1), dict(pe_cost=np.zeros(3)), dict(pe_cost=np.zeros((3, 5))), dict(init_states=np.zeros((2, 3)))):
        with pytest.raises(ValueError):
            tr.evaluate_opf(**dict(dict(episodes=2), **kw))
    assert not fake.calls


def test_evaluate_opf_runs_the_stepwise_loop_with_the_solver_as_the_policy(monkeypatch):
    tr = _cpu_evopf_trainer()
    before = tr.evaluate(2, horizon=2, seed=3)
    fake = FakeOpfFree()
    monkeypatch.setattr(tr.base_env, "_opf_free_kernel", lambda: fake, raising=True)
    H = 3
    res = tr.evaluate_opf(3, seed=7, horizon=H, record=True, constraints=True, pe_cost=0.5, tol=1e-3, max_iters=11)
    assert res.path == "opf" and res.seed == 7 and res.horizon == H and res.episodes == 3 and len(fake.calls) == H
    assert all(c["obs"].shape == (3, 57) and (c["tol"], c["max_iters"]) == (1e-3, 11) for c in fake.calls)
    assert all(np.array_equal(c["pe_cost"].numpy(), np.full((3, 5), 0.5, np.float32)) for c in fake.calls)
    assert (res.length == H).all() and res.opf_iters.shape == (3, H) and res.opf_iters.dtype == np.int32
    assert (res.opf_iters == 7).all() and (res.proj_iters == 7 * H).all()
    tj = res.trajectory
    # step 0 is the reset observation of evaluate()'s episodes under the same seed: the same day, the same initial soc
    assert np.array_equal(tj.obs[:, 0], ev.reset(7, np.arange(3), 0).astype(np.float32))
    assert np.array_equal(res.opf_converged, tj.obs[:, :, 14] >= 0)
    assert np.array_equal(tj.obs[:, 1], fake.calls[1]["obs"].numpy())           # the solver read the env's own observation rows
    assert np.array_equal(tj.action[:, :, 38:], np.full((3, H, 5), -0.005, np.float32))
    assert np.array_equal(tj.proposal, tj.action[:, :, tr.base_env.partial_actions]) and (tj.iters == 7).all()
    reward = tr.base_env.reward_fn(tj.obs.reshape(-1, 57).astype(np.float64), tj.action.reshape(-1, 43).astype(np.float64))
    assert np.allclose(tj.reward.reshape(-1), reward, rtol=1e-5, atol=1e-5)
    assert np.allclose(res.ret, tj.reward.sum(axis=1), rtol=1e-5) and res.constraints is not None
    again = tr.evaluate_opf(3, seed=7, horizon=H, pe_cost=0.5)
    assert np.array_equal(again.ret, res.ret) and again.trajectory is None and again.constraints is None
    # a policy's evaluation carries no solver fields, and is what it was before the controller ran
    after = tr.evaluate(2, horizon=2, seed=3)
    assert after.opf_iters is None and after.opf_converged is None and after.path == "stepwise"
    for f in before.FIELDS:
        assert np.array_equal(getattr(before, f), getattr(after, f)), f
    # the idle-battery dispatch goes to the fixed-pe function with pe = None
    fixed = FakeOpf()
    monkeypatch.setattr(tr.base_env, "_opf_kernel", lambda: fixed, raising=True)
    zero = tr.evaluate_opf(2, seed=7, horizon=2, pe="zero", record=1)
    assert len(fixed.calls) == 2 and all(c["pe"] is None and c["width"] == 57 for c in fixed.calls)
    assert (zero.trajectory.action[:, :, 38:] == 0).all() and zero.trajectory.episodes == 1


# ------------------------------------------------------------------------------------------------ binding and C ABI
def test_binding_is_a_backend_function():
    assert callable(ops.evopf_opf_free) and not hasattr(ops.EvopfKernels, "evopf_opf_free") and not hasattr(ob, "evopf_opf_free")
    assert list(inspect.signature(ops.evopf_opf_free).parameters) == ["kernels", "obs", "pe_cost", "action", "info", "tol", "max_iters"]
    env = EVOPFEnv(device="cpu")
    with pytest.raises(_lib.RpoHipError):                        # CPU tensors are refused like by every other op
        ops.evopf_opf_free(env.kernels, torch.zeros(2, 57), None, torch.zeros(2, 43), torch.zeros(2, 4), 1e-4, 40)
    for kw in (dict(obs=torch.zeros(3, 57)), dict(obs=torch.zeros(2, 56)), dict(obs=torch.zeros(2, 28)), dict(action=torch.zeros(2, 42)),
               dict(info=torch.zeros(2, 3)), dict(pe_cost=torch.zeros(2, 4)), dict(pe_cost=torch.zeros(3, 5)),
               dict(obs=torch.zeros(2, 114)[:, ::2])):
        args = dict(dict(obs=torch.zeros(2, 57), pe_cost=None, action=torch.zeros(2, 43), info=torch.zeros(2, 4)), **kw)
        with pytest.raises(_lib.RpoHipError, match="evopf_opf_free"):
            ops.evopf_opf_free(env.kernels, args["obs"], args["pe_cost"], args["action"], args["info"], 1e-4, 40)


def test_entry_point_is_declared_exported_and_refuses_before_any_launch():
    V, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert _lib.PROTOTYPES["rpo_evopf_opf_free"] == [I, V, I, V, V, V, F, I, V, V]
    assert _lib.PROTOTYPES["rpo_evopf_opf"] == [I, V, I, V, V, V, F, I, V, V]          # the existing entry points keep their signatures
    assert _lib.PROTOTYPES["rpo_evopf_opf_state"] == [I, V, I, V, V, V, F, I, V, V, V, V]
    assert _lib.CONST["RPO_ABI_VERSION"] == 6                                          # an added entry point: no new ABI version
    lib = _lib.load()
    assert hasattr(lib, "rpo_evopf_opf_free")
    good = dict(n=4, obs=None, obs_stride=57, pe_cost=None, action_out=None, info_out=None, tol=1e-4, max_iters=40, consts_dev=None,
                stream=None)

    def call(**kw):
        return lib.rpo_evopf_opf_free(*dict(good, **kw).values())
    # sizes before pointers: these answer without looking at a pointer
    for kw in (dict(n=0), dict(n=-2), dict(max_iters=-1), dict(tol=0.0), dict(tol=-1e-4), dict(tol=float("nan")), dict(obs_stride=56),
               dict(obs_stride=28), dict(obs_stride=0)):
        assert call(**kw) == ARG, kw
    assert call() == NULL and call(max_iters=0) == NULL
    if torch.cuda.device_count() == 0:
        # host addresses stand in for device pointers (a refusal dereferences nothing): never where a GPU is visible.  A call
        # that got as far as a launch would answer a HIP error code here, neither RPO_ERR_ARG nor RPO_ERR_NULL.
        buf = (ctypes.c_float * 1024)()
        r = ctypes.c_void_p(ctypes.addressof(buf))
        full = dict(obs=r, pe_cost=r, action_out=r, info_out=r, consts_dev=r)
        for name in ("obs", "action_out", "info_out", "consts_dev"):
            assert call(**dict(full, **{name: None})) == NULL, name
        assert call(**dict(full, n=0)) == ARG and call(**dict(full, obs_stride=56)) == ARG
        assert call(**dict(full, pe_cost=None)) not in (0, ARG, NULL)     # pe_cost may be NULL: this one reaches the launch, and fails there
