"""The safety filter of EVOPF-v0 without a GPU: the float64 yardstick (tests/evopf_nearest_f64.py) on the 70 fixture rows and the
three families of targets of tests/golden/evopf_nearest.npz, against scipy's SLSQP answers stored there; the public surface
(``EVOPFEnv.nearest_feasible``, ``NearestResult``, ``trainer.evaluate_filtered``) over a stand-in for the backend function; the
C-ABI entry point ``rpo_evopf_nearest`` and its refusals.  The kernel itself: tests/test_evopf_nearest_gpu.py.

Conditions of the yardstick (fixed by the issue, measured here in brackets): on every family the helper converges on the 65 feasible
rows and on none of the 5 infeasible ones, in 8..10 iterations [8..10]; its objective is within 1e-4 of SLSQP's [3.8e-5, never
below it]; on the already feasible targets the distance is <= 1e-4 [2.8e-5]."""
import ctypes
import functools
import inspect
import os
import types

import numpy as np
import pytest
import torch

import evopf_nearest_f64 as near64
import evopf_opf_free_f64 as free64
import oracle_backend as ob
from oracle import evopf as ev
from rpo_amd import _lib, ops
from rpo_amd.algo import ActResult, evaluate_filtered
from rpo_amd.env.electrical_grid.evopf import EVOPFEnv, NearestResult
from test_evopf_opf import states
from test_train_step_golden import build_trainer

ARG, NULL = _lib.CONST["RPO_ERR_ARG"], _lib.CONST["RPO_ERR_NULL"]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "evopf_nearest.npz")
TOL = 1e-4
PARTIAL = np.asarray(ev.GRID.partial_actions)


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def helper(family):
    """The helper's results on the 70 rows for one family of targets -- computed once, shared and left unchanged."""
    z = golden()
    return near64.solve_nearest_many(z["obs"].astype(np.float64), z["target_" + family], tol=TOL, max_iters=40)


FEASIBLE = np.arange(70) < 65                                   # fixture_rows(): the 5 infeasible observations stand last


# ------------------------------------------------------------------------------------------------ the yardstick
def test_fixture_holds_the_stated_rows_and_targets():
    z = golden()
    rows, obs = free64.fixture_rows()
    assert np.array_equal(z["rows"], rows) and np.array_equal(z["obs"], obs) and z["obs"].dtype == np.float32
    o64 = obs.astype(np.float64)
    with np.load(os.path.join(os.path.dirname(GOLDEN), "evopf_opf_free.npz")) as f:
        point = f["slsqp_point"][rows]
    assert np.array_equal(z["target_uniform"], near64.target_uniform(o64))
    assert np.array_equal(z["target_near"], near64.target_near(o64, point))
    assert np.allclose(z["target_feasible"][FEASIBLE], helper("uniform")["action"][FEASIBLE][:, PARTIAL], rtol=0, atol=1e-9)
    assert np.array_equal(z["target_feasible"][~FEASIBLE], z["target_uniform"][~FEASIBLE]) and all(np.isfinite(z["target_" + f]).all() for f in near64.FAMILIES)
    hi, lo = (np.stack(x) for x in zip(*(free64.box(o) for o in o64)))
    t = z["target_uniform"]
    assert (t >= lo[:, near64.PB]).all() and (t <= hi[:, near64.PB]).all()
    for fam in near64.FAMILIES:                                  # SLSQP's classes are the fixture's: 65 feasible, 5 not
        eq = z["slsqp_eq_resid_" + fam]
        assert (eq[FEASIBLE] < 1e-6).all() and (eq[~FEASIBLE] > 1e-3).all()
    assert list(PARTIAL) == [1, 2, 3, 4, 10, 11, 12, 15, 17, 38, 39, 40, 41, 42] and os.path.getsize(GOLDEN) < 256 * 1024


@pytest.mark.parametrize("family", near64.FAMILIES)
def test_helper_converges_where_the_problem_is_feasible(family):
    r = helper(family)
    conv = r["converged"]
    print("%s: converged %d of 65 feasible and %d of 5 infeasible rows, iterations %d..%d"
          % (family, conv[FEASIBLE].sum(), conv[~FEASIBLE].sum(), r["iters"][conv].min(), r["iters"][conv].max()))
    assert conv[FEASIBLE].all() and not conv[~FEASIBLE].any()
    assert r["iters"][FEASIBLE].min() >= 8 and r["iters"][FEASIBLE].max() <= 10 and (r["iters"][~FEASIBLE] == 40).all()
    z = golden()
    assert free64.infeasibility(z["obs"][FEASIBLE], r["action"][FEASIBLE]).max() <= TOL
    assert (r["action"][:, ev.GRID.va0] == ev.GRID.slack_va[0]).all()
    w = np.stack([near64.default_weight(o) for o in z["obs"].astype(np.float64)])
    assert np.allclose(r["distance"][FEASIBLE], near64.distance(r["action"], z["target_" + family], w)[FEASIBLE], rtol=0, atol=1e-12)


@pytest.mark.parametrize("family", near64.FAMILIES)
def test_helper_against_slsqp(family):
    r = helper(family)
    dev = r["distance"][FEASIBLE] - golden()["slsqp_objective_" + family][FEASIBLE]
    print("%s: helper's objective - SLSQP's in [%.3g, %.3g]" % (family, dev.min(), dev.max()))
    assert np.abs(dev).max() <= 1e-4


def test_feasible_targets_stay_put():
    r = helper("feasible")
    z = golden()
    mv = near64.moved(z["obs"][FEASIBLE], r["action"][FEASIBLE], z["target_feasible"][FEASIBLE])
    print("feasible targets: distance <= %.3g, moved <= %.3g half-widths" % (r["distance"][FEASIBLE].max(), mv.max()))
    assert r["distance"][FEASIBLE].max() <= 1e-4


def test_helper_weights_and_the_flat_start():
    z = golden()
    obs, t = z["obs"][3].astype(np.float64), z["target_uniform"][3]
    base = near64.solve_nearest(obs, t)
    same = near64.solve_nearest(obs, t, weight=near64.default_weight(obs))
    assert np.array_equal(base["action"], same["action"]) and base["distance"] == same["distance"]
    w = near64.default_weight(obs)
    w[9:] *= 100.0                                               # the batteries a hundred times dearer: they move less
    heavy = near64.solve_nearest(obs, t, weight=w)
    mv = lambda r: near64.moved(obs[None], r["action"][None], t[None])[0, 9:].sum()     # noqa: E731
    assert heavy["converged"] and mv(heavy) < mv(base)
    flat = near64.solve_nearest(obs, t, max_iters=0)
    assert not flat["converged"] and flat["iters"] == 0 and np.array_equal(flat["action"], free64.flat_start(obs))
    s = near64.half_widths(obs)
    assert np.allclose(s[:4], 0.5 * (ev.GRID.pmax - ev.GRID.pmin)[1:]) and np.allclose(s[4:9], 0.5 * (ev.GRID.vmax - ev.GRID.vmin)[ev.GRID.spv])
    bad = near64.solve_nearest(obs, np.where(np.arange(14) == 2, np.nan, t))
    assert not bad["converged"] and bad["iters"] == 40          # a NaN in a stop quantity: not converged


# ------------------------------------------------------------------------------------------------ surface over a stand-in
class FakeNearest(object):
    """Stands in for ``ops.evopf_nearest`` on CPU tensors: the answer is the target with idle batteries (pe = 0), distance 0.25 (with
    a weight: its first entry), residual 5e-5, 7 iterations, converged on the even rows -- and keeps what it was called with."""

    def __init__(self):
        self.calls = []

    def __call__(self, kernels, obs, target, weight, action, info, tol, max_iters):
        self.calls.append(dict(obs=obs.clone(), target=target.clone(), weight=None if weight is None else weight.clone(), tol=tol,
                               max_iters=max_iters, action=action, info=info))
        action.copy_(target[:, :43])
        action[:, 38:] = 0.0
        info[:, 0] = 0.25 if weight is None else float(weight.reshape(-1)[0])
        info[:, 1] = 5e-5
        info[:, 2] = 7.0
        info[:, 3] = (torch.arange(obs.shape[0]) % 2 == 0).float()


@pytest.fixture
def fake_env(monkeypatch):
    env = EVOPFEnv(backend=ob, device="cpu")
    fake = FakeNearest()
    monkeypatch.setattr(env, "_nearest_kernel", lambda: fake, raising=True)
    return env, fake


def _actions(n, seed=1):
    return np.random.default_rng(seed).uniform(0.01, 0.1, size=(n, 43)).astype(np.float32)


def test_nearest_result_and_the_three_forms_of_the_action(fake_env):
    env, fake = fake_env
    s, a = states(5), _actions(5)
    r = env.nearest_feasible(s, a)
    assert isinstance(r, NearestResult) and len(fake.calls) == 1 and fake.calls[0]["weight"] is None
    assert (fake.calls[0]["tol"], fake.calls[0]["max_iters"]) == (1e-4, 40) and fake.calls[0]["obs"].shape == (5, 57)
    assert r.action.shape == (5, 43) and r.target.shape == (5, 14) and r.moved.shape == (5, 14)
    assert np.array_equal(r.target.numpy(), a[:, PARTIAL]) and np.array_equal(fake.calls[0]["target"].numpy()[:, PARTIAL], a[:, PARTIAL])
    assert r.converged.tolist() == [True, False, True, False, True] and r.iters.tolist() == [7] * 5 and r.iters.dtype == torch.int32
    assert torch.equal(r.distance, torch.full((5,), 0.25)) and torch.equal(r.residual, torch.full((5,), 5e-5))
    assert r.converged_rate() == pytest.approx(0.6) and "n=5" in repr(r)
    # moved: |y - t| / half-width of the variable's box -- the stand-in idles the batteries, nothing else moves
    p_max, p_min = ev.battery_bounds(s[:, 28:33].astype(np.float64))
    want = np.abs(a[:, 38:]) / (0.5 * (p_max - p_min))
    assert (r.moved[:, :9] == 0).all() and np.allclose(r.moved.numpy()[:, 9:], want, rtol=1e-5)
    host = r.numpy()
    assert set(host) == {"action", "distance", "residual", "iters", "converged", "target", "moved"}
    assert host["iters"].dtype == np.int32 and host["converged"].dtype == bool and np.array_equal(host["moved"], r.moved.numpy())
    # [n, 14] in partial_actions order, and an ActResult: the same 14 numbers reach the kernel
    b = env.nearest_feasible(s, a[:, PARTIAL])
    assert np.array_equal(fake.calls[-1]["target"].numpy()[:, PARTIAL], a[:, PARTIAL]) and fake.calls[-1]["target"].shape == (5, 43)
    assert torch.equal(b.target, r.target) and torch.equal(b.action[:, PARTIAL], r.action[:, PARTIAL])
    act = ActResult(torch.tensor(a), torch.zeros(5, 14), torch.zeros(5, dtype=torch.int32))
    c = env.nearest_feasible(torch.tensor(s), act, tol=1e-3, max_iters=9)
    assert torch.equal(c.action, r.action) and (fake.calls[-1]["tol"], fake.calls[-1]["max_iters"]) == (1e-3, 9)
    one = env.nearest_feasible(s[0], a[0])
    assert one.action.shape == (1, 43) and one.target.shape == (1, 14)
    # weights: [14] and [n, 14], float32 and contiguous at the kernel
    for w in (np.arange(1.0, 15.0), np.tile(np.arange(1.0, 15.0), (5, 1)), torch.full((14,), 2.0)):
        d = env.nearest_feasible(s, a, weight=w)
        got = fake.calls[-1]["weight"]
        assert got.dtype == torch.float32 and got.is_contiguous() and tuple(got.shape) == tuple(np.shape(w))
        assert float(d.distance[0]) == float(np.asarray(w).reshape(-1)[0])


def test_nearest_feasible_argument_checks_and_out_reuse(fake_env):
    env, fake = fake_env
    s, a = states(4), _actions(4)
    for args, kw in (((s[:, :28], a), {}), ((s, a[:3]), {}), ((s, a[:, :13]), {}), ((s, a[:, :38]), {}), ((s, np.zeros((4, 2, 7))), {}),
                     ((s, a), dict(tol=0.0)), ((s, a), dict(tol=float("nan"))), ((s, a), dict(max_iters=-1)), ((s, a), dict(max_iters=1.5)),
                     ((s, a), dict(weight=np.ones(13))), ((s, a), dict(weight=np.ones((3, 14)))), ((s, a), dict(weight=np.zeros(14))),
                     ((s, a), dict(weight=-np.ones(14))), ((s, a), dict(weight=np.full(14, np.inf))),
                     ((s, a), dict(weight=np.where(np.arange(14) == 3, np.nan, 1.0))), ((s, a), dict(out="x")),
                     ((s, a), dict(out=env.nearest_feasible(states(3), _actions(3))))):
        before = len(fake.calls)
        with pytest.raises(ValueError, match="nearest_feasible"):
            env.nearest_feasible(*args, **kw)
        assert len(fake.calls) == before
    first = env.nearest_feasible(s, a)
    again = env.nearest_feasible(states(4, seed=1), _actions(4, seed=2), out=first)
    assert again is first and fake.calls[-1]["action"] is first.action and fake.calls[-1]["info"] is first.info
    assert np.array_equal(first.target.numpy(), _actions(4, seed=2)[:, PARTIAL])
    assert list(inspect.signature(env.nearest_feasible).parameters) == ["obs", "action", "weight", "tol", "max_iters", "out"]


def test_not_implemented_with_a_reason_without_the_kernel():
    env = EVOPFEnv(backend=ob, device="cpu")
    s, a = states(2), _actions(2)
    with pytest.raises(NotImplementedError, match="evopf_opf|evopf_nearest"):
        env.nearest_feasible(s, a)
    hip_on_cpu = EVOPFEnv(device="cpu")
    with pytest.raises(NotImplementedError, match="GPU"):
        hip_on_cpu.nearest_feasible(s, a)
    with pytest.raises(NotImplementedError, match="GPU"):
        hip_on_cpu._nearest_kernel()
    for e in (env, hip_on_cpu):                                   # evaluate_filtered: the same reasons, before anything is built
        tr = types.SimpleNamespace(base_env=e, kernels=types.SimpleNamespace(name="EVOPF-v0"))
        with pytest.raises(NotImplementedError, match="evopf_opf|evopf_nearest" if e is env else "GPU"):
            evaluate_filtered(tr)
    cart = types.SimpleNamespace(base_env=object(), kernels=types.SimpleNamespace(name="CartSafe-v0"))
    with pytest.raises(NotImplementedError, match="EVOPF-v0"):
        evaluate_filtered(cart)


@functools.lru_cache(maxsize=None)
def _cpu_evopf_trainer():
    torch.manual_seed(4)
    tr = build_trainer("ddpg", "evopf", ob, torch.device("cpu"), fused=False, num_envs=2, use_graph=False, capacity=32)
    tr.vec.reset()
    return tr


def test_evaluate_filtered_refusals(monkeypatch):
    tr = _cpu_evopf_trainer()
    sig = inspect.signature(tr.evaluate_filtered).parameters
    names = ["episodes", "seed", "horizon", "init_states", "record", "constraints", "weight", "tol", "max_iters", "fallback",
             "eval_steps", "eval_lr", "scenarios"]
    assert list(sig) == names and list(inspect.signature(evaluate_filtered).parameters) == ["tr"] + names
    assert (sig["fallback"].default, sig["tol"].default, sig["max_iters"].default, sig["episodes"].default) == ("policy", 1e-4, 40, 10)
    # the neighbours keep their parameter lists
    assert list(inspect.signature(tr.evaluate_opf).parameters)[-4:] == ["pe", "pe_cost", "tol", "max_iters"]
    assert list(inspect.signature(tr.evaluate).parameters)[-1] == "scenarios"
    assert list(inspect.signature(tr.base_env.opf).parameters)[-1] == "pe_cost"
    with pytest.raises(NotImplementedError, match="evopf_opf|evopf_nearest"):       # the oracle backend has no solver
        tr.evaluate_filtered(2)
    fake = FakeNearest()
    monkeypatch.setattr(tr.base_env, "_nearest_kernel", lambda: fake, raising=True)
    for kw in (dict(fallback="opf"), dict(fallback=None), dict(tol=0.0), dict(max_iters=-1), dict(max_iters=1.5), dict(episodes=0),
               dict(horizon=0), dict(record=5), dict(constraints=1), dict(weight=np.zeros(14)), dict(weight=np.ones((3, 14))),
               dict(init_states=np.zeros((2, 3))), dict(eval_steps=-1), dict(eval_lr=float("nan"))):
        with pytest.raises(ValueError):
            tr.evaluate_filtered(**dict(dict(episodes=2), **kw))
    with pytest.raises(NotImplementedError, match="EVOPF-v0"):   # scenarios are played by the HIP step kernel on a GPU
        tr.evaluate_filtered(2, scenarios=object())
    assert not fake.calls


def test_evaluate_filtered_runs_the_policy_then_the_filter(monkeypatch):
    tr = _cpu_evopf_trainer()
    H, n = 3, 4
    policy = tr.evaluate(n, horizon=H, seed=7, record=True)
    fake = FakeNearest()
    monkeypatch.setattr(tr.base_env, "_nearest_kernel", lambda: fake, raising=True)
    res = tr.evaluate_filtered(n, seed=7, horizon=H, record=True, constraints=True, tol=1e-3, max_iters=11)
    assert res.path == "filtered" and res.seed == 7 and res.horizon == H and res.episodes == n and len(fake.calls) == H
    assert all(c["obs"].shape == (n, 57) and (c["tol"], c["max_iters"]) == (1e-3, 11) and c["weight"] is None for c in fake.calls)
    assert (res.length == H).all() and res.filter_iters.shape == (n, H) and res.filter_iters.dtype == np.int32
    assert (res.filter_iters == 7).all() and (res.proj_iters == 7 * H).all() and res.filter_distance.dtype == np.float32
    assert (res.filter_distance == 0.25).all() and res.opf_iters is None and res.constraints is not None
    even = np.arange(n) % 2 == 0
    assert np.array_equal(res.filter_converged, np.repeat(even[:, None], H, axis=1))
    tj, ptj = res.trajectory, policy.trajectory
    # the same episodes as evaluate(seed): hour 0 is its observation, and the filter was given the policy's action
    assert np.array_equal(tj.obs[:, 0], ptj.obs[:, 0]) and np.array_equal(tj.obs[:, 0], ev.reset(7, np.arange(n), 0).astype(np.float32))
    assert np.array_equal(fake.calls[0]["target"].numpy(), ptj.action[:, 0])
    assert np.array_equal(tj.proposal[:, 0], ptj.action[:, 0][:, PARTIAL])
    assert all(np.array_equal(tj.proposal[:, i], fake.calls[i]["target"].numpy()[:, PARTIAL]) for i in range(H))
    assert np.array_equal(tj.obs[:, 1], fake.calls[1]["obs"].numpy())           # the filter read the env's own observation rows
    # fallback="policy": converged rows step the filter's answer (idle batteries here), the others the policy's own action -- a
    # select per row: the odd episodes ARE evaluate()'s, bit for bit, over the whole horizon
    assert (tj.action[even][:, :, 38:] == 0).all()
    assert all(np.array_equal(tj.action[even][:, i, :38], fake.calls[i]["target"].numpy()[even][:, :38]) for i in range(H))
    for name in ("obs", "action", "reward", "eq", "ineq"):
        assert np.array_equal(getattr(tj, name)[~even], getattr(ptj, name)[~even]), name
    assert np.array_equal(res.ret[~even], policy.ret[~even]) and not np.array_equal(res.ret[even], policy.ret[even])
    # fallback="last": every row steps the solver's iterate
    last = tr.evaluate_filtered(n, seed=7, horizon=H, record=True, fallback="last", weight=np.full(14, 3.0))
    assert (last.trajectory.action[:, :, 38:] == 0).all() and (last.filter_distance == 3.0).all()
    assert np.array_equal(last.trajectory.action[even], tj.action[even]) and np.array_equal(last.filter_converged, res.filter_converged)
    assert all(torch.equal(c["weight"], torch.full((14,), 3.0)) for c in fake.calls[H:])
    # the budget overrides reach the policy, not the filter
    short = tr.evaluate_filtered(n, seed=7, horizon=1, record=True, eval_steps=0)
    assert np.array_equal(short.trajectory.proposal[:, 0], tr.evaluate(n, horizon=1, seed=7, record=True, eval_steps=0).trajectory.action[:, 0][:, PARTIAL])
    again = tr.evaluate_filtered(n, seed=7, horizon=H, tol=1e-3, max_iters=11)
    assert np.array_equal(again.ret, res.ret) and again.trajectory is None and again.constraints is None
    after = tr.evaluate(n, horizon=H, seed=7, record=True)         # a policy's evaluation carries no filter fields and is what it was
    assert after.filter_iters is None and after.filter_converged is None and after.filter_distance is None
    for f in policy.FIELDS:
        assert np.array_equal(getattr(policy, f), getattr(after, f)), f


# ------------------------------------------------------------------------------------------------ binding and C ABI
def test_binding_is_a_backend_function():
    assert callable(ops.evopf_nearest) and not hasattr(ops.EvopfKernels, "evopf_nearest") and not hasattr(ob, "evopf_nearest")
    assert list(inspect.signature(ops.evopf_nearest).parameters) == ["kernels", "obs", "target", "weight", "action", "info", "tol", "max_iters"]
    env = EVOPFEnv(device="cpu")
    good = dict(obs=torch.zeros(2, 57), target=torch.zeros(2, 43), weight=None, action=torch.zeros(2, 43), info=torch.zeros(2, 4))
    with pytest.raises(_lib.RpoHipError):                        # CPU tensors are refused like by every other op
        ops.evopf_nearest(env.kernels, *good.values(), 1e-4, 40)
    for kw in (dict(obs=torch.zeros(3, 57)), dict(obs=torch.zeros(2, 56)), dict(action=torch.zeros(2, 42)), dict(info=torch.zeros(2, 3)),
               dict(target=torch.zeros(2, 14)), dict(target=torch.zeros(3, 43)), dict(target=torch.zeros(2, 86)[:, ::2]),
               dict(weight=torch.zeros(13)), dict(weight=torch.zeros(3, 14)), dict(weight=torch.zeros(2, 28)[:, ::2]),
               dict(obs=torch.zeros(2, 114)[:, ::2])):
        with pytest.raises(_lib.RpoHipError, match="evopf_nearest"):
            ops.evopf_nearest(env.kernels, *dict(good, **kw).values(), 1e-4, 40)


def test_entry_point_is_declared_exported_and_refuses_before_any_launch():
    V, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert _lib.PROTOTYPES["rpo_evopf_nearest"] == [I, V, I, V, I, V, I, V, V, F, I, V, V]
    assert _lib.PROTOTYPES["rpo_evopf_opf_free"] == [I, V, I, V, V, V, F, I, V, V]     # the existing entry points keep their signatures
    assert _lib.PROTOTYPES["rpo_evopf_opf"] == [I, V, I, V, V, V, F, I, V, V]
    assert _lib.CONST["RPO_ABI_VERSION"] == 6                                          # an added entry point: no new ABI version
    lib = _lib.load()
    assert hasattr(lib, "rpo_evopf_nearest") and lib.rpo_abi_version() == 6
    good = dict(n=4, obs=None, obs_stride=57, target=None, target_stride=43, weight=None, weight_stride=0, action_out=None,
                info_out=None, tol=1e-4, max_iters=40, consts_dev=None, stream=None)

    def call(**kw):
        return lib.rpo_evopf_nearest(*dict(good, **kw).values())
    # sizes before pointers: these answer without looking at a pointer
    for kw in (dict(n=0), dict(n=-2), dict(max_iters=-1), dict(tol=0.0), dict(tol=-1e-4), dict(tol=float("nan")), dict(obs_stride=56),
               dict(obs_stride=0), dict(target_stride=42), dict(target_stride=14), dict(target_stride=0), dict(weight_stride=1),
               dict(weight_stride=13), dict(weight_stride=-14), dict(weight_stride=28)):
        assert call(**kw) == ARG, kw
    assert call() == NULL and call(max_iters=0) == NULL and call(weight_stride=14) == NULL
    if torch.cuda.device_count() == 0:
        # host addresses stand in for device pointers (a refusal dereferences nothing): never where a GPU is visible.  A call
        # that got as far as a launch would answer a HIP error code here, neither RPO_ERR_ARG nor RPO_ERR_NULL.
        buf = (ctypes.c_float * 1024)()
        r = ctypes.c_void_p(ctypes.addressof(buf))
        full = dict(obs=r, target=r, weight=r, action_out=r, info_out=r, consts_dev=r)
        for name in ("obs", "target", "action_out", "info_out", "consts_dev"):
            assert call(**dict(full, **{name: None})) == NULL, name
        assert call(**dict(full, n=0)) == ARG and call(**dict(full, target_stride=42)) == ARG
        assert call(**dict(full, weight=None)) not in (0, ARG, NULL)      # weight may be NULL: this one reaches the launch, and fails there
