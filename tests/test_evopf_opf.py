"""The single-step AC-OPF of EVOPF-v0 without a GPU: the float64 yardstick (tests/evopf_opf_f64.py) against finite differences
and against scipy's SLSQP answers in tests/golden/evopf_opf.npz; the public surface (``EVOPFEnv.opf`` / ``opt_solve``,
``EvalTrajectory.opf_gap``) over a stand-in for the backend function; the C-ABI entry point ``rpo_evopf_opf`` and its refusals.
The kernel itself: tests/test_evopf_opf_gpu.py."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import evopf_opf_f64 as opf64
import oracle_backend as ob
from oracle import evopf as ev
from rpo_amd import _lib, ops
from rpo_amd.algo import EvalTrajectory, OpfGap, opf_gap
from rpo_amd.env.electrical_grid.evopf import EVOPFEnv, OpfResult

ARG, NULL = _lib.CONST["RPO_ERR_ARG"], _lib.CONST["RPO_ERR_NULL"]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "evopf_opf.npz")
TOL = 1e-4
AMBIG_CAP = 0.02            # share of the states that may fall between "feasible" and "infeasible"


def classes(z):
    """(feasible, infeasible, left out) masks from SLSQP's final equality residual, and the cap on the third."""
    eq = z["slsqp_eq_resid"]
    feas, infeas = eq < 1e-6, eq > 1e-3
    other = ~(feas | infeas)
    assert other.mean() <= AMBIG_CAP, "left out: %d of %d" % (other.sum(), len(eq))
    return feas, infeas, other


# ------------------------------------------------------------------------------------------------ the yardstick
def test_hessian_against_central_differences_of_eq_jac():
    rng = np.random.default_rng(0)
    for _ in range(4):
        a = np.zeros(43)
        a[ev.GRID.vm0:ev.GRID.va0] = rng.uniform(0.94, 1.06, 14)
        a[ev.GRID.va0:ev.GRID.pe0] = rng.uniform(-0.3, 0.3, 14)
        lam = rng.normal(size=28) * 10
        H = opf64.lagr_hessian(a, lam)
        fd = np.zeros_like(H)
        for j in range(ev.GRID.vm0, ev.GRID.pe0):
            e = np.zeros(43)
            e[j] = 1e-5
            fd[:, j] = lam @ (ev.eq_jac((a + e)[None])[0] - ev.eq_jac((a - e)[None])[0]) / 2e-5
        assert np.abs(H - fd).max() <= 1e-6 * np.abs(H).max()
        assert np.array_equal(H, H.T) or np.abs(H - H.T).max() <= 1e-12 * np.abs(H).max()


def test_fixture_holds_the_stated_states():
    with np.load(GOLDEN) as z:
        demand, pe = opf64.fixture_states()
        assert z["demand"].shape == (384, 28) and np.array_equal(z["demand"], demand) and np.array_equal(z["pe"], pe)
        assert (pe[:48] == 0).all() and (pe[48:96] != 0).all() and pe.min() >= -0.18 and pe.max() <= 0.2 / 0.9
        assert os.path.getsize(GOLDEN) < 512 * 1024


def test_helper_against_slsqp_on_all_states():
    with np.load(GOLDEN) as z:
        z = {k: z[k] for k in z.files}
    feas, infeas, other = classes(z)
    print("feasible %d, infeasible %d, left out %d" % (feas.sum(), infeas.sum(), other.sum()))
    r = opf64.solve_many(z["demand"][feas], z["pe"][feas], tol=TOL, max_iters=25)
    assert r["converged"].all() and r["iters"].max() <= 25
    infeasibility = opf64.infeasibility(z["demand"][feas], r["action"])
    dev = r["cost"] - z["slsqp_cost"][feas]
    print("iterations %d..%d, infeasibility <= %.3g, cost - SLSQP in [%.3g, %.3g]"
          % (r["iters"].min(), r["iters"].max(), infeasibility.max(), dev.min(), dev.max()))
    assert infeasibility.max() <= TOL
    assert np.abs(dev).max() <= 1e-4
    bad = opf64.solve_many(z["demand"][infeas], z["pe"][infeas], tol=TOL, max_iters=80)
    assert not bad["converged"].any() and (bad["iters"] == 80).all()


def test_helper_without_iterations_is_the_flat_start():
    demand, pe = opf64.fixture_states()
    r = opf64.solve(demand[50], pe[50], max_iters=0)
    assert not r["converged"] and r["iters"] == 0 and np.array_equal(r["action"], opf64.flat_start(pe[50]))


# ------------------------------------------------------------------------------------------------ surface over a stand-in
class FakeOpf(object):
    """Stands in for ``ops.evopf_opf`` on CPU tensors: cost = 1 + pd[0], converged iff qd[0] >= 0, action = (pd[:5] in pg, the
    given pe, zeros elsewhere), 7 iterations, residual 5e-5 -- and keeps what it was called with."""

    def __init__(self):
        self.calls = []

    def __call__(self, kernels, obs, pe, action, info, tol, max_iters):
        self.calls.append(dict(obs=obs[:, :28].clone(), pe=None if pe is None else pe.clone(), tol=tol, max_iters=max_iters,
                               width=obs.shape[1], action=action, info=info))
        action.zero_()
        action[:, :5] = obs[:, :5]
        if pe is not None:
            action[:, 38:] = pe
        info[:, 0] = 1.0 + obs[:, 0]
        info[:, 1] = 5e-5
        info[:, 2] = 7.0
        info[:, 3] = (obs[:, 14] >= 0).float()


@pytest.fixture
def fake_env(monkeypatch):
    env = EVOPFEnv(backend=ob, device="cpu")
    fake = FakeOpf()
    monkeypatch.setattr(env, "_opf_kernel", lambda: fake, raising=True)
    return env, fake


def states(n, seed=0):
    rng = np.random.default_rng(seed)
    s = rng.uniform(0.1, 1.0, size=(n, 57)).astype(np.float32)
    s[::3, 14] = -s[::3, 14]                                     # every third row: "not converged" to the stand-in
    return s


def test_opf_takes_observations_or_demands(fake_env):
    env, fake = fake_env
    s = states(5)
    pe = np.full((5, 5), 0.1, dtype=np.float32)
    a = env.opf(s, pe=pe)
    b = env.opf(s[:, :28], pe=pe, tol=1e-3, max_iters=9)
    assert isinstance(a, OpfResult) and [c["width"] for c in fake.calls] == [57, 28]
    assert torch.equal(fake.calls[0]["obs"], fake.calls[1]["obs"]) and torch.equal(fake.calls[0]["pe"], fake.calls[1]["pe"])
    assert (fake.calls[0]["tol"], fake.calls[0]["max_iters"]) == (1e-4, 40) and (fake.calls[1]["tol"], fake.calls[1]["max_iters"]) == (1e-3, 9)
    assert torch.equal(a.action, b.action) and torch.equal(a.cost, b.cost)
    assert a.action.shape == (5, 43) and a.cost.shape == (5,) and a.residual.shape == (5,)
    assert a.iters.dtype == torch.int32 and a.iters.tolist() == [7] * 5
    assert a.converged.dtype == torch.bool and a.converged.tolist() == [False, True, True, False, True]
    assert a.converged_rate() == pytest.approx(0.6)
    host = a.numpy()
    assert set(host) == {"action", "cost", "residual", "iters", "converged"} and host["iters"].dtype == np.int32
    assert np.array_equal(host["action"][:, 38:], pe) and np.allclose(host["cost"], 1.0 + s[:, 0])
    assert env.opf(s).action[:, 38:].abs().max() == 0 and fake.calls[-1]["pe"] is None          # pe=None: the reference's problem
    one = env.opf(s[0])                                                                          # one state
    assert one.action.shape == (1, 43)


def test_opf_argument_checks(fake_env):
    env, fake = fake_env
    s = states(4)
    for kw in (dict(tol=0.0), dict(tol=-1.0), dict(tol=float("nan")), dict(max_iters=-1), dict(max_iters=2.5)):
        with pytest.raises(ValueError):
            env.opf(s, **kw)
    for bad in (s[:, :27], s[:, :29], np.zeros((0, 57), np.float32), np.zeros((2, 3, 57), np.float32)):
        with pytest.raises(ValueError):
            env.opf(bad)
    for pe in (np.zeros((3, 5), np.float32), np.zeros((4, 4), np.float32)):
        with pytest.raises(ValueError):
            env.opf(s, pe=pe)
    assert not fake.calls
    assert env.opf(s, max_iters=0).action.shape == (4, 43) and fake.calls[-1]["max_iters"] == 0


def test_opf_out_reuses_and_validates(fake_env):
    env, fake = fake_env
    s = states(4)
    first = env.opf(s)
    again = env.opf(states(4, seed=1), out=first)
    assert again is first and fake.calls[-1]["action"] is first.action and fake.calls[-1]["info"] is first.info
    for bad in (env.opf(states(3)), "x", OpfResult(torch.zeros(4, 43, dtype=torch.float64), torch.zeros(4, 4)),
                OpfResult(torch.zeros(4, 43), torch.zeros(4, 5)), OpfResult(torch.zeros(4, 86)[:, ::2], torch.zeros(4, 4))):
        with pytest.raises(ValueError):
            env.opf(s, out=bad)


def test_opt_solve_has_the_reference_shape(fake_env):
    env, fake = fake_env
    X = states(6)[:, :28]
    Y, total, each = env.opt_solve(X)
    assert Y.shape == (6, 38) and Y.dtype == np.float64 and isinstance(total, float) and isinstance(each, float)
    assert total > 0 and each == pytest.approx(total / 6)
    conv = X[:, 14] >= 0
    assert np.isnan(Y[~conv]).all() and np.isfinite(Y[conv]).all() and np.allclose(Y[conv][:, :5], X[conv][:, :5])
    assert fake.calls[-1]["pe"] is None and fake.calls[-1]["tol"] == 1e-4
    Y2, _, _ = env.opt_solve(torch.from_numpy(X), solver_type="hip", tol=1e-3)
    assert np.array_equal(np.isnan(Y2), np.isnan(Y)) and fake.calls[-1]["tol"] == 1e-3
    with pytest.raises(NotImplementedError, match="pypower"):
        env.opt_solve(X, solver_type="pypower")
    with pytest.raises(ValueError):
        env.opt_solve(states(6))                                  # observations: opt_solve takes demands, like the reference


def trajectory(E=3, H=4, lengths=(4, 2, 0), seed=2):
    rng = np.random.default_rng(seed)
    obs = states(E * H, seed).reshape(E, H, 57)
    action = rng.uniform(0.0, 0.5, size=(E, H, 43)).astype(np.float32)
    length = np.array(lengths)
    valid = np.arange(H)[None, :] < length[:, None]
    zeros = np.zeros((E, H), dtype=np.float32)
    ineq = rng.uniform(0, 2e-3, size=(E, H)).astype(np.float32)
    return EvalTrajectory(1e-3, obs=obs, proposal=np.zeros((E, H, 14), np.float32), action=action, reward=zeros, done=zeros != 0,
                          ineq=ineq, eq=zeros, iters=zeros.astype(np.int32), valid=valid, length=length)


def test_opf_gap_places_nans_and_round_trips(fake_env, tmp_path):
    env, fake = fake_env
    tj = trajectory()
    gap = tj.opf_gap(env, tol=1e-3, max_iters=30)
    assert isinstance(gap, OpfGap) and len(fake.calls) == 1 and fake.calls[0]["obs"].shape[0] == 6      # one launch, valid steps only
    assert (fake.calls[0]["tol"], fake.calls[0]["max_iters"]) == (1e-3, 30)
    assert np.array_equal(fake.calls[0]["pe"].numpy(), tj.action[tj.valid][:, 38:])
    conv = tj.valid & (tj.obs[:, :, 14] >= 0)
    assert conv.any() and (tj.valid & ~conv).any()
    for name in OpfGap.ARRAYS:
        assert getattr(gap, name).shape == (3, 4)
    assert np.array_equal(gap.converged, conv) and np.array_equal(gap.valid, tj.valid)
    assert np.array_equal(np.isnan(gap.cost_policy), ~tj.valid)
    assert np.array_equal(np.isnan(gap.cost_opt), ~conv) and np.array_equal(np.isnan(gap.gap), ~conv)
    want = ev.obj_fn(tj.action[tj.valid].astype(np.float64))
    assert np.allclose(gap.cost_policy[tj.valid], want, rtol=1e-5)
    assert np.allclose(gap.cost_opt[conv], 1.0 + tj.obs[:, :, 0][conv])
    assert np.allclose(gap.gap[conv], (gap.cost_policy[conv] - gap.cost_opt[conv]) / gap.cost_opt[conv])
    assert (gap.gap[conv] < 0).any()                             # not clipped
    assert gap.converged_rate() == pytest.approx(conv.sum() / tj.valid.sum())
    assert gap.mean() == pytest.approx(np.nanmean(gap.gap)) and gap.quantile(0.5) == pytest.approx(np.nanquantile(gap.gap, 0.5))
    only = gap.feasible_only(1e-3)
    keep = conv & (tj.ineq <= 1e-3)
    assert keep.any() and (conv & ~keep).any() and np.array_equal(np.isnan(only.gap), ~keep)
    assert np.array_equal(only.cost_opt, gap.cost_opt, equal_nan=True)
    path = str(tmp_path / "gap.npz")
    gap.save(path)
    back = OpfGap.load(path)
    assert (back.tol, back.max_iters) == (1e-3, 30)
    for name in OpfGap.ARRAYS:
        assert np.array_equal(getattr(back, name), getattr(gap, name), equal_nan=True), name
    assert np.array_equal(opf_gap(tj, env, tol=1e-3, max_iters=30).gap, gap.gap, equal_nan=True)      # the exported function
    empty = trajectory(lengths=(0, 0, 0)).opf_gap(env)
    assert np.isnan(empty.gap).all() and np.isnan(empty.mean()) and np.isnan(empty.converged_rate()) and len(fake.calls) == 2


def test_opf_gap_argument_checks(fake_env):
    env, fake = fake_env
    tj = trajectory()
    with pytest.raises(TypeError):
        opf_gap(tj, object())
    tj.obs = tj.obs[:, :, :6]
    with pytest.raises(ValueError):
        opf_gap(tj, env)
    assert not fake.calls


def test_not_implemented_with_a_reason_without_the_kernel():
    env = EVOPFEnv(backend=ob, device="cpu")
    X = states(2)[:, :28]
    for call in (lambda: env.opf(X), lambda: env.opt_solve(X), lambda: trajectory().opf_gap(env)):
        with pytest.raises(NotImplementedError, match="evopf_opf"):
            call()
    with pytest.raises(NotImplementedError, match="pypower"):
        env.opt_solve(X, solver_type="pypower")
    hip_on_cpu = EVOPFEnv(device="cpu")
    for call in (lambda: hip_on_cpu.opf(X), lambda: hip_on_cpu.opt_solve(X)):
        with pytest.raises(NotImplementedError, match="GPU"):
            call()


# ------------------------------------------------------------------------------------------------ binding and C ABI
def test_binding_is_a_backend_function():
    assert callable(ops.evopf_opf) and not hasattr(ops.EvopfKernels, "opf") and not hasattr(ops.EvopfKernels, "evopf_opf")
    assert list(inspect.signature(ops.evopf_opf).parameters) == ["kernels", "obs", "pe", "action", "info", "tol", "max_iters"]
    assert not hasattr(ob, "evopf_opf")
    env = EVOPFEnv(device="cpu")
    with pytest.raises(_lib.RpoHipError):                        # CPU tensors are refused like by every other op
        ops.evopf_opf(env.kernels, torch.zeros(2, 57), None, torch.zeros(2, 43), torch.zeros(2, 4), 1e-4, 40)
    for kw in (dict(obs=torch.zeros(3, 57)), dict(obs=torch.zeros(2, 27)), dict(action=torch.zeros(2, 42)), dict(info=torch.zeros(2, 3)),
               dict(pe=torch.zeros(2, 4)), dict(obs=torch.zeros(2, 114)[:, ::2])):
        args = dict(dict(obs=torch.zeros(2, 57), pe=None, action=torch.zeros(2, 43), info=torch.zeros(2, 4)), **kw)
        with pytest.raises(_lib.RpoHipError, match="evopf_opf"):
            ops.evopf_opf(env.kernels, args["obs"], args["pe"], args["action"], args["info"], 1e-4, 40)


def test_entry_point_is_declared_exported_and_refuses_before_any_launch():
    proto = _lib.PROTOTYPES["rpo_evopf_opf"]
    V, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert proto == [I, V, I, V, V, V, F, I, V, V]
    assert _lib.CONST["RPO_ABI_VERSION"] == 6
    lib = _lib.load()
    assert hasattr(lib, "rpo_evopf_opf")
    good = dict(n=4, obs=None, obs_stride=57, pe=None, action_out=None, info_out=None, tol=1e-4, max_iters=40, consts_dev=None,
                stream=None)

    def call(**kw):
        return lib.rpo_evopf_opf(*dict(good, **kw).values())
    # sizes before pointers: these answer without looking at a pointer
    for kw in (dict(n=0), dict(n=-2), dict(max_iters=-1), dict(tol=0.0), dict(tol=-1e-4), dict(tol=float("nan")), dict(obs_stride=27),
               dict(obs_stride=0)):
        assert call(**kw) == ARG, kw
    assert call() == NULL and call(obs_stride=28, max_iters=0) == NULL
    if torch.cuda.device_count() == 0:
        # host addresses stand in for device pointers (a refusal dereferences nothing): never where a GPU is visible.  A call
        # that got as far as a launch would answer a HIP error code here, neither RPO_ERR_ARG nor RPO_ERR_NULL.
        buf = (ctypes.c_float * 1024)()
        r = ctypes.c_void_p(ctypes.addressof(buf))
        full = dict(obs=r, pe=r, action_out=r, info_out=r, consts_dev=r)
        for name in ("obs", "action_out", "info_out", "consts_dev"):
            assert call(**dict(full, **{name: None})) == NULL, name
        assert call(**dict(full, n=0)) == ARG and call(**dict(full, obs_stride=27)) == ARG
        assert call(**dict(full, pe=None)) not in (0, ARG, NULL)     # pe may be NULL: this one reaches the launch, and fails there
