"""The single-step AC-OPF of EVOPF-v0 without a GPU: the float64 yardstick (tests/evopf_opf_f64.py) against finite differences
and against scipy's SLSQP answers in tests/golden/evopf_opf.npz; the public surface (``EVOPFEnv.opf`` / ``opt_solve``,
``EvalTrajectory.opf_gap``) over a stand-in for the backend function; the C-ABI entry point ``rpo_evopf_opf`` and its refusals.
The kernel itself: tests/test_evopf_opf_gpu.py.

One iteration at a time (tests/test_evopf_opf_f64_gpu.py on the device): the float32 emulation ``emu_opf`` passes every checker
of ``step_ref`` on the trajectory states of the 70 fixture rows and on the synthetic states under both constants tables, the
constants C_REF are what it measures there, every seeded mutation fails a checker on those same inputs, ``step_ref`` iterated is
``solve()`` as it was before the refactor, and the state seam's entry point and keywords refuse what they must."""
import ctypes
import functools
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

    def __call__(self, kernels, obs, pe, action, info, tol, max_iters, state_in=None, state_out=None):
        self.calls.append(dict(obs=obs[:, :28].clone(), pe=None if pe is None else pe.clone(), tol=tol, max_iters=max_iters,
                               width=obs.shape[1], action=action, info=info, state_in=state_in, state_out=state_out))
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
    assert list(inspect.signature(ops.evopf_opf).parameters) == ["kernels", "obs", "pe", "action", "info", "tol", "max_iters", "state_in",
                                                                        "state_out"]
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


# ------------------------------------------------------------------------------------------------ one iteration at a time
def _solve_before_refactor(demand, pe=None, tol=1e-4, max_iters=40, grid=opf64.GRID):
    """``evopf_opf_f64.solve`` as it stood before ``ip_eval`` / ``ip_advance`` were cut out of it, kept verbatim: what
    test_step_ref_iterated_is_solve holds the refactored helper to, bit for bit (both run on the same LAPACK)."""
    ev_, NBND, NG, NX, NEQ, XIDX = ev, opf64.NBND, opf64.NG, opf64.NX, opf64.NEQ, opf64.XIDX
    XMAX, XMIN, COST1, COST2, Z0, GAMMA0, XI, SIGMA = (opf64.XMAX, opf64.XMIN, opf64.COST1, opf64.COST2, opf64.Z0, opf64.GAMMA0,
                                                       opf64.XI, opf64.SIGMA)
    s = np.asarray(demand, dtype=np.float64)[None, :2 * opf64.NB]
    pe = np.zeros(grid.ne) if pe is None else np.asarray(pe, dtype=np.float64)
    a = opf64.flat_start(pe, grid)
    h = np.concatenate([a[:NBND] - XMAX, XMIN - a[:NBND]])
    z = np.maximum(-h, Z0)
    gamma = GAMMA0
    mu = gamma / z
    lam = np.zeros(NEQ)
    it, converged = 0, False
    while True:
        g = ev_.eq_resid(s, a[None], grid)[0]
        J = ev_.eq_jac(a[None], grid)[0][:, XIDX]
        h = np.concatenate([a[:NBND] - XMAX, XMIN - a[:NBND]])
        df = np.zeros(NX)
        df[:NG] = COST2 * a[:NG] + COST1
        dmu = np.zeros(NX)
        dmu[:NBND] = mu[:NBND] - mu[NBND:]
        lx = df + J.T @ lam + dmu
        with np.errstate(all="ignore"):
            residual = max(np.abs(g).max(), h.max(), np.abs(lx).max(), float(z @ mu))
        if residual < tol:
            converged = True
            break
        if it >= max_iters:
            break
        with np.errstate(all="ignore"):
            M = opf64.lagr_hessian(a, lam, grid)[np.ix_(XIDX, XIDX)]
            M[np.arange(NG), np.arange(NG)] += COST2
            M[np.arange(NBND), np.arange(NBND)] += mu[:NBND] / z[:NBND] + mu[NBND:] / z[NBND:]
            N = lx.copy()
            N[:NBND] += (mu[:NBND] * h[:NBND] + gamma) / z[:NBND] - (mu[NBND:] * h[NBND:] + gamma) / z[NBND:]
            K = np.zeros((NX + NEQ, NX + NEQ))
            K[:NX, :NX], K[:NX, NX:], K[NX:, :NX] = M, J.T, J
            try:
                sol = np.linalg.solve(K, np.concatenate([-N, -g]))
            except np.linalg.LinAlgError:
                sol = np.full(NX + NEQ, np.nan)
            dx, dlam = sol[:NX], sol[NX:]
            dh = np.concatenate([dx[:NBND], -dx[:NBND]])
            dz = -h - z - dh
            dm = -mu + (gamma - mu * dz) / z
            neg = dz < 0
            alpha_p = min(XI * np.min(z[neg] / -dz[neg]), 1.0) if neg.any() else 1.0
            neg = dm < 0
            alpha_d = min(XI * np.min(mu[neg] / -dm[neg]), 1.0) if neg.any() else 1.0
            a[XIDX] += alpha_p * dx
            z = z + alpha_p * dz
            lam = lam + alpha_d * dlam
            mu = mu + alpha_d * dm
            gamma = SIGMA * float(z @ mu) / (2 * NBND)
        it += 1
    return dict(action=a, cost=float(ev_.obj_fn(a[None], grid)[0]), iters=it, converged=converged, residual=float(residual))


def test_step_ref_iterated_is_solve():
    """``step_ref`` on the reference's float64 case, iterated from the flat start, walks ``solve()``'s iterates -- and ``solve()``
    itself, which now runs on the same two functions, returns what it did before, bit for bit."""
    demand, pe = opf64.fixture_states()
    for i in (0, 50, 100, 191, 383):
        old = _solve_before_refactor(demand[i], pe[i], tol=TOL, max_iters=40)
        new = opf64.solve(demand[i], pe[i], tol=TOL, max_iters=40)
        for k in ("action", "cost", "iters", "converged", "residual"):
            assert np.array_equal(old[k], new[k], equal_nan=True), (i, k)
        state = opf64.join_state(*opf64.flat_state(pe[i]))[None]
        for it in range(old["iters"] + 1):
            r = opf64.step_ref(None, demand[i][None], state, bound=False)
            assert (r["stop"][0, 3] < TOL) == (it == old["iters"] and bool(old["converged"])), (i, it)
            if it < old["iters"]:
                state = r["state"]
        assert np.array_equal(state[0, :43], old["action"]) and r["stop"][0, 3] == old["residual"], i


OPF_SEED, OPF_N, KMAX = 3, 65, 12


@functools.lru_cache(maxsize=None)
def opf_inputs():
    """The inputs of the GPU file with the emulation in the kernel's place: name -> (table, demand, states [n, 168], step_ref
    there); the trajectory states k = 0 .. 12 of the 70 fixture rows stacked (910 rows) and opf_states under both tables."""
    import evopf_f64 as E
    tab = E.consts_table()
    shifted = opf64.shifted_table(tab)
    demand, pe = opf64.fixture_rows()

    def run(state, iters):
        return opf64.emu_opf(tab, demand, pe if state is None else state, 1e-30, iters)["state"]
    traj = opf64.trajectory_states(run, KMAX).reshape(-1, opf64.OPF_STATE)
    out = {"trajectory": (tab, np.tile(demand, (KMAX + 1, 1)), traj)}
    for name, t in (("synthetic", tab), ("synthetic_shifted", shifted)):
        d, st = opf64.opf_states(OPF_N, OPF_SEED, t)
        out[name] = (t, d, st)
    return {k: v + (opf64.step_ref(*v),) for k, v in out.items()}


def emulation_ratios(mut=()):
    """One emulated step (and the stop quantities and the cost) from every input state against step_ref -> ({group: worst ratio},
    {name: rows not judged}, violations of the pivot rule)."""
    worst, left, picks = {}, {}, 0
    for name, (tab, demand, states, ref) in opf_inputs().items():
        out = opf64.emu_opf(tab, demand, states, 1e-30, 1, mut)
        at = opf64.emu_opf(tab, demand, states, 1e-30, 0, mut)
        r, unj = opf64.check_step(ref, out["state"])
        r["opf_stop"], _ = opf64.check_stop(ref, np.concatenate([at["stop"], at["info"][:, 1:2]], axis=1))
        rc, uc = opf64.ratios("opf_cost", out["info"][:, 0], *opf64.cost_ref(tab, out["action"]))
        r["opf_cost"] = float(rc[~uc].max())
        for g, v in r.items():
            worst[g] = max(worst.get(g, 0.0), v)
        left[name], picks = unj, picks + out["picks"]
    return worst, left, picks


@functools.lru_cache(maxsize=None)
def emulation():
    return emulation_ratios()


def test_emulation_passes_every_checker():
    worst, left, picks = emulation()
    print({g: round(v, 3) for g, v in worst.items()}, {k: int(v.sum()) for k, v in left.items()})
    assert set(worst) == set(opf64.C_REF) and picks == 0
    for group, ratio in worst.items():
        assert ratio <= 1.0, (group, ratio)
    # rows not judged: the NaN row; late iterates (and only late ones, k >= 4) of the trajectories, the five infeasible rows from
    # k = 8 on; of the synthetic states the wide odd rows -- never one of the rows built for a purpose
    traj = left["trajectory"].reshape(KMAX + 1, 70)
    assert not traj[:4].any() and not traj[:10, :65].any() and traj[:, :65].mean() <= 0.05
    for name in ("synthetic", "synthetic_shifted"):
        rows = np.nonzero(left[name])[0]
        assert 9 in rows and not (set(rows) - {9}) & set(range(opf64.N_SPECIAL)) and (rows[rows != 9] % 2 == 1).all()
        assert len(rows) <= 0.4 * OPF_N
    print("not judged: trajectory %s per k, synthetic %s" % (traj.sum(axis=1).tolist(), [int(left[k].sum()) for k in ("synthetic", "synthetic_shifted")]))


def test_yardstick_constants():
    """C_REF[group] is the emulation's own worst error in units of eps32 * bound (ratio * MARGIN * C_REF) on these inputs: not
    above it, and not below 0.9 of it."""
    worst, _, _ = emulation()
    for group, c in opf64.C_REF.items():
        measured = worst[group] * opf64.MARGIN * c
        print("%-10s measured %.4f  C_REF %.3f" % (group, measured, c))
        assert 0.9 * c <= measured <= c, (group, measured, c)


@pytest.mark.parametrize("mut", opf64.MUTATIONS)
def test_mutation_fails_a_checker(mut):
    worst, _, picks = emulation_ratios((mut,))
    print(mut, {g: round(v, 2) for g, v in worst.items()}, "pivot rule violations", picks)
    assert max(worst.values()) > 1.0 or picks > 0, mut


# ------------------------------------------------------------------------------------------------ the state seam: keywords, ABI
def test_opf_state_keywords_pass_through_and_are_checked(fake_env):
    env, fake = fake_env
    s = states(4)
    st_in, st_out = torch.zeros(4, 168), torch.empty(4, 168)
    res = env.opf(s, state_in=st_in, state_out=st_out, max_iters=1)
    assert isinstance(res, OpfResult) and fake.calls[-1]["state_in"] is st_in and fake.calls[-1]["state_out"] is st_out
    assert fake.calls[-1]["pe"] is None and fake.calls[-1]["max_iters"] == 1
    env.opf(s, state_out=st_out)
    assert fake.calls[-1]["state_in"] is None and fake.calls[-1]["state_out"] is st_out
    env.opf(s, pe=np.zeros((4, 5), np.float32), state_out=st_out)                  # pe with state_out alone is fine
    env.opf(s)
    assert fake.calls[-1]["state_in"] is None and fake.calls[-1]["state_out"] is None
    n = len(fake.calls)
    bad = (torch.zeros(3, 168), torch.zeros(4, 167), torch.zeros(4, 168, dtype=torch.float64), torch.zeros(4, 336)[:, ::2],
           torch.zeros(168), np.zeros((4, 168), np.float32))
    for name in ("state_in", "state_out"):
        for t in bad:
            with pytest.raises(ValueError, match=name):
                env.opf(s, **{name: t})
    with pytest.raises(ValueError, match="pe"):
        env.opf(s, pe=np.zeros((4, 5), np.float32), state_in=st_in)
    assert len(fake.calls) == n                                                   # refused before the backend was called


def test_binding_checks_the_state_arguments():
    env = EVOPFEnv(device="cpu")
    base = dict(obs=torch.zeros(2, 57), pe=None, action=torch.zeros(2, 43), info=torch.zeros(2, 4))

    def call(**kw):
        a = dict(base, **kw)
        ops.evopf_opf(env.kernels, a["obs"], a["pe"], a["action"], a["info"], 1e-4, 40, state_in=a.get("state_in"),
                      state_out=a.get("state_out"))
    assert ops.OPF_STATE == _lib.CONST["RPO_EVOPF_OPF_STATE"] == opf64.OPF_STATE == 168
    for name in ("state_in", "state_out"):
        for t in (torch.zeros(3, 168), torch.zeros(2, 167), torch.zeros(2, 168, dtype=torch.float64), torch.zeros(2, 336)[:, ::2]):
            with pytest.raises(_lib.RpoHipError, match="evopf_opf: %s" % name):
                call(**{name: t})
    with pytest.raises(_lib.RpoHipError, match="pe must be None"):
        call(pe=torch.zeros(2, 5), state_in=torch.zeros(2, 168))
    with pytest.raises(_lib.RpoHipError):                        # well-formed CPU tensors: refused like by every other op
        call(state_in=torch.zeros(2, 168), state_out=torch.zeros(2, 168))


def test_state_entry_point_is_declared_exported_and_refuses_before_any_launch():
    V, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert _lib.PROTOTYPES["rpo_evopf_opf_state"] == [I, V, I, V, V, V, F, I, V, V, V, V]
    assert _lib.PROTOTYPES["rpo_evopf_opf"] == [I, V, I, V, V, V, F, I, V, V]        # the existing entry point keeps its signature
    assert _lib.CONST["RPO_ABI_VERSION"] == 6                                        # an added entry point: no new ABI version
    lib = _lib.load()
    assert hasattr(lib, "rpo_evopf_opf_state")
    good = dict(n=4, obs=None, obs_stride=57, pe=None, action_out=None, info_out=None, tol=1e-4, max_iters=40, consts_dev=None,
                state_in=None, state_out=None, stream=None)

    def call(**kw):
        return lib.rpo_evopf_opf_state(*dict(good, **kw).values())
    for kw in (dict(n=0), dict(n=-2), dict(max_iters=-1), dict(tol=0.0), dict(tol=-1e-4), dict(tol=float("nan")), dict(obs_stride=27)):
        assert call(**kw) == ARG, kw
    assert call() == NULL and call(max_iters=0) == NULL
    buf = (ctypes.c_float * 1024)()
    r = ctypes.c_void_p(ctypes.addressof(buf))                   # (compared against NULL only; a refusal dereferences nothing)
    assert call(pe=r, state_in=r) == ARG                          # pe together with state_in: before the NULL checks, before a launch
    assert call(pe=r, state_out=r) == NULL and call(state_in=r, state_out=r) == NULL
    if torch.cuda.device_count() == 0:
        full = dict(obs=r, action_out=r, info_out=r, consts_dev=r, state_in=r, state_out=r)
        for name in ("obs", "action_out", "info_out", "consts_dev"):
            assert call(**dict(full, **{name: None})) == NULL, name
        assert call(**dict(full, pe=r)) == ARG
        assert call(**full) not in (0, ARG, NULL)                 # complete arguments reach the launch, and fail there without a GPU


def test_iteration_classes_hold_a_third_of_the_converged_rows():
    """The rows the GPU file holds to EQUAL iteration counts (float64 residual outside [tol / 2, 2 tol] at every iterate): at least
    a third of the converging ones, on its 70 rows and on the fixture's first 70 states."""
    demand, pe = opf64.fixture_rows()
    iters, conv, decisive = opf64.iteration_classes(demand, pe, TOL)
    ref = opf64.solve_many(demand.astype(np.float64), pe.astype(np.float64), tol=TOL, max_iters=40)
    assert np.array_equal(iters, ref["iters"]) and np.array_equal(conv, ref["converged"])
    first = opf64.fixture_states()
    _, conv0, decisive0 = opf64.iteration_classes(first[0][:70], first[1][:70], TOL)
    print("decisive: %d of %d converged (the GPU file's rows), %d of %d (the fixture's first 70)"
          % ((decisive & conv).sum(), conv.sum(), (decisive0 & conv0).sum(), conv0.sum()))
    assert conv.sum() == 65 and (decisive & conv).sum() * 3 >= conv.sum()
    assert conv0.sum() == 69 and (decisive0 & conv0).sum() * 3 >= conv0.sum()
