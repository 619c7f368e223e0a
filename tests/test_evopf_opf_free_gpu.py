"""``rpo_evopf_opf_free`` on the MI355X: the free-pe instance of the float32 AC-OPF kernel against the float64 yardstick
(tests/evopf_opf_free_f64.py) on observations of tests/golden/evopf_opf_free.npz, the isolation of its rows, its plumbing, the
fixed-pe kernel at the free optimum's pe, ``opf_gap(pe="free")`` and ``trainer.evaluate_opf`` end to end.

Observations: the fixture's first 65 plus its 5 infeasible ones (70 rows), in launches of n = 1, 3, 4, 5, 65 rows (one wave, a
ragged workgroup, a full one, one over -- the fifth row an infeasible state --, seventeen workgroups with a one-wave tail) and all
70.  Limits, from the issue's reasoning: the ``converged`` flags equal the helper's and the classes SLSQP's final equality residual
gives; a converged row has, re-evaluated in float64 with ``oracle.evopf``, max(|eq_resid|, excess over any of the 58 bounds) <=
2 tol, at most 25 iterations, an objective within 1e-4 (the stop tolerance; the helper's own stopping error is 1.2e-5) of the
float64 helper's and a ``cost`` within 1e-6 of float64 ``obj_fn`` of the returned point.  Every test prints the largest values it saw.

Largest values observed on the MI355X over all 384 observations of the fixture (tools/bench_opf.py --free,
profiles/opf_free_bench.json): 379 converged and 5 not, the classes of the fixture, with the helper's iteration count on every
observation (9..14); |objective - helper's| <= 2.3e-6; infeasibility of the returned points <= 9.7e-5 (the helper's own points:
9.8e-5); |returned cost - float64 obj_fn of the returned point| <= 1.2e-7.  On the 70 rows here: the fixed-pe kernel at the free
optimum's pe returns the free cost within 8.6e-6; ``opf_gap(pe="free")`` of a barely trained policy: 116 of 192 steps feasible
within 1e-3, gaps there 0.22 .. 18.7 in units of obj_fn; ``evaluate_opf`` at 4 x 24: all 96 steps converged, max |eq| 8.5e-5, no
inequality violated, step-0 reward 0.72 .. 2.5 above the idle-battery dispatch's.
"""
import functools

import numpy as np
import pytest
import torch

import evopf_opf_free_f64 as free64
from oracle import evopf as ev
from test_evopf_opf_free import TOL, classes, golden
from test_train_step_golden import build_trainer

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
SIZES = (1, 3, 4, 5, 65)


@functools.lru_cache(maxsize=None)
def _setup():
    """(env, obs [70, 57] f32 on the device, judged feasible, left out, the helper's results on the float32 observations) --
    computed once, shared and left unchanged by the tests."""
    from rpo_amd.env import EVOPFEnv
    assert torch.cuda.is_available()
    feas, infeas, other = classes(golden())
    rows, obs = free64.fixture_rows()
    assert infeas[rows].sum() == 5 and infeas[rows][65:].all()
    ref = free64.solve_free_many(obs.astype(np.float64), tol=TOL, max_iters=40)
    return EVOPFEnv(device=DEV), torch.tensor(obs, device=DEV), feas[rows], other[rows], ref


def _bits(res):
    return res.action.clone(), res.info.clone()


def _same(a, b):
    """bitwise, NaNs included"""
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


@pytest.mark.parametrize("n", SIZES + (70,))
def test_against_the_float64_yardstick(n):
    env, obs, feas, other, ref = _setup()
    sel = np.arange(n) if n != 5 else np.array([0, 1, 2, 3, 65])            # (n = 5: the row beyond the workgroup is an infeasible one)
    res = env.opf(obs[sel], pe="free", tol=TOL, max_iters=40)
    out = res.numpy()
    o64 = obs[sel].cpu().numpy().astype(np.float64)
    judged = ~other[sel]
    assert np.array_equal(out["converged"][judged], feas[sel][judged])
    assert np.array_equal(out["converged"][judged], ref["converged"][sel][judged])
    conv = out["converged"] & judged
    if n >= 65:
        assert conv.sum() >= 64 and (n == 65 or (~out["converged"]).sum() == 5)
    a = out["action"][conv].astype(np.float64)
    infeasibility = free64.infeasibility(o64[conv], a)
    own = free64.infeasibility(o64[conv], ref["action"][sel][conv])
    dev = out["objective"][conv] - ref["objective"][sel][conv]
    dev64 = free64.objective(o64[conv], a) - ref["objective"][sel][conv]
    if conv.any():
        print("n=%d: iterations %d..%d (helper %d..%d), infeasibility <= %.3g (helper's points: %.3g), |objective - helper| <= %.3g "
              "(float64 objective of the point: %.3g), |cost - f64 obj_fn| <= %.3g"
              % (n, out["iters"][conv].min(), out["iters"][conv].max(), ref["iters"][sel][conv].min(), ref["iters"][sel][conv].max(),
                 infeasibility.max(), own.max(), np.abs(dev).max(), np.abs(dev64).max(), np.abs(out["cost"][conv] - ev.obj_fn(a)).max()))
    assert np.isfinite(out["action"][conv]).all() and (out["residual"][conv] < TOL).all()
    assert (infeasibility <= 2 * TOL).all()
    assert (out["iters"][conv] <= 25).all()
    assert (np.abs(dev) <= 1e-4).all()
    assert (np.abs(out["cost"][conv] - ev.obj_fn(a)) <= 1e-6).all()
    assert (out["action"][:, 24] == np.float32(ev.GRID.slack_va[0])).all()
    assert (out["iters"][~out["converged"]] == 40).all()
    assert np.array_equal(out["pe_cost"], np.repeat(np.float32(5.0) * obs[sel].cpu().numpy()[:, 33:34], 5, axis=1))


def test_rows_do_not_depend_on_their_neighbours():
    env, obs, feas, other, ref = _setup()
    base = _bits(env.opf(obs, pe="free"))
    assert _same(base, _bits(env.opf(obs, pe="free")))                       # two calls
    perm = torch.tensor(np.random.default_rng(0).permutation(70), device=DEV)
    shuffled = _bits(env.opf(obs[perm], pe="free"))
    assert _same((base[0][perm], base[1][perm]), shuffled)                  # a permutation of the rows permutes the outputs
    # the 5 infeasible states interleaved with feasible ones, every workgroup of four holding one or two of them
    good = np.nonzero(feas)[0][:10]
    bad = np.nonzero(~feas & ~other)[0]
    mixed = np.array([good[0], bad[0], good[1], good[2], bad[1], good[3], bad[2], good[4], good[5], good[6], bad[3], good[7],
                      good[8], bad[4], good[9]])
    m = torch.tensor(mixed, device=DEV)
    assert _same((base[0][m], base[1][m]), _bits(env.opf(obs[m], pe="free")))
    g = torch.tensor(good, device=DEV)
    assert _same((base[0][g], base[1][g]), _bits(env.opf(obs[g], pe="free")))
    print("70 rows: two calls, a permutation, 5 infeasible rows interleaved: same bits")


def test_plumbing():
    env, obs, feas, other, ref = _setup()
    n = 9
    base = _bits(env.opf(obs[:n], pe="free"))
    # pe_cost=None is the explicit (we / wg) * price tensor
    explicit = ((env.we / env.wg) * obs[:n, 33:34]).expand(-1, 5).contiguous()
    assert _same(base, _bits(env.opf(obs[:n], pe="free", pe_cost=explicit)))
    other_cost = env.opf(obs[:n], pe="free", pe_cost=-explicit)
    assert not torch.equal(other_cost.action[:, 38:], base[0][:, 38:])       # ... and the cost is read: its sign moves pe
    # strided observation rows: a column slice of a wider tensor
    wide = torch.full((n, 100), float("nan"), device=DEV)
    wide[:, 7:64] = obs[:n]
    assert not wide[:, 7:64].is_contiguous() and _same(base, _bits(env.opf(wide[:, 7:64], pe="free")))
    # out= reuse, and outputs prefilled with NaN are fully overwritten
    out = env.opf(obs[n:2 * n], pe="free")
    out.action.fill_(float("nan"))
    out.info.fill_(float("nan"))
    again = env.opf(obs[:n], pe="free", out=out)
    assert again is out and _same(base, _bits(out)) and not torch.isnan(out.action).any() and not torch.isnan(out.info).any()
    # max_iters = 0: the flat start with pe at the middle of its box, not converged
    flat = env.opf(obs[:n], pe="free", max_iters=0).numpy()
    want = np.stack([free64.flat_start(o) for o in obs[:n].cpu().numpy().astype(np.float64)])
    print("flat start: |action - float64 flat start| <= %.3g" % np.abs(flat["action"] - want).max())
    assert not flat["converged"].any() and (flat["iters"] == 0).all() and np.abs(flat["action"] - want).max() <= 1e-6
    assert np.isfinite(flat["residual"]).all() and (flat["residual"] > TOL).all()
    assert np.abs(flat["cost"] - ev.obj_fn(want)).max() <= 1e-6


def test_an_empty_battery_box_ends_not_converged():
    env, obs, feas, other, ref = _setup()
    n = 9
    base = _bits(env.opf(obs[:n], pe="free"))
    broken = obs[:n].clone()
    broken[5, 28:33] = 2.0                                        # far above B_HIGH: p_max < p_min
    hi, lo = ev.battery_bounds(np.full(5, 2.0))
    assert (hi < lo).all()
    got = env.opf(broken, pe="free")
    host = got.numpy()
    print("empty box: converged %s, iterations %d, residual %.3g" % (host["converged"][5], host["iters"][5], host["residual"][5]))
    assert not host["converged"][5] and host["iters"][5] == 40
    keep = torch.tensor([0, 1, 2, 3, 4, 6, 7, 8], device=DEV)
    assert _same((base[0][keep], base[1][keep]), (got.action[keep], got.info[keep]))


def test_the_fixed_pe_kernel_agrees_at_the_free_optimum():
    env, obs, feas, other, ref = _setup()
    res = env.opf(obs, pe="free")
    fixed = env.opf(obs, pe=res.action[:, 38:].contiguous()).numpy()
    zero = env.opf(obs, pe=None).numpy()
    out = res.numpy()
    conv = out["converged"]
    assert fixed["converged"][conv].all()
    dev = np.abs(fixed["cost"][conv].astype(np.float64) - out["cost"][conv])
    hi, lo = ev.battery_bounds(obs.cpu().numpy().astype(np.float64)[:, 28:33])
    both = conv & zero["converged"] & (lo <= 0).all(axis=1) & (hi >= 0).all(axis=1)
    over = out["objective"][both].astype(np.float64) - zero["cost"][both]
    print("|fixed-pe cost at pe* - free cost| <= %.3g on %d rows; free objective - objective at pe = 0 <= %.3g on %d rows (mean %.3g)"
          % (dev.max(), conv.sum(), over.max(), both.sum(), over.mean()))
    assert (dev <= 1e-4).all()
    # (a state of charge of exactly B_LOW or B_HIGH rounds to float32 on either side: 0 is then in the box or a hair outside)
    assert both.sum() >= 30 and (over <= 1e-4).all()


@functools.lru_cache(maxsize=None)
def _trainer():
    from rpo_amd import ops
    torch.manual_seed(5)
    tr = build_trainer("ddpg", "evopf256", ops, DEV, num_envs=16, use_graph=False)
    tr.vec.reset()
    return tr


def _state(tr):
    v = tr.vec
    return [t.clone() for t in (v.ctrl, v.internal, v.obs, v.ep_len, v.ep_ret, v.ep_count, tr.policy_params(), tr.agent.flat.data,
                                tr.buffer.rows)]


def test_opf_gap_free_end_to_end():
    tr = _trainer()
    tj = tr.evaluate(8, record=True, seed=0).trajectory
    gap = tj.opf_gap(tr.base_env, tol=TOL, max_iters=40, pe="free")
    assert gap.gap.shape == tj.valid.shape and tj.valid.sum() >= 8
    assert np.array_equal(np.isnan(gap.gap), ~(gap.converged & tj.valid)) and not gap.converged[~tj.valid].any()
    assert np.isfinite(gap.cost_policy[tj.valid]).all() and np.array_equal(np.isnan(gap.cost_policy), ~tj.valid)
    judged = gap.converged & tj.valid & (gap.violation <= 1e-3)
    print("opf_gap(pe='free'): converged %.3f of %d steps, %d steps with a policy action feasible within 1e-3, gap there in [%.4g, %.4g]; "
          "all converged steps: [%.4g, %.4g]" % (gap.converged_rate(), tj.valid.sum(), judged.sum(),
                                                 gap.gap[judged].min() if judged.any() else np.nan,
                                                 gap.gap[judged].max() if judged.any() else np.nan, np.nanmin(gap.gap), np.nanmax(gap.gap)))
    assert (gap.gap[judged] >= -1e-4).all()                      # the free optimum is no worse than any feasible action
    # a step's entries are the single calls' values
    e, s = (int(x) for x in np.argwhere(gap.converged)[0])
    o = torch.tensor(tj.obs[e, s][None], device=DEV)
    single = tr.base_env.opf(o, pe="free")
    assert gap.cost_opt[e, s] == np.float64(single.objective.cpu().numpy()[0])
    assert gap.gap[e, s] == gap.cost_policy[e, s] - gap.cost_opt[e, s]


def _hand_loop(tr, n, H, seed, pe):
    """evaluate_opf written out: env.opf on the env's observation rows, the env step, the accumulators."""
    from rpo_amd.algo.evaluation import EvalResult, _initial_env
    env, k = tr.base_env, tr.kernels
    v = _initial_env(tr, n, seed, None)
    acc = torch.zeros(n, 8, device=DEV)
    rows = torch.zeros(n, k.ring_floats, device=DEV)
    iters = torch.zeros(n, dtype=torch.int32, device=DEV)
    log = []
    for i in range(H):
        r = env.opf(v.obs, pe="free" if pe == "free" else None)
        v.action.copy_(r.action)
        iters.copy_(r.info[:, 2])
        log.append(r.info.clone())
        v.step(v.action, rows=rows, cap_steps=1, auto_reset=False)
        tr.backend.eval_accumulate(rows, k.cols, iters, i, v.viol_thresh, acc)
    return EvalResult(acc.cpu().numpy(), "opf", H, seed), torch.stack(log, dim=1).cpu().numpy()


@pytest.mark.parametrize("n,H", [(5, 4), (4, 24)])
def test_evaluate_opf(n, H):
    tr = _trainer()
    before = _state(tr)
    res = tr.evaluate_opf(n, seed=3, horizon=H, record=True, constraints=True)
    assert res.path == "opf" and res.episodes == n and res.horizon == H and (res.length == H).all() and not res.nonfinite.any()
    hand, log = _hand_loop(tr, n, H, 3, "free")
    for f in res.FIELDS:
        assert np.array_equal(getattr(res, f), getattr(hand, f)), f                       # bitwise: the same launches
    assert np.array_equal(res.opf_iters, log[:, :, 2].astype(np.int32)) and np.array_equal(res.opf_converged, log[:, :, 3] > 0.5)
    assert np.array_equal(res.proj_iters, res.opf_iters.sum(axis=1))
    again = tr.evaluate_opf(n, seed=3, horizon=H)                                           # the same seed reproduces itself,
    for f in res.FIELDS:                                                                    # with and without record / constraints
        assert np.array_equal(getattr(res, f), getattr(again, f)), f
    assert again.trajectory is None and np.array_equal(again.opf_iters, res.opf_iters)
    tj = res.trajectory
    policy = tr.evaluate(n, seed=3, horizon=H, record=True).trajectory
    assert np.array_equal(tj.obs[:, 0], policy.obs[:, 0])                                  # evaluate()'s episodes: the same day, the same soc,
    assert np.array_equal(tj.obs[:, :, :28], policy.obs[:, :, :28]) and np.array_equal(tj.obs[:, :, 33:], policy.obs[:, :, 33:])
    assert np.array_equal(tj.proposal, tj.action[:, :, tr.base_env.partial_actions]) and np.array_equal(tj.iters, res.opf_iters)
    conv = res.opf_converged
    print("evaluate_opf %d x %d: converged %d of %d steps, iterations %d..%d, on converged steps max_eq <= %.3g, max_ineq <= %.3g; "
          "return %.4f (policy's %.4f)" % (n, H, conv.sum(), conv.size, res.opf_iters.min(), res.opf_iters.max(), tj.eq[conv].max(),
                                           tj.ineq[conv].max(), res.ret.mean(), policy.reward.sum(axis=1).mean()))
    assert conv.any()
    assert (tj.eq[conv] <= 2 * TOL).all() and (tj.ineq[conv] <= 2 * TOL).all()
    assert np.array_equal(res.constraints.eq_max.max(axis=1), res.max_eq)
    # the idle-battery dispatch, and the first step's reward against it
    zero = tr.evaluate_opf(n, seed=3, horizon=H, pe="zero", record=True)
    hand0, _ = _hand_loop(tr, n, H, 3, "zero")
    for f in zero.FIELDS:
        assert np.array_equal(getattr(zero, f), getattr(hand0, f)), f
    assert (zero.trajectory.action[:, :, 38:] == 0).all()
    both = conv[:, 0] & zero.opf_converged[:, 0]
    diff = tj.reward[:, 0].astype(np.float64) - zero.trajectory.reward[:, 0]
    print("step 0: reward(free) - reward(zero) in [%.4g, %.4g] on %d episodes" % (diff[both].min(), diff[both].max(), both.sum()))
    assert both.any() and (diff[both] >= -tr.base_env.wg * 1e-4).all()
    # init_states are honoured
    init = torch.tensor(policy.obs[:, 1], device=DEV)
    init[:, 28:33] = 0.5
    injected = tr.evaluate_opf(n, seed=3, horizon=2, init_states=init, record=True)
    assert np.array_equal(injected.trajectory.obs[:, 0], init.cpu().numpy())
    torch.cuda.synchronize()
    for x, y in zip(before, _state(tr)):
        assert torch.equal(x, y)                                 # networks, env lanes, ctrl and replay: bitwise unchanged
