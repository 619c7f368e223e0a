"""``rpo_evopf_opf`` on the MI355X: the float32 kernel against the float64 yardstick (tests/evopf_opf_f64.py) on states of
tests/golden/evopf_opf.npz, the isolation of its rows, its plumbing, and ``opf_gap`` / ``opt_solve`` end to end.

States: the fixture's first 65 plus its 5 infeasible ones (70 rows), in launches of n = 1, 3, 4, 5, 65 rows (one wave, a ragged
workgroup, a full one, one over, seventeen workgroups with a one-wave tail) and all 70.  Limits, from the issue's reasoning: the
``converged`` flags equal the classes SLSQP's final equality residual gives (< 1e-6 feasible, > 1e-3 infeasible, at most 2 % in
between, which are left out); a converged row has, re-evaluated in float64 with ``oracle.evopf``, max(|eq_resid|, bound excess)
<= 2 tol (tol plus the float32 rounding of 14-term flows with |Y| <= 40, about 7e-5), at most 25 iterations, and a cost within
1e-4 (the stop tolerance) of the float64 helper's.

Largest values observed on the MI355X over all 384 states of the fixture (tools/bench_opf.py, profiles/opf_bench.json): 379
converged and 5 not, the classes of the fixture, with the helper's iteration counts (9..12); |cost - helper's| <= 1.2e-6;
infeasibility of the returned points <= 8.9e-5 (the helper's own points: 8.9e-5); |returned cost - float64 obj_fn of the returned
point| <= 1.2e-7.  The float32 Hessian, formed in the kernel, changed no iteration count against the float64 helper.
"""
import functools
import os

import numpy as np
import pytest
import torch

import evopf_opf_f64 as opf64
from oracle import evopf as ev
from test_evopf_opf import AMBIG_CAP, GOLDEN, TOL, classes
from test_train_step_golden import build_trainer

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
SIZES = (1, 3, 4, 5, 65)


@functools.lru_cache(maxsize=None)
def _setup():
    """(env, rows, demand [70, 28] f32, pe [70, 5] f32, judged feasible, left out, the helper's results) -- computed once, shared
    and left unchanged by the tests."""
    from rpo_amd.env import EVOPFEnv
    assert torch.cuda.is_available()
    with np.load(GOLDEN) as z:
        z = {k: z[k] for k in z.files}
    feas, infeas, other = classes(z)
    rows = np.concatenate([np.arange(65), np.setdiff1d(np.nonzero(infeas)[0], np.arange(65))])
    assert len(rows) == 70 and infeas[rows].sum() == 5 and other[rows].mean() <= AMBIG_CAP
    demand, pe = z["demand"][rows].astype(np.float32), z["pe"][rows].astype(np.float32)
    ref = opf64.solve_many(demand.astype(np.float64), pe.astype(np.float64), tol=TOL, max_iters=40)
    env = EVOPFEnv(device=DEV)
    return env, rows, torch.tensor(demand, device=DEV), torch.tensor(pe, device=DEV), feas[rows], other[rows], ref


def _bits(res):
    return res.action.clone(), res.info.clone()


def _same(a, b):
    """bitwise, NaNs included"""
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


@pytest.mark.parametrize("n", SIZES + (70,))
def test_against_the_float64_yardstick(n):
    env, rows, demand, pe, feas, other, ref = _setup()
    sel = np.arange(n) if n != 5 else np.array([0, 1, 2, 3, 67])           # (n = 5: the row beyond the workgroup is an infeasible one)
    out = env.opf(demand[sel], pe=pe[sel], tol=TOL, max_iters=40).numpy()
    judged = ~other[sel]
    assert np.array_equal(out["converged"][judged], feas[sel][judged])
    assert np.array_equal(out["converged"][judged], ref["converged"][sel][judged])
    conv = out["converged"] & judged
    if n >= 65:
        assert conv.sum() >= 64 and (n == 65 or (~out["converged"]).sum() == 5)
    a = out["action"][conv].astype(np.float64)
    infeasibility = opf64.infeasibility(demand[sel].cpu().numpy()[conv], a)
    own = opf64.infeasibility(demand[sel].cpu().numpy()[conv], ref["action"][sel][conv])
    dev = out["cost"][conv] - ref["cost"][sel][conv]
    if conv.any():
        print("n=%d: iterations %d..%d, infeasibility <= %.3g (helper's points: %.3g), |cost - helper| <= %.3g, |cost - f64 obj_fn| <= %.3g"
              % (n, out["iters"][conv].min(), out["iters"][conv].max(), infeasibility.max(), own.max(), np.abs(dev).max(),
                 np.abs(out["cost"][conv] - ev.obj_fn(a)).max()))
    assert np.isfinite(out["action"][conv]).all() and (out["residual"][conv] < TOL).all()
    assert (infeasibility <= 2 * TOL).all()
    assert (out["iters"][conv] <= 25).all()
    assert (np.abs(dev) <= 1e-4).all()
    # the 43-vector is complete: slack angle and pe as given
    assert np.array_equal(out["action"][:, 38:], pe[sel].cpu().numpy()) and (out["action"][:, 24] == np.float32(ev.GRID.slack_va[0])).all()
    assert (out["iters"][~out["converged"]] == 40).all()


def test_rows_do_not_depend_on_their_neighbours():
    env, rows, demand, pe, feas, other, ref = _setup()
    base = _bits(env.opf(demand, pe=pe))
    assert _same(base, _bits(env.opf(demand, pe=pe)))                       # two calls
    perm = torch.tensor(np.random.default_rng(0).permutation(70), device=DEV)
    shuffled = _bits(env.opf(demand[perm], pe=pe[perm]))
    assert _same((base[0][perm], base[1][perm]), shuffled)                  # a permutation of the rows permutes the outputs
    # the 5 infeasible states interleaved with feasible ones, every workgroup of four holding one or two of them
    good = np.nonzero(feas)[0][:10]
    bad = np.nonzero(~feas & ~other)[0]
    mixed = np.array([good[0], bad[0], good[1], good[2], bad[1], good[3], bad[2], good[4], good[5], good[6], bad[3], good[7],
                      good[8], bad[4], good[9]])
    m = torch.tensor(mixed, device=DEV)
    got = _bits(env.opf(demand[m], pe=pe[m]))
    assert _same((base[0][m], base[1][m]), got)
    alone = _bits(env.opf(demand[torch.tensor(good, device=DEV)], pe=pe[torch.tensor(good, device=DEV)]))
    assert _same((base[0][good], base[1][good]), alone)


def test_plumbing():
    env, rows, demand, pe, feas, other, ref = _setup()
    n = 9
    base = _bits(env.opf(demand[:n], pe=pe[:n]))
    # strided observation rows: a column slice of a wider tensor, and full observations
    wide = torch.full((n, 100), float("nan"), device=DEV)
    wide[:, 7:35] = demand[:n]
    assert not wide[:, 7:35].is_contiguous() and _same(base, _bits(env.opf(wide[:, 7:35], pe=pe[:n])))
    obs = torch.cat([demand[:n], torch.full((n, 29), float("nan"), device=DEV)], dim=1)
    assert _same(base, _bits(env.opf(obs, pe=pe[:n])))
    # pe=None equals zeros
    zero = _bits(env.opf(demand[:n], pe=torch.zeros(n, 5, device=DEV)))
    assert _same(zero, _bits(env.opf(demand[:n])))
    # out= reuse, and outputs prefilled with NaN are fully overwritten
    out = env.opf(demand[n:2 * n], pe=pe[n:2 * n])
    out.action.fill_(float("nan"))
    out.info.fill_(float("nan"))
    again = env.opf(demand[:n], pe=pe[:n], out=out)
    assert again is out and _same(base, _bits(out)) and not torch.isnan(out.action).any() and not torch.isnan(out.info).any()
    # max_iters = 0: the flat start, not converged
    flat = env.opf(demand[:n], pe=pe[:n], max_iters=0).numpy()
    want = np.stack([opf64.flat_start(p) for p in pe[:n].cpu().numpy().astype(np.float64)])
    assert not flat["converged"].any() and (flat["iters"] == 0).all() and np.abs(flat["action"] - want).max() <= 1e-6
    assert np.isfinite(flat["residual"]).all() and (flat["residual"] > TOL).all()
    assert np.abs(flat["cost"] - ev.obj_fn(want)).max() <= 1e-6


@functools.lru_cache(maxsize=None)
def _trainer():
    from rpo_amd import ops
    torch.manual_seed(5)
    tr = build_trainer("ddpg", "evopf256", ops, DEV, num_envs=16, use_graph=False)
    tr.vec.reset()
    return tr


def _state(tr):
    v = tr.vec
    return [t.clone() for t in (v.ctrl, v.internal, v.obs, v.ep_len, v.ep_ret, v.ep_count)]


def test_opf_gap_end_to_end_and_purity():
    env, rows, demand, pe, feas, other, ref = _setup()
    tr = _trainer()
    res = tr.evaluate(8, record=True, seed=0)
    tj = res.trajectory
    before = _state(tr)
    gap = tj.opf_gap(tr.base_env, tol=TOL, max_iters=40)
    direct = tr.base_env.opf(tr.vec.obs, pe=None)
    torch.cuda.synchronize()
    for x, y in zip(before, _state(tr)):
        assert torch.equal(x, y)                                             # ctrl word and env state: bitwise unchanged
    assert direct.action.shape == (16, 43)
    assert gap.gap.shape == tj.valid.shape and tj.valid.sum() >= 8
    assert np.array_equal(np.isnan(gap.gap), ~(gap.converged & tj.valid)) and not gap.converged[~tj.valid].any()
    assert np.isfinite(gap.cost_policy[tj.valid]).all() and np.array_equal(np.isnan(gap.cost_policy), ~tj.valid)
    print("opf_gap: converged %.3f, mean gap %.4g, median %.4g" % (gap.converged_rate(), gap.mean(), gap.quantile(0.5)))
    idx = np.argwhere(tj.valid)
    picks = [tuple(idx[k]) for k in np.linspace(0, len(idx) - 1, 6).astype(int)]
    o =torch.tensor(np.stack([tj.obs[e, s] for e, s in picks]), device=DEV)
    a = torch.tensor(np.stack([tj.action[e, s] for e, s in picks]), device=DEV)
    single = env.opf(o, pe=a[:, 38:].contiguous()).numpy()
    policy = env.obj_fn(a).cpu().numpy()
    for k, (e, s) in enumerate(picks):
        assert abs(gap.cost_policy[e, s] - policy[k]) <= 1e-6 * abs(policy[k])     # (obj_fn: a float32 sum of ten terms in torch)
        assert bool(gap.converged[e, s]) == bool(single["converged"][k])
        if single["converged"][k]:
            assert gap.cost_opt[e, s] == np.float64(single["cost"][k])
            assert gap.gap[e, s] == (gap.cost_policy[e, s] - gap.cost_opt[e, s]) / gap.cost_opt[e, s]


def test_opt_solve():
    env, rows, demand, pe, feas, other, ref = _setup()
    X = demand[:12].cpu().numpy()
    Y, total, each = env.opt_solve(X)
    want = env.opf(demand[:12]).numpy()
    assert Y.shape == (12, 38) and isinstance(total, float) and isinstance(each, float) and total > 0 and each > 0
    conv = want["converged"]
    assert conv.any() and np.array_equal(Y[conv], want["action"][conv][:, :38].astype(np.float64)) and np.isnan(Y[~conv]).all()
