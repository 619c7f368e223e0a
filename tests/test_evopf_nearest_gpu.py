"""``rpo_evopf_nearest`` on the MI355X: the safety filter -- the nearest-feasible instance of the float32 interior-point kernel --
against the float64 yardstick (tests/evopf_nearest_f64.py) on the 70 rows and three families of targets of
tests/golden/evopf_nearest.npz, the isolation of its rows, its plumbing, the containment of NaNs, and
``trainer.evaluate_filtered`` end to end.

Limits, from the issue's reasoning, none of them measured in advance: at tol = 1e-4 and max_iters = 40 the converged set equals the
helper's (the fixture's 65 feasible rows); a converged row is finite, has residual < tol and at most 25 iterations (the helper:
8..10), a float64 infeasibility <= 2 tol (``evopf_opf_free_f64.infeasibility``) and a distance within
1e-4 + |lambda_helper|_inf * |eq_resid_64(y_gpu)|_1 of the helper's: the stop tolerance plus the first-order value of the returned
point's own equality error; a row that does not converge stops at 40 iterations.  On the already feasible targets (family c) the
distance is within that allowance of 0, and no controlled component moves by more than four times the helper's own worst ``moved``
on that family (the factor: a float32 stop one iteration earlier or later).  Every test prints the largest values it saw;
tools/bench_nearest.py writes them into profiles/nearest_bench.json.

Largest values observed on the MI355X (profiles/nearest_bench.json): on every family 65 rows converged and 5 not, with the helper's
iteration count on every row (8..10); residual <= 9.9e-5, infeasibility <= 9.4e-6, |distance - helper's| <= 9.1e-6 against an
allowance >= 1.0e-4; feasible targets: distance <= 2.8e-5, moved <= 5.21e-3 half-widths (the helper's own 5.20e-3, bound 2.08e-2);
pe weights x 100: the sum of moved over pe falls by 3.9e-3 .. 0.71 on all 65 rows; ``evaluate_filtered`` at 8 x 24: all 192 steps
converged in 7..9 iterations, max |eq| 7.6e-6 and no bound exceeded, where the untrained actor's own actions violate 2 tol on 91 %
of the steps.
"""
import functools

import numpy as np
import pytest
import torch

import evopf_nearest_f64 as near64
import evopf_opf_free_f64 as free64
from oracle import evopf as ev
from test_evopf_nearest import FEASIBLE, PARTIAL, TOL, golden
from test_train_step_golden import build_trainer

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
FAMILIES = near64.FAMILIES


@functools.lru_cache(maxsize=None)
def _setup():
    """(env, obs [70, 57] f32 on the device, {family: target [70, 14] f32 on the device}, {family: the helper's results on the
    float32 observations and targets}) -- computed once, shared and left unchanged by the tests."""
    from rpo_amd.env import EVOPFEnv
    assert torch.cuda.is_available()
    z = golden()
    obs = z["obs"]
    t32 = {f: z["target_" + f].astype(np.float32) for f in FAMILIES}
    ref = {f: near64.solve_nearest_many(obs.astype(np.float64), t32[f].astype(np.float64), tol=TOL, max_iters=40) for f in FAMILIES}
    for f in FAMILIES:
        assert np.array_equal(ref[f]["converged"], FEASIBLE)
    return EVOPFEnv(device=DEV), torch.tensor(obs, device=DEV), {f: torch.tensor(t32[f], device=DEV) for f in FAMILIES}, ref


def _allowance(o64, action, lam):
    """1e-4 + |lambda_helper|_inf * |eq_resid_64(y_gpu)|_1, per row."""
    eq = ev.eq_resid(o64, np.asarray(action, dtype=np.float64))
    return 1e-4 + np.abs(lam).max(axis=1) * np.abs(eq).sum(axis=1)


def _bits(res):
    return res.action.clone(), res.info.clone()


def _same(a, b):
    """bitwise, NaNs included"""
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("n", (65, 70))
def test_against_the_float64_yardstick(n, family):
    env, obs, targets, refs = _setup()
    ref = refs[family]
    res = env.nearest_feasible(obs[:n], targets[family][:n], tol=TOL, max_iters=40)
    out = res.numpy()
    o64 = obs[:n].cpu().numpy().astype(np.float64)
    conv = out["converged"]
    a = out["action"][conv].astype(np.float64)
    infeasibility = free64.infeasibility(o64[conv], a) if conv.any() else np.zeros(0)
    dev = np.abs(out["distance"][conv] - ref["distance"][:n][conv])
    allow = _allowance(o64[conv], a, ref["lam"][:n][conv])
    differ = (out["iters"][conv] != ref["iters"][:n][conv]).sum()
    if conv.any():
        print("n=%d %s: converged %d, iterations %d..%d (helper %d..%d; %d rows differ), residual <= %.3g, infeasibility <= %.3g, "
              "|distance - helper| <= %.3g (allowance >= %.3g, worst ratio %.3g)"
              % (n, family, conv.sum(), out["iters"][conv].min(), out["iters"][conv].max(), ref["iters"][:n][conv].min(),
                 ref["iters"][:n][conv].max(), differ, out["residual"][conv].max(), infeasibility.max(), dev.max(), allow.min(),
                 (dev / allow).max()))
    assert np.array_equal(conv, ref["converged"][:n]) and np.array_equal(conv, FEASIBLE[:n])
    assert np.isfinite(out["action"][conv]).all() and np.isfinite(out["distance"][conv]).all() and (out["residual"][conv] < TOL).all()
    assert (out["iters"][conv] <= 25).all()
    assert (out["iters"][~conv] == 40).all()
    assert (infeasibility <= 2 * TOL).all()
    assert (dev <= allow).all()
    assert (out["action"][:, 24] == np.float32(ev.GRID.slack_va[0])).all()
    assert np.array_equal(out["target"], targets[family][:n].cpu().numpy())


def test_feasible_targets_stay_put():
    env, obs, targets, refs = _setup()
    ref = refs["feasible"]
    out = env.nearest_feasible(obs, targets["feasible"], tol=TOL, max_iters=40).numpy()
    o64 = obs.cpu().numpy().astype(np.float64)
    conv = out["converged"]
    assert np.array_equal(conv, FEASIBLE)
    own = near64.moved(o64[conv], ref["action"][conv], targets["feasible"].cpu().numpy().astype(np.float64)[conv]).max()
    allow = _allowance(o64[conv], out["action"][conv], ref["lam"][conv])
    print("feasible targets: distance <= %.3g (allowance >= %.3g), moved <= %.3g half-widths (helper's own: %.3g, bound %.3g)"
          % (out["distance"][conv].max(), allow.min(), out["moved"][conv].max(), own, 4 * own))
    assert (out["distance"][conv] <= allow).all()
    assert out["moved"][conv].max() <= 4 * own
    # moved is |y - t| / half-width, in float64 from the returned point
    want = near64.moved(o64[conv], out["action"][conv], out["target"][conv])
    assert np.allclose(out["moved"][conv], want, rtol=1e-4, atol=1e-6)


def test_rows_do_not_depend_on_their_neighbours():
    env, obs, targets, refs = _setup()
    t = targets["uniform"]
    base = _bits(env.nearest_feasible(obs, t))
    assert _same(base, _bits(env.nearest_feasible(obs, t)))                 # two calls
    perm = torch.tensor(np.random.default_rng(0).permutation(70), device=DEV)
    assert _same((base[0][perm], base[1][perm]), _bits(env.nearest_feasible(obs[perm], t[perm])))
    # sub-batches ragged against four rows per workgroup; the fifth row of the last one is an infeasible observation
    for sel in ([7], [0, 1, 2], [3, 4, 5, 6], [0, 1, 2, 3, 65], [64, 66, 10]):
        s = torch.tensor(sel, device=DEV)
        assert _same((base[0][s], base[1][s]), _bits(env.nearest_feasible(obs[s], t[s]))), sel
    # a view of a wider tensor: row stride > 57, and a target view with row stride > 43
    wide = torch.full((70, 100), float("nan"), device=DEV)
    wide[:, 7:64] = obs
    twide = torch.full((70, 64), float("nan"), device=DEV)
    twide[:, 3:46] = 0.0
    twide[:, 3:46].index_copy_(1, torch.tensor(PARTIAL, device=DEV), t)
    assert not wide[:, 7:64].is_contiguous() and _same(base, _bits(env.nearest_feasible(wide[:, 7:64], twide[:, 3:46])))
    print("70 rows: two calls, a permutation, sub-batches of 1, 3, 4, 5 rows, strided views: same bits")


def test_plumbing():
    from rpo_amd.algo import ActResult
    env, obs, targets, refs = _setup()
    n = 65
    t = targets["uniform"][:n]
    first = env.nearest_feasible(obs[:n], t)
    base = _bits(first)
    # [n, 14], [n, 43] and an ActResult: the same bits (the other 29 components are not read)
    full = torch.full((n, 43), float("nan"), device=DEV)
    full[:, torch.tensor(PARTIAL, device=DEV)] = t
    assert _same(base, _bits(env.nearest_feasible(obs[:n], full)))
    act = ActResult(full, t, torch.zeros(n, dtype=torch.int32, device=DEV))
    assert _same(base, _bits(env.nearest_feasible(obs[:n], act)))
    # an explicit weight table with the default's formula: within the yardstick's allowance of the helper
    lo, hi = env.update(obs[:n])
    w = 1.0 / (0.5 * (hi - lo)) ** 2
    o64 = obs[:n].cpu().numpy().astype(np.float64)
    ref = refs["uniform"]
    explicit = env.nearest_feasible(obs[:n], t, weight=w).numpy()
    allow = _allowance(o64, explicit["action"], ref["lam"][:n])
    dev = np.abs(explicit["distance"] - ref["distance"][:n])
    print("explicit default weights: |distance - helper| <= %.3g (allowance >= %.3g); against weight=None: %.3g"
          % (dev.max(), allow.min(), np.abs(explicit["distance"] - first.numpy()["distance"]).max()))
    assert explicit["converged"].all() and (dev <= allow).all()
    one_row = env.nearest_feasible(obs[:n], t, weight=torch.full((14,), 3.0, device=DEV))
    per_row = env.nearest_feasible(obs[:n], t, weight=torch.full((n, 14), 3.0, device=DEV))
    assert _same(_bits(one_row), _bits(per_row)) and not _same(_bits(one_row), base)
    # the batteries a hundred times dearer: they move less
    heavy_w = w.clone()
    heavy_w[:, 9:] *= 100.0
    heavy = env.nearest_feasible(obs[:n], t, weight=heavy_w)
    both = (heavy.converged & first.converged).cpu().numpy()
    before, after = first.moved[:, 9:].sum(dim=1).cpu().numpy()[both], heavy.moved[:, 9:].sum(dim=1).cpu().numpy()[both]
    print("pe weights x 100: sum of moved over pe changes by %.3g .. %.3g on %d rows" % ((after - before).min(), (after - before).max(), both.sum()))
    assert both.any() and (after <= before).all() and (after < before).any()
    # max_iters = 0: the flat start, not converged, with a finite residual above tol
    flat = env.nearest_feasible(obs[:n], t, max_iters=0).numpy()
    want = np.stack([free64.flat_start(o) for o in o64])
    assert not flat["converged"].any() and (flat["iters"] == 0).all() and np.abs(flat["action"] - want).max() <= 1e-6
    assert np.isfinite(flat["residual"]).all() and (flat["residual"] > TOL).all()
    # out= reuse: nothing is left of an earlier infeasible row
    out = env.nearest_feasible(obs[5:70], targets["uniform"][5:70])
    assert not out.converged[-5:].any()
    for buf in (out.action, out.info, out.target, out.moved):
        buf.fill_(float("nan"))
    again = env.nearest_feasible(obs[:n], t, out=out)
    assert again is out and _same(base, _bits(out)) and torch.equal(out.moved, first.moved) and torch.equal(out.target, t)
    assert not any(torch.isnan(b).any() for b in (out.action, out.info, out.target, out.moved))


def test_a_nan_stays_in_its_row():
    env, obs, targets, refs = _setup()
    n, bad = 9, 5
    o, t = obs[:n], targets["near"][:n]
    base = _bits(env.nearest_feasible(o, t))
    keep = torch.tensor([i for i in range(n) if i != bad], device=DEV)
    nan = float("nan")
    t_bad, o_bad, w_bad = t.clone(), o.clone(), torch.ones(n, 14, device=DEV)
    t_bad[bad, 6] = nan
    o_bad[bad, 3] = nan
    w_bad[bad, 11] = nan
    clean_w = _bits(env.nearest_feasible(o, t, weight=torch.ones(n, 14, device=DEV)))
    for what, got, clean in (("target", env.nearest_feasible(o, t_bad), base), ("observation", env.nearest_feasible(o_bad, t), base),
                             ("weight", env.nearest_feasible(o, t, weight=w_bad), clean_w)):
        host = got.numpy()
        print("NaN in the %s of row %d: converged %s, iterations %d" % (what, bad, host["converged"][bad], host["iters"][bad]))
        assert not host["converged"][bad] and host["iters"][bad] == 40, what
        assert _same((clean[0][keep], clean[1][keep]), (got.action[keep], got.info[keep])), what
    # a weight that is not a finite number > 0 ends its row the same way (a device tensor's values are not read on the host)
    for v in (0.0, -1.0, float("inf")):
        w = torch.ones(n, 14, device=DEV)
        w[bad, 0] = v
        got = env.nearest_feasible(o, t, weight=w)
        assert not bool(got.converged[bad]) and int(got.iters[bad]) == 40 and _same((clean_w[0][keep], clean_w[1][keep]), (got.action[keep], got.info[keep]))


# ------------------------------------------------------------------------------------------------ whole episodes
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


def _hand_loop(tr, n, H, seed, fallback, init_states=None):
    """evaluate_filtered written out: the trainer's evaluation action, env.nearest_feasible on it, the select, the env step, the
    accumulators."""
    from rpo_amd.algo.evaluation import EvalResult, _initial_env
    env, k = tr.base_env, tr.kernels
    v = _initial_env(tr, n, seed, init_states)
    acc = torch.zeros(n, 8, device=DEV)
    rows = torch.zeros(n, k.ring_floats, device=DEV)
    iters = torch.zeros(n, dtype=torch.int32, device=DEV)
    log = []
    with torch.no_grad():
        for i in range(H):
            tr._eval_action(v, iters=iters)
            policy = v.action.clone()
            r = env.nearest_feasible(v.obs, policy)
            v.action.copy_(torch.where(r.converged[:, None], r.action, policy) if fallback == "policy" else r.action)
            iters.copy_(r.info[:, 2])
            log.append(r.info.clone())
            v.step(v.action, rows=rows, cap_steps=1, auto_reset=False)
            tr.backend.eval_accumulate(rows, k.cols, iters, i, v.viol_thresh, acc)
    return EvalResult(acc.cpu().numpy(), "filtered", H, seed), torch.stack(log, dim=1).cpu().numpy()


def test_evaluate_filtered():
    tr = _trainer()
    before = _state(tr)
    n, H, seed = 8, 24, 3
    res = tr.evaluate_filtered(n, seed=seed, record=True, constraints=True)
    assert res.path == "filtered" and res.episodes == n and res.horizon == H and (res.length == H).all() and not res.nonfinite.any()
    hand, log = _hand_loop(tr, n, H, seed, "policy")
    for f in res.FIELDS:
        assert np.array_equal(getattr(res, f), getattr(hand, f)), f                       # bitwise: the same launches
    assert np.array_equal(res.filter_iters, log[:, :, 2].astype(np.int32)) and np.array_equal(res.filter_converged, log[:, :, 3] > 0.5)
    assert np.array_equal(res.filter_distance, log[:, :, 0]) and np.array_equal(res.proj_iters, res.filter_iters.sum(axis=1))
    again = tr.evaluate_filtered(n, seed=seed)                                              # with and without record / constraints
    for f in res.FIELDS:
        assert np.array_equal(getattr(res, f), getattr(again, f)), f
    assert again.trajectory is None and np.array_equal(again.filter_iters, res.filter_iters)
    tj = res.trajectory
    policy = tr.evaluate(n, seed=seed, record=True)
    ptj = policy.trajectory
    assert np.array_equal(tj.obs[:, 0], ptj.obs[:, 0])                                     # evaluate(seed)'s episodes: hour 0 is its observation
    assert np.array_equal(tj.proposal[:, 0], ptj.action[:, 0][:, PARTIAL])                 # ... and the filter was given its action
    # precondition: the untrained actor's own actions violate the constraints on these episodes -- else the next check is vacuous
    worst = np.maximum(ptj.eq, ptj.ineq)
    policy_rate = (worst[ptj.valid] > 2 * TOL).mean()
    conv = res.filter_converged
    print("evaluate_filtered %d x %d: converged %d of %d steps, iterations %d..%d, on converged steps max_eq <= %.3g, max_ineq <= %.3g; "
          "the policy's own violation rate at 2 tol: %.3f; return %.4f (policy's %.4f)"
          % (n, H, conv.sum(), conv.size, res.filter_iters[conv].min(), res.filter_iters[conv].max(), tj.eq[conv].max(),
             tj.ineq[conv].max(), policy_rate, res.ret.mean(), policy.ret.mean()))
    assert policy_rate > 0
    assert conv.any() and (tj.eq[conv] <= 2 * TOL).all() and (tj.ineq[conv] <= 2 * TOL).all()
    assert (np.maximum(tj.eq, tj.ineq)[conv] > 2 * TOL).mean() == 0
    assert np.array_equal(tj.action[conv][:, 24], np.full(conv.sum(), np.float32(ev.GRID.slack_va[0])))
    torch.cuda.synchronize()
    for x, y in zip(before, _state(tr)):
        assert torch.equal(x, y)                                 # networks, env lanes, ctrl and replay: bitwise unchanged


def test_evaluate_filtered_fallback_and_scenarios():
    tr = _trainer()
    env, obs, targets, refs = _setup()
    before = _state(tr)
    n, H, seed, e = 8, 2, 3, 2
    assert not refs["uniform"]["converged"][65]                  # the float64 helper: fixture row 65 has no feasible dispatch
    init = torch.tensor(tr.evaluate(n, seed=seed, horizon=1, record=True).trajectory.obs[:, 0], device=DEV)
    init[e] = obs[65]                                            # ... and is hour 0 of episode 2
    policy = tr.evaluate(n, seed=seed, horizon=H, init_states=init, record=True).trajectory
    kept = tr.evaluate_filtered(n, seed=seed, horizon=H, init_states=init, record=True, fallback="policy")
    last = tr.evaluate_filtered(n, seed=seed, horizon=H, init_states=init, record=True, fallback="last")
    assert np.array_equal(kept.trajectory.obs[:, 0], init.cpu().numpy())
    assert not kept.filter_converged[e, 0] and kept.filter_iters[e, 0] == 40 and np.array_equal(kept.filter_converged, last.filter_converged)
    check = near64.solve_nearest(kept.trajectory.obs[e, 0].astype(np.float64), kept.trajectory.proposal[e, 0].astype(np.float64))
    assert not check["converged"]                                # the helper on the very problem the filter was given
    bad = ~kept.filter_converged[:, 0]
    own = policy.action[:, 0]
    single = env.nearest_feasible(init, torch.tensor(own, device=DEV)).action.cpu().numpy()
    assert np.array_equal(kept.trajectory.action[bad, 0].view(np.int32), own[bad].view(np.int32))          # the policy's own action
    assert np.array_equal(last.trajectory.action[bad, 0].view(np.int32), single[bad].view(np.int32))       # the solver's iterate
    assert not np.array_equal(own[e], single[e])
    good = kept.filter_converged[:, 0]
    assert good.any() and np.array_equal(kept.trajectory.action[good, 0], single[good]) and np.array_equal(last.trajectory.action[good, 0], single[good])
    for fb, r in (("policy", kept), ("last", last)):
        hand, _ = _hand_loop(tr, n, H, seed, fb, init)
        for f in r.FIELDS:                                       # (NaNs included: "last" steps the iterate of an infeasible solve)
            assert np.array_equal(getattr(r, f), getattr(hand, f), equal_nan=True), (fb, f)
    # scenarios: episode e plays day e % 3, the same hour 0 as evaluate(scenarios=)
    from rpo_amd.algo import evaluate_filtered
    S = tr.base_env.scenarios(3, seed=9)
    fed = tr.evaluate_filtered(n, seed=seed, horizon=H, scenarios=S, record=True)
    ref = tr.evaluate(n, seed=seed, horizon=H, scenarios=S, record=True)
    assert fed.path == "filtered" and np.array_equal(fed.days, np.arange(n) % 3) and np.array_equal(fed.days, ref.days)
    assert np.array_equal(fed.trajectory.obs[:, 0], ref.trajectory.obs[:, 0]) and np.array_equal(fed.trajectory.obs[:3, 0], fed.trajectory.obs[3:6, 0])
    same = evaluate_filtered(tr, n, seed=seed, horizon=H, scenarios=S)
    assert np.array_equal(same.ret, fed.ret) and tr.evaluate_filtered(n, seed=seed, horizon=H).days is None
    torch.cuda.synchronize()
    for x, y in zip(before, _state(tr)):
        assert torch.equal(x, y)
