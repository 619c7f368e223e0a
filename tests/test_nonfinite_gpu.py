"""The failure word and the NaN rows of every launch that carries them in training, acting and evaluation (MI355X), against the
float64 statement of tests/nonfinite_f64.py (held against the oracle backend on the CPU by tests/test_nonfinite.py).

Contract (include/rpo_hip.h: RPO_CTRL_NONFINITE, rpo_cartsafe_step, rpo_mlp_forward): a lane stepped with a NaN
action or reaching a non-finite next state raises ctrl[RPO_CTRL_NONFINITE] = 1 + the vector step once; its outputs are non-finite
where float64 gives that; every other lane keeps its bits.  No tolerance anywhere: lanes outside the reference's bad set are
compared bit for bit with the same launch without the plant, planted lanes as non-finite masks, forms with each other under
NaN-aware bit equality.

    rollout     the one-launch rollout as 16-lane tiles, 64-lane tiles and the streaming form with 16- and 64-lane groups
                (rollout_wide 0, 1, 3, 4; the streaming form is the default from 65 536 lanes, the headline) and the single-stage
                chain, at 133 lanes: lane plants (0x7FC00000, 0xFFC00000, 0x7F800000 in one component of lanes 0, 15, 16, 63, 64,
                132; two lanes at once), parameter plants (either NaN sign in one element of every layer of the actor), a second
                launch with another bad lane.  The fused forms take SpringPendulum's observation from different arrays (the row
                tiles recompute it from the internal state, the streaming form reads the stored one), which every launch leaves
                consistent: they get the plant in the state with the observation rewritten from it; the chain, which reads the
                two arrays in different launches, also gets each array alone.  ctrl = NULL is no input of the rollout (refused
                by the binding); the step kernels' is pinned by tests/test_envs_f64_gpu.py::test_nonfinite_rows.
    act         ops.*.policy_act forms 1, 2, 3 and the stepwise path: masks of action, proposal and residuals; no flag.
    evaluate    trainer.evaluate() on both paths, with a record, a constraint report and observation noise, evaluate_budgets and
                evaluate_policies; a lane that finished keeps its row; the accumulators through ops.eval_summarize (133 and 1 025
                rows) into ops.eval_keep_best.
    ride        the riding launches (rpo_split_critic_fwd_a_ride / _fwd_b_ride / _bwd_b_ride) from captured windows against the
                serial windows (schedule ride=0) with a poisoned lane and a poisoned parameter.

The statement the kernels are held to is nonfinite_f64's clips="fmax": the env step's own clamps BEHIND the failure test are
fminf / fmaxf (a flagged NaN action is stepped as the clipped force), as tests/test_envs_f64_gpu.py pins for the step kernels.
"""
import numpy as np
import pytest
import torch

import nonfinite_f64 as nf
from rpo_amd.algo import NonFiniteError
from test_train_step_golden import build_trainer

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning")]
DEV = torch.device("cuda")
CASES = [("ddpg", "cart"), ("sac", "cart"), ("ddpg", "pendulum"), ("sac", "pendulum")]
FORMS = {"tiles16": 0, "tiles64": 1, "stream16": 3, "stream64": 4, "chain": None}      # rollout_wide, or the single-stage chain
_H, _REF, _OUT = {}, {}, {}


@pytest.fixture(scope="module")
def hip():
    from rpo_amd import ops
    assert torch.cuda.is_available()
    return ops


def harness(algo, envname, chain=False):
    """One trainer per (algo, env, one-launch | chain), its snapshot and the launch without a plant."""
    key = (algo, envname, chain)
    if key not in _H:
        torch.manual_seed(5)
        tr = build_trainer(algo, envname, __import__("rpo_amd").ops, DEV, num_envs=nf.N, use_graph=False, capacity=16,
                           schedule=dict(fused_rollout=0) if chain else None)
        assert bool(tr._rollout_pipeline) == (not chain)
        _H[key] = nf.StepHarness(tr, sync=torch.cuda.synchronize)
    return _H[key]


def reference(h, name, compute):
    """The float64 reference of a case, computed once per (algo, env) and shared by the forms."""
    key = (h.spec.env, h.spec.gauss, name)
    if key not in _REF:
        _REF[key] = compute()
    return _REF[key]


def stream_applies(tr):
    """What rollout_stream.hip asks of a launch before it takes it (otherwise rollout_wide 3 / 4 fall back to the row tiles)."""
    d = tr.fused.descs["actor"]
    return d.E == 128 and d.H == 256 and d.A == 0 and d.tensors["W0"].data_ptr() % 16 == 0


def findings(wrong):
    """The cases that went wrong, then the first 20 findings in full."""
    cases = sorted(set(w.split(":")[0].split(" form ")[0] for w in wrong))
    return "%d findings in the cases %s; the first 20:\n%s" % (len(wrong), ", ".join(cases), "\n".join(wrong[:20]))


def cross_form(h, form, name, out):
    """All forms equal each other under NaN-aware bit equality: the first form to run a case keeps its outputs."""
    key = (h.spec.env, h.spec.gauss, name)
    first = _OUT.setdefault(key, (form, out))
    if first[0] == form:
        return []
    return ["%s: %s differs from the form %s (NaN-aware bits)" % (name, k, first[0]) for k in ("internal", "obs", "action", "rows")
            if not nf.same_nan_aware(out[k], first[1][k])]


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("algo,envname", CASES)
def test_rollout_forms(hip, algo, envname, form):
    chain = form == "chain"
    h = harness(algo, envname, chain)
    sp, tr = h.spec, h.tr
    if FORMS[form] in (3, 4):
        assert stream_applies(tr)
    sel = {} if chain else dict(rollout_wide=FORMS[form])
    wrong = []
    with hip.tuning(**sel):
        assert chain or hip.tuning.get("rollout_wide") == FORMS[form]
        clean = h.run()
        assert int(clean["ctrl"][nf.NF_IDX]) == 0 and int(clean["ctrl"][nf.T_IDX]) == nf.T0 + 1
        wrong += cross_form(h, form, "clean", clean)
        # ---- lane plants
        for name, target, plants in nf.lane_cases(sp.env, None if chain else ("state",)):
            internal, obs = nf.planted_state(sp.env, h.internal0, h.obs0, target, plants)
            ref = reference(h, name, lambda: nf.vector_step(sp, internal, obs, h.ep_len0, nf.T0, "fmax"))
            assert sorted(np.flatnonzero(ref["bad"])) == sorted(p[0] for p in plants) and ref["word"] == nf.T0 + 1
            out = h.run(internal, obs)
            wrong += nf.check_step(name, out, clean, ref, nf.N, sp)
            if target == "state":                                # (the fused forms do not run the other targets)
                wrong += cross_form(h, form, name, out)
        # ---- the diverged actor
        for name, field, bits in nf.param_cases(sp.gauss):
            with h.planted_param(field, bits) as index:
                out = h.run()
            ref = reference(h, name, lambda: nf.vector_step(sp.with_param(field, index, nf.f32_of(bits)), h.internal0, h.obs0, h.ep_len0,
                                                            nf.T0, "fmax"))
            assert ref["bad"].all() and ref["word"] == nf.T0 + 1
            wrong += nf.check_step(name, out, clean, ref, nf.N, sp)
            wrong += cross_form(h, form, name, out)
        # ---- first step, sticky: a second launch at T0 + 1 with another bad lane
        internal, obs = nf.planted_state(sp.env, h.internal0, h.obs0, "state", [(16, 1, nf.NEG_QNAN)])
        first = h.run(internal, obs)
        internal, obs = nf.planted_state(sp.env, first["internal"], first["obs"], "state", [(63, 0, nf.QNAN)])
        h.set_state(internal, obs)
        second = h.step()
        if int(second["ctrl"][nf.NF_IDX]) != nf.T0 + 1 or int(second["ctrl"][nf.T_IDX]) != nf.T0 + 2:
            wrong.append("second launch: word %d, step counter %d" % (int(second["ctrl"][nf.NF_IDX]), int(second["ctrl"][nf.T_IDX])))
        cap = second["rows"].shape[0] // nf.N
        if not np.isnan(second["rows"].reshape(cap, nf.N, -1)[nf.T0 + 1, 63, sp.cols["action"][0]]):
            wrong.append("second launch: lane 63 stepped with a finite action")
        assert nf.same_bits(h.run()["rows"], clean["rows"])       # every parameter element and every state was put back
    assert not wrong, findings(wrong)


# ================================================================================================================ policy_act
@pytest.mark.parametrize("algo,envname", CASES)
def test_policy_act_forms(hip, algo, envname):
    h = harness(algo, envname)
    sp, tr = h.spec, h.tr
    assert stream_applies(tr)
    h.restore()
    fields = ("action", "proposal", "eq_resid", "ineq_resid")

    def run(obs, form):
        x = torch.as_tensor(obs, device=DEV)
        if form == "stepwise":
            tr.schedule["fused_act"] = 0
            try:
                r = tr.act(x)
            finally:
                tr.schedule["fused_act"] = 1
            assert r.path == "stepwise"
        else:
            r = tr.act(x, form=form)
            assert r.path == "fused" and r.form == ("tile" if form == 1 else "stream")
        torch.cuda.synchronize()
        return {f: getattr(r, f).float().cpu().numpy().reshape(nf.N, -1) for f in fields}
    forms = (1, 2, 3, "stepwise")
    clean = {f: run(h.obs0, f) for f in forms}
    wrong = []
    for name, _, plants in nf.lane_cases(sp.env, ("obs",) if sp.env == "pendulum" else ("state",)):
        _, obs = nf.planted_state(sp.env, h.internal0, h.obs0, "obs" if sp.env == "pendulum" else "state", plants)
        ref = nf.act(sp, obs)
        lanes = sorted(p[0] for p in plants)
        assert sorted(np.flatnonzero(ref["action"].any(axis=1))) == lanes, name
        outs = {f: run(obs, f) for f in forms}
        keep = np.ones(nf.N, bool)
        keep[lanes] = False
        for f in forms:
            for k in fields:
                got = outs[f][k]
                if not np.array_equal(nf.nonfinite(got)[lanes], ref[k].reshape(nf.N, -1)[lanes]):
                    wrong.append("%s form %s: %s of the planted lanes is non-finite at %s, float64 gives %s"
                                 % (name, f, k, np.argwhere(nf.nonfinite(got)[lanes]).tolist(), np.argwhere(ref[k].reshape(nf.N, -1)[lanes]).tolist()))
                if not nf.same_bits(got[keep], clean[f][k][keep]):
                    wrong.append("%s form %s: %s of another lane changed" % (name, f, k))
                if not nf.same_nan_aware(got, outs[1][k]):
                    wrong.append("%s form %s: %s differs from the row tile" % (name, f, k))
    assert int(tr.vec.ctrl[nf.NF_IDX]) == 0                       # acting raises no flag
    assert not wrong, findings(wrong)


# ================================================================================================================ evaluation


class path(object):
    """``with path(tr, fused):`` -- trainer.evaluate() on the fused or the stepwise path."""

    def __init__(self, tr, fused):
        self.tr, self.fused = tr, int(fused)

    def __enter__(self):
        self.old = self.tr.schedule.get("fused_eval", 1)
        self.tr.schedule["fused_eval"] = self.fused

    def __exit__(self, *exc):
        self.tr.schedule["fused_eval"] = self.old
        return False


def check_eval(name, r, clean, ref, wrong):
    if not np.array_equal(r.nonfinite, ref["nonfinite"]):
        wrong.append("%s: nonfinite %s, the reference gives %s" % (name, np.flatnonzero(r.nonfinite), np.flatnonzero(ref["nonfinite"])))
    bad = ref["nonfinite"]
    if not np.array_equal(r.length[bad], ref["length"][bad]):
        wrong.append("%s: lengths of the bad episodes %s, the reference gives %s" % (name, r.length[bad], ref["length"][bad]))
    got = np.stack([~np.isfinite(getattr(r, k)) for k in nf.ACC_SLOTS], axis=1)
    if not np.array_equal(got[bad], ref["nan"][bad]):
        wrong.append("%s: non-finite slots of the bad episodes %s, the reference gives %s" % (name, got[bad].tolist(), ref["nan"][bad].tolist()))
    for k in clean.FIELDS:
        if getattr(r, k)[~bad].tobytes() != getattr(clean, k)[~bad].tobytes():
            wrong.append("%s: %s of another episode differs from the clean evaluation" % (name, k))
    if r.constraints is not None:
        c = r.constraints
        for k, m in (("ineq_max", ref["con_ineq"]), ("eq_max", ref["con_eq"])):
            if not np.array_equal(~np.isfinite(np.asarray(getattr(c, k)))[bad], m[bad]):
                wrong.append("%s: the report's %s cells of the bad episodes are non-finite elsewhere than the reference's" % (name, k))


def same_results(a, b):
    return all(nf.same_nan_aware(np.asarray(getattr(a, k), np.float64).astype(np.float32), np.asarray(getattr(b, k), np.float64).astype(np.float32))
               for k in a.FIELDS)


@pytest.mark.parametrize("algo,envname", CASES)
def test_evaluation_lane_plants(hip, algo, envname):
    h = harness(algo, envname)
    sp, tr = h.spec, h.tr
    h.restore()
    init = nf.eval_init(h)
    clean = {}
    for fused in (1, 0):
        with path(tr, fused):
            clean[fused] = tr.evaluate(nf.N, init_states=init, horizon=3, seed=1, constraints=True)
            assert clean[fused].path == ("fused" if fused else "stepwise") and not clean[fused].nonfinite.any()
            assert clean[fused].length[7] == 1
    wrong = []
    for name, _, plants in nf.eval_plants(sp.env):
        bad_init, _ = nf.planted_state(sp.env, init, nf.get_obs(sp, init), "state", plants)
        ref = nf.evaluate(sp, bad_init, 3, "fmax")
        assert sorted(np.flatnonzero(ref["nonfinite"])) == sorted(p[0] for p in plants), name
        res = {}
        for fused in (1, 0):
            with path(tr, fused):
                res[fused] = tr.evaluate(nf.N, init_states=bad_init, horizon=3, seed=1, constraints=True)
            check_eval("%s %s" % (name, res[fused].path), res[fused], clean[fused], ref, wrong)
        if not same_results(res[1], res[0]):
            wrong.append("%s: fused and stepwise differ (NaN-aware bits)" % name)
    assert int(tr.vec.ctrl[nf.NF_IDX]) == 0 and int(tr.vec.ctrl[nf.T_IDX]) == nf.T0      # the evaluation owns its ctrl
    assert not wrong, findings(wrong)


@pytest.mark.parametrize("algo,envname", [("ddpg", "cart"), ("sac", "pendulum")])
def test_evaluation_variants(hip, algo, envname):
    """The other entry points once each, on one two-lane plant: a record, observation noise (additive and finite: it moves no
    mask), every budget of evaluate_budgets, and evaluate_policies with the live actor beside a poisoned copy."""
    h = harness(algo, envname)
    sp, tr = h.spec, h.tr
    h.restore()
    init = nf.eval_init(h)
    plants = [(15, 1, nf.NEG_QNAN), (64, 0, nf.QNAN)]
    bad_init, _ = nf.planted_state(sp.env, init, nf.get_obs(sp, init), "state", plants)
    ref = nf.evaluate(sp, bad_init, 3, "fmax")
    wrong = []
    sigma = [0.01] * tr.kernels.obs_dim
    for kw in (dict(record=8), dict(obs_noise=sigma), dict(record=8, constraints=True, obs_noise=sigma)):
        res = {}
        for fused in (1, 0):
            with path(tr, fused):
                c = tr.evaluate(nf.N, init_states=init, horizon=3, seed=1, **kw)
                res[fused] = tr.evaluate(nf.N, init_states=bad_init, horizon=3, seed=1, **kw)
            assert res[fused].path == ("fused" if fused else "stepwise")
            check_eval("%s %s" % (sorted(kw), res[fused].path), res[fused], c, ref, wrong)
        if not same_results(res[1], res[0]):
            wrong.append("%s: fused and stepwise differ (NaN-aware bits)" % sorted(kw))
    # every budget in one launch: 0 (Complete only) and the trainer's
    import copy
    budgets = [0, sp.eval_K]
    clean = tr.evaluate_budgets(nf.N, eval_steps=budgets, init_states=init, horizon=3, seed=1, constraints=True)
    sweep = tr.evaluate_budgets(nf.N, eval_steps=budgets, init_states=bad_init, horizon=3, seed=1, constraints=True)
    assert sweep.path == "fused"
    for g, b in enumerate(budgets):
        spb = copy.copy(sp)
        spb.eval_K = b
        check_eval("budget %d" % b, sweep[g], clean[g], nf.evaluate(spb, bad_init, 3, "fmax"), wrong)
    # many actors in one launch: the live one, and a copy with a NaN in its hidden bias
    params = tr.policy_params()
    with h.planted_param("b0", nf.NEG_QNAN) as index:
        poisoned = tr.policy_params()
    assert int(torch.isnan(poisoned).sum()) == 1 and not bool(torch.isnan(tr.policy_params()).any())
    clean = tr.evaluate_policies([None, params], nf.N, init_states=init, horizon=3, seed=1)
    sweep = tr.evaluate_policies([None, poisoned], nf.N, init_states=bad_init, horizon=3, seed=1)
    assert sweep.path == "fused"
    check_eval("policies: live", sweep[0], clean[0], ref, wrong)
    ref_all = nf.evaluate(sp.with_param("b0", index, float("nan")), bad_init, 3, "fmax")
    assert ref_all["nonfinite"].all()
    check_eval("policies: poisoned", sweep[1], clean[1], ref_all, wrong)
    assert int(tr.vec.ctrl[nf.NF_IDX]) == 0
    assert not wrong, findings(wrong)


@pytest.mark.parametrize("algo,envname", [("ddpg", "cart"), ("sac", "pendulum")])
def test_finished_lane_keeps_its_row_and_the_curve_refuses_the_point(hip, algo, envname):
    """Horizon 1, then the state of the lane that finished is poisoned and the evaluation continues: its row keeps its bits on both
    paths.  The accumulators of a poisoned evaluation go through rpo_eval_summarize -- one workgroup (133 rows) and several
    (1 025) -- whose RPO_CURVE_NONFINITE must be the count, and that row is never taken by rpo_eval_keep_best."""
    from rpo_amd.algo import evaluation as ev
    h = harness(algo, envname)
    sp, tr = h.spec, h.tr
    h.restore()
    init = nf.eval_init(h)
    scale, base = tr._box_affine
    k = tr.kernels
    W = hip.EVAL_LEN
    accs = {}
    for fused in (1, 0):
        v = ev._initial_env(tr, nf.N, 1, torch.as_tensor(init, device=DEV))
        acc = torch.zeros(nf.N, W, device=DEV)
        rows = torch.zeros(nf.N, k.ring_floats, device=DEV)
        iters = torch.zeros(nf.N, dtype=torch.int32, device=DEV)

        def steps(t0, n):
            with torch.no_grad():
                for t in range(t0, t0 + n):
                    if fused:
                        k.evaluate(tr.fused.descs["actor"], tr._gauss_policy, scale, base, v.internal, None if v.obs is v.internal else v.obs,
                                   v.action, v.ep_len, v.ep_ret, v.ep_count, v.ctrl, acc, t, 1, tr._box_lo, tr._box_hi, tr.eval_steps,
                                   tr.eval_lr, tr.corr_eps, tr.corr_momentum, v.max_episode_steps, v.viol_thresh)
                    else:
                        tr._eval_action(v, iters=iters)
                        v.step(v.action, rows=rows, cap_steps=1, auto_reset=False)
                        hip.eval_accumulate(rows, k.cols, iters, t, v.viol_thresh, acc)
        steps(0, 1)
        torch.cuda.synchronize()
        word = acc[:, hip.CONST["RPO_EVAL_WORD"]].view(torch.int32).cpu().numpy()
        assert not word[7] & hip.CONST["RPO_EVAL_ALIVE"] and word[6] & hip.CONST["RPO_EVAL_ALIVE"]
        before = acc[7].clone()
        internal, obs = nf.planted_state(sp.env, v.internal.cpu().numpy(), v.obs.cpu().numpy(), "state", [(7, 1, nf.QNAN), (6, 1, nf.NEG_QNAN)])
        v.internal.copy_(torch.as_tensor(internal, device=DEV))
        if v.obs is not v.internal:
            v.obs.copy_(torch.as_tensor(obs, device=DEV))
        steps(1, 2)
        torch.cuda.synchronize()
        assert torch.equal(acc[7].view(torch.int32), before.view(torch.int32)), "the finished lane's row changed (fused=%d)" % fused
        r = ev.EvalResult(acc.cpu().numpy(), "x", 3, 1)
        assert np.flatnonzero(r.nonfinite).tolist() == [6] and r.length[7] == 1 and r.length[6] == 3
        # the evaluation's own ctrl took the word -- 1 + ITS step counter, which only the stepwise path's step launches advance
        assert int(v.ctrl[nf.NF_IDX]) == (1 if fused else 2) and int(tr.vec.ctrl[nf.NF_IDX]) == 0
        accs[fused] = acc
    assert nf.same_nan_aware(accs[1].cpu().numpy(), accs[0].cpu().numpy())
    # ---- summarize + keep_best
    ws = torch.zeros(hip.CURVE_WS, dtype=torch.float64, device=DEV)
    NFC = hip.CONST["RPO_CURVE_NONFINITE"]
    good = torch.zeros(nf.N, W, device=DEV)
    v = ev._initial_env(tr, nf.N, 1, torch.as_tensor(init, device=DEV))
    with torch.no_grad():
        ev._run_fused(tr, v, good, 3)
    good_row = torch.zeros(hip.CURVE_LEN, dtype=torch.float64, device=DEV)
    hip.eval_summarize(good, tr.vec.ctrl, good_row, ws)
    assert float(good_row[NFC]) == 0.0
    src = torch.arange(8, dtype=torch.float32, device=DEV)
    for n, want in ((nf.N, 1), (1025, None)):
        acc = accs[1] if n == nf.N else accs[1].repeat(8, 1)[:n].contiguous()
        want = int(((acc[:, hip.CONST["RPO_EVAL_WORD"]].view(torch.int32) & hip.CONST["RPO_EVAL_NONFINITE"]) != 0).sum()) if want is None else want
        assert want >= 1
        row = torch.zeros(hip.CURVE_LEN, dtype=torch.float64, device=DEV)
        hip.eval_summarize(acc, tr.vec.ctrl, row, ws)
        assert float(row[NFC]) == want, (n, float(row[NFC]), want)
        # without an incumbent: not taken
        best, best_row, point = torch.full((8,), -7.0, device=DEV), torch.zeros(hip.CURVE_LEN, dtype=torch.float64, device=DEV), \
            torch.full((1,), -1, dtype=torch.int64, device=DEV)
        hip.eval_keep_best(src, best, row, best_row, point, 0, 1.0)
        assert int(point[0]) == -1 and float(best[0]) == -7.0
        # with one: the clean row is taken, the poisoned one never replaces it -- not even with a return made to look better
        hip.eval_keep_best(src, best, good_row, best_row, point, 1, 1.0)
        assert int(point[0]) == 1 and torch.equal(best, src)
        better = row.clone()
        better[hip.CONST["RPO_CURVE_STATS"]] = 1e9
        for cand in (row, better):
            hip.eval_keep_best(src + 1, best, cand, best_row, point, 2, 1.0)
            assert int(point[0]) == 1 and torch.equal(best, src) and torch.equal(best_row, good_row)


# ================================================================================================================ riding launches
def _ride_run(hip, ride, plant, monkeypatch):
    monkeypatch.setenv("RPO_GRAPH_CYCLE", "4")
    monkeypatch.setenv("RPO_VERBOSE", "0")
    torch.manual_seed(5)
    tr = build_trainer("sac", "cart", hip, DEV, num_envs=nf.N, use_graph=True, capacity=64, schedule=dict(ride=ride))
    assert tr._ride_ok(True) == bool(ride)
    tr.vec.reset()
    tr.run_steps(24)                                            # three eager windows, the capture, two replays
    torch.cuda.synchronize()
    tr._harvest(final=True)
    assert int(tr.vec.ctrl[nf.NF_IDX]) == 0
    keys = [k for k, e in tr._graphs.entries.items() if isinstance(k, tuple) and e["graph"] is not None]
    assert any(len(k) == 4 and k[3] == "ride" for k in keys) == bool(ride) and keys
    t0 = tr._t
    plant(tr)
    tr.run_steps(4)                                             # ONE replayed window: rollout t0, then t0 + 1 .. t0 + 3 riding
    torch.cuda.synchronize()
    with pytest.raises(NonFiniteError, match="vector step %d " % t0):
        tr._harvest(final=True)
    assert int(tr.vec.ctrl[nf.NF_IDX]) == t0 + 1 and int(tr.vec.ctrl[nf.T_IDX]) == t0 + 4
    return tr, t0


def _lane_plant(bits):
    def plant(tr):
        internal, _ = nf.planted_state("cart", tr.vec.internal.cpu().numpy(), None, "state", [(64, 0, bits)])     # x: stays NaN
        tr.vec.internal.copy_(torch.as_tensor(internal, device=DEV))
    return plant


def _param_plant(tr):
    t = tr.fused.descs["actor"].tensors["W0"]
    t.detach().view(-1)[nf.param_index(t)] = float("nan")


@pytest.mark.parametrize("what", ["lane-7FC00000", "lane-FFC00000", "parameter"])
def test_riding_launches(hip, what, monkeypatch):
    plant = _param_plant if what == "parameter" else _lane_plant(int(what[5:], 16))
    a, t0 = _ride_run(hip, 1, plant, monkeypatch)
    b, t1 = _ride_run(hip, 0, plant, monkeypatch)
    assert t0 == t1
    n, c = nf.N, a.kernels.cols
    ring = a.buffer.rows.cpu().numpy().reshape(a.buffer.capacity, n, -1)
    for t in range(t0, t0 + 4):                                 # the lane (or every lane) is stepped with a NaN action in each step
        lanes = [64] if what != "parameter" else list(range(n))
        assert np.isnan(ring[t % a.buffer.capacity][lanes, c["action"][0]]).all(), t
    if what != "parameter":
        keep = np.arange(n) != 64
        assert np.isfinite(ring[t0 % a.buffer.capacity][keep][:, :a.kernels.row_floats]).all()
    for k, x, y in (("ring", a.buffer.rows, b.buffer.rows), ("state", a.vec.internal, b.vec.internal), ("action", a.vec.action, b.vec.action),
                    ("parameters", a.agent.flat.data, b.agent.flat.data)):
        assert nf.same_nan_aware(x.cpu().numpy(), y.cpu().numpy()), k
    assert torch.equal(a.vec.ep_len, b.vec.ep_len) and torch.equal(a.vec.ep_count, b.vec.ep_count)


# ================================================================================================================ EVOPF-v0
EV_N, EV_SEED, EV_BASE = 64, 77, 5
EV_HOUR, EV_COL = 1, 3                                          # the table entry that is poisoned: pd[3] of hour 1 of day 1
EV_ENTRY = 48 + 28 * EV_HOUR + EV_COL                           # (RPO_EVOPF_SCEN_DAY layout: price[48] | 24 x (pd[14], qd[14]))


def _evopf_actions(n):
    """[n, 43] in the neighbourhood of a dispatch (as test_scenarios_gpu._actions): nothing the step could not take."""
    g = torch.Generator().manual_seed(3)
    a = torch.zeros(n, 43)
    a[:, 0:10] = torch.rand(n, 10, generator=g) * 0.6
    a[:, 10:24] = 1.0 + 0.05 * (torch.rand(n, 14, generator=g) - 0.5)
    a[:, 24:38] = 0.2 * (torch.rand(n, 14, generator=g) - 0.5)
    a[:, 38:43] = 0.4 * (torch.rand(n, 5, generator=g) - 0.5)
    return a.to(DEV)


def _evopf_tables(bits):
    from test_scenarios_gpu import _days
    table = _days().table(DEV).clone()
    assert table.shape[0] == 3 and bool(torch.isfinite(table).all())
    bad = table.clone()
    bad[1, EV_ENTRY:EV_ENTRY + 1].view(torch.int32).fill_(int(np.array([bits], np.uint32).view(np.int32)[0]))
    return table, bad


@pytest.mark.parametrize("bits", [nf.QNAN, nf.NEG_QNAN], ids=["7FC00000", "FFC00000"])
@pytest.mark.parametrize("seam", ["bank-uniform", "bank-cycle", "scenario"])
def test_evopf_nan_table_row(hip, seam, bits):
    """rpo_evopf_step_bank / rpo_evopf_step_scenario, 64 lanes on a bank of 3 days, a NaN demand in ONE entry of day 1's hour 1.
    The reset (hour 0) is clean; the first step copies hour 1's demand into the next observation: exactly the lanes on day 1 --
    the deal's host restatement (tests/test_scenario_bank.py) -- reach a non-finite next state, in exactly that entry (the
    demand entries of an observation are copies of the table row, include/rpo_hip.h; everything else of the row is computed
    from the finite state and action); all other lanes keep their bits; the word is T0 + 1."""
    from test_scenario_bank import bank_days
    from test_scenarios_gpu import _env
    env = _env()
    k = env.kernels
    ep0 = (np.arange(EV_N) % 4).astype(np.int32)
    action = _evopf_actions(EV_N)
    if seam == "scenario":
        day = np.arange(EV_N) % 3
    else:
        day = bank_days(EV_SEED, EV_BASE + np.arange(EV_N), ep0.astype(np.int64), 3, seam[5:], EV_N)
    lanes = np.flatnonzero(day == 1)
    assert 0 < len(lanes) < EV_N

    def run(table):
        if seam == "scenario":
            v = env.make_vec(EV_N, seed=EV_SEED, env_id_base=EV_BASE, scenario=(table, torch.as_tensor(day.astype(np.int32), device=DEV)))
        else:
            v = env.make_vec(EV_N, seed=EV_SEED, env_id_base=EV_BASE, bank=(table, seam[5:], EV_N))
            v.ep_count.copy_(torch.as_tensor(ep0, device=DEV))
        v.reset()
        v.ctrl[nf.T_IDX] = nf.T0
        rows = torch.zeros(EV_N, k.ring_floats, device=DEV)
        start = v.internal.clone()
        v.step(action, rows=rows, cap_steps=1, auto_reset=seam != "scenario")
        torch.cuda.synchronize()
        return dict(start=start.cpu().numpy(), internal=v.internal.cpu().numpy(), rows=rows.cpu().numpy(), ctrl=v.ctrl.cpu().numpy(),
                    ep_len=v.ep_len.cpu().numpy())
    table, bad_table = _evopf_tables(bits)
    clean, out = run(table), run(bad_table)
    assert int(clean["ctrl"][nf.NF_IDX]) == 0 and np.isfinite(clean["rows"]).all() and np.isfinite(clean["internal"]).all()
    assert nf.same_bits(out["start"], clean["start"])             # hour 0 does not read the entry
    assert int(out["ctrl"][nf.NF_IDX]) == nf.T0 + 1 and int(out["ctrl"][nf.T_IDX]) == nf.T0 + 1
    keep = np.ones(EV_N, bool)
    keep[lanes] = False
    assert nf.same_bits(out["rows"][keep], clean["rows"][keep]) and nf.same_bits(out["internal"][keep], clean["internal"][keep])
    assert np.array_equal(out["ep_len"], clean["ep_len"])
    want_row = np.zeros((len(lanes), out["rows"].shape[1]), bool)
    want_row[:, k.cols["next_state"][0] + EV_COL] = True
    want_state = np.zeros((len(lanes), out["internal"].shape[1]), bool)
    want_state[:, EV_COL] = True
    assert np.array_equal(nf.nonfinite(out["rows"][lanes]), want_row)
    assert np.array_equal(nf.nonfinite(out["internal"][lanes]), want_state)
    # everything else of those lanes' rows is what the clean table gives
    assert nf.same_bits(np.where(want_row, 0, out["rows"][lanes]), np.where(want_row, 0, clean["rows"][lanes]))


@pytest.mark.parametrize("bits", [nf.QNAN, nf.NEG_QNAN], ids=["7FC00000", "FFC00000"])
def test_evopf_evaluation(hip, bits):
    """trainer.evaluate() on EVOPF-v0 through rpo_evopf_evaluate (schedule fused_eval_evopf=1) and stepwise (0): a NaN demand in the
    initial state of four lanes (the fused kernel has no table-fed instance; a NaN table row reaches the stepwise path only, below).
    The actor reads the NaN, the action and with it the step's residuals are NaN: exactly those episodes are nonfinite, all others
    keep their bits, both paths agree."""
    from test_scenarios_gpu import _days, _trainer
    tr = _trainer()
    v = tr.base_env.make_vec(EV_N, seed=3)
    v.reset()
    init = v.internal.cpu().numpy()
    lanes = [0, 15, 16, 63]
    bad_init = init.copy()
    for lane in lanes:
        bad_init.view(np.uint32)[lane, EV_COL] = bits
    old = tr.schedule.get("fused_eval_evopf", 0)
    res = {}
    try:
        for switch in (1, 0):
            tr.schedule["fused_eval_evopf"] = switch
            clean = tr.evaluate(EV_N, init_states=init, horizon=3, seed=1)
            r = res[switch] = tr.evaluate(EV_N, init_states=bad_init, horizon=3, seed=1)
            assert r.path == clean.path == ("fused" if switch else "stepwise")
            assert not clean.nonfinite.any() and np.flatnonzero(r.nonfinite).tolist() == lanes
            keep = ~r.nonfinite
            for f in r.FIELDS:
                assert getattr(r, f)[keep].tobytes() == getattr(clean, f)[keep].tobytes(), (switch, f)
            assert np.isnan(r.max_eq[lanes]).all() and (r.length[lanes] >= 1).all()
        assert same_results(res[1], res[0])
        # the NaN table row: episode e plays day e % 3; hour 1's demand is what step 1 observes
        S = _days()[0:3]
        table = S.table(tr.device)
        saved = table[1, EV_ENTRY].clone()
        clean = tr.evaluate(EV_N, horizon=3, seed=1, scenarios=S)
        try:
            table[1, EV_ENTRY:EV_ENTRY + 1].view(torch.int32).fill_(int(np.array([bits], np.uint32).view(np.int32)[0]))
            r = tr.evaluate(EV_N, horizon=3, seed=1, scenarios=S)
        finally:
            table[1, EV_ENTRY] = saved
        assert r.path == "stepwise" and not clean.nonfinite.any()
        assert np.array_equal(r.nonfinite, np.arange(EV_N) % 3 == 1)
        keep = ~r.nonfinite
        for f in r.FIELDS:
            assert getattr(r, f)[keep].tobytes() == getattr(clean, f)[keep].tobytes(), f
    finally:
        tr.schedule["fused_eval_evopf"] = old
    assert int(tr.vec.ctrl[nf.NF_IDX]) == 0
