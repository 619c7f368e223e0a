"""The EVOPF yardstick of tests/evopf_f64.py checked on the CPU: the float32 emulation of the kernels passes every checker and stays
under the 2 % cap of ambiguous rows on the committed inputs, C_REF is what the emulation measures, seeded mutations of the
emulation each fail at least one checker, and the float64 formulas agree with oracle/evopf.py and the reference's fixtures."""
import os

import numpy as np
import pytest

import evopf_f64 as E
from oracle import evopf as oe

HERE = os.path.dirname(os.path.abspath(__file__))
TAB = E.consts_table()
TAB_DYN = E.consts_table(static=False)
# corr_lr of the scripts; corr_eps 1e-4, not their 1e-5: the running bound of a balance (~470 eps32 = 4e-5) is LARGER than 1e-5, so at
# 1e-5 every feasible lane's stop decision lies inside the float32 noise of its own residual (ambiguous); at 1e-4 it is decidable
LR, EPS, K = 1e-4, 1e-4, 10
LR_BIG, EPS_BIG = 1e-2, 2e-2
NEWTON_TOL, NEWTON_M = 1e-3, 6              # (1e-5, the scripts' value, lies inside the bound of ||delta|| at a converged point)
NU = np.random.RandomState(8).uniform(0, 1, 58).astype(np.float32)
NU[::7] = 0.0


def golden(name):
    return np.load(os.path.join(HERE, "golden", name + ".npz"))


def _merge(dst, src):
    for k, v in src.items():
        dst[k] = max(dst.get(k, 0.0), float(v))


def closed_forms(n, mut=()):
    """Every closed-form checker on the emulation at n rows -> ({group: ratio}, {name: ambiguous share})."""
    out, amb = {}, {}
    s, a = E.make_rows(n, n)
    rng = np.random.RandomState(n)
    eq, iq = E.emu_resid(TAB, s, a, mut)
    _merge(out, E.check_resid(TAB, s, a, eq, iq))
    ge = rng.randn(n, 28).astype(np.float32)
    for sign in (0, 1):
        _merge(out, E.check_vjp(TAB, a, ge, E.emu_vjp(TAB, a, ge, sign, mut), sign))
    _merge(out, E.check_step(TAB, s, a, E.emu_step(TAB, s, a, mut)))
    ids, ep = np.arange(n) + 5, rng.randint(0, 4, n)
    hour = np.concatenate([[0, 22, 23, 24, 25], rng.randint(0, 26, n)])[:n]
    r, unj = E.check_episode(TAB, 9, ids, ep, hour, E.emu_episode(TAB, 9, ids, ep, hour, mut))
    _merge(out, r)
    amb["episode"] = unj
    return out, amb


def lagrangian_case(n, mut=()):
    s, a = E.mask_rows(n, n, spread=0.05)
    gnu = np.random.RandomState(n).uniform(0, 1, 58).astype(np.float32)
    out, amb = {}, 0.0
    for overwrite in (0, 1):
        loss, g, gn = E.emu_lagrangian(TAB, s, a, NU, 1.0 / n, 0.7, gnu, overwrite, mut)
        r, amb = E.check_lagrangian(TAB, s, a, NU, 1.0 / n, 0.7, gnu, overwrite, loss, g, gn)
        _merge(out, r)
    return out, {"lagrangian": amb}


def solve_case(n, mut=()):
    out, amb = {}, {}
    s, a = E.mask_rows(n, n + 1, spread=0.03)
    for tab in (TAB, TAB_DYN):
        g, _ = E.emu_ipg(tab, s, a, mut)
        r, share = E.check_ipg(tab, s, a, g)
        _merge(out, {"ipg": r})
        amb["ipg"] = share
    rng = np.random.RandomState(n)
    s2, ap = E.basic_rows(n, n)
    act = E.emu_newton(TAB, s2, ap, 1e-5, 50)[0]
    g1, gb, g2 = (rng.randn(n, 43).astype(np.float32) for _ in range(3))
    for tab in (TAB, TAB_DYN):
        _merge(out, {"cbwd": E.check_cbwd(tab, act, g1, gb, g2, E.emu_cbwd(tab, act, g1, gb, g2, mut))})
    _merge(out, {"cbwd": E.check_cbwd(TAB, act, g1, None, None, E.emu_cbwd(TAB, act, g1, None, None, mut))})
    return out, amb


def handover_case(mut=()):
    s, a = E.handover_rows(TAB, 8, 3)
    assert len(a) == 16
    ratio = E.pivot_ratio(TAB, a) * 64
    assert (ratio[0::2] > 1).all() and (ratio[1::2] < 1).all()
    out = {}
    for tab in (TAB, TAB_DYN):
        g, ok = E.emu_ipg(tab, s, a, mut)
        if tab is TAB and not mut:
            assert ok[0::2].all() and not ok[1::2].any()
        _merge(out, {"ipg": E.check_ipg(tab, s, a, g)[0]})
    return out


def gross_rows(n, seed, scale=1.6):
    """Voltages far off any operating point: near-singular Jacobians the static order must hand to partial pivoting."""
    s, a = E.make_rows(n, seed, spread=0.0, edges=False)
    rng = np.random.RandomState(seed)
    a[:, E.VM0:E.VA0] += scale * 0.25 * rng.randn(n, 14).astype(np.float32)
    a[:, E.VA0:E.PE0] += scale * 0.8 * rng.randn(n, 14).astype(np.float32)
    return s, a


def newton_case(n, mut=(), tol=NEWTON_TOL):
    s, ap = E.basic_rows(n, n)
    z = E.emu_proposal(TAB, s, ap, None, E.NOISE_CLIP_ONLY, False, 0.0, 0, np.arange(n), 0)
    out, amb = {}, {}
    for tab in (TAB, TAB_DYN):
        outs = [E.emu_newton(tab, s, z, tol, m, mut)[0] for m in range(1, NEWTON_M + 1)]
        r, share = E.check_newton(tab, s, outs, tol)
        _merge(out, r)
        amb["newton"] = share
    return out, amb


def grg_case(n, mut=(), lr=LR, k=K, momentum=True, eps=EPS):
    s, ap = E.basic_rows(n, n)
    z = E.emu_proposal(TAB, s, ap, None, E.NOISE_CLIP_ONLY, False, 0.0, 0, np.arange(n), 0)
    start = E.emu_newton(TAB, s, z, 1e-5, 50)[0]
    outs, iters = E.emu_grg(TAB, s, start, k, lr, eps, 0.0, mut)
    out, share = E.check_grg(TAB, s, list(outs), [np.minimum(iters, j) for j in range(k + 1)], lr, eps)
    amb_stops = (int((iters < k).sum()), int((iters == k).sum()))
    amb = {"grg": share}
    grg_case.last_counts = amb_stops
    if momentum:
        o, it = E.emu_grg(TAB, s, start, k, lr, eps, 0.5, mut)
        r, left = E.check_momentum(TAB, s, start, o[-1], it, k, lr, eps, 0.5)
        _merge(out, r)
        amb["grg_mom"] = left
    return out, amb


def proposal_case(n):
    s, ap = E.basic_rows(n, n)
    rng = np.random.RandomState(n)
    noise, raw = rng.randn(n, 14).astype(np.float32), (2.0 * rng.randn(n, 14)).astype(np.float32)
    out = {}
    eps_t = E.eps_at(0.5, 0.05, 0.01, 5)
    for mode in range(5):
        for is_raw in (False, True):
            x = raw if is_raw else ap
            z = E.emu_proposal(TAB, s, x, noise, mode, is_raw, eps_t, 7, np.arange(n) + 3, 5)
            _merge(out, E.check_proposal(TAB, s, x, noise, mode, is_raw, eps_t, 7, np.arange(n) + 3, 5, z))
    return out


@pytest.fixture(scope="module")
def emulation():
    """Every checker on the unmutated emulation, once: ({group: worst ratio}, {comparison: largest ambiguous share})."""
    out, amb = {}, {}
    for n in E.LANES:
        r, a = closed_forms(n)
        _merge(out, r)
        _merge(amb, a)
    for n in E.LAG_ROWS:
        r, a = lagrangian_case(n)
        _merge(out, r)
        _merge(amb, a)
    for n in (5, 65, 257):
        r, a = solve_case(n)
        _merge(out, r)
        _merge(amb, a)
        _merge(out, proposal_case(n))
    _merge(out, handover_case())
    for n in (5, 65, 257):
        r, a = newton_case(n)
        _merge(out, r)
        _merge(amb, a)
    r, a = grg_case(64)
    _merge(out, r)
    _merge(amb, a)
    assert grg_case.last_counts[0] >= 1 and grg_case.last_counts[1] >= 32     # feasible lanes stop after step 0, the others take all ten
    for kw in (dict(lr=LR_BIG, k=2), dict(eps=EPS_BIG, k=3)):
        r, a = grg_case(65, momentum=False, **kw)
        _merge(out, r)
        _merge(amb, a)
    assert min(grg_case.last_counts) >= 1                      # corr_eps on both sides of the lanes' largest violations
    return out, amb


def test_emulation_passes_every_checker(emulation):
    out, _ = emulation
    print({k: round(v, 3) for k, v in sorted(out.items())})
    assert set(out) >= set(E.C_REF) - {"grg_mom"}
    for group, ratio in out.items():
        assert ratio <= 1.0, (group, ratio)


def test_yardstick(emulation):
    """C_REF[group] is the emulation's own worst error in units of eps32 * bound (ratio * MARGIN * C_REF), rounded up: fails on
    a drift beyond 2x, so the constants of evopf_f64.py cannot go stale."""
    out, _ = emulation
    for group, c in E.C_REF.items():
        measured = out[group] * E.MARGIN * c
        print("%-12s measured %.4f  C_REF %.3f" % (group, measured, c))
        assert 0.5 * c <= measured <= c, (group, measured, c)


def test_ambiguous_rows_stay_under_the_cap(emulation):
    _, amb = emulation
    print({k: round(v, 4) for k, v in sorted(amb.items())})
    for name, share in amb.items():
        assert share <= E.AMBIG_CAP, (name, share)


MUTATIONS = [
    ("jac_sign_block", lambda m: solve_case(65, m)[0]),                 # a sign in one Jacobian block (d real / d angle)
    ("battery_autograd_sign", lambda m: solve_case(65, m)[0]),          # the autograd sign of the battery columns where eq_jac's is due
    ("vjp_sign_swapped", lambda m: closed_forms(65, m)[0]),             # ... and eq_jac's where the autograd sign is asked for
    ("dead_fill_in", lambda m: solve_case(65, m)[0]),                   # one fill-in column treated as dead
    ("ge_mask", lambda m: lagrangian_case(257, m)[0]),                  # >= for > in a bound mask (g_j exactly 0 is in the rows)
    ("lr_other_only", lambda m: grg_case(64, m, k=2, momentum=False)[0]),   # lr applied to the `other` block only
    ("stop_inf_norm", lambda m: newton_case(65, m, tol=3e-3)[0]),       # Newton stop on the inf-norm of delta
    ("tail_before_update", lambda m: newton_case(65, m)[0]),            # qg taken before the last update
    ("eff_swapped", lambda m: closed_forms(65, m)[0]),                  # battery efficiency branches swapped
    ("clip_after_eff", lambda m: closed_forms(65, m)[0]),               # the clip applied after the efficiency
    ("t24_not_zeroed", lambda m: closed_forms(65, m)[0]),               # t >= 24 not zeroed
    ("price_shift", lambda m: closed_forms(65, m)[0]),                  # price window shifted by one hour
    ("price_past_midnight", lambda m: closed_forms(65, m)[0]),          # the window not zero past midnight
    ("no_relu_viol", lambda m: closed_forms(65, m)[0]),                 # fmaxf(ineq, 0) missing in the stored violations
    ("no_pe_in_balance", lambda m: closed_forms(65, m)[0]),             # pe left out of the active-power balance
    ("pivot_twice", lambda m: solve_case(65, m)[0]),                    # a pivot normalised twice
    ("no_k0", lambda m: grg_case(64, m, k=2, momentum=False)[0]),       # the stop test applied before the first iteration
    ("never_overwrite", lambda m: lagrangian_case(257, m)[0]),          # overwrite = 1 accumulating onto the old loss
]


@pytest.mark.parametrize("name,run", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_mutation_fails_a_checker(name, run):
    out = run((name,))
    assert max(out.values()) > 1.0, (name, out)


def test_reward_without_the_constant_cost_term_fails():
    """case14's cost constants c0 are all zero, so the term only shows with a table whose RPO_EVOPF_C_CONST is not."""
    tab = TAB.copy()
    tab[E.OFF["CONST"]] = np.float32(0.37)
    s, a = E.make_rows(65, 65)
    assert max(E.check_step(tab, s, a, E.emu_step(tab, s, a)).values()) <= 1.0
    assert E.check_step(tab, s, a, E.emu_step(tab, s, a, ("reward_no_const",)))["step_reward"] > 1.0


def test_pivot_test_off_fails_on_near_singular_rows():
    """Without the 2^-6 pivot-ratio test the static order keeps rows it must hand to partial pivoting: the bound catches it on
    grossly perturbed voltages (pivot ratios down to 1e-8), where the unmutated emulation (and partial pivoting alone) stay inside.
    The componentwise bound grows with the conditioning of the row, so it only convicts the static order where its pivot growth
    is what loses the digits: the 2^-6 test is far on the safe side of that."""
    s, a = gross_rows(128, 4)
    g, ok = E.emu_ipg(TAB, s, a)
    assert ok.any() and ok.mean() < 0.5
    assert E.check_ipg(TAB, s, a, g)[0] <= 1.0
    assert E.check_ipg(TAB, s, a, E.emu_ipg(TAB_DYN, s, a)[0])[0] <= 1.0
    assert E.check_ipg(TAB, s, a, E.emu_ipg(TAB, s, a, ("no_pivot_test",))[0])[0] > 1.0


def test_nan_row_stop_count_is_the_reference_s():
    """rpo_ddpg.py:271-272: torch.max propagates a NaN and NaN > corr_eps is false, so a term that holds a NaN cannot keep the loop
    going.  A NaN pe at the slack generator enters no Newton equation: the completed action is finite but for that pe and the slack
    pg = -resid; after the unconditional step 0 both max |eq_resid| and max ineq_dist are NaN: ONE iteration, whatever the other
    components violate.  A stop test that drops the NaN (fmaxf) iterates on the finite violations to the budget."""
    s, ap = E.basic_rows(8, 8)
    ap[3, 9] = np.nan
    start = E.emu_newton(TAB, s, ap, 1e-5, 50)[0]
    assert np.isnan(start[3]).sum() == 2 and np.isnan(start[3, [E.PG0, E.PE0]]).all()
    outs, iters = E.emu_grg(TAB, s, start, 6, LR, EPS)
    assert iters[2] == 6 and iters[3] == 1
    assert E.check_grg(TAB, s, list(outs), [np.minimum(iters, j) for j in range(7)], LR, EPS)[0]["grg"] <= 1.0
    outs_m, iters_m = E.emu_grg(TAB, s, start, 6, LR, EPS, mut=("nan_dropped",))
    assert iters_m[3] == 6
    assert E.check_grg(TAB, s, list(outs_m), [np.minimum(iters_m, j) for j in range(7)], LR, EPS)[0]["grg"] > 1.0


def test_formulas_against_the_oracle_and_the_reference_fixtures():
    """The float64 side (B64E, float32 table) against oracle/evopf.py (float64 tables) and the reference's own float32 results, at
    the oracle tests' tolerances: the restatement is the same functions."""
    s, a = E.make_rows(64, 3)
    s64, a64 = s.astype(np.float64), a.astype(np.float64)
    c = E.Tab(E.B64E, TAB)
    S, Ac = E.cols(E.B64E, s), E.cols(E.B64E, a)
    eq = E.val(E.B64E, E.eq_resid(E.B64E, c, S, Ac, E.flows(E.B64E, c, Ac)))
    np.testing.assert_allclose(eq, oe.eq_resid(s64, a64), atol=2e-5)
    np.testing.assert_allclose(E.val(E.B64E, E.ineq_resid(E.B64E, c, S, Ac)), oe.ineq_resid(s64, a64), atol=2e-6)
    jv, _ = E.dense_jac(TAB, a)
    np.testing.assert_allclose(jv, oe.eq_jac(a64), atol=2e-5)
    st = E.step(E.B64E, c, S, Ac)
    hours = np.arange(64) % 24
    want = oe.step(s64, a64, hours.astype(np.int64), np.ones(64, np.int64), 5, np.arange(64), auto_reset=False)
    np.testing.assert_allclose(st["reward"].v, want["reward"], rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(E.val(E.B64E, st["soc"]), want["next_state"][:, 28:33], atol=1e-6)
    obs = E.episode_obs(E.B64E, c, 5, np.arange(64), np.ones(64, np.int64), hours + 1)
    got = E.val(E.B64E, [obs[j] for j in E.DATA_COLS])
    np.testing.assert_allclose(got, want["next_state"][:, E.DATA_COLS], rtol=1e-5, atol=2e-5)
    smooth, asm = E.make_rows(32, 6, spread=0.03, edges=False)
    full = np.array([E.reduced_grad_ref(j, m, g[0])[0] for j, m, g in
                     zip(*E.dense_jac(TAB, asm), E.mask_choices(*E.mask_margins(TAB, smooth, asm)))])
    ref = oe.ineq_partial_grad(smooth.astype(np.float64), asm.astype(np.float64))
    np.testing.assert_allclose(full, ref, atol=2e-3 * np.abs(ref).max())
    fx = golden("evopf_env")
    jv, _ = E.dense_jac(TAB, fx["AX"])
    got = np.array([E.reduced_grad_ref(j, np.zeros_like(j), g[0])[0] for j, g in
                    zip(jv, E.mask_choices(*E.mask_margins(TAB, fx["S"], fx["AX"])))])
    np.testing.assert_allclose(got, fx["ineq_partial_grad"], atol=2e-3 * np.abs(fx["ineq_partial_grad"]).max())
    a_f = E.emu_newton(TAB, fx["S"], fx["AP"], 1e-5, 50)[0]
    np.testing.assert_allclose(a_f, fx["A"], atol=5e-5)
    step_fx = golden("evopf_step")
    c2 = E.Tab(E.B64E, TAB)
    r = E.step(E.B64E, c2, E.cols(E.B64E, step_fx["state"]), E.cols(E.B64E, step_fx["action"]))
    np.testing.assert_allclose(r["reward"].v, step_fx["reward"], rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(E.val(E.B64E, r["eq"]), step_fx["eq_viol"], atol=2e-5)
    np.testing.assert_allclose(E.val(E.B64E, r["ineq"]), step_fx["ineq_viol"], atol=2e-6)
