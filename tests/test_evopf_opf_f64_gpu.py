"""``evopf_opf_kernel`` on the MI355X held to float64 ONE ITERATION AT A TIME through the state seam (``rpo_evopf_opf_state``:
state_in / state_out rows of 168 floats), the way tests/test_evopf_f64_gpu.py holds the Newton and GRG loops.  The yardstick, its
bound, the measured constants and the inputs are tests/evopf_opf_f64.py's (``step_ref``, ``C_REF``, ``fixture_rows``,
``opf_states``); tests/test_evopf_opf.py shows on the CPU, with the float32 emulation in the kernel's place and on these same
inputs, that 14 seeded mutations of the iteration each fail a checker here.

Inputs: the 70 rows of test_evopf_opf_gpu (65 feasible + the fixture's 5 infeasible) along their own trajectories k = 0 .. 12, and
``opf_states(65, 3)`` under the case's constants table and under one with a phase shifter (an asymmetric Ybus: the case's own is
exactly symmetric, so on it Yr / Yi read transposed or not is the same thing).  Launches of n = 1, 3, 4, 5 and 65 rows: one wave, a
ragged workgroup of four, a full one, one over, seventeen workgroups with a one-wave tail.  Every output and state buffer has
sentinel words behind it.  What the kernel reports of the stop test is ``residual`` (the largest of the three quantities): that is
what is judged on the device; the three one by one are judged on the emulation.  Every test prints its ratios under ``-s``.
"""
import functools

import numpy as np
import pytest
import torch

import evopf_f64 as E
import evopf_opf_f64 as opf64
from test_envs_f64_gpu import Buf

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
SIZES = (1, 3, 4, 5, 65)
TINY_TOL = 1e-30            # no lane stops
SEED, NSYN, KMAX = 3, 65, 12
TOL = 1e-4


@functools.lru_cache(maxsize=None)
def _setup():
    """(ops, {table name: (table, EvopfKernels)}, demand [70, 28], pe [70, 5]) -- computed once, shared and left unchanged."""
    from rpo_amd import ops
    assert torch.cuda.is_available()
    tab = E.consts_table()
    tabs = {"case": tab, "shifted": opf64.shifted_table(tab)}
    demand, pe = opf64.fixture_rows()
    return ops, {k: (t, ops.EvopfKernels(t)) for k, t in tabs.items()}, demand, pe


def launch(demand, pe=None, state_in=None, tol=TINY_TOL, max_iters=1, table="case", state_out=True):
    """One launch through ``ops.evopf_opf`` on sentinel-backed buffers prefilled with NaN -> dict(action, info, state or None)."""
    ops, tabs, _, _ = _setup()
    n = demand.shape[0]
    nan = lambda *shape: np.full(shape, np.nan, np.float32)                                                 # noqa: E731
    action, info, out = Buf(nan(n, 43)), Buf(nan(n, 4)), (Buf(nan(n, 168)) if state_out else None)
    d = torch.from_numpy(np.ascontiguousarray(demand, np.float32)).to(DEV)
    p = None if pe is None else torch.from_numpy(np.ascontiguousarray(pe, np.float32)).to(DEV)
    s = None if state_in is None else Buf(state_in)
    ops.evopf_opf(tabs[table][1], d, p, action.view, info.view, tol, max_iters, state_in=None if s is None else s.view,
                  state_out=None if out is None else out.view)
    torch.cuda.synchronize()
    if s is not None:
        assert np.array_equal(E.bits(s.get()), E.bits(np.asarray(state_in, np.float32))), "the launch wrote its input"
    return dict(action=action.get(), info=info.get(), state=None if out is None else out.get())


def same(a, b):
    """bitwise, NaNs included"""
    return a.shape == b.shape and np.array_equal(E.bits(a), E.bits(b))


@functools.lru_cache(maxsize=None)
def _trajectory():
    """The kernel's own states after k = 0 .. 12 single steps on the 70 rows [13, 70, 168], every launch max_iters = 1 from the
    state_out before it."""
    _, _, demand, pe = _setup()

    def run(state, iters):
        r = launch(demand, pe=pe if state is None else None, state_in=state, max_iters=iters)
        assert (r["info"][:, 2] == iters).all() and not r["info"][:, 3].any()
        return r["state"]
    return opf64.trajectory_states(run, KMAX)


@functools.lru_cache(maxsize=None)
def _synthetic(table):
    ops, tabs, _, _ = _setup()
    demand, states = opf64.opf_states(NSYN, SEED, tabs[table][0])
    return demand, states, opf64.step_ref(tabs[table][0], demand, states)


def _rows(ref, n):
    return {k: v[:n] for k, v in ref.items()}


# ------------------------------------------------------------------------------------------------ 1, 2: one step against float64
def test_one_step_at_a_time_along_the_trajectories():
    _, tabs, demand, pe = _setup()
    states = _trajectory()
    worst, left_k = {}, []
    for k in range(KMAX + 1):
        ref = opf64.step_ref(tabs["case"][0], demand, states[k])
        at = launch(demand, state_in=states[k], max_iters=0, state_out=False)
        r = {"opf_stop": opf64.check_stop(ref, at["info"][:, 1])[0]}
        left = np.zeros(70, bool)
        if k < KMAX:
            step, left = opf64.check_step(ref, states[k + 1])
            r.update(step)
        print("k=%2d %s not judged %s" % (k, {g: round(v, 3) for g, v in sorted(r.items())}, np.nonzero(left)[0].tolist()))
        left_k.append(left)
        for g, v in r.items():
            worst[g] = max(worst.get(g, 0.0), v)
    print("worst", {g: round(v, 3) for g, v in sorted(worst.items())})
    left_k = np.stack(left_k)
    # not judged (a step length beyond first order): none before k = 4, feasible rows only once they have converged (k >= 10)
    assert not left_k[:4].any() and not left_k[:10, :65].any() and left_k[:, :65].mean() <= 0.05
    for g, v in worst.items():
        assert v <= 1.0, (g, v)


@pytest.mark.parametrize("n,table", [(n, "case") for n in SIZES] + [(NSYN, "shifted")])
def test_one_step_from_the_synthetic_states(n, table):
    demand, states, ref = _synthetic(table)
    out = launch(demand[:n], state_in=states[:n], max_iters=1, table=table)
    at = launch(demand[:n], state_in=states[:n], max_iters=0, table=table)
    r, left = opf64.check_step(_rows(ref, n), out["state"])
    r["opf_stop"], unj = opf64.check_stop(_rows(ref, n), at["info"][:, 1])
    print("n=%d %s: %s not judged %s" % (n, table, {g: round(v, 3) for g, v in sorted(r.items())}, np.nonzero(left)[0].tolist()))
    assert same(at["state"], states[:n]) and same(at["action"], states[:n, :43]) and (at["info"][:, 2] == 0).all()
    special = set(range(min(n, opf64.N_SPECIAL))) - {9}
    assert not special & set(np.nonzero(left)[0]) and not special & set(np.nonzero(unj)[0])     # the rows built for a purpose: judged
    assert left.sum() <= 0.4 * max(n, 10)
    for g, v in r.items():
        assert v <= 1.0, (g, v)
    if n > 9:                                                     # the NaN in lambda only propagates
        assert np.isnan(at["info"][9, 1]) and at["info"][9, 3] == 0 and out["info"][9, 2] == 1 and np.isnan(out["info"][9, 1])


# ------------------------------------------------------------------------------------------------ 3: the stop decision, exact
def test_stop_decision_is_the_kernels_own_residual_against_tol():
    _, tabs, demand, pe = _setup()
    states = _trajectory()
    seen = set()
    for k in (7, 8, 9):                                            # iterates around the stop: residuals on both sides of a tolerance
        ref = opf64.step_ref(tabs["case"][0], demand, states[k], bound=False)
        tol = float(np.median(ref["stop"][:, 3]))
        r = launch(demand, state_in=states[k], tol=tol, max_iters=0, state_out=False)
        want = r["info"][:, 1] < np.float32(tol)
        assert np.array_equal(r["info"][:, 3] != 0, want), k
        assert want.any() and not want.all(), (k, tol)
        seen |= set(want.tolist())
    assert seen == {True, False}
    full = launch(demand, pe=pe, tol=TOL, max_iters=40)
    want = full["info"][:, 1] < np.float32(TOL)
    assert np.array_equal(full["info"][:, 3] != 0, want) and want.sum() == 65
    assert (full["info"][~want, 2] == 40).all() and (full["info"][want, 2] < 40).all()
    d, s, _ = _synthetic("case")                                   # a NaN residual means not converged, at any tolerance
    r = launch(d[:12], state_in=s[:12], tol=1e30, max_iters=0, state_out=False)
    assert np.isnan(r["info"][9, 1]) and r["info"][9, 3] == 0 and (r["info"][np.arange(12) != 9, 3] == 1).all()


# ------------------------------------------------------------------------------------------------ 4: the seam, bitwise
def test_seam_is_consistent_bitwise():
    ops, tabs, demand, pe = _setup()
    a, b = 3, 4
    first = launch(demand, pe=pe, max_iters=a)
    second = launch(demand, state_in=first["state"], max_iters=b)
    whole = launch(demand, pe=pe, max_iters=a + b)
    assert same(second["action"], whole["action"]) and same(second["state"], whole["state"])
    assert same(second["info"][:, [0, 1, 3]], whole["info"][:, [0, 1, 3]])
    assert (first["info"][:, 2] == a).all() and (second["info"][:, 2] == b).all() and (whole["info"][:, 2] == a + b).all()
    for r in (first, second, whole):
        assert same(r["state"][:, :43], r["action"])
    # rpo_evopf_opf == rpo_evopf_opf_state with both pointers NULL == with state_out alone
    plain = launch(demand, pe=pe, tol=TOL, max_iters=40, state_out=False)
    with_out = launch(demand, pe=pe, tol=TOL, max_iters=40)
    nan = lambda *shape: np.full(shape, np.nan, np.float32)                                                 # noqa: E731
    action, info = Buf(nan(70, 43)), Buf(nan(70, 4))
    d, p = torch.from_numpy(demand).to(DEV), torch.from_numpy(pe).to(DEV)
    from rpo_amd import _lib
    _lib.check(_lib.load().rpo_evopf_opf_state(70, ops._p(d), 28, ops._p(p), ops._p(action.view), ops._p(info.view), TOL, 40,
                                               tabs["case"][1]._c(d), None, None, ops._stream()), "rpo_evopf_opf_state")
    torch.cuda.synchronize()
    for r in (with_out, dict(action=action.get(), info=info.get())):
        assert same(plain["action"], r["action"]) and same(plain["info"], r["info"])
    # the flat start given as a state is the flat start
    flat = opf64.flat_state32(tabs["case"][0], pe)
    given = launch(demand, state_in=flat, tol=TOL, max_iters=40)
    assert same(given["action"], with_out["action"]) and same(given["info"], with_out["info"]) and same(given["state"], with_out["state"])
    assert same(launch(demand, pe=pe, max_iters=0)["state"], flat)


def test_rows_do_not_depend_on_their_neighbours_nan_row_included():
    d, s, _ = _synthetic("case")
    assert np.isnan(s[9]).any() and 9 % 4 in (1, 2)                # the NaN row sits in the middle of its workgroup
    base = launch(d, state_in=s, tol=TOL, max_iters=3)
    assert np.isnan(base["info"][9, 1]) and base["info"][9, 3] == 0 and base["info"][9, 2] == 3
    perm = np.random.default_rng(0).permutation(NSYN)
    shuffled = launch(d[perm], state_in=s[perm], tol=TOL, max_iters=3)
    for k in ("action", "info", "state"):
        assert same(base[k][perm], shuffled[k]), k
    s2 = s.copy()
    s2[9] = s[0]                                                   # the same workgroup without the NaN: its neighbours' bits stay
    clean = launch(d[8:12], state_in=s2[8:12], tol=TOL, max_iters=3)
    for k in ("action", "info", "state"):
        assert same(base[k][[8, 10, 11]], clean[k][[0, 2, 3]]), k


# ------------------------------------------------------------------------------------------------ 5: iteration counts
def test_iteration_counts_against_the_helper():
    _, _, demand, pe = _setup()
    iters, conv, decisive = opf64.iteration_classes(demand, pe, TOL)
    out = launch(demand, pe=pe, tol=TOL, max_iters=40, state_out=False)
    got, gconv = out["info"][:, 2].astype(np.int32), out["info"][:, 3] != 0
    both = conv & gconv
    print("converged %d (helper %d), iterations %d..%d (helper %d..%d), |difference| <= %d; held to equality: %d of %d"
          % (gconv.sum(), conv.sum(), got[both].min(), got[both].max(), iters[both].min(), iters[both].max(),
             np.abs(got - iters)[both].max(), (decisive & both).sum(), both.sum()))
    assert both.sum() == 65 and np.array_equal(conv, gconv)
    assert (np.abs(got - iters)[both] <= 1).all()
    assert np.array_equal(got[decisive & both], iters[decisive & both])
    assert (decisive & both).sum() * 3 >= both.sum()


# ------------------------------------------------------------------------------------------------ 6: whole trajectories
def test_whole_trajectories_within_the_sum_of_the_step_tolerances():
    _, tabs, demand, pe = _setup()
    got = [launch(demand, pe=pe, max_iters=k)["state"] for k in range(KMAX + 1)]
    ratio, left = opf64.trajectory_ratios(tabs["case"][0], demand, pe, got)
    for k in range(KMAX + 1):
        print("k=%2d worst %.3g (row %d), left out %d" % (k, ratio[k].max(), ratio[k].argmax(), left[k].sum()))
    assert not left[:5].any() and left[:, :65].mean() <= 0.05
    over = np.argwhere(ratio > 1.0)
    assert not len(over), [(int(k), int(r), float(ratio[k, r])) for k, r in over[:10]]


# ------------------------------------------------------------------------------------------------ 7: cost
@pytest.mark.parametrize("n", SIZES)
def test_cost_is_obj_fn_of_the_returned_point(n):
    _, tabs, demand, pe = _setup()
    out = launch(demand[:n], pe=pe[:n], tol=TOL, max_iters=40, state_out=False)
    r, unj = opf64.ratios("opf_cost", out["info"][:, 0], *opf64.cost_ref(tabs["case"][0], out["action"]))
    print("n=%d cost: worst ratio %.3f" % (n, r.max()))
    assert not unj.any() and r.max() <= 1.0


# ------------------------------------------------------------------------------------------------ 8: refusal
def test_pe_with_state_in_is_refused_before_any_launch():
    ops, tabs, demand, pe = _setup()
    from rpo_amd import _lib
    from rpo_amd.env import EVOPFEnv
    n = 4
    sent = np.full((n, 43), 7.0, np.float32)
    action, info, state = Buf(sent), Buf(np.full((n, 4), 7.0, np.float32)), Buf(np.full((n, 168), 7.0, np.float32))
    d, p = torch.from_numpy(demand[:n]).to(DEV), torch.from_numpy(pe[:n]).to(DEV)
    s = torch.from_numpy(opf64.flat_state32(tabs["case"][0], pe[:n])).to(DEV)
    rc = _lib.load().rpo_evopf_opf_state(n, ops._p(d), 28, ops._p(p), ops._p(action.view), ops._p(info.view), TOL, 40,
                                         tabs["case"][1]._c(d), ops._p(s), ops._p(state.view), ops._stream())
    torch.cuda.synchronize()
    assert rc == _lib.CONST["RPO_ERR_ARG"]
    assert (action.get() == 7.0).all() and (info.get() == 7.0).all() and (state.get() == 7.0).all()      # nothing ran
    with pytest.raises(_lib.RpoHipError, match="pe must be None"):
        ops.evopf_opf(tabs["case"][1], d, p, action.view, info.view, TOL, 40, state_in=s)
    with pytest.raises(ValueError, match="pe"):
        EVOPFEnv(device=DEV).opf(d, pe=p, state_in=s)
    assert (action.get() == 7.0).all() and (info.get() == 7.0).all()
