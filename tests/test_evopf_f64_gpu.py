"""The EVOPF-v0 launches (rpo_evopf_resid, _eq_vjp, _ineq_partial_grad, _complete_bwd, _lagrangian, _act_project, _reset, _step) called
through rpo_amd.ops against the float64 yardstick of tests/evopf_f64.py.  Needs an MI355X.

Every element of every output within MARGIN (4) * C_REF[group] * eps32 * bound of float64 (plus the explicit intrinsic ulps), the
bound being the running magnitude sum for closed forms and the componentwise |inv J| ((|J| + m_J) |x| + |b| + m_b) for everything
that passes through a solve; at 1, 3, 4, 5, 63, 64, 65 and 257 lanes (four lanes share a workgroup) and 1, 255, 256, 257 and 513
rows of the Lagrangian, with strided observations, NULL optional outputs and sentinel words behind every buffer.  Iterative paths
are held ONE iteration at a time from the kernel's own previous iterate (max_steps = k / newton_max_iters = m for every k, m); stop
decisions and iteration counts exactly, except lanes whose float64 stop quantity or mask lies within its own bound of the
threshold (both outcomes accepted, at most 2 % of a comparison).  The static elimination order and RPO_EVOPF_PIVOT=dynamic are
each judged against float64, never against each other.  Every test prints its ratios (1 = the tolerance) under -s.
"""
import os

import numpy as np
import pytest
import torch

import evopf_f64 as E
from test_envs_f64_gpu import Buf, bits, check_stats, new_ctrl

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = -12345.0
TAB = E.consts_table()
LR, EPS, K = 1e-4, 1e-4, 10                     # (see test_evopf_f64.py: corr_eps 1e-5 lies inside the bound of a balance)
NEWTON_TOL, NEWTON_M = 1e-3, 6
NU = np.random.RandomState(8).uniform(0, 1, 58).astype(np.float32)
NU[::7] = 0.0
WORST, AMBIG = {}, {}


@pytest.fixture(scope="module")
def ops():
    from rpo_amd import ops as _ops
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    yield _ops
    print("\nworst ratios (1 = tolerance):", {k: round(v, 3) for k, v in sorted(WORST.items())})
    print("largest ambiguous shares:", {k: round(v, 4) for k, v in sorted(AMBIG.items())})


@pytest.fixture(scope="module")
def kern(ops):
    k = ops.EvopfKernels(TAB)
    assert k.static_order
    return k


@pytest.fixture(scope="module")
def kern_dyn(ops):
    old = os.environ.get("RPO_EVOPF_PIVOT")
    os.environ["RPO_EVOPF_PIVOT"] = "dynamic"
    try:
        k = ops.EvopfKernels(TAB)
    finally:
        if old is None:
            del os.environ["RPO_EVOPF_PIVOT"]
        else:
            os.environ["RPO_EVOPF_PIVOT"] = old
    assert not k.static_order
    return k


def note(ratios, ambig=None):
    for group, value in ratios.items():
        value = float(value)
        WORST[group] = max(WORST.get(group, 0.0), value)
        print("%-12s ratio %.3f" % (group, value))
        assert value <= 1.0, (group, value)
    for name, share in (ambig or {}).items():
        AMBIG[name] = max(AMBIG.get(name, 0.0), float(share))
        assert share <= E.AMBIG_CAP, (name, share)


class Strided(object):
    """[n, 57] observations as a row view of a [n, 64] buffer (state_stride = 64), sentinels in the gaps and behind."""

    def __init__(self, s):
        n = s.shape[0]
        host = np.full((n + 1, 64), SENT, np.float32)
        host[:n, :57] = s
        self.buf = torch.from_numpy(host).to(DEV)
        self.view = self.buf[:n, :57]
        self.host = host

    def check(self):
        assert (bits(self.buf.cpu().numpy()) == bits(self.host)).all(), "the launch wrote into its observations"


def out_buf(n, d, dtype=torch.float32):
    return Buf(np.full((n, d) if d else (n,), SENT if dtype == torch.float32 else 0x5A5A5A5A), dtype)


# ================================================================================================================ closed forms
@pytest.mark.parametrize("n", E.LANES)
def test_resid(kern, n):
    s, a = E.make_rows(n, n)
    S, A = Strided(s), Buf(a)
    eq, iq = out_buf(n, 28), out_buf(n, 58)
    kern.resid(S.view, A.view, eq.view, iq.view)
    note(E.check_resid(TAB, s, a, eq.get(), iq.get()))
    eq2, iq2 = out_buf(n, 28), out_buf(n, 58)
    kern.resid(S.view, A.view, eq2.view, None)
    kern.resid(S.view, A.view, None, iq2.view)
    assert (bits(eq2.get()) == bits(eq.get())).all() and (bits(iq2.get()) == bits(iq.get())).all()
    S.check()


@pytest.mark.parametrize("sign", [0, 1])
@pytest.mark.parametrize("n", E.LANES)
def test_eq_vjp(kern, n, sign):
    _, a = E.make_rows(n, n)
    ge = np.random.RandomState(n).randn(n, 28).astype(np.float32)
    out = out_buf(n, 43)
    kern.eq_vjp(Buf(a).view, Buf(ge).view, out.view, autograd_sign=sign)
    note(E.check_vjp(TAB, a, ge, out.get(), sign))


@pytest.mark.parametrize("overwrite", [0, 1])
@pytest.mark.parametrize("n", E.LAG_ROWS)
def test_lagrangian(kern, n, overwrite):
    """grad_action (g_j exactly 0 and +-1 ulp are in the rows; nu has zeros), grad_nu accumulated onto non-zero values, the loss
    written or accumulated; NULL optional outputs; two runs give the same bits."""
    s, a = E.mask_rows(n, n, spread=0.05)
    gnu0 = np.random.RandomState(n).uniform(0, 1, 58).astype(np.float32)
    S, A, N = Strided(s), Buf(a), Buf(NU)
    runs = []
    for _ in range(2):
        loss, g, gnu = Buf(np.array([0.7], np.float32)), out_buf(n, 43), Buf(gnu0)
        kern.lagrangian(A.view, N.view, 1.0 / n, loss.view, g.view, gnu.view, obs=S.view, overwrite=overwrite)
        runs.append((loss.get(), g.get(), gnu.get()))
    assert all((bits(x) == bits(y)).all() for x, y in zip(*runs))
    loss, g, gnu = runs[0]
    r, amb = E.check_lagrangian(TAB, s, a, NU, 1.0 / n, 0.7, gnu0, overwrite, float(loss[0]), g, gnu)
    note(r, {"lagrangian": amb})
    loss2 = Buf(np.array([0.7], np.float32))
    kern.lagrangian(A.view, N.view, 1.0 / n, loss2.view, None, None, obs=S.view, overwrite=overwrite)
    assert bits(loss2.get())[0] == bits(loss)[0]
    g2 = out_buf(n, 43)
    kern.lagrangian(A.view, N.view, 1.0 / n, None, g2.view, None, obs=S.view, overwrite=overwrite)
    assert (bits(g2.get()) == bits(g)).all()
    zero = Buf(np.zeros(58, np.float32))
    lz, gz = Buf(np.array([0.7], np.float32)), out_buf(n, 43)
    kern.lagrangian(A.view, zero.view, 1.0 / n, lz.view, gz.view, None, obs=S.view, overwrite=1)
    assert float(lz.get()[0]) == 0.0 and not gz.get().any()                         # nu = 0
    S.check()


# ================================================================================================================ reset and step
@pytest.mark.parametrize("n", E.LANES)
def test_reset(kern, n):
    seed, base = 77, 5
    count = (np.arange(n) % 7).astype(np.int32)
    st, L, R, C = out_buf(n, 57), out_buf(n, 0, torch.int32), out_buf(n, 0), Buf(count, torch.int32)
    kern.reset(st.view, st.view, L.view, R.view, C.view, seed, base)
    got = st.get()
    r, unj = E.check_episode(TAB, seed, base + np.arange(n), count, np.zeros(n, np.int64), got[:, E.DATA_COLS])
    note(r, {"episode": unj})
    assert (bits(got[:, 28:33]) == bits(np.float32(0.2))).all()                      # the one part without a transcendental
    assert not L.get().any() and not R.get().any() and (C.get() == count).all()


def step_words(n, seed, max_steps):
    rng = np.random.RandomState(seed)
    ep_len = rng.choice([0, 5, 21, 22, 23, max_steps - 1, max_steps - 2], n).astype(np.int32)
    ep_len[:4] = [0, 22, 23, 21][:n]
    return ep_len, rng.uniform(-50, 0, n).astype(np.float32), rng.randint(0, 5, n).astype(np.int32)


def run_step(ops, kern, s, a, words, max_steps, auto_reset, seed, base, rows=True, stats=True, ctrl=True, t=5, cap=3):
    n = s.shape[0]
    S, A = Buf(s), Buf(a)
    L, R, C = Buf(words[0], torch.int32), Buf(words[1]), Buf(words[2], torch.int32)
    ring = Buf(np.full((cap * n, 248), SENT, np.float32)) if rows else None
    sts = ops.new_stats(8, DEV) if stats else None
    c = new_ctrl(ops, t) if ctrl else None
    kern.step(S.view, S.view, A.view, L.view, R.view, C.view, ring.view if rows else None, cap, sts, c, max_steps, auto_reset, 1e-3,
              seed, base)
    torch.cuda.synchronize()
    return dict(state=S.get(), action=A.get(), ep_len=L.get(), ep_ret=R.get(), ep_count=C.get(), ring=ring.get() if rows else None,
                stats=sts, ctrl=c.cpu().numpy() if ctrl else None)


@pytest.mark.parametrize("auto_reset,max_steps", [(True, 24), (False, 24), (True, 12)])
@pytest.mark.parametrize("n", E.LANES)
def test_step(ops, kern, n, auto_reset, max_steps):
    """Hours 0, 22, 23, 24 (the last data hour, done, the all-zero next observation), max_episode_steps below 24, auto_reset on and
    off, the price window crossing midnight, the lanes whose Philox words are the extremes of the power-factor and exponential
    draws; copies, done, episode words, statistics and the ctrl words exactly; the flag stays down."""
    seed, base, t, cap = 31, 0, 5, 3
    s, a = E.make_rows(n, n)
    words = step_words(n, n, max_steps)
    if n >= 64:
        for env, ep, hour in E.extreme_episodes(seed, n, episodes=range(5)).values():
            if hour >= 1:
                words[0][env], words[2][env] = hour - 1, ep
    got = run_step(ops, kern, s, a, words, max_steps, auto_reset, seed, base, t=t, cap=cap)
    C = kern.cols
    row = got["ring"][(t % cap) * n:(t % cap + 1) * n]
    other = np.delete(got["ring"], np.s_[(t % cap) * n:(t % cap + 1) * n], axis=0)
    assert (other == np.float32(SENT)).all()
    assert (bits(row[:, :57]) == bits(s)).all() and (bits(row[:, 57:100]) == bits(a)).all() and not row[:, 245:].any()
    nxt = row[:, C["next_state"][0]:C["next_state"][1]]
    fields = dict(eq=row[:, 159:187], ineq=row[:, 187:245], reward=row[:, 157], soc=nxt[:, 28:33])
    note(E.check_step(TAB, s, a, fields))
    length = words[0].astype(np.int64) + 1
    ids = base + np.arange(n)
    r, unj = E.check_episode(TAB, seed, ids, words[2], length, nxt[:, E.DATA_COLS])
    note(r, {"episode": unj})
    assert not nxt[length >= 24][:, E.DATA_COLS].any()                               # t >= 24: all-zero episode data
    done = (length >= 24) | (length >= max_steps)
    assert ((row[:, 158] == 1.0) == done).all() and np.isin(row[:, 158], [0.0, 1.0]).all()
    ret = words[1] + row[:, 157]                                                      # (float32 + float32)
    if auto_reset:
        fresh = got["state"][done]
        r, unj = E.check_episode(TAB, seed, ids[done], words[2][done] + 1, np.zeros(int(done.sum()), np.int64), fresh[:, E.DATA_COLS])
        note(r, {"episode": unj})
        assert (bits(fresh[:, 28:33]) == bits(np.float32(0.2))).all()
        assert (got["ep_count"] == words[2] + done).all() and (got["ep_len"] == np.where(done, 0, length)).all()
        assert (bits(got["ep_ret"]) == bits(np.where(done, np.float32(0), ret).astype(np.float32))).all()
    else:
        assert (got["ep_count"] == words[2]).all() and (got["ep_len"] == length).all() and (bits(got["ep_ret"]) == bits(ret)).all()
    keep = ~done if auto_reset else np.ones(n, bool)
    assert (bits(got["state"][keep]) == bits(nxt[keep])).all()
    max_eq = np.fmax.reduce(np.abs(row[:, 159:187]), axis=1)
    max_ineq = np.fmax.reduce(row[:, 187:245], axis=1)
    check_stats(ops, got["stats"][t], row[:, 157], done, length >= 24, np.where(done, ret, 0).astype(np.float32),
                np.where(done, length, 0), max_ineq, max_eq, 1e-3)
    assert got["ctrl"][ops.CONST["RPO_CTRL_T"]] == t + 1 and got["ctrl"][ops.CONST["RPO_CTRL_NONFINITE"]] == 0


def test_step_reward_carries_the_constant_cost_term(ops):
    """case14's cost constants c0 are all zero: the term -wg * const / scale only shows with a table whose RPO_EVOPF_C_CONST is not."""
    tab = TAB.copy()
    tab[E.OFF["CONST"]] = np.float32(0.37)
    n = 5
    s, a = E.make_rows(n, n)
    got = run_step(ops, ops.EvopfKernels(tab), s, a, step_words(n, n, 24), 24, True, 31, 0, stats=False, cap=1, t=0)
    row = got["ring"]
    fields = dict(eq=row[:, 159:187], ineq=row[:, 187:245], reward=row[:, 157], soc=row[:, 128:133])
    note(E.check_step(tab, s, a, fields))
    assert E.check_step(TAB, s, a, fields)["step_reward"] > 1.0


def test_step_nan_action_raises_the_flag_and_moves_no_other_lane(ops, kern):
    n, seed = 65, 31
    s, a = E.make_rows(n, n)
    words = step_words(n, n, 24)
    clean = run_step(ops, kern, s, a, words, 24, True, seed, 0, stats=False)
    bad = a.copy()
    bad[37, E.PG0 + 1] = np.nan
    got = run_step(ops, kern, s, bad, words, 24, True, seed, 0, stats=False, rows=False)
    assert clean["ctrl"][ops.CONST["RPO_CTRL_NONFINITE"]] == 0 and got["ctrl"][ops.CONST["RPO_CTRL_NONFINITE"]] == 6
    keep = np.arange(n) != 37
    for key in ("state", "ep_len", "ep_ret", "ep_count"):
        x, y = got[key][keep], clean[key][keep]
        assert (bits(x) == bits(y)).all() if x.dtype == np.float32 else (x == y).all()
    no_ctrl = run_step(ops, kern, s, a, words, 24, True, seed, 0, stats=False, rows=False, ctrl=False)
    assert (bits(no_ctrl["state"]) == bits(clean["state"])).all()


# ================================================================================================================ single solves
def both_orders(kern, kern_dyn):
    return ((kern, E.consts_table(True)), (kern_dyn, E.consts_table(False)))


@pytest.mark.parametrize("n", E.LANES)
def test_ineq_partial_grad(kern, kern_dyn, n):
    s, a = E.mask_rows(n, n + 1, spread=0.03)
    for k, tab in both_orders(kern, kern_dyn):
        S, out = Strided(s), out_buf(n, 43)
        k.ineq_partial_grad(S.view, Buf(a).view, out.view)
        r, amb = E.check_ipg(tab, s, a, out.get())
        note({"ipg": r}, {"ipg": amb})
        S.check()


def test_ineq_partial_grad_on_both_sides_of_the_pivot_hand_over(kern, kern_dyn):
    """Jacobians whose smallest static pivot lies just above and just below 2^-6 of the largest (found on the CPU with the
    emulation): both sides meet the same bound, in both environments; the recorded divergence fixture stays finite."""
    s, a = E.handover_rows(TAB, 8, 3)
    assert len(a) == 16
    for k, tab in both_orders(kern, kern_dyn):
        out = out_buf(16, 43)
        k.ineq_partial_grad(Buf(s).view, Buf(a).view, out.view)
        note({"ipg": E.check_ipg(tab, s, a, out.get())[0]})
    fx = np.load(os.path.join(E.HERE, "golden", "evopf_newton_divergence.npz"))
    s1, ap1 = fx["s"][None].astype(np.float32), fx["a"][None][:, E.PARTA].astype(np.float32)
    act, it = out_buf(1, 43), out_buf(1, 0, torch.int32)
    kern.act_project(Buf(s1).view, Buf(ap1).view, None, act.view, it.view, E.NOISE_NONE, 0.0, 0.0, 0.0, 0.0, 0.0, 10, LR, 1e-5, 0.0)
    g = out_buf(1, 43)
    kern.ineq_partial_grad(Buf(s1).view, Buf(act.get()).view, g.view)
    assert np.isfinite(act.get()).all() and np.isfinite(g.get()).all() and 0 <= it.get()[0] <= 10


@pytest.mark.parametrize("n", E.LANES)
def test_complete_bwd(kern, kern_dyn, n):
    s, ap = E.basic_rows(n, n)
    act = E.emu_newton(TAB, s, ap, 1e-5, 50)[0]
    rng = np.random.RandomState(n)
    g1, gb, g2 = (rng.randn(n, 43).astype(np.float32) for _ in range(3))
    for k, tab in both_orders(kern, kern_dyn):
        for b, c in ((gb, g2), (None, g2), (gb, None), (None, None)):
            out = out_buf(n, 14)
            k.complete_bwd(None, Buf(g1).view, out.view, action=Buf(act).view, grad_action_b=None if b is None else Buf(b).view,
                           grad_action2=None if c is None else Buf(c).view)
            note({"cbwd": E.check_cbwd(tab, act, g1, b, c, out.get())})


# ================================================================================================================ act_project
def project(k, s, ap, noise, mode, raw, max_steps, lr, eps, momentum, tol=None, m=None, seed=7, base=3, ctrl=None, strided=True,
            want_iters=True, eps_sched=(0.5, 0.05, 0.01)):
    n = s.shape[0]
    S = Strided(s) if strided else Buf(s)
    act, it = out_buf(n, 43), out_buf(n, 0, torch.int32)
    k.newton_tol, k.newton_max_iters = (1e-5 if tol is None else tol), (50 if m is None else m)
    try:
        k.act_project(S.view, None if ap is None else Buf(ap).view, None if noise is None else Buf(noise).view, act.view,
                      it.view if want_iters else None, mode, eps_sched[0], eps_sched[1], eps_sched[2], 0.0, 0.0, max_steps, lr, eps,
                      momentum, seed=seed, env_id_base=base, ctrl=ctrl, ap_is_raw=raw)
    finally:
        k.newton_tol, k.newton_max_iters = 1e-5, 50
    torch.cuda.synchronize()
    if strided:
        S.check()
    return act.get(), (it.get() if want_iters else None)


@pytest.mark.parametrize("raw", [False, True])
@pytest.mark.parametrize("mode", range(5))
def test_proposal_of_every_noise_mode(ops, kern, mode, raw):
    n = 65
    s, ap = E.basic_rows(n, n)
    rng = np.random.RandomState(n)
    noise, rawv = rng.randn(n, 14).astype(np.float32), (2.0 * rng.randn(n, 14)).astype(np.float32)
    x = rawv if raw else ap
    act, _ = project(kern, s, None if mode == E.NOISE_UNIFORM else x, noise if mode == E.NOISE_EXPLICIT else None, mode, raw, 0, LR, EPS,
                     0.0, ctrl=new_ctrl(ops, 5), want_iters=False)
    eps_t = E.eps_at(0.5, 0.05, 0.01, 5)
    note(E.check_proposal(TAB, s, x, noise, mode, raw, eps_t, 7, np.arange(n) + 3, 5, act[:, E.PARTA]))


@pytest.mark.parametrize("n", [1, 3, 4, 5, 63, 64, 65, 257])
def test_newton_one_update_at_a_time(kern, kern_dyn, n):
    """newton_max_iters = 1 .. 6 from the flat start (caps 1 and 2 cut the loop short): iterate m + 1 is one float64 Newton step from
    the kernel's iterate m, the stop test ||delta||_2 < tol held exactly, qg / slack pg = -resid at the final point; a newton_tol
    large enough stops after the first update."""
    s, ap = E.basic_rows(n, n)
    for k, tab in both_orders(kern, kern_dyn):
        outs = [project(k, s, ap, None, E.NOISE_CLIP_ONLY, False, 0, LR, EPS, 0.0, tol=NEWTON_TOL, m=m)[0] for m in range(1, NEWTON_M + 1)]
        r, amb = E.check_newton(tab, s, outs, NEWTON_TOL)
        note(r, {"newton": amb})
        first, it = project(k, s, ap, None, E.NOISE_CLIP_ONLY, False, 0, LR, EPS, 0.0, tol=1e3, m=NEWTON_M)
        assert (bits(first) == bits(outs[0])).all() and not it.any()


def grg_outputs(k, s, ap, steps, lr, eps, momentum=0.0):
    runs = [project(k, s, ap, None, E.NOISE_CLIP_ONLY, False, j, lr, eps, momentum) for j in range(steps + 1)]
    return [r[0] for r in runs], [r[1] for r in runs]


@pytest.mark.parametrize("n,lr,eps,steps", [(64, LR, EPS, K), (65, 1e-2, EPS, 2), (65, LR, 2e-2, 3), (257, LR, EPS, 2), (5, LR, EPS, 2),
                                            (1, LR, EPS, 2), (3, LR, EPS, 2), (4, LR, EPS, 2), (63, LR, EPS, 2)])
def test_grg_one_iteration_at_a_time(kern, kern_dyn, n, lr, eps, steps):
    """max_steps = 0 .. K: output k + 1 = output k - lr * the float64 reduced gradient at output k; iters = the number of steps the
    float64 stop test allows (all ten at lr 1e-4; lanes feasible from the start take the reference's one unconditional step)."""
    s, ap = E.basic_rows(n, n)
    for k, tab in both_orders(kern, kern_dyn)[:1 if steps == K else 2]:
        outs, iters = grg_outputs(k, s, ap, steps, lr, eps)
        r, amb = E.check_grg(tab, s, outs, iters, lr, eps)
        note(r, {"grg": amb})
    if steps == K:
        assert (iters[-1] == K).sum() >= 32
        got, it = project(kern, s, ap, None, E.NOISE_CLIP_ONLY, False, K, lr, eps, 0.5)
        r, left = E.check_momentum(TAB, s, outs[0], got, it, K, lr, eps, 0.5)
        note(r, {"grg_mom": left})


def test_grg_feasible_row_and_nan_rows(kern):
    """A lane with no violated bound: the reference's one unconditional iteration (step == 0) with a zero gradient, bits untouched.
    NaN rows end after the iterations torch.max(...) > corr_eps gives (rpo_ddpg.py:271-272: torch.max propagates a NaN and
    NaN > corr_eps is false, so a term that holds a NaN cannot keep the loop going): ONE, for all three kinds --
      a NaN demand or a NaN pg at a pv generator reaches Newton's right-hand side: the whole completed action is NaN;
      a NaN pe at the slack generator enters no Newton equation: only the slack pg = -resid and that pe are NaN, every other
      component stays finite and violated -- a stop test that drops the NaN (fmaxf) iterates on those to the budget.
    No other lane moves by a bit."""
    n, budget = 8, 6
    s, ap = E.basic_rows(n, n)
    clean, it0 = project(kern, s, ap, None, E.NOISE_NONE, False, budget, LR, EPS, 0.0)
    start, _ = project(kern, s, ap, None, E.NOISE_NONE, False, 0, LR, EPS, 0.0)
    hi, lo = E.bounds(E.F32E, E.Tab(E.F32E, TAB), E.cols(E.F32E, s))
    row_of = lambda x, r: np.broadcast_to(x, (n,))[r]                                   # noqa: E731
    feasible = np.array([all(h is None or lo[v] is None or (row_of(lo[v], r) <= start[r, v] <= row_of(h, r)) for v, h in enumerate(hi))
                         for r in range(n)])
    one_step, _ = project(kern, s, ap, None, E.NOISE_NONE, False, 1, LR, EPS, 0.0)
    for r in np.nonzero(feasible)[0]:
        assert (bits(one_step[r]) == bits(start[r])).all()
    assert it0[3] == budget and it0[2] == budget                  # (the lanes that get a NaN below would otherwise use the budget)
    s2, ap2 = s.copy(), ap.copy()
    s2[1, 3] = np.nan                                             # a NaN demand
    ap2[2, 1] = np.nan                                            # a NaN pg at a pv generator
    ap2[3, 9] = np.nan                                            # a NaN pe at the slack generator
    got, it = project(kern, s2, ap2, None, E.NOISE_NONE, False, budget, LR, EPS, 0.0)
    keep = np.ones(n, bool)
    keep[[1, 2, 3]] = False
    assert (bits(got[keep]) == bits(clean[keep])).all() and (it[keep] == it0[keep]).all()
    assert np.isnan(got[1]).sum() > 30 and np.isnan(got[2]).sum() > 30
    assert np.isnan(got[3, [E.PG0, E.PE0]]).all() and np.isnan(got[3]).sum() == 2
    assert (it[[1, 2, 3]] == 1).all(), it
