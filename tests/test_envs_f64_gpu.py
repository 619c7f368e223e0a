"""The env-step, constraint and projection launches (rpo_cartsafe_step / rpo_pendulum_step, rpo_<env>_resid, _ineq_partial_grad,
_complete_bwd, _lagrangian, _act_project, _project_profile, rpo_pendulum_project_batchref) called directly through rpo_amd.ops,
against the float64 restatement of tests/envs_f64.py.  Needs an MI355X.

Float outputs: EVERY element of every launch within MARGIN (4) * C_REF_* * eps32 * magnitude sum of float64 (envs_f64.py; C_REF_*
is the float32 emulation's own error against float64 over the same kinds of input, measured on the CPU by
test_envs_f64.py::test_yardstick), at 1, 63, 64, 65, 255, 256, 257 and 513 rows, on the wide state boxes and the edge rows
(x_dot = +-0 and denormal, n_c through 0, actions on and beyond the clip, next states ON the thresholds, the fmodf wrap, cos -> 0,
|a|^2 - 32 within ulps of 0), 8-but-not-16-byte aligned views, NULL outputs, a ring slot in the middle, strided observations.
Discontinuous iterations are compared ONE iteration at a time from the kernel's own previous iterate; ambiguous predicates accept
either value and may touch at most 2 % of the rows of a comparison.  Exact: copies, the CartSafe reward, done (the float32
predicate on the STORED next state AND the reference's float64 test of it), the episode words, auto-reset against the Philox oracle,
stop decisions and iteration counts, statistics as functions of the stored rows, the ctrl words, every element past a buffer's end.

Worst ratios measured on an MI355X, in units of eps32 * magnitude sum (the limit is 4 * C_REF_*: 0.9 for cart_acc, 1.5 to 2.0 for
the others; every test prints its own under -s):
    CartSafe step    violations 0.465, next x / x_dot / theta / theta_dot 0.488, accelerations 0.251
    pendulum step    pre-step cos / sin 0.448, violations 0.384, next observation and theta 0.495, reward 0.479
    constraint API   cart: resid 0.499, ineq_partial_grad 0.366, complete_bwd 0.454, lagrangian 0.332
                     pendulum: resid 0.354, ineq_partial_grad 0.280, complete_bwd 0.478, lagrangian 0.480
    exploration + completion   cart 0.470, pendulum 0.437
    one GRG iteration / residuals of an iterate   cart 0.497, pendulum 0.493, batch-coupled 0.458 (momentum 0)
    momentum 0.5 trajectories: per-lane inside the figures above; batch-coupled, in units of K single-step bounds: 0.319
Ambiguous rows per comparison: none in the steps and the per-lane loops below 513 rows, at most 0.4 % widened in the batched loop;
no row was left out there; the batched momentum trajectory leaves out 0 / 2 / 4 rows of 17 / 256 / 300.  107 cases, 4.1 s.
"""
import numpy as np
import pytest
import torch

import envs_f64 as ef
from oracle import cartsafe as ocs
from oracle import philox

pytestmark = pytest.mark.gpu

DEV = "cuda"
PAD = 64
SENT = -12345.0
NS = [1, 63, 64, 65, 255, 256, 257, 513]
BIG = 2048 * 256 + 256 + 7                      # a second grid-stride pass of a few workgroups, and a ragged tail
CART_LR, PEND_LR, EPS, K = 2e-2, 2e-3, 1e-5, 10
NU6 = np.array([0.3, 0.0, 1.5, 0.2, 0.7, 0.05], np.float32)
WORST = {}


@pytest.fixture(scope="module")
def ops():
    from rpo_amd import ops as _ops
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    yield _ops
    print("\nworst ratios (eps32 * magnitude sum):", {k: round(v, 3) for k, v in sorted(WORST.items())})


def note(group, value, limit=None):
    value = float(value)
    WORST[group] = max(WORST.get(group, 0.0), value)
    limit = ef.tol_c(group) if limit is None else limit
    print("%-12s worst %.3f (limit %.2f)" % (group, value, limit))
    assert value <= limit, (group, value, limit)


class Buf(object):
    """A device buffer of ``values`` with PAD sentinel elements behind it (and, with ``skew``, 2 elements = 8 bytes in front: the
    view is then 8- but not 16-byte aligned); ``view`` is what the launch gets."""

    def __init__(self, values, dtype=torch.float32, skew=False):
        np_dtype = {torch.float32: np.float32, torch.int32: np.int32, torch.int64: np.int64}[dtype]
        values = np.ascontiguousarray(values, dtype=np_dtype)
        self.off, self.n, self.shape = (2 if skew else 0), values.size, values.shape
        self.sent = np_dtype(SENT) if dtype == torch.float32 else np_dtype(0x5A5A5A5A)
        host = np.full(self.off + self.n + PAD, self.sent, dtype=np_dtype)
        host[self.off:self.off + self.n] = values.reshape(-1)
        self.buf = torch.from_numpy(host).to(DEV)
        self.view = self.buf[self.off:self.off + self.n].view(*self.shape)
        assert self.view.data_ptr() % 16 == (8 if skew else 0)

    def get(self):
        host = self.buf.cpu().numpy()
        assert (host[:self.off] == self.sent).all() and (host[self.off + self.n:] == self.sent).all(), "the launch wrote outside its buffer"
        return host[self.off:self.off + self.n].reshape(self.shape).copy()


def new_ctrl(ops, t=5):
    c = torch.zeros(ops.CTRL_LEN, dtype=torch.int64, device=DEV)
    c[ops.CONST["RPO_CTRL_T"]] = t
    return c


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def episode_words(n, seed, max_steps):
    rng = np.random.RandomState(seed + 31)
    ep_len = rng.choice([0, 17, max_steps - 1, max_steps - 2], n).astype(np.int32)
    return ep_len, rng.uniform(0, 50, n).astype(np.float32), rng.randint(0, 9, n).astype(np.int32)


def check_stats(ops, srow, reward, done, term, ret_done, len_done, max_ineq, max_eq, thresh):
    """The statistics row as a function of the STORED rows: counts and maxima exact, sums within n eps32 sum |v|."""
    s = ops.reduce_stats(srow).cpu().numpy().astype(np.float64)
    S = ops.STAT
    n = len(reward)

    def close(name, vals):
        vals = np.asarray(vals, np.float64)
        if not np.isfinite(vals).all():
            assert not np.isfinite(s[S[name]]), name
            return
        assert abs(s[S[name]] - vals.sum()) <= n * ef.EPS32 * np.abs(vals).sum() + 1e-30, (name, s[S[name]], vals.sum())
    close("reward_sum", reward)
    assert s[S["episodes"]] == done.sum() and s[S["terminated"]] == (term & done).sum()
    assert s[S["length_sum"]] == len_done.sum()
    close("return_sum", ret_done)
    close("max_ineq_sum", max_ineq)
    close("max_eq_sum", max_eq)
    assert s[S["viol_count"]] == (np.fmax(max_ineq, max_eq) > np.float32(thresh)).sum()
    fin = lambda v: np.float32(np.fmax.reduce(np.concatenate([[0.0], v])))           # noqa: E731  fmaxf from 0
    assert np.float32(s[S["max_ineq_max"]]) == fin(max_ineq) and np.float32(s[S["max_eq_max"]]) == fin(max_eq)


# ================================================================================================================ CartSafe step
def run_cart_step(ops, k, st, act, words, max_steps, auto_reset, skew=False, rows=True, stats=True, ctrl=True, cap=3, t=5, seed=99, base=1000):
    n = st.shape[0]
    S, A = Buf(st, skew=skew), Buf(act)
    L, R, C = Buf(words[0], torch.int32), Buf(words[1]), Buf(words[2], torch.int32)
    ring = Buf(np.full((cap * n, k.ring_floats), SENT, np.float32), skew=skew) if rows else None
    sts = ops.new_stats(8, DEV) if stats else None
    c = new_ctrl(ops, t) if ctrl else None
    k.step(S.view, S.view, A.view, L.view, R.view, C.view, ring.view if rows else None, cap, sts, c, max_steps, auto_reset, 1e-3, seed, base)
    torch.cuda.synchronize()
    return dict(state=S.get(), action=A.get(), ep_len=L.get(), ep_ret=R.get(), ep_count=C.get(), ring=ring.get() if rows else None,
                stats=sts, ctrl=c.cpu().numpy() if ctrl else None)


@pytest.mark.parametrize("partial", [1, 0])
@pytest.mark.parametrize("n", NS)
def test_cart_step(ops, n, partial):
    table = ocs.Constants(partial).as_array()
    k = ops.CartSafeKernels(table, partial)
    st, act, tag = ef.cart_rows(n, seed=n + partial)
    max_steps, cap, t = 200, 3, 5
    words = episode_words(n, n, max_steps)
    o = run_cart_step(ops, k, st, act, words, max_steps, False)
    slot = (t % cap) * n
    rows = o["ring"][slot:slot + n]
    # float outputs, every row; the sign predicate's ambiguous rows accept the neighbouring signs (none by construction here)
    r, amb = ef.check_cart_step(st, act, table, partial, rows)
    assert amb.mean() <= ef.AMBIG_CAP
    for g, v in r.items():
        note(g, v.max())
    # exact
    assert np.array_equal(bits(rows[:, 0:6]), bits(st)) and np.array_equal(bits(rows[:, 6:8]), bits(act))
    assert np.all(rows[:, 14] == 1.0)
    nlen = words[0] + 1
    term = ef.cart_terminated_f32(rows[:, 8:14])
    done = term | (nlen >= max_steps)
    np.testing.assert_array_equal(rows[:, 15], done.astype(np.float32))                       # the float32 predicate, no row exempt
    np.testing.assert_array_equal(term, ef.cart_terminated_ref(rows[:, 8:14]))                # == the reference's float64 test
    assert np.all(rows[:, 23] == 0.0)
    pad = rows[:, 24:]
    assert np.all((pad == 0.0) | (pad == np.float32(SENT)))                                   # ring padding: zero or untouched
    other = np.delete(o["ring"], np.s_[slot:slot + n], axis=0)
    assert np.all(other == np.float32(SENT))                                                  # the other ring slots are untouched
    assert np.array_equal(bits(o["state"]), bits(rows[:, 8:14]))                              # no auto-reset: the state moves on
    np.testing.assert_array_equal(o["ep_len"], nlen)
    assert np.array_equal(bits(o["ep_ret"]), bits(words[1] + np.float32(1.0)))
    np.testing.assert_array_equal(o["ep_count"], words[2])
    assert np.array_equal(bits(o["action"]), bits(act))
    T, NF = ops.CONST["RPO_CTRL_T"], ops.CONST["RPO_CTRL_NONFINITE"]
    assert o["ctrl"][T] == t + 1 and o["ctrl"][NF] == 0 and o["ctrl"][ops.CONST["RPO_CTRL_ARRIVE"]] == 0
    ret = words[1] + np.float32(1.0)
    check_stats(ops, o["stats"][t % 8], rows[:, 14], done, term, ret[done], nlen[done], np.fmax.reduce(rows[:, 17:23], axis=1),
                np.abs(rows[:, 16]), 1e-3)
    assert float(o["stats"][(t + 1) % 8].abs().max()) == 0.0
    # an 8-but-not-16-byte aligned state / ring takes the per-lane path: the same bits
    m = run_cart_step(ops, k, st, act, words, max_steps, False, skew=True)
    assert np.array_equal(bits(m["ring"][slot:slot + n, :24]), bits(rows[:, :24])) and np.array_equal(bits(m["state"]), bits(o["state"]))
    mp = m["ring"][:, 24:]
    assert np.all((mp == 0.0) | (mp == np.float32(SENT)))
    assert np.all(np.delete(m["ring"], np.s_[slot:slot + n], axis=0) == np.float32(SENT))
    # rows, stats and ctrl NULL: the same state and episode words, nothing else written (t = 0)
    z = run_cart_step(ops, k, st, act, words, max_steps, False, rows=False, stats=False, ctrl=False)
    assert np.array_equal(bits(z["state"]), bits(o["state"])) and np.array_equal(z["ep_len"], o["ep_len"])
    # auto-reset: done lanes restart from the Philox oracle's state of (seed, env id, episode + 1)
    a = run_cart_step(ops, k, st, act, words, max_steps, True)
    assert np.array_equal(bits(a["ring"][slot:slot + n, :24]), bits(rows[:, :24]))
    fresh = philox.cart_reset(99, np.arange(n) + 1000, words[2] + 1)                        # float32 lo + u * span: the kernel's form
    assert fresh.dtype == np.float32 and np.array_equal(bits(a["state"][done]), bits(fresh[done]))
    assert np.array_equal(bits(a["state"][~done]), bits(rows[~done, 8:14]))
    np.testing.assert_array_equal(a["ep_count"], words[2] + done)
    np.testing.assert_array_equal(a["ep_len"], np.where(done, 0, nlen))
    assert np.array_equal(bits(a["ep_ret"]), bits(np.where(done, np.float32(0), ret)))


def test_cart_step_second_grid_pass(ops):
    """2048 * 256 + 256 + 7 rows: workgroups 0 and 1 take a second tile, the last 7 rows the per-lane path.  Cheap assertions: the
    rows of a random sample and of the whole second pass against float64, done exact on every row, and the launch split in two gives
    the same bits."""
    partial, n = 1, BIG
    table = ocs.Constants(partial).as_array()
    k = ops.CartSafeKernels(table, partial)
    st, act, tag = ef.cart_rows(n, seed=3)
    words = (np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros(n, np.int32))
    o = run_cart_step(ops, k, st, act, words, 200, False, cap=1, t=0)
    rows = o["ring"]
    pick = np.concatenate([np.random.RandomState(0).choice(n, 4096, replace=False), np.arange(2048 * 256, n)])
    r, amb = ef.check_cart_step(st[pick], act[pick], table, partial, rows[pick])
    assert amb.mean() <= ef.AMBIG_CAP
    for g, v in r.items():
        note(g, v.max())
    term = ef.cart_terminated_f32(rows[:, 8:14])
    np.testing.assert_array_equal(rows[:, 15], term.astype(np.float32))
    np.testing.assert_array_equal(term, ef.cart_terminated_ref(rows[:, 8:14]))
    assert np.array_equal(bits(rows[:, 0:6]), bits(st)) and np.array_equal(bits(o["state"]), bits(rows[:, 8:14]))
    h = 2048 * 128
    lo = run_cart_step(ops, k, st[:h], act[:h], tuple(w[:h] for w in words), 200, False, cap=1, t=0)
    hi = run_cart_step(ops, k, st[h:], act[h:], tuple(w[h:] for w in words), 200, False, cap=1, t=0, base=1000 + h)
    assert np.array_equal(bits(np.concatenate([lo["ring"], hi["ring"]])[:, :24]), bits(rows[:, :24]))


# ================================================================================================================ pendulum step
def run_pend_step(ops, k, st, act, words, max_steps, auto_reset, rows=True, stats=True, ctrl=True, obs=True, cap=3, t=5, seed=17, base=64):
    n = st.shape[0]
    S, A = Buf(st), Buf(act)
    O = Buf(np.full((n, 5), SENT, np.float32)) if obs else None
    L, R, C = Buf(words[0], torch.int32), Buf(words[1]), Buf(words[2], torch.int32)
    ring = Buf(np.full((cap * n, k.ring_floats), SENT, np.float32)) if rows else None
    sts = ops.new_stats(8, DEV) if stats else None
    c = new_ctrl(ops, t) if ctrl else None
    k.step(S.view, O.view if obs else None, A.view, L.view, R.view, C.view, ring.view if rows else None, cap, sts, c, max_steps, auto_reset,
           1e-3, seed, base)
    torch.cuda.synchronize()
    return dict(state=S.get(), obs=O.get() if obs else None, ep_len=L.get(), ep_ret=R.get(), ep_count=C.get(),
                ring=ring.get() if rows else None, stats=sts, ctrl=c.cpu().numpy() if ctrl else None)


@pytest.mark.parametrize("n", NS)
def test_pendulum_step(ops, n):
    k = ops.PendulumKernels()
    st, act, tag = ef.pend_rows(n, seed=n)
    max_steps, cap, t = 200, 3, 5
    words = episode_words(n, n, max_steps)
    o = run_pend_step(ops, k, st, act, words, max_steps, False)
    slot = (t % cap) * n
    rows = o["ring"][slot:slot + n]
    r = ef.check_pend_step(st, act, rows, o["state"][:, 0])
    for g, v in r.items():
        note(g, v.max())
    assert np.array_equal(bits(rows[:, 2:5]), bits(st[:, 1:4])) and np.array_equal(bits(rows[:, 5:7]), bits(act))
    nint = o["state"]
    assert np.array_equal(bits(nint[:, 1:]), bits(rows[:, 9:12]))                              # theta_dot (clipped), l, l_dot as stored
    assert np.all(np.abs(nint[:, 1]) <= 8.0)
    assert np.array_equal(bits(o["obs"][:, :2]), bits(rows[:, 7:9])) and np.array_equal(bits(o["obs"][:, 2:]), bits(nint[:, 1:]))
    nlen = words[0] + 1
    term = ef.pend_terminated_f32(nint)
    done = term | (nlen >= max_steps)
    np.testing.assert_array_equal(rows[:, 13], done.astype(np.float32))
    np.testing.assert_array_equal(term, ef.pend_terminated_ref(nint))
    assert np.all(np.delete(o["ring"], np.s_[slot:slot + n], axis=0) == np.float32(SENT))
    np.testing.assert_array_equal(o["ep_len"], nlen)
    ret = words[1] + rows[:, 12]
    assert np.array_equal(bits(o["ep_ret"]), bits(ret))
    T, NF = ops.CONST["RPO_CTRL_T"], ops.CONST["RPO_CTRL_NONFINITE"]
    assert o["ctrl"][T] == t + 1 and o["ctrl"][NF] == 0
    check_stats(ops, o["stats"][t % 8], rows[:, 12], done, term, ret[done], nlen[done], rows[:, 15], np.abs(rows[:, 14]), 1e-3)
    z = run_pend_step(ops, k, st, act, words, max_steps, False, rows=False, stats=False, ctrl=False, obs=False)
    assert np.array_equal(bits(z["state"]), bits(nint)) and np.array_equal(z["ep_len"], o["ep_len"])
    a = run_pend_step(ops, k, st, act, words, max_steps, True)
    assert np.array_equal(bits(a["ring"][slot:slot + n]), bits(rows))
    fresh = philox.pendulum_reset(17, np.arange(n) + 64, words[2] + 1)
    assert fresh.dtype == np.float32 and np.array_equal(bits(a["state"][done]), bits(fresh[done]))
    assert np.array_equal(bits(a["obs"][done, 2:]), bits(fresh[done, 1:]))
    assert np.array_equal(bits(a["state"][~done]), bits(nint[~done]))
    np.testing.assert_array_equal(a["ep_count"], words[2] + done)
    np.testing.assert_array_equal(a["ep_len"], np.where(done, 0, nlen))


def test_pendulum_step_second_grid_pass(ops):
    n = BIG
    k = ops.PendulumKernels()
    st, act, tag = ef.pend_rows(n, seed=3)
    words = (np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros(n, np.int32))
    o = run_pend_step(ops, k, st, act, words, 200, False, cap=1, t=0)
    rows = o["ring"]
    pick = np.concatenate([np.random.RandomState(0).choice(n, 4096, replace=False), np.arange(2048 * 256, n)])
    for g, v in ef.check_pend_step(st[pick], act[pick], rows[pick], o["state"][pick, 0]).items():
        note(g, v.max())
    term = ef.pend_terminated_f32(o["state"])
    np.testing.assert_array_equal(rows[:, 13], term.astype(np.float32))
    np.testing.assert_array_equal(term, ef.pend_terminated_ref(o["state"]))
    assert np.array_equal(bits(rows[:, 5:7]), bits(act))


# ================================================================================================================ non-finite rows
@pytest.mark.parametrize("env", ["cart", "pend"])
def test_nonfinite_rows(ops, env):
    """A NaN action, a NaN state and an infinite state, one row each, among finite rows at ctrl[RPO_CTRL_T] = 7: the other rows keep
    their bits, the failure word becomes 8 and stays 8, ctrl = NULL writes nothing, and float64 decides where NaN may come out."""
    n = 300
    T, NF = ops.CONST["RPO_CTRL_T"], ops.CONST["RPO_CTRL_NONFINITE"]
    words = (np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros(n, np.int32))
    if env == "cart":
        table = ocs.Constants(1).as_array()
        k = ops.CartSafeKernels(table, 1)
        st, act, tag = ef.cart_rows(n, 4, wide=False)
        run = lambda s, a, **kw: run_cart_step(ops, k, s, a, words, 200, False, cap=1, **kw)                  # noqa: E731
        def judge(s, a, o):
            r, amb = ef.check_cart_step(s, a, table, 1, o["ring"])
            assert amb.mean() <= ef.AMBIG_CAP
            return r
    else:
        k = ops.PendulumKernels()
        st, act, tag = ef.pend_rows(n, 4, wide=False)
        run = lambda s, a, **kw: run_pend_step(ops, k, s, a, words, 200, False, cap=1, **kw)                  # noqa: E731
        judge = lambda s, a, o: ef.check_pend_step(s, a, o["ring"], o["state"][:, 0])                          # noqa: E731
    clean = run(st, act, t=7)
    assert clean["ctrl"][NF] == 0
    bad_s, bad_a = st.copy(), act.copy()
    bad_a[5, 0], bad_s[9, 3 if env == "cart" else 0], bad_s[13, 1] = np.nan, np.nan, np.inf
    o = run(bad_s, bad_a, t=7)
    assert o["ctrl"][NF] == 8 and o["ctrl"][T] == 8
    keep = np.ones(n, bool)
    keep[[5, 9, 13]] = False
    assert np.array_equal(bits(o["ring"][keep]), bits(clean["ring"][keep])) and np.array_equal(bits(o["state"][keep]), bits(clean["state"][keep]))
    for g, v in judge(bad_s, bad_a, o).items():
        note(g, v.max())
    # sticky: a later launch (t = 8) with another bad row leaves 8
    c = new_ctrl(ops, 8)
    c[NF] = 8
    bad2 = act.copy()
    bad2[77, 1] = np.nan
    S, A = Buf(st, skew=False), Buf(bad2)
    L, R, C = Buf(words[0], torch.int32), Buf(words[1]), Buf(words[2], torch.int32)
    if env == "cart":
        k.step(S.view, S.view, A.view, L.view, R.view, C.view, None, 1, None, c, 200, False, 1e-3, 1, 0)
    else:
        k.step(S.view, None, A.view, L.view, R.view, C.view, None, 1, None, c, 200, False, 1e-3, 1, 0)
    torch.cuda.synchronize()
    assert int(c[NF]) == 8 and int(c[T]) == 9
    run(bad_s, bad_a, ctrl=False, rows=False, stats=False)                                    # ctrl = NULL: nothing to write, no fault


# ================================================================================================================ constraint API
@pytest.mark.parametrize("partial", [1, 0])
@pytest.mark.parametrize("n", NS)
def test_cart_constraint_api(ops, n, partial):
    table = ocs.Constants(partial).as_array()
    k = ops.CartSafeKernels(table, partial)
    B = ef.B64
    st, act, tag = ef.cart_rows(n, seed=n + 7)
    act[: n // 3] = ef.cart_join(partial, ef.cart_proposals(n, n)[: n // 3], act[: n // 3, 0])       # box corners, reduced thresholds
    if n >= 2:
        act[0], act[1] = (10.0, 3.0), (-2.0, -10.0)                 # g_2 = 10 * 1 + 3 * 0 - 10 = 0 and g_5 = 0 EXACTLY: masks off
    c64 = ef.CartTab(B, table, partial)
    A_, EQ, IN = Buf(act), Buf(np.full(n, SENT, np.float32)), Buf(np.full((n, 6), SENT, np.float32))
    k.resid(None, A_.view, EQ.view, IN.view)
    with np.errstate(all="ignore"):
        h, g = ef.cart_eq_ineq(B, c64, B.inp(act[:, 0]), B.inp(act[:, 1]))
        note("cart_resid", max(ef.ratio(EQ.get(), h).max(), max(ef.ratio(IN.get()[:, j], g[j]).max() for j in range(6))))
        k.resid(None, A_.view, None, IN.view)
        k.resid(None, A_.view, EQ.view, None)
        EQ.get(), IN.get()
        # ineq_partial_grad: rows with an ambiguous predicate accept either value of up to three
        ST = Buf(np.full((n, 2), SENT, np.float32))
        k.ineq_partial_grad(None, A_.view, ST.view)
        r, left = ef.check_ipg("cart", ST.get(), act, table=table, partial=partial)
        assert left.mean() <= ef.AMBIG_CAP
        note("cart_ipg", r.max())
        ga = np.random.RandomState(n).randn(n, 2).astype(np.float32)
        GA, GP = Buf(ga), Buf(np.full(n, SENT, np.float32))
        k.complete_bwd(None, GA.view, GP.view)
        note("cart_cbwd", ef.ratio(GP.get(), ef.cart_complete_bwd(B, table, partial, ga)).max())
        # Lagrangian: per-row gradient against float64 (autograd-checked on the CPU), sums against float64 sums of the rows
        scale = 1.0 / n
        NU, LOSS, GNU, GACT = Buf(NU6), Buf(np.zeros(1, np.float32)), Buf(np.zeros(6, np.float32)), Buf(np.full((n, 2), SENT, np.float32))
        k.lagrangian(A_.view, NU.view, scale, LOSS.view, GACT.view, GNU.view)
        l = ef.cart_lagrangian(B, table, partial, act, NU6, scale)
        r, left, zero = ef.check_lagrangian("cart", GACT.get(), act, NU6, scale, table=table, partial=partial)
        assert not left.any()
        assert zero.sum() >= (2 if n >= 2 else 0)
        note("cart_lag", r.max())
        dist = np.stack([d.v for d in l["dist"]], axis=1)
        dmag = np.stack([B.mag(d) for d in l["dist"]], axis=1)
        s32 = float(np.float32(scale))
        want_nu = s32 * dist.sum(axis=0)
        tol_nu = s32 * ((n + 8) * ef.EPS32 * np.abs(dist).sum(axis=0) + ef.tol_c("cart_lag") * ef.EPS32 * dmag.sum(axis=0)) + 1e-30
        assert np.all(np.abs(GNU.get() - want_nu) <= tol_nu), (GNU.get(), want_nu, tol_nu)
        nu64 = NU6.astype(np.float64)
        assert abs(float(LOSS.get()[0]) - float(want_nu @ nu64)) <= float(tol_nu @ nu64) * 2 + 1e-30


@pytest.mark.parametrize("n", NS)
def test_pendulum_constraint_api(ops, n):
    k = ops.PendulumKernels()
    B = ef.B64
    st, act, tag = ef.pend_rows(n, seed=n + 7, half_pi=True)
    obs = ef.pend_obs32(st)
    wide = np.full((n, 16), SENT, np.float32)                     # strided observations: columns 7..11 of a gathered batch
    wide[:, 7:12] = obs
    W = Buf(wide)
    ov = W.view[:, 7:12]
    A_, EQ, IN = Buf(act), Buf(np.full(n, SENT, np.float32)), Buf(np.full(n, SENT, np.float32))
    k.resid(ov, A_.view, EQ.view, IN.view)
    with np.errstate(all="ignore"):
        e = ef.pend_eq_of_obs(B, obs)
        h, g = ef.pend_resid(B, e, B.inp(act[:, 0]), B.inp(act[:, 1]))
        note("pend_resid", max(ef.ratio(EQ.get(), h).max(), ef.ratio(IN.get(), g).max()))
        O2, EQ2 = Buf(obs), Buf(np.full(n, SENT, np.float32))
        k.resid(O2.view, A_.view, EQ2.view, None)
        assert np.array_equal(bits(EQ2.get()), bits(EQ.get()))                                  # contiguous == strided
        ST = Buf(np.full((n, 2), SENT, np.float32))
        k.ineq_partial_grad(ov, A_.view, ST.view)
        r, left = ef.check_ipg("pend", ST.get(), act, obs=obs)
        assert not left.any()
        note("pend_ipg", r.max())
        ga = np.random.RandomState(n).randn(n, 2).astype(np.float32)
        GA, GP = Buf(ga), Buf(np.full(n, SENT, np.float32))
        k.complete_bwd(ov, GA.view, GP.view)
        note("pend_cbwd", ef.ratio(GP.get(), ef.pend_complete_bwd(B, obs, ga)).max())
        acts = act.copy()
        g32 = np.array(ef.pend_g32_actions(), np.float32)
        acts[: min(n, len(g32))] = g32[: min(n, len(g32))]
        scale = 1.0 / n
        A2, NU, LOSS, GNU, GACT = Buf(acts), Buf(np.array([0.37], np.float32)), Buf(np.zeros(1, np.float32)), Buf(np.zeros(1, np.float32)), \
            Buf(np.full((n, 2), SENT, np.float32))
        k.lagrangian(A2.view, NU.view, scale, LOSS.view, GACT.view, GNU.view)
        l = ef.pend_lagrangian(B, acts, 0.37, scale)
        gact = GACT.get()
        r, left, zero_rows = ef.check_lagrangian("pend", gact, acts, 0.37, scale)     # |a|^2 - 32 within ulps of 0: either mask value
        note("pend_lag", r.max())
        zero = l["margin"].v == 0                                    # g = 0 exactly (16 + 16 - 32): the strict mask gives 0 exactly
        assert zero.sum() >= min(n, 2) and np.all(gact[zero] == 0.0)
        s32 = float(np.float32(scale))
        want = s32 * l["dist"].v.sum()
        tol = s32 * ((n + 8) * ef.EPS32 * np.abs(l["dist"].v).sum() + ef.tol_c("pend_lag") * ef.EPS32 * B.mag(l["dist"]).sum()) + 1e-30
        assert abs(float(GNU.get()[0]) - want) <= tol and abs(float(LOSS.get()[0]) - float(np.float32(0.37)) * want) <= tol


# ================================================================================================================ per-lane projection
def run_profile(ops, k, env, n, obs, ap, steps, lr, momentum, strided=False):
    AP, ACT, IT = Buf(ap), Buf(np.full((n, 2), SENT, np.float32)), Buf(np.zeros(n, np.int32), torch.int32)
    PR = Buf(np.full((steps + 1, n, 4), SENT, np.float32))
    if env == "cart":
        k.project_profile(None, AP.view, ACT.view, IT.view, steps, lr, EPS, momentum, PR.view)
    else:
        if strided:
            wide = np.full((n, 16), SENT, np.float32)
            wide[:, 7:12] = obs
            O = Buf(wide)
            ov = O.view[:, 7:12]
        else:
            O = Buf(obs)
            ov = O.view
        k.project_profile(ov, AP.view, ACT.view, IT.view, steps, lr, EPS, momentum, PR.view)
    torch.cuda.synchronize()
    return PR.get(), IT.get(), ACT.get()


def judge_profile(env, planes, iters, lr, **kw):
    c = ef.check_profile(env, planes, iters, lr, EPS, **kw)
    share = c["amb"].mean(axis=1).max() if planes.shape[0] > 1 else 0.0
    print("share of rows with an ambiguous predicate per iteration (max): %.4f, left out: %.4f" % (share, c["left"].mean(axis=1).max()))
    assert c["left"].mean(axis=1).max() <= ef.AMBIG_CAP
    note(env + "_grg", max(c["grg"].max(initial=0.0), c["resid"].max()))
    assert c["stop_ok"].all(), "stop decision / iteration count against the kernel's own reported residuals"
    return c


@pytest.mark.parametrize("partial", [1, 0])
@pytest.mark.parametrize("n", NS)
def test_cart_projection_one_iteration_at_a_time(ops, n, partial):
    table = ocs.Constants(partial).as_array()
    k = ops.CartSafeKernels(table, partial)
    ap = ef.cart_proposals(n, seed=n)
    planes, iters, action = run_profile(ops, k, "cart", n, None, ap, K, CART_LR, 0.0)
    c = judge_profile("cart", planes, iters, CART_LR, table=table, partial=partial)
    assert np.array_equal(bits(action), bits(planes[K, :, :2]))
    # act_project at the budget K gives plane K and the same counts; iters may be NULL
    AP, ACT, IT = Buf(ap), Buf(np.full((n, 2), SENT, np.float32)), Buf(np.zeros(n, np.int32), torch.int32)
    k.act_project(None, AP.view, None, ACT.view, IT.view, ops.NOISE_NONE, 0, 0, 0, -10, 10, K, CART_LR, EPS, 0.0)
    assert np.array_equal(bits(ACT.get()), bits(action)) and np.array_equal(IT.get(), iters)
    k.act_project(None, AP.view, None, ACT.view, None, ops.NOISE_NONE, 0, 0, 0, -10, 10, K, CART_LR, EPS, 0.0)
    assert np.array_equal(bits(ACT.get()), bits(action))
    # momentum 0.5 as a whole trajectory, on the rows whose momentum-0 history carried no ambiguous predicate
    clean = ~(c["left"] | c["amb"]).any(axis=0)
    assert (~clean).mean() <= ef.AMBIG_CAP
    mplanes, miters, maction = run_profile(ops, k, "cart", n, None, ap, K, CART_LR, 0.5)
    p, o, it64, tclean = ef.project_b64("cart", ap, K, CART_LR, EPS, 0.5, table=table, partial=partial)
    gp, go = ef.cart_split(partial, maction)
    note("cart_grg", np.maximum(ef.ratio(gp, p), ef.ratio(go, o))[clean].max(initial=0.0))
    assert np.array_equal(bits(maction), bits(mplanes[K, :, :2]))
    both = clean & tclean                                          # no ambiguous mask or stop predicate along the momentum trajectory either
    np.testing.assert_array_equal(miters[both], it64[both])


@pytest.mark.parametrize("n", NS)
def test_pendulum_projection_one_iteration_at_a_time(ops, n):
    k = ops.PendulumKernels()
    obs, ap, tag = ef.pend_proposals(n, seed=n, half_pi=(n == 513))       # cos theta -> 0 (C_o_inv ~ 1e7): six rows of the 513
    planes, iters, action = run_profile(ops, k, "pend", n, obs, ap, K, PEND_LR, 0.0, strided=True)
    c = judge_profile("pend", planes, iters, PEND_LR, obs=obs)
    AP, O, ACT, IT = Buf(ap), Buf(obs), Buf(np.full((n, 2), SENT, np.float32)), Buf(np.zeros(n, np.int32), torch.int32)
    k.act_project(O.view, AP.view, None, ACT.view, IT.view, ops.NOISE_NONE, 0, 0, 0, -6, 6, K, PEND_LR, EPS, 0.0)
    assert np.array_equal(bits(ACT.get()), bits(action)) and np.array_equal(IT.get(), iters)
    k.act_project(O.view, AP.view, None, ACT.view, None, ops.NOISE_NONE, 0, 0, 0, -6, 6, K, PEND_LR, EPS, 0.0)
    assert np.array_equal(bits(ACT.get()), bits(action))
    clean = ~(c["left"] | c["amb"]).any(axis=0)
    assert (~clean).mean() <= ef.AMBIG_CAP
    mplanes, miters, maction = run_profile(ops, k, "pend", n, obs, ap, K, PEND_LR, 0.5)
    p, o, it64, tclean = ef.project_b64("pend", ap, K, PEND_LR, EPS, 0.5, obs=obs)
    note("pend_grg", np.maximum(ef.ratio(maction[:, 0], p), ef.ratio(maction[:, 1], o))[clean].max(initial=0.0))
    # iteration counts under momentum: on the rows whose float64 momentum trajectory met no ambiguous mask or stop predicate
    # (few for this env: after completion |h| sits at round-off, inside the accumulated guard of corr_eps)
    both = clean & tclean
    np.testing.assert_array_equal(miters[both], it64[both])
    if n == 513:                                                  # the evaluation budget at the larger step: stop decisions in bulk
        planes, iters, action = run_profile(ops, k, "pend", n, obs, ap, 50, 2e-2, 0.0)
        judge_profile("pend", planes, iters, 2e-2, obs=obs)


@pytest.mark.parametrize("env", ["cart", "pend"])
def test_exploration_and_completion(ops, env):
    """RPO_NOISE_EXPLICIT at t = 40 (eps_t = max(0.1, 1 - 0.01 * 40) = 0.6): a_o is completed from the NOISED, clipped a_p; a NaN
    proposal passes through the clip (rpo_clamp) and the loop, which then stops after its first iteration -- NaN violates nothing."""
    n = 513
    rng = np.random.RandomState(3)
    noise = rng.randn(n).astype(np.float32)
    ctrl = new_ctrl(ops, 40)
    eps_t = float(np.float32(1.0) - np.float32(0.01) * np.float32(40.0))
    if env == "cart":
        table = ocs.Constants(1).as_array()
        k = ops.CartSafeKernels(table, 1)
        ap = ef.cart_proposals(n, 1)
        lo, hi, lr, obs, O = -10.0, 10.0, CART_LR, None, None
        kw = dict(table=table, partial=1)
    else:
        k = ops.PendulumKernels()
        obs, ap, tag = ef.pend_proposals(n, 1)
        lo, hi, lr, O = -6.0, 6.0, PEND_LR, Buf(obs)
        kw = dict(obs=obs)
    ap[7] = np.nan
    AP, NZ, ACT, IT = Buf(ap), Buf(noise), Buf(np.full((n, 2), SENT, np.float32)), Buf(np.zeros(n, np.int32), torch.int32)
    k.act_project(O.view if O else None, AP.view, NZ.view, ACT.view, IT.view, ops.NOISE_EXPLICIT, 1.0, 0.1, 0.01, lo, hi, 0, lr, EPS, 0.0, 0, 0, ctrl, None)
    got = ACT.get()
    assert np.isnan(got[7]).all() and np.all(IT.get() == 0)
    note(env + "_act", ef.check_explore(env, got, ap, noise, eps_t, lo, hi, **kw).max())
    k.act_project(O.view if O else None, AP.view, NZ.view, ACT.view, IT.view, ops.NOISE_EXPLICIT, 1.0, 0.1, 0.01, lo, hi, 5, lr, EPS, 0.0, 0, 0, ctrl, None)
    assert np.isnan(ACT.get()[7]).all() and IT.get()[7] == 1 and np.isfinite(np.delete(ACT.get(), 7, axis=0)).all()
    assert int(ctrl[ops.CONST["RPO_CTRL_T"]]) == 40 and int(ctrl[ops.CONST["RPO_CTRL_NONFINITE"]]) == 0          # read-only here


# ================================================================================================================ batched projection
def batch_lr(n):
    return 2e-3 * min(1.0, 256.0 / n)


def run_batch(ops, k, obs, ap, steps, lr, momentum=0.0):
    n = len(ap)
    O, AP, ACT, IT = Buf(obs), Buf(ap), Buf(np.full((n, 2), SENT, np.float32)), Buf(np.full(1, -1, np.int32), torch.int32)
    k.project_batchref(O.view, AP.view, ACT.view, IT.view, steps, lr, EPS, momentum)
    torch.cuda.synchronize()
    return ACT.get(), int(IT.get()[0])


@pytest.mark.parametrize("n", [1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 300, 1000, 1023, 1024])
def test_batched_projection_one_budget_at_a_time(ops, n):
    """rpo_pendulum_project_batchref at max_steps = 0..K (n <= 256: the register-tiled 1024-thread form; above: one thread per
    sample -- the dispatch has no other branch): budget k == the float64 coupled step applied to budget k - 1, or budget k - 1 bit
    for bit when iters_out says no k-th step was taken; the batch-global stop decided from float64."""
    k = ops.PendulumKernels()
    obs, ap = ef.batch_inputs(n)
    lr = batch_lr(n)
    prev, it = run_batch(ops, k, obs, ap, 0, lr)
    assert it == 0
    e = ef.pend_eq_of_obs(ef.B64, obs)
    with np.errstate(all="ignore"):
        note("pend_act", max(ef.ratio(prev[:, 0], ef.B64.inp(ap)).max(), ef.ratio(prev[:, 1], ef.pend_complete(ef.B64, e, ef.B64.inp(ap))).max()))
    first = prev
    worst, share, itp = 0.0, 0.0, 0
    for b in range(1, K + 1):
        cur, it = run_batch(ops, k, obs, ap, b, lr)
        c = ef.check_batch_budget(obs, prev, cur, it == b, lr, EPS, b)
        assert c["stop_ok"] or c["stop_open"], (b, it)
        assert it == b or it == itp, "a budget that took no step repeats the count"
        worst, share = max(worst, c["ratio"].max()), max(share, c["widened"].mean())
        prev, itp = cur, it
    print("widened share per budget (max): %.4f" % share)
    assert share <= ef.AMBIG_CAP
    note("batch_grg", worst)
    cur, it = run_batch(ops, k, obs, ap, 1, 0.05)                # the large step at K = 1
    c = ef.check_batch_budget(obs, first, cur, it == 1, 0.05, EPS, 1)
    assert c["stop_ok"] and c["widened"].mean() <= ef.AMBIG_CAP
    note("batch_grg", c["ratio"].max())


@pytest.mark.parametrize("kind", ["feasible", "one_first", "one_last"])
@pytest.mark.parametrize("n", [17, 256, 300])
def test_batched_projection_stop_is_batch_global(ops, n, kind):
    """theta = 0 rows (C_p = 0, C_o = 1: h = 0 exactly, no stop margin near its guard).  An all-feasible batch stops after its
    first iteration with every row unchanged by the second budget; ONE infeasible row -- row 0 or row n - 1, the lanes that
    publish dgp and the stop word -- keeps the whole batch stepping (rpo_ddpg.py:271-272)."""
    k = ops.PendulumKernels()
    obs, ap = ef.batch_inputs(n, kind)
    lr = batch_lr(n)
    prev, it = run_batch(ops, k, obs, ap, 0, lr)
    took = []
    for b in range(1, 5):
        cur, it = run_batch(ops, k, obs, ap, b, lr)
        c = ef.check_batch_budget(obs, prev, cur, it == b, lr, EPS, b)
        assert not c["stop_open"] and c["stop_ok"], (b, it)
        note("batch_grg", c["ratio"].max())
        assert not c["widened"].any()
        took.append(it == b)
        if kind == "feasible" and b >= 2:
            assert it == 1 and np.array_equal(bits(cur), bits(prev))
        prev = cur
    assert took == ([True, False, False, False] if kind == "feasible" else [True] * 4)
    if kind != "feasible":
        first, _ = run_batch(ops, k, obs, ap, 0, lr)
        assert (bits(prev) != bits(first)).any(axis=1).all()       # every row moved: the feasible ones were carried along


@pytest.mark.parametrize("n", [17, 256, 300])
def test_batched_projection_momentum_trajectory(ops, n):
    """corr_momentum = 0.5 at the budget K as a whole trajectory (the register-tiled form and one thread per sample; the old step
    lives in registers in both): against the float64 coupled trajectory within K x the single-step tolerance, on the rows whose
    momentum-0 budgets carried no widened predicate and whose float64 momentum trajectory kept every predicate K single-step
    guards away from 0; at most 2 % of the rows may be left out.  The batch-global iteration count must be float64's."""
    k = ops.PendulumKernels()
    obs, ap = ef.batch_inputs(n)
    lr = batch_lr(n)
    prev, it = run_batch(ops, k, obs, ap, 0, lr)
    widened = np.zeros(n, bool)
    for b in range(1, K + 1):
        cur, it = run_batch(ops, k, obs, ap, b, lr)
        widened |= ef.check_batch_budget(obs, prev, cur, it == b, lr, EPS, b)["widened"]
        prev = cur
    got, it = run_batch(ops, k, obs, ap, K, lr, momentum=0.5)
    c = ef.check_batch_momentum(obs, ap, got, K, lr, EPS, 0.5)
    assert not c["stop_open"] and it == c["iters"]
    judged = ~widened & c["clean"]
    print("left out: %d of %d rows" % ((~judged).sum(), n))
    assert (~judged).mean() <= ef.AMBIG_CAP
    note("batch_mom", c["ratio"][judged].max(), ef.tol_c("batch_grg"))
    assert (bits(got) != bits(prev)).any()                          # (the momentum term moved the result)
