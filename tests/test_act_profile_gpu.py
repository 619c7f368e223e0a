"""trainer.act(obs, profile=True) on the MI355X: the profile planes of ONE launch against K + 1 separate act() calls, bit for bit,
on the fused path (rpo_<env>_policy_act_profile) and the stand-alone path (rpo_<env>_project_profile, schedule fused_act=0).

Trainers and inputs are tests/test_act_gpu.py's (its ``_setup``: 64 lanes, 8 training steps, the valid rows of
``evaluate(1000, seed=11, record=True)``; its ``_shifted(tr, SHIFT[env])`` block).  Every comparison runs once inside the block
(rows that need many iterations) and once outside it (rows that are feasible after Complete and take the one unconditional
iteration).

``eval_lr`` multiplier: LR_MULT = 10.  With the budget K = 7 the existing ``act()`` must show all three kinds of row: rows that
use the whole budget (iters == K), rows whose stop test fires inside it (1 < iters < K) and, unshifted, rows that stop after
the unconditional iteration (iters == 1).  Checked first through the oracle backend on the CPU (3000 recorded rows per case, K = 7;
multipliers 1, 3, 10, 30, 100, 300): at 10 the shifted rows give CartSafe {5, 6, 7} (RPODDPG 278 / 2134 / 588, RPOSAC
22 / 2822 / 156) and SpringPendulum every value 1..7 (RPODDPG 1500 rows at 7, RPOSAC 2676); at 1 and 3 every CartSafe row
takes 7, at 30 no CartSafe row and at most one SpringPendulum row does, from 100 nearly every row stops at 1.  Unshifted, every
row of every case takes 1.  ``test_inputs_exercise_all_three_kinds_of_row`` asserts the property on the device's inputs.
"""
import ctypes

import pytest
import torch

from test_act_gpu import CASES, SHIFT, _rows, _setup, _shifted
from test_train_step_golden import build_trainer

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
K = 7
LR_MULT = 10.0
SIZES = (1, 17, 1000, 12293)      # one row; a ragged 16-row tile; many workgroups; 64-row workgroups with a ragged tail


@pytest.fixture(scope="module")
def hip():
    from rpo_amd import ops
    assert torch.cuda.is_available()
    return ops


class _standalone(object):
    """schedule fused_act = 0 inside the block: act() takes the stepwise path."""

    def __init__(self, tr):
        self.tr = tr

    def __enter__(self):
        self.tr.schedule["fused_act"] = 0

    def __exit__(self, *exc):
        self.tr.schedule["fused_act"] = 1
        return False


def _planes_equal_calls(tr, x, p, kw, path):
    """Plane b of the profiled result ``p`` is act(x, eval_steps=b) on the same path, for every b; its other fields are act(x, K)."""
    assert p.path == path and p.profile.K == kw["eval_steps"] and tuple(p.profile.data.shape) == (kw["eval_steps"] + 1, x.shape[0], 4)
    for b in range(kw["eval_steps"] + 1):
        r = tr.act(x, eval_steps=b, eval_lr=kw["eval_lr"], form=1 if path == "fused" else 0)
        assert r.path == path and r.profile is None
        assert torch.equal(p.profile.action(b), r.action), b
        assert torch.equal(p.profile.eq(b), r.eq_resid[:, 0]), b
        assert torch.equal(p.profile.ineq(b), r.ineq_resid.max(dim=1).values), b
        assert torch.equal(p.profile.iters_at(b), r.iters), b
    for f in r.FIELDS:                                           # (r: the call at the budget K)
        assert torch.equal(getattr(p, f), getattr(r, f)), f


@pytest.mark.parametrize("algo,envname", CASES)
def test_planes_equal_the_separate_calls_bit_for_bit(hip, algo, envname):
    tr, _, obs = _setup(algo, envname)
    kw = dict(eval_steps=K, eval_lr=LR_MULT * tr.eval_lr)
    for shift in (SHIFT[envname], 0.0):
        with _shifted(tr, shift):
            for n in SIZES:
                x = _rows(obs, n)
                fused = tr.act(x, profile=True, **kw)
                _planes_equal_calls(tr, x, fused, kw, "fused")
                with _standalone(tr):
                    alone = tr.act(x, profile=True, **kw)
                    _planes_equal_calls(tr, x, alone, kw, "stepwise")
                assert torch.equal(fused.profile.data, alone.profile.data), (n, shift)
                assert torch.equal(fused.profile.iters, alone.profile.iters), (n, shift)


@pytest.mark.parametrize("algo,envname", CASES)
def test_inputs_exercise_all_three_kinds_of_row(hip, algo, envname):
    """A property of the inputs (of the EXISTING act()), not of the code under test: see the module docstring."""
    tr, _, obs = _setup(algo, envname)
    x = _rows(obs, 1000)
    with _shifted(tr, SHIFT[envname]):
        it = tr.act(x, eval_steps=K, eval_lr=LR_MULT * tr.eval_lr).iters
    plain = tr.act(x, eval_steps=K, eval_lr=LR_MULT * tr.eval_lr).iters
    print(algo, envname, "shifted iters:", torch.bincount(it, minlength=K + 1).tolist(), "unshifted:", torch.bincount(plain, minlength=K + 1).tolist())
    assert bool((it == K).any()), "no row uses the whole budget"
    assert bool(((it > 1) & (it < K)).any()), "no row stops strictly inside the budget"
    assert bool((plain == 1).any()), "no unshifted row stops after the unconditional iteration"


@pytest.mark.parametrize("algo,envname", [("ddpg", "cart"), ("sac", "pendulum")])
def test_edge_budgets_and_out_reuse(hip, algo, envname):
    tr, _, obs = _setup(algo, envname)
    x = _rows(obs, 1000)
    lr = LR_MULT * tr.eval_lr
    with _shifted(tr, SHIFT[envname]):
        for path in ("fused", "stepwise"):
            if path == "stepwise":
                tr.schedule["fused_act"] = 0
            try:
                p0 = tr.act(x, profile=True, eval_steps=0, eval_lr=lr)
                assert tuple(p0.profile.data.shape) == (1, 1000, 4) and int(p0.iters.abs().max()) == 0
                _planes_equal_calls(tr, x, p0, dict(eval_steps=0, eval_lr=lr), path)
                _planes_equal_calls(tr, x, tr.act(x, profile=True, eval_steps=1, eval_lr=lr), dict(eval_steps=1, eval_lr=lr), path)
                # every plane of every row is written: a NaN-filled buffer holds no NaN afterwards; reuse gives equal bits
                p = tr.act(x, profile=True, eval_steps=K, eval_lr=lr)
                ref, ptr = p.profile.data.clone(), p.profile.data.data_ptr()
                p.profile.data.fill_(float("nan"))
                again = tr.act(x, profile=True, eval_steps=K, eval_lr=lr, out=p)
                assert again is p and again.profile.data.data_ptr() == ptr and again.path == path
                assert not bool(torch.isnan(again.profile.data).any())
                assert torch.equal(again.profile.data, ref)
                third = tr.act(x, profile=True, eval_steps=K, eval_lr=lr, out=again)
                assert third.profile.data.data_ptr() == ptr and torch.equal(third.profile.data, ref)
            finally:
                tr.schedule["fused_act"] = 1


@pytest.mark.parametrize("algo,envname", [("ddpg", "cart"), ("sac", "pendulum")])
def test_rows_are_independent(hip, algo, envname):
    """Permuting the input rows permutes the profile's rows."""
    tr, _, obs = _setup(algo, envname)
    n = 1000
    x = _rows(obs, n)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(3)).to(DEV)
    kw = dict(profile=True, eval_steps=K, eval_lr=LR_MULT * tr.eval_lr)
    with _shifted(tr, SHIFT[envname]):
        a, b = tr.act(x, **kw), tr.act(x[perm].contiguous(), **kw)
        assert a.path == "fused" and int(a.iters.max()) >= 2
        assert torch.equal(b.profile.data, a.profile.data[:, perm])
        assert torch.equal(b.profile.iters, a.profile.iters[perm])
        with _standalone(tr):
            c = tr.act(x[perm].contiguous(), **kw)
        assert c.path == "stepwise" and torch.equal(c.profile.data, a.profile.data[:, perm])


def test_evopf_sweeps(hip):
    """EVOPF-v0 (evopf256, n = 4, K = 2): the planes are three act() calls; a0, a1 are the first two action components and the
    equality entry is the row's equality residual of largest magnitude, with its sign."""
    torch.manual_seed(5)
    tr = build_trainer("ddpg", "evopf256", hip, DEV, num_envs=16, use_graph=False)
    tr.vec.reset()
    tr.run_steps(4)
    x = tr.vec.obs[:4].clone()
    p = tr.act(x, profile=True, eval_steps=2)
    assert p.path == "sweep" and tuple(p.profile.data.shape) == (3, 4, 4)
    for b in range(3):
        r = tr.act(x, eval_steps=b)
        assert torch.equal(p.profile.action(b), r.action[:, :2])
        assert torch.equal(p.profile.eq(b), r.eq_resid.gather(1, r.eq_resid.abs().argmax(dim=1, keepdim=True))[:, 0])
        assert torch.equal(p.profile.ineq(b), r.ineq_resid.max(dim=1).values)
        assert torch.equal(p.profile.iters_at(b), r.iters)
    for f in r.FIELDS:
        assert torch.equal(getattr(p, f), getattr(r, f)), f


def test_refusals(hip):
    tr, _, obs = _setup("ddpg", "cart")
    x = _rows(obs, 1000)
    with pytest.raises(ValueError):
        tr.act(x, profile=True, form=1)
    # a profile above RPO_TRACE_MAX_BYTES: refused by shape arithmetic (the row view below is 1 GiB + 16 bytes of profile at
    # K = 7 and itself 24 bytes of storage: nothing of that size is allocated)
    cap = hip.CONST["RPO_TRACE_MAX_BYTES"]
    n_big = cap // (16 * (K + 1)) + 1
    with pytest.raises(ValueError) as e:
        tr.act(x[:1].expand(n_big, -1), profile=True, eval_steps=K)
    assert str(n_big - 1) in str(e.value)                        # (the message names the largest n that fits)
    good = tr.act(x, profile=True, eval_steps=K)
    for bad in (tr.act(x), tr.act(x[:999].contiguous(), profile=True, eval_steps=K), good):
        with pytest.raises(ValueError):                          # no profile; another n; another K
            tr.act(x, profile=True, eval_steps=K + 1 if bad is good else K, out=bad)
    torch.manual_seed(5)
    la = build_trainer("ddpgla", "cart", hip, DEV, num_envs=16, use_graph=False, fused=False)
    with pytest.raises(ValueError):
        la.act(x, profile=True)


def test_nothing_is_disturbed(hip, monkeypatch):
    tr, _, obs = _setup("ddpg", "cart")
    x = _rows(obs, 1000)
    v = tr.vec
    before = dict(flat=tr.agent.flat.data.clone(), ctrl=v.ctrl.clone(), internal=v.internal.clone(), ep_len=v.ep_len.clone(),
                  ep_ret=v.ep_ret.clone(), ep_count=v.ep_count.clone())
    tr.act(x, profile=True, eval_steps=K)
    with _standalone(tr):
        tr.act(x, profile=True, eval_steps=K)
    torch.cuda.synchronize()
    after = dict(flat=tr.agent.flat.data, ctrl=v.ctrl, internal=v.internal, ep_len=v.ep_len, ep_ret=v.ep_ret, ep_count=v.ep_count)
    for name, t in before.items():
        assert torch.equal(t, after[name]), name

    monkeypatch.setenv("RPO_GRAPH_CYCLE", "4")                   # ... and training goes on as if the call had not happened

    def fresh():
        torch.manual_seed(5)
        t = build_trainer("ddpg", "cart", hip, DEV, num_envs=512, use_graph=True)
        t.vec.reset()
        return t
    a = fresh()
    a.run_steps(4)
    a.run_steps(16)
    b = fresh()
    b.run_steps(4)
    r = b.act(_rows(obs, 4096), profile=True, eval_steps=K)
    assert r.path == "fused" and r.profile.n == 4096
    b.run_steps(16)
    torch.cuda.synchronize()
    for k in ("internal", "ep_len", "ep_ret", "ep_count", "ctrl"):
        assert torch.equal(getattr(a.vec, k), getattr(b.vec, k)), k
    assert torch.equal(a.buffer.rows, b.buffer.rows)
    assert torch.equal(a.agent.flat.data, b.agent.flat.data)
    assert torch.equal(a.agent.critic_target_flat, b.agent.critic_target_flat)


def test_direct_abi_calls(hip):
    from rpo_amd import _lib
    lib, ERR_ARG = _lib.load(), hip.CONST["RPO_ERR_ARG"]
    n = 1000
    vp = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())   # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    new = lambda *shape, dt=torch.float32: torch.zeros(*shape, dtype=dt, device=DEV)   # noqa: E731
    for algo, envname in (("ddpg", "cart"), ("sac", "pendulum")):
        tr, _, obs = _setup(algo, envname)
        k, net = tr.kernels, tr.fused.descs["actor"].net_struct()
        x = _rows(obs, n)
        scale, base = tr._box_affine
        action, ap, iters = new(n, 2), tr._eval_partial(x).clone(), new(n, dt=torch.int32)
        buf = new((K + 1) * n * 4 + 4)
        grg = (tr.eval_lr, tr.corr_eps, tr.corr_momentum)
        if envname == "cart":
            consts = ctypes.c_void_p(k.consts.ctypes.data)
            fused = lambda prof, steps: lib.rpo_cartsafe_policy_act_profile(   # noqa: E731
                ctypes.byref(net), 0, scale, base, n, vp(x), 6, vp(action), None, None, None, None, tr._box_lo, tr._box_hi, steps,
                *grg, consts, k.partial, prof, stream)
            alone = lambda prof, steps: lib.rpo_cartsafe_project_profile(   # noqa: E731
                n, vp(ap), vp(action), vp(iters), steps, *grg, consts, k.partial, prof, stream)
        else:
            fused = lambda prof, steps: lib.rpo_pendulum_policy_act_profile(   # noqa: E731
                ctypes.byref(net), 1, scale, base, n, vp(x), 5, vp(action), None, None, None, None, tr._box_lo, tr._box_hi, steps,
                *grg, prof, stream)
            alone = lambda prof, steps: lib.rpo_pendulum_project_profile(   # noqa: E731
                n, vp(x), 5, vp(ap), vp(action), vp(iters), steps, *grg, prof, stream)
        ref = tr.act(x, profile=True, eval_steps=K)
        for call in (fused, alone):
            assert call(None, K) == ERR_ARG                      # a NULL profile
            assert call(vp(buf), -1) == ERR_ARG                  # K < 0
            assert call(vp(buf[1:]), K) == ERR_ARG               # a profile offset by 4 bytes
            buf.zero_()
            assert call(vp(buf), K) == 0
            assert torch.equal(buf[:(K + 1) * n * 4].view(K + 1, n, 4), ref.profile.data)
            assert torch.equal(action, ref.action) and float(buf[(K + 1) * n * 4:].abs().max()) == 0   # (nothing behind the last plane)
    torch.cuda.synchronize()
