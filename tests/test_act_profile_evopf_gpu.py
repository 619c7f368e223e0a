"""trainer.act(obs, profile=True) on EVOPF-v0 under schedule ``profile_evopf=1`` on the MI355X: the planes of ONE launch of
``rpo_evopf_project_profile`` against K + 1 separate ``act()`` calls (the existing stepwise kernels, ``rpo_evopf_act_project`` +
``rpo_evopf_resid``) and against the sweep (``profile_evopf=0``), bit for bit.

Trainers and inputs: ``build_trainer(algo, "evopf256", ..., num_envs=16, use_graph=False, schedule=dict(profile_evopf=1))`` after
``run_steps(4)`` and the valid rows of ``evaluate(16, seed=4, record=True)`` -- tests/test_act_gpu.py's
``test_stepwise_only_configurations``.

The rows must exercise the loop.  At the default settings (``eval_lr = 1e-4``, ``corr_eps = 1e-5``) nearly every row uses the
whole budget, so the comparisons run with K = 12, ``eval_lr = LR_MULT * tr.eval_lr`` and ``tr.corr_eps = CORR_EPS`` (``_loose``).
Values taken: LR_MULT = 3, CORR_EPS = 0.05.  Through the oracle backend on the CPU (64-wide networks, 16 recorded rows) they gave
RPODDPG 4 rows at 1 iteration, 6 rows at 2-3 and 6 rows at 12, RPOSAC 10 rows at 1, 4 rows in between and 2 rows at 12; at the
multipliers 10 and 30 no CPU row stopped strictly inside the budget for ``corr_eps`` from 0.02 to 0.2.  The 256-wide networks
on the device are other weights, so ``test_inputs_exercise_all_three_kinds_of_row`` asserts the property on the first 37 rows of
the device's own input (it prints the histogram of the iteration counts).  On the MI355X these values gave, for iterations 0..12,
RPODDPG [0, 23, 4, 1, 1, 1, 0, 0, 0, 0, 1, 0, 6] and RPOSAC [0, 18, 6, 1, 0, 1, 0, 2, 0, 0, 0, 1, 8] rows of the 37: all three kinds.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from test_train_step_golden import build_trainer

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
K = 12
LR_MULT = 3.0
CORR_EPS = 0.05
ROWS = 37
SIZES = (1, 3, 5, ROWS)           # ragged four-wave workgroups (1, 3, 5 rows) and ten workgroups with a one-wave tail


@functools.lru_cache(maxsize=None)
def _setup(algo):
    """(trainer with profile_evopf=1, observations [>= ROWS, 57]) -- shared by the tests of a case and left unchanged by them."""
    from rpo_amd import ops
    assert torch.cuda.is_available()
    torch.manual_seed(5)
    tr = build_trainer(algo, "evopf256", ops, DEV, num_envs=16, use_graph=False, schedule=dict(profile_evopf=1))
    tr.vec.reset()
    tr.run_steps(4)
    t = tr.evaluate(16, seed=4, record=True).trajectory
    obs = torch.tensor(t.obs[t.valid], device=DEV).contiguous()
    assert obs.shape[0] >= ROWS and tr.schedule["profile_evopf"] == 1
    return tr, obs


class _loose(object):
    """``corr_eps = CORR_EPS`` inside the block; ``kw``: the budget and the step size of the calls."""

    def __init__(self, tr):
        self.tr = tr
        self.kw = dict(eval_steps=K, eval_lr=LR_MULT * tr.eval_lr)

    def __enter__(self):
        self.old = self.tr.corr_eps
        self.tr.corr_eps = CORR_EPS
        return self.kw

    def __exit__(self, *exc):
        self.tr.corr_eps = self.old
        return False


class _swept(object):
    """schedule profile_evopf = 0 inside the block: act(profile=True) sweeps."""

    def __init__(self, tr):
        self.tr = tr

    def __enter__(self):
        self.tr.schedule["profile_evopf"] = 0

    def __exit__(self, *exc):
        self.tr.schedule["profile_evopf"] = 1
        return False


def _signed_absmax_np(eq):
    """The lowest-index rule restated: per row the entry of largest magnitude with its sign; among equal magnitudes the lowest
    index; a NaN wins over everything, the first one."""
    out = np.empty(eq.shape[0], dtype=np.float32)
    for i, row in enumerate(eq):
        nan = np.nonzero(np.isnan(row))[0]
        if nan.size:
            j = int(nan[0])
        else:
            mag = np.abs(row)
            j = int(np.nonzero(mag == mag.max())[0][0])
        out[i] = row[j]
    return out


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def _planes_equal_calls(tr, x, p, steps, lr):
    """Plane b of the profiled result ``p`` is act(x, eval_steps=b) of the stepwise kernels, for every b; its other fields are
    the call at the budget."""
    assert p.path == "stepwise" and p.form is None and p.profile.K == steps
    assert tuple(p.profile.data.shape) == (steps + 1, x.shape[0], 4)
    for b in range(steps + 1):
        r = tr.act(x, eval_steps=b, eval_lr=lr)
        assert r.path == "stepwise" and r.profile is None
        assert torch.equal(p.profile.action(b), r.action[:, :2]), b
        assert torch.equal(p.profile.ineq(b), r.ineq_resid.max(dim=1).values), b
        assert torch.equal(p.profile.iters_at(b), r.iters), b
        assert np.array_equal(_bits(p.profile.eq(b)), _signed_absmax_np(r.eq_resid.cpu().numpy()).view(np.uint32)), b
        assert torch.equal(p.profile.eq(b).abs(), r.eq_resid.abs().max(dim=1).values), b
    for f in r.FIELDS:                                           # (r: the call at the budget)
        assert torch.equal(getattr(p, f), getattr(r, f)), f


@pytest.mark.parametrize("algo", ["ddpg", "sac"])
def test_inputs_exercise_all_three_kinds_of_row(algo):
    """A property of the inputs (of the EXISTING act()), not of the code under test: see the module docstring."""
    tr, obs = _setup(algo)
    with _loose(tr) as kw:
        it = tr.act(obs[:ROWS], **kw).iters
    print(algo, "iters histogram 0..K:", torch.bincount(it, minlength=K + 1).tolist())
    assert bool((it == 1).any()), "no row stops after the unconditional iteration"
    assert bool(((it > 1) & (it < K)).any()), "no row stops strictly inside the budget"
    assert bool((it == K).any()), "no row uses the whole budget"


@pytest.mark.parametrize("algo", ["ddpg", "sac"])
def test_planes_equal_the_separate_calls_bit_for_bit(algo):
    tr, obs = _setup(algo)
    with _loose(tr) as kw:
        for n in SIZES:
            x = obs[:n].contiguous()
            _planes_equal_calls(tr, x, tr.act(x, profile=True, **kw), K, kw["eval_lr"])
    # ... and at the trainer's own settings (nearly every row takes the whole budget)
    x = obs[:ROWS].contiguous()
    _planes_equal_calls(tr, x, tr.act(x, profile=True, eval_steps=5), 5, tr.eval_lr)


@pytest.mark.parametrize("algo", ["ddpg", "sac"])
def test_switch_on_equals_switch_off(algo):
    tr, obs = _setup(algo)
    x = obs[:ROWS].contiguous()
    with _loose(tr) as kw:
        # torch's argmax (the sweep) and the kernel both take the lowest index among equal magnitudes; the comparison is about one
        # residual per row only if no row has two of equal largest magnitude and opposite sign, at any budget
        ties = 0
        for b in range(K + 1):
            eq = tr.act(x, eval_steps=b, eval_lr=kw["eval_lr"]).eq_resid
            top = eq.abs().max(dim=1, keepdim=True).values
            ties += int((((eq == top).any(dim=1)) & ((eq == -top).any(dim=1)) & (top[:, 0] > 0)).sum())
        assert ties == 0
        on = tr.act(x, profile=True, **kw)
        with _swept(tr):
            off = tr.act(x, profile=True, **kw)
    assert on.path == "stepwise" and off.path == "sweep" and on.form is None and off.form is None
    assert torch.equal(on.profile.data, off.profile.data) and torch.equal(on.profile.iters, off.profile.iters)
    for f in on.FIELDS:
        assert torch.equal(getattr(on, f), getattr(off, f)), f


def test_edge_budgets_and_out_reuse():
    tr, obs = _setup("ddpg")
    x = obs[:ROWS].contiguous()
    with _loose(tr) as kw:
        lr = kw["eval_lr"]
        p0 = tr.act(x, profile=True, eval_steps=0, eval_lr=lr)
        assert tuple(p0.profile.data.shape) == (1, ROWS, 4) and int(p0.iters.abs().max()) == 0
        _planes_equal_calls(tr, x, p0, 0, lr)
        p1 = tr.act(x, profile=True, eval_steps=1, eval_lr=lr)
        assert int(p1.iters.min()) == 1                         # the unconditional iteration
        _planes_equal_calls(tr, x, p1, 1, lr)
        # every plane of every row is written: a NaN-filled buffer holds no NaN afterwards; reuse allocates no new profile
        p = tr.act(x, profile=True, **kw)
        ref = {f: getattr(p, f).clone() for f in p.FIELDS}
        ptrs = {f: getattr(p, f).data_ptr() for f in p.FIELDS}
        data, ptr = p.profile.data.clone(), p.profile.data.data_ptr()
        p.profile.data.fill_(float("nan"))
        p.action.fill_(float("nan"))
        again = tr.act(x, profile=True, out=p, **kw)
        assert again is p and again.path == "stepwise" and again.profile.data.data_ptr() == ptr
        assert not bool(torch.isnan(again.profile.data).any()) and torch.equal(again.profile.data, data)
        for f in p.FIELDS:
            assert getattr(again, f).data_ptr() == ptrs[f] and torch.equal(getattr(again, f), ref[f]), f
        q = tr.act(x, profile=True, residuals=False, **kw)
        assert q.eq_resid is None and torch.equal(q.profile.data, data) and torch.equal(q.iters, p.iters)
        for bad in (tr.act(x, **kw), tr.act(x[:5].contiguous(), profile=True, **kw)):
            with pytest.raises(ValueError):                      # _check's refusals apply unchanged: no profile; another n
                tr.act(x, profile=True, out=bad, **kw)
        with pytest.raises(ValueError):
            tr.act(x, profile=True, form=1, **kw)


def test_non_contiguous_observation_view():
    """The observation rows of a wider tensor (a row stride above 57) give the planes of the dense copy."""
    tr, obs = _setup("sac")
    x = obs[:ROWS].contiguous()
    wide = torch.full((ROWS, 80), float("nan"), device=DEV)
    wide[:, :57] = x
    view = wide[:, :57]
    assert not view.is_contiguous()
    with _loose(tr) as kw:
        a, b = tr.act(x, profile=True, **kw), tr.act(view, profile=True, **kw)
        assert b.path == "stepwise" and torch.equal(a.profile.data, b.profile.data) and torch.equal(a.iters, b.iters)
        assert torch.equal(a.action, b.action)
        # the binding itself takes the strided rows (act() may have made them dense)
        k = tr.kernels
        ap = tr._eval_partial(x).clone()
        action, iters = torch.zeros(ROWS, k.action_dim, device=DEV), torch.zeros(ROWS, dtype=torch.int32, device=DEV)
        data = torch.empty(K + 1, ROWS, 4, device=DEV)
        tr.backend.evopf_project_profile(k, view, ap, action, iters, K, kw["eval_lr"], tr.corr_eps, tr.corr_momentum, data, **tr._act_kw)
        assert torch.equal(data, a.profile.data) and torch.equal(action, a.action) and torch.equal(iters, a.iters)


@pytest.mark.parametrize("algo", ["ddpg", "sac"])
def test_rows_are_independent(algo):
    """Permuting the input rows permutes the profile's rows."""
    tr, obs = _setup(algo)
    x = obs[:ROWS].contiguous()
    perm = torch.randperm(ROWS, generator=torch.Generator().manual_seed(3)).to(DEV)
    with _loose(tr) as kw:
        a, b = tr.act(x, profile=True, **kw), tr.act(x[perm].contiguous(), profile=True, **kw)
    assert a.path == "stepwise" and int(a.iters.max()) >= 2
    assert torch.equal(b.profile.data, a.profile.data[:, perm]) and torch.equal(b.profile.iters, a.profile.iters[perm])
    assert torch.equal(b.action, a.action[perm])


@pytest.mark.parametrize("algo", ["ddpg", "sac"])
def test_nothing_is_disturbed(algo):
    tr, obs = _setup(algo)
    x = obs[:ROWS].contiguous()
    v, ag = tr.vec, tr.agent

    def state():
        s = dict(flat=ag.flat.data, critic_target=ag.critic_target_flat, ctrl=v.ctrl, internal=v.internal, obs=v.obs, ep_len=v.ep_len,
                 ep_ret=v.ep_ret, ep_count=v.ep_count, replay=tr.buffer.rows)
        if getattr(ag, "actor_target_flat", None) is not None:
            s["actor_target"] = ag.actor_target_flat
        for name in ("actor_optim", "critic_optim", "nju_optim", "lamb_optim"):
            o = getattr(ag, name)
            s[name + ".m"], s[name + ".v"], s[name + ".step"] = o.exp_avg, o.exp_avg_sq, o.step_dev
        return s
    before = {k: t.clone() for k, t in state().items()}
    with _loose(tr) as kw:
        r = tr.act(x, profile=True, **kw)
    assert r.path == "stepwise"
    torch.cuda.synchronize()
    for name, t in state().items():
        assert torch.equal(before[name], t), name


def test_direct_abi_call():
    """A plane buffer pre-filled with a NaN payload: fully overwritten for the n rows, untouched behind (K + 1) * n * 4 floats."""
    from rpo_amd import _lib, ops
    tr, obs = _setup("ddpg")
    lib, k, n = _lib.load(), tr.kernels, ROWS
    x = obs[:n].contiguous()
    vp = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    payload = np.uint32(0x7FC12345)
    with _loose(tr) as kw:
        ref = tr.act(x, profile=True, **kw)
        ap = tr._eval_partial(x).clone()
        action, iters = torch.zeros(n, k.action_dim, device=DEV), torch.zeros(n, dtype=torch.int32, device=DEV)
        used, tail = (K + 1) * n * 4, 64
        buf = torch.from_numpy(np.full(used + tail, payload, dtype=np.uint32).view(np.float32)).to(DEV)
        raw = int(tr._act_kw.get("ap_is_raw", False))
        args = (n, vp(x), 57, vp(ap), raw, vp(action), vp(iters), K, kw["eval_lr"], tr.corr_eps, tr.corr_momentum, k.newton_tol,
                k.newton_max_iters, k._c(action))
        assert lib.rpo_evopf_project_profile(*args, ctypes.c_void_p(buf.data_ptr() + 4), stream) == ops.CONST["RPO_ERR_ARG"]
        assert lib.rpo_evopf_project_profile(*args, None, stream) == ops.CONST["RPO_ERR_NULL"]
        assert bool((_bits(buf) == payload).all())               # (the refusals wrote nothing)
        assert lib.rpo_evopf_project_profile(*args, vp(buf), stream) == 0
        torch.cuda.synchronize()
    got = _bits(buf)
    assert not bool((got[:used] == payload).any()) and not bool(np.isnan(got[:used].view(np.float32)).any())
    assert bool((got[used:] == payload).all())
    assert torch.equal(buf[:used].view(K + 1, n, 4), ref.profile.data)
    assert torch.equal(action, ref.action) and torch.equal(iters, ref.iters)
    # iters may be NULL
    args = args[:6] + (None,) + args[7:]
    assert lib.rpo_evopf_project_profile(*args, vp(buf), stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(buf[:used].view(K + 1, n, 4), ref.profile.data)
