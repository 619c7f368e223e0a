"""trainer.act() on the MI355X: the fused launch (rpo_<env>_policy_act, row-tile and streaming forms) against the stepwise path,
the recorded trajectory of evaluate(), the rows' independence, and the training it must not disturb.

Bit equality.  The fused kernels are built from the pieces of the stand-alone launches (mlp_tile_forward / stream_tile,
gauss_head_row, *_explore_project, eq_ineq / pendulum_resid_kernel's expressions), so every field is EQUAL between the paths.

Inputs: the valid rows of a recorded evaluation (``evaluate(1000, seed=11, record=True)`` after 8 training steps), tiled up to
the sizes the forms need.  On those rows the policy's proposals are feasible after Complete: the GRG loop runs its one
unconditional iteration (``iters == 1``).  So every comparison runs a second time with the actor's last bias shifted
(``SHIFT``: proposals towards the box edge, Complete leaves the inequalities violated, rows take up to ``eval_steps``
iterations), and asserts ``iters.max() >= 2`` there.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from test_train_step_golden import build_trainer

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
CASES = [("ddpg", "cart"), ("sac", "cart"), ("ddpg", "pendulum"), ("sac", "pendulum")]
SHIFT = {"cart": 1.2, "pendulum": 0.8}
FIELDS = ("action", "proposal", "iters", "eq_resid", "ineq_resid")


@pytest.fixture(scope="module")
def hip():
    from rpo_amd import ops
    assert torch.cuda.is_available()
    return ops


@functools.lru_cache(maxsize=None)
def _setup(algo, envname):
    """(trainer, recorded trajectory, its valid observations on the device) -- shared by the tests and left unchanged."""
    from rpo_amd import ops
    torch.manual_seed(5)
    tr = build_trainer(algo, envname, ops, DEV, num_envs=64, use_graph=False)
    tr.vec.reset()
    tr.run_steps(8)                                            # a policy that has moved off its initialisation
    t = tr.evaluate(1000, seed=11, record=True).trajectory
    obs = torch.tensor(t.obs[t.valid], device=DEV)
    assert obs.shape[0] >= 1000
    return tr, t, obs


def _rows(obs, n):
    """n rows: the recorded observations, repeated as often as needed."""
    reps = (n + obs.shape[0] - 1) // obs.shape[0]
    return obs.repeat(reps, 1)[:n].contiguous()


class _shifted(object):
    """The actor's last bias (the mean head's for RPOSAC) moved by ``delta`` inside the block."""

    def __init__(self, tr, delta):
        self.b, self.delta = tr.fused.descs["actor"].tensors["b1"], float(delta)

    def __enter__(self):
        with torch.no_grad():
            self.old = self.b.detach().clone()
            self.b += self.delta

    def __exit__(self, *exc):
        with torch.no_grad():
            self.b.copy_(self.old)
        return False


def _stepwise(tr, obs, **kw):
    tr.schedule["fused_act"] = 0
    try:
        r = tr.act(obs, **kw)
    finally:
        tr.schedule["fused_act"] = 1
    assert r.path == "stepwise" and r.form is None
    return r


def _equal(a, b, sl=slice(None), fields=FIELDS):
    for f in fields:
        assert torch.equal(getattr(a, f)[sl], getattr(b, f)), f


# form 1: n = 1, 17, 1000 (16-row workgroups, ragged last tile), 12 288 + 5 (64-row workgroups, ragged)
# forms 2, 3: n = 17, 1000, 4101 (partial last tile, partial last group, waves without a tile); form 0 at all of them
SIZES = {1: (1, 17, 1000, 12293), 2: (17, 1000, 4101), 3: (17, 1000, 4101), 0: (1, 17, 1000, 4101, 12293)}


@pytest.mark.parametrize("form", [1, 2, 3, 0])
@pytest.mark.parametrize("algo,envname", CASES)
def test_fused_equals_stepwise_bit_for_bit(hip, algo, envname, form):
    tr, _, obs = _setup(algo, envname)
    for shift in (0.0, SHIFT[envname]):
        with _shifted(tr, shift):
            for n in SIZES[form]:
                x = _rows(obs, n)
                a, b = tr.act(x, form=form), _stepwise(tr, x)
                assert a.path == "fused" and a.form == ("stream" if form >= 2 else "tile")
                _equal(a, b)
                assert int(a.iters.max()) >= (2 if shift else 1), (n, shift)
            if shift:
                assert float(a.max_ineq().max()) > 0            # (the budget does not reach feasibility from the box edge)
    # the overrides reach the launch: Complete only, and another budget / step size
    x = _rows(obs, 1000)
    with _shifted(tr, SHIFT[envname]):
        a0 = tr.act(x, eval_steps=0, form=form)
        _equal(a0, _stepwise(tr, x, eval_steps=0))
        assert int(a0.iters.abs().max()) == 0
        _equal(tr.act(x, eval_steps=7, eval_lr=3.0 * tr.eval_lr, form=form), _stepwise(tr, x, eval_steps=7, eval_lr=3.0 * tr.eval_lr))


@pytest.mark.parametrize("algo,envname", CASES)
def test_act_reproduces_the_recorded_trajectory(hip, algo, envname):
    """Every valid (episode, step) of the record: act(t.obs[e, s]) is t.proposal, t.action, t.iters -- what evaluate() and
    eval() actually stepped -- on both paths."""
    tr, t, obs = _setup(algo, envname)
    v = t.valid
    assert int(t.iters[v].max()) >= 1
    for r in (tr.act(obs), _stepwise(tr, obs)):
        z = r.numpy()
        np.testing.assert_array_equal(z["proposal"], t.proposal[v])
        np.testing.assert_array_equal(z["action"], t.action[v])
        np.testing.assert_array_equal(z["iters"], t.iters[v])
    assert tr.act(obs).path == "fused"


@pytest.mark.parametrize("form", [1, 2, 3])
@pytest.mark.parametrize("algo,envname", [("ddpg", "cart"), ("sac", "pendulum")])
def test_rows_are_independent_on_the_device(hip, algo, envname, form):
    """act(obs)[:16] is act(obs[:16]) -- and act(obs)[i] is act(obs[i:i+1]) -- whatever else the launch carries; SpringPendulum
    with batch_reference on (the default) is the case a batch-coupled projection would break."""
    tr, _, obs = _setup(algo, envname)
    assert tr.batch_reference
    with _shifted(tr, SHIFT[envname]):
        small = tr.act(obs[:16].contiguous(), form=1)
        assert int(small.iters.max()) >= 2
        for n in (4096, 16384):                                # 16- and 64-row workgroups; 16- and 64-row groups
            _equal(tr.act(_rows(obs, n), form=form), small, slice(0, 16))
        one = tr.act(obs[7:8], form=1)
        _equal(small, one, slice(7, 8))
        _equal(_stepwise(tr, obs[:300].contiguous()), one, slice(7, 8))


@pytest.mark.parametrize("algo,envname", [("ddpg", "evopf256"), ("ddpgla", "cart"), ("sacla", "cart")])
def test_stepwise_only_configurations(hip, algo, envname):
    torch.manual_seed(5)
    la = algo.endswith("la")
    tr = build_trainer(algo, envname, hip, DEV, num_envs=16, use_graph=False, fused=not la)    # (EVOPF: the fused 256-wide MLPs)
    tr.vec.reset()
    tr.run_steps(4)
    t = tr.evaluate(16, seed=4, record=True).trajectory
    obs = torch.tensor(t.obs[t.valid], device=DEV)[:200].contiguous()
    r = tr.act(obs)
    assert r.path == "stepwise" and r.form is None
    with pytest.raises(ValueError):
        tr.act(obs, form=1)
    env, k, n = tr.base_env, tr.kernels, obs.shape[0]
    with torch.no_grad():                                      # the hand composition
        if la:
            action = tr._deterministic(obs).clone()
            proposal, iters = action, torch.zeros(n, dtype=torch.int32, device=DEV)
        else:
            proposal = tr._eval_partial(obs).clone()
            action = torch.zeros(n, k.action_dim, device=DEV)
            iters = torch.zeros(n, dtype=torch.int32, device=DEV)
            k.act_project(obs, proposal, None, action, iters, hip.NOISE_NONE, 0.0, 0.0, 0.0, tr._box_lo, tr._box_hi, tr.eval_steps,
                          tr.eval_lr, tr.corr_eps, tr.corr_momentum, **tr._act_kw)
        eq, ineq = env.eq_resid(obs, action), env.ineq_resid(obs, action)
    assert torch.equal(r.action, action) and torch.equal(r.proposal, proposal.reshape(n, -1)) and torch.equal(r.iters, iters)
    assert torch.equal(r.eq_resid, eq) and torch.equal(r.ineq_resid, ineq)
    if la:
        assert int(r.iters.abs().max()) == 0 and torch.equal(r.proposal, r.action)
    else:
        assert int(r.iters.max()) >= 1
        v = t.valid                                            # ... and what evaluate() stepped
        np.testing.assert_array_equal(r.numpy()["action"], t.action[v][:200])


@pytest.mark.parametrize("algo,envname", [("ddpg", "cart"), ("sac", "pendulum")])
def test_schedule_key_residuals_and_out(hip, algo, envname):
    tr, _, obs = _setup(algo, envname)
    x = _rows(obs, 1000)
    with _shifted(tr, SHIFT[envname]):
        full = tr.act(x)
        assert full.path == "fused" and full.form == "tile"
        for r in (tr.act(x, residuals=False), _stepwise(tr, x, residuals=False)):
            assert r.eq_resid is None and r.ineq_resid is None
            _equal(r, full, fields=("action", "proposal", "iters"))
        ptrs = {f: getattr(full, f).data_ptr() for f in FIELDS}
        ref = {f: getattr(full, f).clone() for f in FIELDS}
        for f in FIELDS:
            getattr(full, f).fill_(7)
        again = tr.act(x, out=full)
        assert again is full and {f: getattr(again, f).data_ptr() for f in FIELDS} == ptrs
        for f in FIELDS:
            assert torch.equal(getattr(again, f), ref[f]), f
        with pytest.raises(ValueError):
            tr.act(x[:999], out=full)
    # a NaN observation is no error: both paths agree on its row, the other rows keep their bits, no flag is raised.  The NaN
    # REACHES the row's outputs (include/rpo_hip.h, rpo_mlp_forward: the relu of every forward keeps a NaN pre-activation, so
    # the proposal is NaN; Complete and the residuals are arithmetic on it; the GRG loop leaves after its one unconditional
    # iteration, NaN comparing false with corr_eps) -- every form and every plant: tests/test_nonfinite_gpu.py.
    ref = tr.act(x[:64].contiguous())
    bad = x[:64].clone()
    bad[9, 2] = float("nan")
    fused, step = tr.act(bad), _stepwise(tr, bad)
    keep = [i for i in range(64) if i != 9]
    for f in FIELDS:
        a, b = getattr(fused, f).float(), getattr(step, f).float()
        assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0)), f
        assert torch.equal(getattr(fused, f)[keep], getattr(ref, f)[keep]), f
    if envname == "pendulum":
        assert torch.isnan(fused.action[9, 1]) and torch.isnan(fused.ineq_resid[9]).all()      # (Complete: a_y depends on the row)
    for r in (fused, step):                                     # what the NaN row holds
        assert torch.isnan(r.proposal[9]).all() and torch.isnan(r.action[9]).all() and int(r.iters[9]) == 1
        assert torch.isnan(r.eq_resid[9]).all() and torch.isnan(r.ineq_resid[9]).all()
    assert int(tr.vec.ctrl[hip.CONST["RPO_CTRL_NONFINITE"]]) == 0


def test_training_is_undisturbed(hip, monkeypatch):
    monkeypatch.setenv("RPO_GRAPH_CYCLE", "4")

    def fresh():
        torch.manual_seed(5)
        tr = build_trainer("ddpg", "cart", hip, DEV, num_envs=512, use_graph=True)
        tr.vec.reset()
        return tr
    _, _, obs = _setup("ddpg", "cart")
    a = fresh()
    a.run_steps(8)
    b = fresh()
    b.run_steps(4)
    r = b.act(_rows(obs, 4096))
    assert r.path == "fused" and r.n == 4096
    b.run_steps(4)
    torch.cuda.synchronize()
    for k in ("internal", "ep_len", "ep_ret", "ep_count", "ctrl"):
        assert torch.equal(getattr(a.vec, k), getattr(b.vec, k)), k
    assert torch.equal(a.buffer.rows, b.buffer.rows)
    assert torch.equal(a.agent.flat.data, b.agent.flat.data)
    assert torch.equal(a.agent.critic_target_flat, b.agent.critic_target_flat)


def test_direct_abi_calls(hip):
    from rpo_amd import _lib
    tr, _, obs = _setup("sac", "pendulum")
    lib, k, d = _lib.load(), tr.kernels, tr.fused.descs["actor"]
    ERR_ARG = hip.CONST["RPO_ERR_ARG"]
    n = 1000
    x = _rows(obs, n)
    scale, base = tr._box_affine
    args = (d, True, scale, base, x)
    tail = (tr._box_lo, tr._box_hi, tr.eval_steps, tr.eval_lr, tr.corr_eps, tr.corr_momentum)
    new = lambda *shape, dt=torch.float32: torch.zeros(*shape, dtype=dt, device=DEV)   # noqa: E731
    with _shifted(tr, SHIFT["pendulum"]):
        full = dict(action=new(n, 2), proposal=new(n, 1), iters=new(n, dt=torch.int32), eq_resid=new(n, 1), ineq_resid=new(n, 1))
        k.policy_act(*args, full["action"], full["proposal"], full["iters"], full["eq_resid"], full["ineq_resid"], *tail, form=1)
        assert int(full["iters"].max()) >= 2
        # NULL optional outputs: accepted, the remaining outputs keep their bits (every form)
        for form in (1, 2, 3):
            for drop in (("proposal",), ("iters", "eq_resid"), ("proposal", "iters", "eq_resid", "ineq_resid")):
                out = {f: (None if f in drop else torch.zeros_like(t)) for f, t in full.items()}
                k.policy_act(*args, out["action"], out["proposal"], out["iters"], out["eq_resid"], out["ineq_resid"], *tail, form=form)
                for f, t in out.items():
                    assert t is None or torch.equal(t, full[f]), (form, drop, f)
        # a misaligned action: refused
        net = d.net_struct()
        buf = new(2 * n + 1)
        vp = lambda t: ctypes.c_void_p(t.data_ptr())           # noqa: E731
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        call = lambda action, net, form: lib.rpo_pendulum_policy_act(   # noqa: E731
            ctypes.byref(net), 1, scale, base, n, vp(x), 5, action, None, None, None, None, *tail, form, stream)
        assert call(vp(buf[1:]), net, 1) == ERR_ARG
        assert call(vp(buf), net, 1) == 0
        assert torch.equal(buf[:2 * n].view(n, 2), full["action"])
        # an actor of another embed width: refused in every form (Python takes the stepwise path for such actors)
        net.E = 256
        for form in (0, 1, 2, 3):
            assert call(vp(buf), net, form) == ERR_ARG
        net.E = 128
        assert call(vp(buf), net, 4) == ERR_ARG and call(vp(buf), net, -1) == ERR_ARG
        assert lib.rpo_pendulum_policy_act(ctypes.byref(net), 1, scale, base, 0, vp(x), 5, vp(buf), None, None, None, None, *tail, 1,
                                           stream) == ERR_ARG
        assert lib.rpo_pendulum_policy_act(ctypes.byref(net), 1, scale, base, n, vp(x), 4, vp(buf), None, None, None, None, *tail, 1,
                                           stream) == ERR_ARG
    torch.cuda.synchronize()
