"""trainer.act() on the CPU: the stepwise path driven by the oracle backend.

Inputs: observations a recorded evaluation visited (``evaluate(record=True)`` after a few training steps), so the rows are
states the policy really meets.  Under these settings every such row is feasible after Complete: the GRG loop runs its one
unconditional iteration and stops (``iters == 1`` everywhere; checked on this backend for the four classic-control cases).  So
every test that is about the projection runs a second time with the actor's LAST BIAS shifted (``SHIFT``), which pushes the
proposals towards the box edge, where Complete leaves the inequalities violated and the rows take different numbers of
iterations; those tests assert that on their input.
"""
import functools

import numpy as np
import pytest
import torch

import oracle_backend as ob
from test_train_step_golden import build_trainer

DEV = torch.device("cpu")
CLASSIC = [("ddpg", "cart"), ("sac", "cart"), ("ddpg", "pendulum"), ("sac", "pendulum")]
ALL = CLASSIC + [("ddpg", "evopf"), ("sac", "evopf"), ("ddpgla", "cart"), ("sacla", "cart")]
#: shift of the actor's last bias (pre-tanh): cart proposals land near 8 of 10, pendulum near 3.7 of 6 -- infeasible after Complete
SHIFT = {"cart": 1.2, "pendulum": 0.8}
ROWS = 300


@functools.lru_cache(maxsize=None)
def _setup(algo, envname):
    """(trainer, observations [<= ROWS, obs_dim]) -- shared by the tests of a case and left unchanged by them."""
    torch.set_num_threads(1)
    torch.manual_seed(5)
    evopf, la = envname.startswith("evopf"), algo.endswith("la")
    # (EVOPF-v0: a Newton solve per row and step on this backend, and its 64-wide networks have no fused descriptors)
    kw = dict(num_envs=4, fused=False) if evopf else dict(num_envs=64, fused=not la)
    tr = build_trainer(algo, envname, ob, DEV, use_graph=False, **kw)
    tr.vec.reset()
    tr.run_steps(8)
    t = tr.evaluate(1 if evopf else 40, seed=11, record=True).trajectory
    obs = torch.tensor(t.obs[t.valid])[:16 if evopf else ROWS].contiguous()
    assert obs.shape[0] >= (16 if evopf else ROWS)
    return tr, obs


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


def _by_hand(tr, obs, eval_steps=None, eval_lr=None):
    """proposal + process_action(train=False) with the batch-coupled projection off + eq_resid / ineq_resid."""
    env = tr.base_env
    with torch.no_grad():
        if hasattr(tr, "_deterministic"):                        # the Lagrangian baselines: no projection
            action = tr._deterministic(obs).clone()
            proposal, iters = action, torch.zeros(obs.shape[0], dtype=torch.int32)
        else:
            proposal = tr._eval_partial(obs).clone()
            keep = tr.batch_reference, tr.eval_steps, tr.eval_lr
            tr.batch_reference = False
            tr.eval_steps = keep[1] if eval_steps is None else eval_steps
            tr.eval_lr = keep[2] if eval_lr is None else eval_lr
            try:
                action, most = tr.process_action(obs, proposal, train=False)
                _, iters = env.project(obs, proposal, tr.eval_steps, tr.eval_lr, tr.corr_eps, tr.corr_momentum, return_iters=True,
                                       batch_reference=False)
            finally:
                tr.batch_reference, tr.eval_steps, tr.eval_lr = keep
            assert most == int(iters.max())
        return dict(action=action, proposal=proposal.reshape(obs.shape[0], -1), iters=iters,
                    eq_resid=env.eq_resid(obs, action), ineq_resid=env.ineq_resid(obs, action))


def _same(r, ref):
    for f in r.FIELDS:
        assert torch.equal(getattr(r, f), ref[f] if isinstance(ref, dict) else getattr(ref, f)), f


@pytest.mark.parametrize("algo,envname", ALL)
def test_act_is_the_hand_composition(algo, envname):
    tr, obs = _setup(algo, envname)
    r = tr.act(obs)
    assert r.path == "stepwise" and r.form is None and r.n == obs.shape[0]
    assert r.action.dtype == torch.float32 and r.iters.dtype == torch.int32
    k = tr.kernels
    assert tuple(r.action.shape) == (r.n, k.action_dim) and tuple(r.eq_resid.shape) == (r.n, k.eq_num)
    assert tuple(r.ineq_resid.shape) == (r.n, k.ineq_num) and tuple(r.proposal.shape) == (r.n, tr._eval_proposal_dim())
    _same(r, _by_hand(tr, obs))
    if algo.endswith("la"):
        assert int(r.iters.abs().max()) == 0 and torch.equal(r.proposal, r.action)
    else:
        assert int(r.iters.max()) >= 1
    assert torch.equal(r.max_ineq(), r.ineq_resid.max(dim=1).values) and torch.equal(r.max_eq(), r.eq_resid.abs().max(dim=1).values)
    z = r.numpy()
    assert sorted(z) == sorted(r.FIELDS) and np.array_equal(z["action"], r.action.numpy()) and z["iters"].dtype == np.int32
    one = tr.act(obs[3])                                         # [obs_dim]: n = 1
    assert one.n == 1 and tuple(one.action.shape) == (1, k.action_dim)
    assert tr.act(obs.numpy()).n == r.n                          # anything torch.as_tensor accepts


@pytest.mark.parametrize("algo,envname", CLASSIC)
def test_projected_rows_are_the_hand_composition(algo, envname):
    """The same with the proposals pushed towards the box edge: the rows take different numbers of GRG iterations."""
    tr, obs = _setup(algo, envname)
    with _shifted(tr, SHIFT[envname]):
        r = tr.act(obs)
        assert int(r.iters.max()) >= 2 and float(r.max_ineq().max()) > 0
        _same(r, _by_hand(tr, obs))
        # overrides: Complete only; and a budget / step size of the caller's choosing
        r0 = tr.act(obs, eval_steps=0)
        assert int(r0.iters.abs().max()) == 0 and torch.equal(r0.proposal, r.proposal)
        assert torch.equal(r0.action, tr.base_env.complete_partial(obs, r0.proposal))
        _same(tr.act(obs, eval_steps=7, eval_lr=3.0 * tr.eval_lr), _by_hand(tr, obs, 7, 3.0 * tr.eval_lr))
        assert not torch.equal(tr.act(obs, eval_steps=7).action, r.action)
        _same(tr.act(obs), r)                                    # ... for that call only


@pytest.mark.parametrize("algo,envname", [("ddpg", "cart"), ("sac", "pendulum")])
def test_override_equals_a_trainer_built_with_it(algo, envname):
    tr, obs = _setup(algo, envname)
    torch.manual_seed(5)
    other = build_trainer(algo, envname, ob, DEV, use_graph=False, num_envs=64, eval_steps=7, eval_lr=3.0 * tr.eval_lr)
    assert other.eval_steps == 7 and other.eval_lr == 3.0 * tr.eval_lr
    with _shifted(tr, SHIFT[envname]):
        other.agent.actor.load_state_dict(tr.agent.actor.state_dict())
        a, b = tr.act(obs, eval_steps=7, eval_lr=3.0 * tr.eval_lr), other.act(obs)
    assert int(a.iters.max()) >= 2
    _same(a, b)


@pytest.mark.parametrize("algo,envname", [("ddpg", "pendulum"), ("sac", "pendulum"), ("ddpg", "cart")])
def test_rows_are_independent(algo, envname):
    """act(obs)[i] is act(obs[i:i+1]), and a permutation of the rows permutes the result -- with batch_reference ON in the
    trainer (the default), under which SpringPendulum's training batches are projected with a batch-global stop test and the
    sample-coupled step: n = 300 rows of mixed feasibility would all report the batch's iteration count.
    Tolerance: this backend's torch-CPU matmuls round with the batch shape (see test_evaluate.test_seeds_and_horizon), so a
    proposal may move by a few float32 ulps of the box (|ap| <= 10: < 1e-5) between a 1-row and a 300-row call; the GRG step is
    lr * (a gradient of size O(|a|)), so the projected action follows within 1e-4 and a row's stop test may fall one
    iteration earlier or later.  The GPU suite checks the bits."""
    tr, obs = _setup(algo, envname)
    assert tr.batch_reference and obs.shape[0] == ROWS
    with _shifted(tr, SHIFT[envname]):
        r = tr.act(obs)
        assert int(r.iters.max()) >= 2 and len(torch.unique(r.iters)) >= 2     # mixed: a batch-global stop would give ONE value
        for i in range(0, ROWS, 7):
            one = tr.act(obs[i:i + 1])
            assert abs(int(one.iters[0]) - int(r.iters[i])) <= 1, i
            for f in ("action", "proposal", "eq_resid", "ineq_resid"):
                np.testing.assert_allclose(getattr(one, f)[0].numpy(), getattr(r, f)[i].numpy(), rtol=1e-5, atol=1e-4, err_msg=f)
        perm = torch.randperm(ROWS, generator=torch.Generator().manual_seed(3))
        p = tr.act(obs[perm])
        assert int((p.iters - r.iters[perm]).abs().max()) <= 1
        for f in ("action", "proposal", "eq_resid", "ineq_resid"):
            np.testing.assert_allclose(getattr(p, f).numpy(), getattr(r, f)[perm].numpy(), rtol=1e-5, atol=1e-4, err_msg=f)


def test_out_reuses_the_storage():
    tr, obs = _setup("sac", "pendulum")
    a = tr.act(obs)
    ref = {f: getattr(a, f).clone() for f in a.FIELDS}
    ptrs = {f: getattr(a, f).data_ptr() for f in a.FIELDS}
    with _shifted(tr, SHIFT["pendulum"]):
        b = tr.act(obs, out=a)
        assert b is a and {f: getattr(b, f).data_ptr() for f in b.FIELDS} == ptrs
        assert not torch.equal(b.action, ref["action"])
    _same(tr.act(obs, out=a), ref)
    c = tr.act(obs, residuals=False)
    assert c.eq_resid is None and c.ineq_resid is None and not c.residuals
    assert torch.equal(c.action, ref["action"]) and torch.equal(c.iters, ref["iters"]) and torch.equal(c.proposal, ref["proposal"])
    assert tr.act(obs, residuals=False, out=c) is c


def test_validation():
    tr, obs = _setup("ddpg", "cart")
    good = tr.act(obs)
    bad = [dict(obs=obs[:, :5]), dict(obs=obs[:0]), dict(obs=torch.zeros(2, 3, 6)), dict(obs=torch.zeros(7)),
           dict(eval_lr=float("nan")), dict(eval_lr=float("inf")), dict(eval_lr="fast"),
           dict(eval_steps=-1), dict(eval_steps=2.5), dict(eval_steps=True), dict(eval_steps="3"),
           dict(out=tr.act(obs[:5])), dict(out=tr.act(obs, residuals=False)), dict(out=good, residuals=False), dict(out=object()),
           dict(form=1), dict(form=7)]                           # (form: this trainer acts on the stepwise path)
    for kw in bad:
        with pytest.raises(ValueError):
            tr.act(**dict(dict(obs=obs), **kw))
    assert tr.act(obs, eval_steps=np.int64(3), eval_lr=np.float32(0.01)).n == good.n


@pytest.mark.parametrize("algo,envname", [("ddpg", "cart"), ("sac", "pendulum")])
def test_a_nan_row_stays_in_its_row(algo, envname):
    tr, obs = _setup(algo, envname)
    ref = tr.act(obs[:32])
    x = obs[:32].clone()
    x[5, 1] = float("nan")
    with np.errstate(all="ignore"):
        r = tr.act(x)
    assert torch.isnan(r.action[5]).all() and torch.isnan(r.proposal[5]).all()
    rest = [i for i in range(32) if i != 5]
    for f in r.FIELDS:
        assert torch.equal(getattr(r, f)[rest], getattr(ref, f)[rest]), f
    assert int(tr.vec.ctrl[ob.CONST["RPO_CTRL_NONFINITE"]]) == 0   # no control word is involved


@pytest.mark.parametrize("algo,envname", [("ddpg", "cart"), ("sac", "pendulum")])
def test_act_leaves_the_trainer_untouched(algo, envname):
    tr, obs = _setup(algo, envname)

    def snap():
        v = tr.vec
        out = {n: getattr(v, n).clone() for n in ("internal", "obs", "action", "ep_len", "ep_ret", "ep_count", "ctrl", "stats")}
        out.update(flat=tr.agent.flat.data.clone(), target=tr.agent.critic_target_flat.clone(), rows=tr.buffer.rows.clone(),
                   rng=torch.get_rng_state(), nprng=np.random.get_state()[1].copy())
        return out
    before, t, calls = snap(), tr._t, getattr(tr, "_evaluate_calls", 0)
    tr.act(obs)
    tr.act(obs[:1], eval_steps=3, residuals=False)
    after = snap()
    for name, x in before.items():
        assert torch.equal(torch.as_tensor(x), torch.as_tensor(after[name])), name
    assert tr._t == t and getattr(tr, "_evaluate_calls", 0) == calls
