"""trainer.evaluate_budgets() on the MI355X: the fused path (the BUD instances of the evaluation kernel, B x episodes lanes of
one launch sequence with the projection's budget and step size read per lane) against its definition -- group g is, bit for
bit, ``evaluate(eval_steps=eval_steps[g], eval_lr=eval_lr[g])`` with the shared seed -- the "sweep" path, the entry points'
refusals, and that training after a sweep is the training without it.

Trainers are tests/test_act_gpu.py's (cart-RPODDPG, pendulum-RPOSAC after 8 training steps); the actor's last bias is shifted
(``SHIFT``) so that the projection iterates and the budget matters.  Every bit-for-bit test first asserts that the groups'
iteration counts differ and that a step was violated (``assert_budgets_matter``): with budgets ignored the groups would be equal
and the comparison vacuous.  No tolerances: every comparison is on bits."""
import ctypes

import numpy as np
import pytest
import torch

from test_act_gpu import SHIFT, _setup, _shifted
from test_evaluate_budgets import assert_budgets_matter, assert_group_is, assert_sweep_is_the_definition, lr_list
from test_train_step_golden import build_trainer

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
FUSED = [("ddpg", "cart"), ("sac", "pendulum")]
N = 40                                                         # 16-lane tiles straddle the groups: 2.5 tiles per budget
SEED = 21


@pytest.fixture(scope="module")
def hip():
    from rpo_amd import ops
    assert torch.cuda.is_available()
    return ops


def _init_states(tr, n, seed=5):
    """Internal states of another reset stream than the evaluation's."""
    v = tr.base_env.make_vec(n, seed=seed, env_id_base=0, max_episode_steps=tr.max_episode_steps, device=DEV, stats_cap=2)
    v.reset()
    return v.internal.clone()


def _budgets(tr):
    return [0, 1, 3, tr.eval_steps], lr_list(tr, 4)


class _schedule(object):
    """A schedule key set inside the block."""

    def __init__(self, tr, key, value):
        self.s, self.key, self.value = tr.schedule, key, value

    def __enter__(self):
        self.had, self.was = self.key in self.s, self.s.get(self.key)
        self.s[self.key] = self.value

    def __exit__(self, *exc):
        if self.had:
            self.s[self.key] = self.was
        else:
            del self.s[self.key]
        return False


# ------------------------------------------------------------------------------------------------ 1, 2. the definition
@pytest.mark.parametrize("constraints", [False, True])
@pytest.mark.parametrize("inject", [False, True])
@pytest.mark.parametrize("algo,envname", FUSED)
def test_fused_equals_the_definition_bit_for_bit(algo, envname, inject, constraints):
    tr, _, _ = _setup(algo, envname)
    steps, lrs = _budgets(tr)
    kw = dict(episodes=N, seed=SEED, init_states=_init_states(tr, N) if inject else None, constraints=constraints)
    with _shifted(tr, SHIFT[envname]):
        s = tr.evaluate_budgets(eval_steps=steps, eval_lr=lrs, **kw)
        assert s.path == "fused" and s.horizon == 200 and s.seed == SEED and s.episodes == N
        assert all(r.path == "fused" for r in s.results)
        assert_budgets_matter(s)
        assert_sweep_is_the_definition(tr, s, steps, lrs, **kw)
    assert int(s.iters[0].max()) == 0 and s.length.min() >= 1 and not s.nonfinite.any()
    if constraints:
        c = s[3].constraints
        assert c.ineq_max.shape == (N, tr.kernels.ineq_num) and c.names == s[0].constraints.names
        np.testing.assert_array_equal(c.ineq_max.max(1), s.max_ineq[3])


# ------------------------------------------------------------------------------------------------ 3. the 64-lane instance
@pytest.mark.parametrize("algo,envname", FUSED)
def test_the_64_lane_instance(algo, envname):
    """4 x 3100 = 12 400 lanes >= 64 x 192: the 64-lane tiles, the last one ragged (48 of 64 lanes), groups changing inside tiles
    (3100 = 48 x 64 + 28); the definition's 3100-lane calls run the 16-lane instance."""
    tr, _, _ = _setup(algo, envname)
    steps, lrs = _budgets(tr)
    kw = dict(episodes=3100, seed=SEED, horizon=6, constraints=True)
    with _shifted(tr, SHIFT[envname]):
        s = tr.evaluate_budgets(eval_steps=steps, eval_lr=lrs, **kw)
        assert s.path == "fused" and s.horizon == 6
        assert_budgets_matter(s)
        assert_sweep_is_the_definition(tr, s, steps, lrs, **kw)


# ------------------------------------------------------------------------------------------------ 4. launch splits
@pytest.mark.parametrize("algo,envname", FUSED)
def test_launch_splits_are_invisible(hip, algo, envname, monkeypatch):
    tr, _, _ = _setup(algo, envname)
    steps, lrs = _budgets(tr)
    kw = dict(episodes=N, seed=SEED, eval_steps=steps, eval_lr=lrs, constraints=True)
    with _shifted(tr, SHIFT[envname]):
        one = tr.evaluate_budgets(**kw)
        launches = []
        inner = tr.kernels.evaluate_budgets
        monkeypatch.setattr(tr.kernels, "evaluate_budgets", lambda *a, **k: (launches.append((a[12], a[13])), inner(*a, **k))[1])
        monkeypatch.setattr(hip, "EVAL_LANE_STEPS", 4 * N * 3)  # n = B x episodes lanes: 3 steps per launch
        split = tr.evaluate_budgets(**kw)
    assert launches[:3] == [(0, 3), (3, 3), (6, 3)] and len(launches) == 67 and launches[-1] == (198, 2)
    assert one.path == split.path == "fused"
    assert_budgets_matter(one)
    for g in range(4):
        assert_group_is(split[g], one[g])
    assert one.length.max() > 3                                 # (episodes did run on into later launches)


# ------------------------------------------------------------------------------------------------ 5. B = 1, duplicates
@pytest.mark.parametrize("algo,envname", FUSED)
def test_one_budget_is_evaluate_and_duplicates_are_equal(algo, envname):
    tr, _, _ = _setup(algo, envname)
    kw = dict(episodes=N, seed=SEED, constraints=True)
    with _shifted(tr, SHIFT[envname]):
        s = tr.evaluate_budgets(eval_steps=[tr.eval_steps], **kw)
        assert s.path == "fused" and len(s) == 1
        assert_group_is(s[0], tr.evaluate(**kw))                # no override at all: the trainer's budget
        d = tr.evaluate_budgets(eval_steps=[2, 0, 2, 0], eval_lr=[tr.eval_lr, 1.0, tr.eval_lr, 2.0], **kw)
        assert_budgets_matter(d)
        assert_group_is(d[0], d[2])
        assert_group_is(d[1], d[3])                             # (eval_steps = 0: the step size is never used)
        assert_group_is(d[0], tr.evaluate(eval_steps=2, **kw))


# ------------------------------------------------------------------------------------------------ 6. the stand-alone path
@pytest.mark.parametrize("algo,envname", FUSED)
def test_sweep_path_has_the_fused_bits(algo, envname):
    tr, _, _ = _setup(algo, envname)
    steps, lrs = _budgets(tr)
    kw = dict(episodes=N, seed=SEED, eval_steps=steps, eval_lr=lrs, constraints=True)
    with _shifted(tr, SHIFT[envname]):
        fused = tr.evaluate_budgets(**kw)
        with _schedule(tr, "fused_budgets", 0):
            sweep = tr.evaluate_budgets(**kw)
    assert fused.path == "fused" and sweep.path == "sweep"
    assert_budgets_matter(fused)
    for g in range(4):
        assert_group_is(sweep[g], fused[g])


def test_evopf_sweeps_and_a_baseline_is_refused(hip):
    torch.manual_seed(5)
    tr = build_trainer("ddpg", "evopf256", hip, DEV, num_envs=16, use_graph=False)
    kw = dict(episodes=2, seed=SEED, horizon=2, constraints=True)
    steps, lrs = [0, 3], [tr.eval_lr, 2.0 * tr.eval_lr]
    s = tr.evaluate_budgets(eval_steps=steps, eval_lr=lrs, **kw)
    assert s.path == "sweep" and s[0].path == "stepwise"
    assert_sweep_is_the_definition(tr, s, steps, lrs, **kw)
    assert int(s.iters[0].max()) == 0 and int(s.iters[1].max()) > 0
    la = build_trainer("ddpgla", "cart", hip, DEV, num_envs=16, use_graph=False, fused=False)
    with pytest.raises(ValueError, match="projection"):
        la.evaluate_budgets(2, eval_steps=[0, 1])


# ------------------------------------------------------------------------------------------------ 7. the C ABI
@pytest.mark.parametrize("algo,envname", FUSED)
def test_entry_points_refuse_before_any_launch(hip, algo, envname):
    from rpo_amd import _lib
    lib = _lib.load()
    ERR_ARG, ERR_NULL = _lib.CONST["RPO_ERR_ARG"], _lib.CONST["RPO_ERR_NULL"]
    assert _lib.CONST["RPO_ABI_VERSION"] == 6 and lib.rpo_abi_version() == 6
    tr, _, _ = _setup(algo, envname)
    n, k = 32, tr.kernels
    v = tr.base_env.make_vec(n, seed=1, max_episode_steps=tr.max_episode_steps, device=DEV, stats_cap=2)
    v.reset()
    acc = torch.zeros(n, 8, device=DEV)
    con = torch.zeros(n, hip.con_width(k.ineq_num, k.eq_num), device=DEV)
    lane_steps = torch.full((n,), 2, dtype=torch.int32, device=DEV)
    lane_lr = torch.full((n,), tr.eval_lr, device=DEV)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())               # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    scale, base = tr._box_affine
    net = tr.fused.descs["actor"].net_struct()
    state = (vp(v.internal),) if envname == "cart" else (vp(v.internal), vp(v.obs))
    consts = (ctypes.c_void_p(k.consts.ctypes.data), k.partial) if envname == "cart" else ()
    fn = lib.rpo_cartsafe_evaluate_budgets if envname == "cart" else lib.rpo_pendulum_evaluate_budgets

    def call(net, steps, lr, con=None, trace=None):
        return fn(ctypes.byref(net), int(tr._gauss_policy), scale, base, n, *state, vp(v.action), vp(v.ep_len), vp(v.ep_ret),
                  vp(v.ep_count), vp(v.ctrl), vp(acc), 0, 2, tr._box_lo, tr._box_hi, 0, 0.0, tr.corr_eps, tr.corr_momentum,
                  *consts, v.max_episode_steps, v.viol_thresh, trace, 0, 0, con, steps, lr, stream)
    before = v.internal.clone()
    assert call(net, None, vp(lane_lr)) == ERR_NULL
    assert call(net, vp(lane_steps), None) == ERR_NULL
    assert call(net, None, None, con=vp(con)) == ERR_NULL
    net.E = 256
    assert call(net, vp(lane_steps), vp(lane_lr)) == ERR_ARG
    net.E = 128
    assert call(net, vp(lane_steps), vp(lane_lr), trace=vp(con)) == ERR_ARG   # no record with per-lane budgets
    torch.cuda.synchronize()
    assert torch.equal(v.internal, before) and not acc.any()    # nothing was launched
    assert call(net, vp(lane_steps), vp(lane_lr)) == 0 and call(net, vp(lane_steps), vp(lane_lr), con=vp(con)) == 0
    torch.cuda.synchronize()
    assert acc.any()
    with pytest.raises(hip.RpoHipError):                        # the binding checks the lengths the kernel indexes by lane
        k.evaluate_budgets(tr.fused.descs["actor"], tr._gauss_policy, scale, base, v.internal, None if v.obs is v.internal else v.obs,
                           v.action, v.ep_len, v.ep_ret, v.ep_count, v.ctrl, acc, 0, 2, tr._box_lo, tr._box_hi, lane_steps[:n - 1],
                           lane_lr, tr.corr_eps, tr.corr_momentum, v.max_episode_steps, v.viol_thresh)


# ------------------------------------------------------------------------------------------------ 8. nothing else moves
def test_a_sweep_has_no_side_effects_on_the_device(hip, monkeypatch):
    monkeypatch.setenv("RPO_GRAPH_CYCLE", "4")

    def fresh():
        torch.manual_seed(5)
        tr = build_trainer("ddpg", "cart", hip, DEV, num_envs=512, use_graph=True)
        tr.vec.reset()
        return tr
    a = fresh()
    a.run_steps(24)
    b = fresh()
    b.run_steps(8)
    torch.cuda.synchronize()
    snap = {k: getattr(b.vec, k).clone() for k in ("internal", "ep_len", "ep_ret", "ep_count", "ctrl", "stats")}
    rows, flat = b.buffer.rows.clone(), b.agent.flat.data.clone()
    keep = b.eval_steps, b.eval_lr
    s = b.evaluate_budgets(100, eval_steps=[0, 2, 5], eval_lr=[b.eval_lr, 2.0 * b.eval_lr, b.eval_lr], constraints=True)
    assert s.path == "fused"
    with _schedule(b, "fused_budgets", 0):
        assert b.evaluate_budgets(20, eval_steps=[0, 2], horizon=20).path == "sweep"
    torch.cuda.synchronize()
    assert (b.eval_steps, b.eval_lr) == keep
    for k, x in snap.items():
        assert torch.equal(getattr(b.vec, k), x), k
    assert torch.equal(b.buffer.rows, rows) and torch.equal(b.agent.flat.data, flat)
    b.run_steps(16)
    torch.cuda.synchronize()
    for k in ("internal", "ep_len", "ep_ret", "ep_count", "ctrl"):
        assert torch.equal(getattr(a.vec, k), getattr(b.vec, k)), k
    assert torch.equal(a.buffer.rows, b.buffer.rows)
    assert torch.equal(a.agent.flat.data, b.agent.flat.data)
    assert torch.equal(a.agent.critic_target_flat, b.agent.critic_target_flat)
