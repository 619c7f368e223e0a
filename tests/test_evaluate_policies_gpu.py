"""trainer.evaluate_policies() on the MI355X: the fused path (the POL instances of the evaluation kernel: P groups of padded
lanes in one launch sequence, every workgroup on its group's actor out of a bank) against its definition -- group g is, bit for
bit, ``evaluate()`` under ``using_policy(policies[g])`` with the shared seed -- the padding lanes, the entry points' refusals,
the "sweep" path, and that nothing of the trainer is touched.

Trainers are tests/test_act_gpu.py's (cart-RPODDPG, pendulum-RPOSAC after 8 training steps).  The candidates are the live actor,
the live actor with its last bias shifted (``SHIFT``: the projection iterates and steps are violated) and the span of a second
trainer built with another seed.  Every bit-for-bit test first asserts that the policies matter
(``assert_policies_matter``): a kernel that ignored its group would give equal groups and a vacuous comparison.  No tolerances:
every comparison is on bits."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from test_act_gpu import SHIFT, _setup
from test_evaluate_budgets import assert_group_is
from test_evaluate_budgets_gpu import _init_states, _schedule
from test_evaluate_policies import assert_policies_matter, assert_sweep_is_the_definition, shifted_span
from test_train_step_golden import build_trainer

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
FUSED = [("ddpg", "cart"), ("sac", "pendulum")]
N = 40                             # groups of 64 lanes: the third 16-lane tile of a group is half padding, the fourth all padding
SEED = 21
SENTINEL = 0x7FC0DEAD              # a NaN with a payload: no kernel computes it


@pytest.fixture(scope="module")
def hip():
    from rpo_amd import ops
    assert torch.cuda.is_available()
    return ops


@functools.lru_cache(maxsize=None)
def _candidates(algo, envname):
    """(trainer, [the live actor, its last bias shifted, the span of a trainer with another seed]); nothing is left changed."""
    from rpo_amd import ops
    tr, _, _ = _setup(algo, envname)
    torch.manual_seed(6)
    other = build_trainer(algo, envname, ops, DEV, num_envs=64, use_graph=False, seed=12)
    other.vec.reset()
    other.run_steps(8)
    return tr, [None, shifted_span(tr, SHIFT[envname]), other.policy_params()]


def _bits(t):
    return t.detach().contiguous().view(torch.int32) if t.dtype != torch.int64 else t.detach().contiguous()


# ------------------------------------------------------------------------------------------------ 1. the definition
@pytest.mark.parametrize("constraints", [False, True])
@pytest.mark.parametrize("inject", [False, True])
@pytest.mark.parametrize("algo,envname", FUSED)
def test_fused_equals_the_definition_bit_for_bit(algo, envname, inject, constraints):
    tr, policies = _candidates(algo, envname)
    kw = dict(episodes=N, seed=SEED, init_states=_init_states(tr, N) if inject else None, constraints=constraints)
    s = tr.evaluate_policies(policies, **kw)
    assert s.path == "fused" and s.horizon == 200 and s.seed == SEED and s.episodes == N and len(s) == 3
    assert all(r.path == "fused" for r in s.results) and s.names == ("live", "policy[1]", "policy[2]")
    assert_policies_matter(s)
    assert_sweep_is_the_definition(tr, s, policies, **kw)
    assert_group_is(s[0], tr.evaluate(**kw))                    # None: a plain evaluate() with the shared seed
    assert s.length.min() >= 1 and not s.nonfinite.any()
    if constraints:
        c = s[1].constraints
        assert c.ineq_max.shape == (N, tr.kernels.ineq_num) and c.names == s[0].constraints.names
        np.testing.assert_array_equal(c.ineq_max.max(1), s.max_ineq[1])


# ------------------------------------------------------------------------------------------------ 2. the 64-lane instance
@pytest.mark.parametrize("algo,envname", FUSED)
def test_the_64_lane_instance(algo, envname):
    """4 x 3100 episodes in groups of 3136 lanes = 12 544 lanes >= 64 x 192: the 64-lane tiles, the last one of every group
    ragged (28 of 64 lanes live); the definition's 3100-lane calls run the 16-lane instance."""
    tr, policies = _candidates(algo, envname)
    policies = policies + [policies[1]]
    kw = dict(episodes=3100, seed=SEED, horizon=6, constraints=True)
    s = tr.evaluate_policies(policies, **kw)
    assert s.path == "fused" and s.horizon == 6 and len(s) == 4
    assert_policies_matter(s)
    assert_sweep_is_the_definition(tr, s, policies, **kw)       # (group 3 too: the fourth group's ragged tile ends the grid)
    assert_group_is(s[3], s[1])


# ------------------------------------------------------------------------------------------------ 3. launch splits
@pytest.mark.parametrize("algo,envname", FUSED)
def test_launch_splits_are_invisible(hip, algo, envname, monkeypatch):
    tr, policies = _candidates(algo, envname)
    kw = dict(episodes=N, seed=SEED, constraints=True)
    one = tr.evaluate_policies(policies, **kw)
    launches = []
    inner = tr.kernels.evaluate_policies
    monkeypatch.setattr(tr.kernels, "evaluate_policies", lambda *a, **k: (launches.append((a[12], a[13])), inner(*a, **k))[1])
    monkeypatch.setattr(hip, "EVAL_LANE_STEPS", 3 * 64 * 3)     # n = P x padded lanes = 3 x 64: 3 steps per launch
    split = tr.evaluate_policies(policies, **kw)
    assert launches[:3] == [(0, 3), (3, 3), (6, 3)] and len(launches) == 67 and launches[-1] == (198, 2)
    assert one.path == split.path == "fused"
    assert_policies_matter(one)
    for g in range(3):
        assert_group_is(split[g], one[g])
    assert one.length.max() > 3                                 # (episodes did run on into later launches)


# ------------------------------------------------------------------------------------------------ 4. padding lanes
@pytest.mark.parametrize("constraints", [False, True])
@pytest.mark.parametrize("algo,envname", FUSED)
def test_padding_is_never_written(hip, algo, envname, constraints):
    """The wrapper itself on 2 x 64 lanes with 40 episodes per group: accumulators, report, actions and the padding lanes' env
    rows hold a sentinel before; afterwards the 24 padding rows of every group still do and no live row does."""
    from rpo_amd.algo.evaluation import policy_bank
    tr, policies = _candidates(algo, envname)
    k, P, GL = tr.kernels, 2, 64
    live = (torch.arange(P * GL, device=DEV) % GL) < N
    v = tr.base_env.make_vec(P * GL, seed=SEED, max_episode_steps=tr.max_episode_steps, device=DEV, stats_cap=2)
    v.reset()
    acc = torch.zeros(P * GL, 8, device=DEV)
    con = torch.zeros(P * GL, hip.con_width(k.ineq_num, k.eq_num), device=DEV) if constraints else None
    everywhere = [acc, v.action] + ([con] if constraints else [])
    padding_only = [v.internal, v.ep_len, v.ep_ret, v.ep_count] + ([] if v.obs is v.internal else [v.obs])
    for t in everywhere:
        _bits(t).fill_(SENTINEL)
    for t in padding_only:
        _bits(t)[~live] = SENTINEL
    before = [t.clone() for t in padding_only]
    bank, desc = policy_bank(tr, policies[:2])
    scale, base = tr._box_affine
    k.evaluate_policies(desc, tr._gauss_policy, scale, base, v.internal, None if v.obs is v.internal else v.obs, v.action,
                        v.ep_len, v.ep_ret, v.ep_count, v.ctrl, acc, 0, 6, tr._box_lo, tr._box_hi, tr.eval_steps, tr.eval_lr,
                        tr.corr_eps, tr.corr_momentum, v.max_episode_steps, v.viol_thresh, bank, GL, N, con=con)
    torch.cuda.synchronize()
    for t in everywhere:
        rows = _bits(t).reshape(P * GL, -1)
        assert bool((rows[~live] == SENTINEL).all()), "a padding row was written"
        assert bool((rows[live] != SENTINEL).any(dim=1).all()), "a live row was not written"
    for t, was in zip(padding_only, before):
        assert torch.equal(_bits(t)[~live], _bits(was)[~live]), "a padding lane's env row was written"
        assert bool((_bits(t).reshape(P * GL, -1)[live] != SENTINEL).any(dim=1).all())
    assert not torch.equal(v.internal[live], before[0][live])   # (the live lanes were stepped)
    word = acc[:, 7].contiguous().view(torch.int32)[live]
    assert int((word >> 2).min()) >= 1 and int((word >> 2).max()) == 6


# ------------------------------------------------------------------------------------------------ 5. the C ABI
@pytest.mark.parametrize("algo,envname", FUSED)
def test_entry_points_refuse_before_any_launch(hip, algo, envname):
    from rpo_amd import _lib
    from rpo_amd.algo.evaluation import policy_bank
    lib = _lib.load()
    ERR_ARG, ERR_NULL = _lib.CONST["RPO_ERR_ARG"], _lib.CONST["RPO_ERR_NULL"]
    assert _lib.CONST["RPO_ABI_VERSION"] == 6 and lib.rpo_abi_version() == 6
    tr, policies = _candidates(algo, envname)
    k, P, GL = tr.kernels, 2, 64
    n = P * GL
    v = tr.base_env.make_vec(n, seed=1, max_episode_steps=tr.max_episode_steps, device=DEV, stats_cap=2)
    v.reset()
    acc = torch.zeros(n, 8, device=DEV)
    _bits(acc).fill_(SENTINEL)
    con = torch.zeros(n, hip.con_width(k.ineq_num, k.eq_num), device=DEV)
    bank, desc = policy_bank(tr, policies[:2])
    stride = bank.shape[1]
    assert stride % 4 == 0 and bank.data_ptr() % 16 == 0
    vp = lambda t: ctypes.c_void_p(t.data_ptr())               # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    scale, base = tr._box_affine
    net = desc.net_struct()
    state = (vp(v.internal),) if envname == "cart" else (vp(v.internal), vp(v.obs))
    consts = (ctypes.c_void_p(k.consts.ctypes.data), k.partial) if envname == "cart" else ()
    fn = lib.rpo_cartsafe_evaluate_policies if envname == "cart" else lib.rpo_pendulum_evaluate_policies

    def call(actor, stride, group_lanes, episodes, n_envs=n, con=None):
        return fn(actor, int(tr._gauss_policy), scale, base, n_envs, *state, vp(v.action), vp(v.ep_len), vp(v.ep_ret),
                  vp(v.ep_count), vp(v.ctrl), vp(acc), 0, 2, tr._box_lo, tr._box_hi, tr.eval_steps, tr.eval_lr, tr.corr_eps,
                  tr.corr_momentum, *consts, v.max_episode_steps, v.viol_thresh, con, stride, group_lanes, episodes, stream)
    before = v.internal.clone()
    ok = ctypes.byref(net)
    assert call(None, stride, GL, N) == ERR_NULL                # no bank
    assert call(None, stride, GL, N, con=vp(con)) == ERR_NULL
    for bad_stride in (stride + 2, stride + 1, 0, -4):          # not a multiple of 4 floats, not positive
        assert call(ok, bad_stride, GL, N) == ERR_ARG
    for bad_lanes in (32, 96, 0, -64):                          # not a multiple of 64, not positive
        assert call(ok, stride, bad_lanes, min(N, max(bad_lanes, 1))) == ERR_ARG
    assert call(ok, stride, GL, GL + 1) == ERR_ARG              # more episodes than lanes in a group
    assert call(ok, stride, GL, 0) == ERR_ARG and call(ok, stride, GL, -1) == ERR_ARG
    assert call(ok, stride, GL, N, n_envs=n - 32) == ERR_ARG    # n is not P x group_lanes
    assert call(ok, stride, 2 * n, N) == ERR_ARG                # (not even one whole group)
    net.E = 256
    assert call(ok, stride, GL, N) == ERR_ARG
    net.E = 128
    torch.cuda.synchronize()
    assert torch.equal(v.internal, before) and bool((_bits(acc) == SENTINEL).all())    # nothing was launched
    assert call(ok, stride, GL, N) == 0 and call(ok, stride, GL, GL, con=vp(con)) == 0
    torch.cuda.synchronize()
    assert not bool((_bits(acc) == SENTINEL).any())             # (episodes = group_lanes: no padding at all)
    args = (desc, tr._gauss_policy, scale, base, v.internal, None if v.obs is v.internal else v.obs, v.action, v.ep_len, v.ep_ret,
            v.ep_count, v.ctrl, acc, 0, 2, tr._box_lo, tr._box_hi, tr.eval_steps, tr.eval_lr, tr.corr_eps, tr.corr_momentum,
            v.max_episode_steps, v.viol_thresh)
    with pytest.raises(hip.RpoHipError):                        # the binding checks what the kernel indexes by group:
        k.evaluate_policies(*args, bank[:1], GL, N)             # fewer policies in the bank than groups of lanes
    with pytest.raises(hip.RpoHipError):
        k.evaluate_policies(*args, bank, 32, 32)                # lanes that are not P x group_lanes
    with pytest.raises(hip.RpoHipError):
        k.evaluate_policies(tr.fused.descs["actor"], *args[1:], bank, GL, N)   # a descriptor outside the bank


# ------------------------------------------------------------------------------------------------ 6. the stand-alone path
@pytest.mark.parametrize("algo,envname", FUSED)
def test_sweep_path_has_the_fused_bits(algo, envname):
    tr, policies = _candidates(algo, envname)
    kw = dict(episodes=N, seed=SEED, constraints=True)
    flat = tr.agent.flat.data.clone()
    fused = tr.evaluate_policies(policies, **kw)
    with _schedule(tr, "fused_policies", 0):
        sweep = tr.evaluate_policies(policies, **kw)
    assert fused.path == "fused" and sweep.path == "sweep" and all(r.path == "fused" for r in sweep.results)
    assert_policies_matter(fused)
    for g in range(3):
        assert_group_is(sweep[g], fused[g])
    assert torch.equal(_bits(tr.agent.flat.data), _bits(flat))  # the sweep path put the live span back


# ------------------------------------------------------------------------------------------------ 7. nothing is touched
def test_a_sweep_touches_no_trainer_state(hip, monkeypatch):
    monkeypatch.setenv("RPO_GRAPH_CYCLE", "4")

    def fresh():
        torch.manual_seed(5)
        tr = build_trainer("ddpg", "cart", hip, DEV, num_envs=512, use_graph=True)
        tr.vec.reset()
        return tr
    a = fresh()
    a.run_steps(16)
    b = fresh()
    b.run_steps(8)
    torch.cuda.synchronize()
    ag = b.agent
    state = dict(flat=ag.flat.data, critic_target=ag.critic_target_flat, actor_m=ag.actor_optim.exp_avg,
                 actor_v=ag.actor_optim.exp_avg_sq, actor_step=ag.actor_optim.step_dev, critic_m=ag.critic_optim.exp_avg,
                 critic_v=ag.critic_optim.exp_avg_sq, critic_step=ag.critic_optim.step_dev, rows=b.buffer.rows)
    if ag.actor_target_flat is not None:
        state["actor_target"] = ag.actor_target_flat
    state.update({key: getattr(b.vec, key) for key in ("internal", "ep_len", "ep_ret", "ep_count", "ctrl", "stats")})
    snap = {key: t.clone() for key, t in state.items()}
    policies = [None, shifted_span(b, SHIFT["cart"]), _candidates("ddpg", "cart")[1][2]]
    s = b.evaluate_policies(policies, 100, constraints=True)
    assert s.path == "fused"
    assert_policies_matter(s)
    torch.cuda.synchronize()
    for key, t in state.items():
        assert torch.equal(_bits(t), _bits(snap[key])), key
    b.run_steps(8)
    torch.cuda.synchronize()
    for key in ("internal", "ep_len", "ep_ret", "ep_count", "ctrl"):
        assert torch.equal(getattr(a.vec, key), getattr(b.vec, key)), key
    assert torch.equal(a.buffer.rows, b.buffer.rows)
    assert torch.equal(a.agent.flat.data, b.agent.flat.data)
    assert torch.equal(a.agent.critic_target_flat, b.agent.critic_target_flat)
