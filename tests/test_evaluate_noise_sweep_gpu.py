"""trainer.evaluate_noise() on the MI355X: the fused path (the NSW instances of the evaluation kernel: S groups of padded lanes
in one launch sequence, every workgroup under its group's sigma out of a device table, the draw keyed by the episode within the
group) against its definition -- group g is, bit for bit, ``evaluate(obs_noise=levels[g])`` with the shared seed -- the pairing,
the padding lanes, the refusals, the "sweep" path, and that nothing of the trainer is touched.

Trainers are tests/test_act_gpu.py's (cart-RPODDPG, pendulum-RPOSAC after 8 training steps), with the actor's last bias shifted
(``SHIFT``: the projection iterates and steps are violated) while a sweep runs.  Every bit-for-bit test first asserts that the
levels matter (``assert_levels_matter``): a kernel that ignored its group's sigma would give equal groups and a vacuous
comparison.  No tolerances: every comparison is on bits."""
import ctypes

import numpy as np
import pytest
import torch

from test_act_gpu import SHIFT, _setup, _shifted
from test_evaluate_budgets_gpu import _init_states, _schedule
from test_evaluate_noise_sweep import assert_group_is, assert_levels_matter, assert_sweep_is_the_definition, levels_of, widened
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


def _trainer(algo, envname):
    return _setup(algo, envname)[0]


def _bits(t):
    return t.detach().contiguous().view(torch.int32) if t.dtype != torch.int64 else t.detach().contiguous()


# ------------------------------------------------------------------------------------------------ 1, 2. the definition
@pytest.mark.parametrize("constraints", [False, True])
@pytest.mark.parametrize("inject", [False, True])
@pytest.mark.parametrize("algo,envname", FUSED)
def test_fused_equals_the_definition_and_the_sweep_path_bit_for_bit(algo, envname, inject, constraints):
    tr = _trainer(algo, envname)
    levels = levels_of(tr)                                       # [0, 0.05, a vector with two zero columns, 0.2]
    kw = dict(episodes=N, seed=SEED, init_states=_init_states(tr, N) if inject else None, constraints=constraints)
    with _shifted(tr, SHIFT[envname]):
        s = tr.evaluate_noise(obs_noise=levels, **kw)
        assert s.path == "fused" and s.horizon == 200 and s.seed == SEED and s.episodes == N and len(s) == 4
        assert all(r.path == "fused" for r in s.results)
        assert_levels_matter(s)
        assert int(s.viol_steps.max()) > 0 and s.length.min() >= 1 and not s.nonfinite.any()
        assert_sweep_is_the_definition(tr, s, levels, **kw)
        # 2. level 0 is the clean evaluation
        assert_group_is(s[0], tr.evaluate(obs_noise=None, **kw), np.zeros(tr.kernels.obs_dim, np.float32))
        with _schedule(tr, "fused_noise_sweep", 0):
            sweep = tr.evaluate_noise(obs_noise=levels, **kw)
    assert sweep.path == "sweep" and all(r.path == "fused" for r in sweep.results)
    assert sweep.levels.tobytes() == s.levels.tobytes()
    for g in range(4):
        assert_group_is(sweep[g], s[g], s.levels[g])
    if constraints:
        c = s[1].constraints
        assert c.ineq_max.shape == (N, tr.kernels.ineq_num) and c.names == s[0].constraints.names
        np.testing.assert_array_equal(c.ineq_max.max(1), s.max_ineq[1])


# ------------------------------------------------------------------------------------------------ 3. the pairing
@pytest.mark.parametrize("algo,envname", FUSED)
def test_the_same_level_twice_gives_the_same_bits(algo, envname):
    """Groups 1 and 3 (and 2 and 4) carry the same sigma: keyed by the episode within the group they draw the same z and
    are bit-identical; keyed by the lane (g * 64 + e) they would not be."""
    tr = _trainer(algo, envname)
    vec = levels_of(tr)[2]
    with _shifted(tr, SHIFT[envname]):
        s = tr.evaluate_noise(N, obs_noise=[0, 0.1, vec, 0.1, vec], seed=SEED, constraints=True)
    assert s.path == "fused"
    assert_levels_matter(s)
    assert s.ret[0].tobytes() != s.ret[1].tobytes() or s.max_eq[0].tobytes() != s.max_eq[1].tobytes()   # (0.1 is not clean)
    assert_group_is(s[3], s[1], s.levels[1])
    assert_group_is(s[4], s[2], s.levels[2])


# ------------------------------------------------------------------------------------------------ 4. the 64-lane instance
@pytest.mark.parametrize("algo,envname", FUSED)
def test_the_64_lane_instance(algo, envname):
    """4 x 3100 episodes in groups of 3136 lanes = 12 544 lanes >= 64 x 192: the 64-lane tiles, the last one of every group
    ragged (28 of 64 lanes live); the definition's 3100-lane calls run the 16-lane instance."""
    tr = _trainer(algo, envname)
    levels = levels_of(tr)
    kw = dict(episodes=3100, seed=SEED, horizon=6, constraints=True)
    with _shifted(tr, SHIFT[envname]):
        s = tr.evaluate_noise(obs_noise=levels, **kw)
        assert s.path == "fused" and s.horizon == 6 and len(s) == 4
        assert_levels_matter(s)
        assert_sweep_is_the_definition(tr, s, levels, **kw)     # (group 3 too: the fourth group's ragged tile ends the grid)


# ------------------------------------------------------------------------------------------------ 5. launch splits
@pytest.mark.parametrize("algo,envname", FUSED)
def test_launch_splits_are_invisible(hip, algo, envname, monkeypatch):
    tr = _trainer(algo, envname)
    levels = levels_of(tr)
    kw = dict(episodes=N, seed=SEED, constraints=True)
    with _shifted(tr, SHIFT[envname]):
        one = tr.evaluate_noise(obs_noise=levels, **kw)
        launches = []
        inner = tr.kernels.evaluate_noise_sweep
        monkeypatch.setattr(tr.kernels, "evaluate_noise_sweep", lambda *a, **k: (launches.append((a[12], a[13])), inner(*a, **k))[1])
        monkeypatch.setattr(hip, "EVAL_LANE_STEPS", 3 * 64 * 4)  # n = S x padded lanes = 4 x 64: 3 steps per launch
        split = tr.evaluate_noise(obs_noise=levels, **kw)
    assert launches[:3] == [(0, 3), (3, 3), (6, 3)] and len(launches) == 67 and launches[-1] == (198, 2)
    assert one.path == split.path == "fused"
    assert_levels_matter(one)
    for g in range(4):
        assert_group_is(split[g], one[g], one.levels[g])
    assert one.length.max() > 3                                 # (episodes did run on into later launches)


# ------------------------------------------------------------------------------------------------ 6. padding lanes
@pytest.mark.parametrize("constraints", [False, True])
@pytest.mark.parametrize("algo,envname", FUSED)
def test_padding_is_never_touched(hip, algo, envname, constraints):
    """The wrapper itself on 3 x 64 lanes with 40 episodes per group: accumulators, report, actions and the padding lanes' env
    rows hold a sentinel before; afterwards the 24 padding rows of every group still do, and the live rows of group g equal
    those of the noisy entry point on a 40-lane env with sigma g."""
    tr = _trainer(algo, envname)
    k, S, GL, steps = tr.kernels, 3, 64, 6
    levels = widened(tr, levels_of(tr)[:S])
    live = (torch.arange(S * GL, device=DEV) % GL) < N
    make = dict(seed=SEED, max_episode_steps=tr.max_episode_steps, device=DEV, stats_cap=2)
    small = tr.base_env.make_vec(N, **make)
    small.reset()
    v = tr.base_env.make_vec(S * GL, **make)
    v.internal.view(S, GL, -1)[:, :N].copy_(small.internal)
    if v.obs is not v.internal:
        v.obs.view(S, GL, -1)[:, :N].copy_(small.obs)
    W = hip.con_width(k.ineq_num, k.eq_num)
    acc = torch.zeros(S * GL, 8, device=DEV)
    con = torch.zeros(S * GL, W, device=DEV) if constraints else None
    everywhere = [acc, v.action] + ([con] if constraints else [])
    padding_only = [v.internal, v.ep_len, v.ep_ret, v.ep_count] + ([] if v.obs is v.internal else [v.obs])
    for t in everywhere:
        _bits(t).fill_(SENTINEL)
    for t in padding_only:
        _bits(t).reshape(S * GL, -1)[~live] = SENTINEL
    before = [t.clone() for t in padding_only]
    table = torch.zeros(S, 8, device=DEV)
    table[:, :k.obs_dim] = torch.from_numpy(levels).to(DEV)
    scale, base = tr._box_affine

    def args(e, a):
        return (tr.fused.descs["actor"], tr._gauss_policy, scale, base, e.internal, None if e.obs is e.internal else e.obs, e.action,
                e.ep_len, e.ep_ret, e.ep_count, e.ctrl, a, 0, steps, tr._box_lo, tr._box_hi, tr.eval_steps, tr.eval_lr, tr.corr_eps,
                tr.corr_momentum, e.max_episode_steps, e.viol_thresh)
    with _shifted(tr, SHIFT[envname]):
        k.evaluate_noise_sweep(*args(v, acc), table, SEED, GL, N, con=con)
        torch.cuda.synchronize()
        for t in everywhere:
            rows = _bits(t).reshape(S * GL, -1)
            assert bool((rows[~live] == SENTINEL).all()), "a padding row was written"
            assert bool((rows[live] != SENTINEL).any(dim=1).all()), "a live row was not written"
        for t, was in zip(padding_only, before):
            assert torch.equal(_bits(t).reshape(S * GL, -1)[~live], _bits(was).reshape(S * GL, -1)[~live]), "a padding lane's env row was written"
        word = acc[:, 7].contiguous().view(torch.int32)[live]
        assert int((word >> 2).min()) >= 1 and int((word >> 2).max()) == steps
        seen = set()
        for g in range(S):                                       # the grouped reference: one 40-lane launch per level
            e = tr.base_env.make_vec(N, **make)
            e.reset()
            a = torch.zeros(N, 8, device=DEV)
            c = torch.zeros(N, W, device=DEV) if constraints else None
            kw = dict(con=c) if constraints else {}
            if levels[g].any():
                kw["noise"] = (levels[g], SEED)
            k.evaluate(*args(e, a), **kw)
            torch.cuda.synchronize()
            rows = slice(g * GL, g * GL + N)
            pairs = [(acc[rows], a), (v.action[rows], e.action), (v.internal[rows], e.internal), (v.ep_len[rows], e.ep_len),
                     (v.ep_ret[rows], e.ep_ret), (v.ep_count[rows], e.ep_count)]
            pairs += [(con[rows], c)] if constraints else []
            pairs += [] if v.obs is v.internal else [(v.obs[rows], e.obs)]
            for x, y in pairs:
                assert torch.equal(_bits(x), _bits(y)), "group %d differs from its 40-lane launch" % g
            seen.add(_bits(v.internal[rows]).cpu().numpy().tobytes())
        assert len(seen) == S                                    # (the levels took the episodes to different states)


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
    fill = (b.buffer.size, b.buffer.pointer, b.buffer._steps_host)    # the replay ring's fill counter (host mirror of ctrl[0])
    s = b.evaluate_noise(100, obs_noise=[0, 0.05, 0.5], constraints=True)
    assert s.path == "fused"
    assert_levels_matter(s)
    torch.cuda.synchronize()
    for key, t in state.items():
        assert torch.equal(_bits(t), _bits(snap[key])), key
    assert (b.buffer.size, b.buffer.pointer, b.buffer._steps_host) == fill
    assert b.buffer.ctrl is b.vec.ctrl or torch.equal(b.buffer.ctrl, snap["ctrl"])
    b.run_steps(8)
    torch.cuda.synchronize()
    for key in ("internal", "ep_len", "ep_ret", "ep_count", "ctrl"):
        assert torch.equal(getattr(a.vec, key), getattr(b.vec, key)), key
    assert torch.equal(a.buffer.rows, b.buffer.rows)
    assert torch.equal(a.agent.flat.data, b.agent.flat.data)
    assert torch.equal(a.agent.critic_target_flat, b.agent.critic_target_flat)


# ------------------------------------------------------------------------------------------------ 8. refusals
@pytest.mark.parametrize("algo,envname", FUSED)
def test_refusals_come_before_any_launch(hip, algo, envname, monkeypatch):
    from rpo_amd import _lib
    lib = _lib.load()
    ERR_ARG, ERR_NULL = _lib.CONST["RPO_ERR_ARG"], _lib.CONST["RPO_ERR_NULL"]
    assert _lib.CONST["RPO_ABI_VERSION"] == 6 and lib.rpo_abi_version() == 6
    tr = _trainer(algo, envname)
    k, S, GL = tr.kernels, 2, 64
    O = k.obs_dim
    launched = []
    with monkeypatch.context() as m:                             # the trainer's entry point: ValueError, nothing launched
        m.setattr(k, "evaluate_noise_sweep", lambda *a, **kw: launched.append("sweep"))
        m.setattr(k, "evaluate", lambda *a, **kw: launched.append("evaluate"))
        for bad in ([], [0.0] * 65, [0, [0.1] * (O - 1)], [0, [0.1] * (O + 1)], [0, -0.1], [0, float("nan")], [float("inf")],
                    [0, [0.1] * (O - 1) + [-1.0]]):
            with pytest.raises(ValueError):
                tr.evaluate_noise(N, obs_noise=bad, seed=SEED)
        assert launched == []
    n = S * GL
    v = tr.base_env.make_vec(n, seed=1, max_episode_steps=tr.max_episode_steps, device=DEV, stats_cap=2)
    v.reset()
    acc = torch.zeros(n, 8, device=DEV)
    _bits(acc).fill_(SENTINEL)
    con = torch.zeros(n, hip.con_width(k.ineq_num, k.eq_num), device=DEV)
    table = torch.zeros(S, 8, device=DEV)
    table[1, :O] = 0.1
    vp = lambda t: ctypes.c_void_p(t.data_ptr())               # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    scale, base = tr._box_affine
    desc = tr.fused.descs["actor"]
    net = desc.net_struct()
    state = (vp(v.internal),) if envname == "cart" else (vp(v.internal), vp(v.obs))
    consts = (ctypes.c_void_p(k.consts.ctypes.data), k.partial) if envname == "cart" else ()
    fn = lib.rpo_cartsafe_evaluate_noise_sweep if envname == "cart" else lib.rpo_pendulum_evaluate_noise_sweep

    def call(actor, sigma, group_lanes, episodes, n_envs=n, con=None):
        return fn(actor, int(tr._gauss_policy), scale, base, n_envs, *state, vp(v.action), vp(v.ep_len), vp(v.ep_ret),
                  vp(v.ep_count), vp(v.ctrl), vp(acc), 0, 2, tr._box_lo, tr._box_hi, tr.eval_steps, tr.eval_lr, tr.corr_eps,
                  tr.corr_momentum, *consts, v.max_episode_steps, v.viol_thresh, con, sigma, SEED, group_lanes, episodes, stream)
    before = v.internal.clone()
    ok = ctypes.byref(net)
    assert call(None, vp(table), GL, N) == ERR_NULL             # no actor
    assert call(ok, None, GL, N) == ERR_NULL                    # no sigma table
    assert call(ok, None, GL, N, con=vp(con)) == ERR_NULL
    assert call(ok, ctypes.c_void_p(table.data_ptr() + 2), GL, N) == ERR_ARG    # not 4-byte aligned
    for bad_lanes in (32, 96, 40, 0, -64):                      # not a multiple of 64, not positive
        assert call(ok, vp(table), bad_lanes, min(N, max(bad_lanes, 1))) == ERR_ARG
    assert call(ok, vp(table), GL, GL + 1) == ERR_ARG           # more episodes than lanes in a group
    assert call(ok, vp(table), GL, 0) == ERR_ARG and call(ok, vp(table), GL, -1) == ERR_ARG
    assert call(ok, vp(table), GL, N, n_envs=n - 32) == ERR_ARG    # n is not S x group_lanes
    assert call(ok, vp(table), 2 * n, N) == ERR_ARG             # (not even one whole group)
    net.E = 256
    assert call(ok, vp(table), GL, N) == ERR_ARG
    net.E = 128
    torch.cuda.synchronize()
    assert torch.equal(v.internal, before) and bool((_bits(acc) == SENTINEL).all())    # nothing was launched
    assert call(ok, vp(table), GL, N) == 0 and call(ok, vp(table), GL, GL, con=vp(con)) == 0
    torch.cuda.synchronize()
    assert not bool((_bits(acc) == SENTINEL).any())             # (episodes = group_lanes: no padding at all)
    args = (desc, tr._gauss_policy, scale, base, v.internal, None if v.obs is v.internal else v.obs, v.action, v.ep_len, v.ep_ret,
            v.ep_count, v.ctrl, acc, 0, 2, tr._box_lo, tr._box_hi, tr.eval_steps, tr.eval_lr, tr.corr_eps, tr.corr_momentum,
            v.max_episode_steps, v.viol_thresh)
    with pytest.raises(hip.RpoHipError):                        # the binding checks what the kernel indexes by group:
        k.evaluate_noise_sweep(*args, table[:1], SEED, GL, N)   # fewer rows in the table than groups of lanes
    with pytest.raises(hip.RpoHipError):
        k.evaluate_noise_sweep(*args, table, SEED, 32, 32)      # lanes that are not S x group_lanes
    with pytest.raises(hip.RpoHipError):
        k.evaluate_noise_sweep(*args, table[:, :6].contiguous(), SEED, GL, N)    # not [S, 8]
