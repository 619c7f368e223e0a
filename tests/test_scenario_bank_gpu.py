"""Training on a scenario bank on the MI355X: the deal (rpo_evopf_bank_days) against its host restatement, the bank step
(rpo_evopf_reset_bank / rpo_evopf_step_bank) against the table-fed step bit for bit inside an episode and across its end, whole
training runs on a bank that deals the Philox days against the plain trainer bit for bit (eager, hipGraph windows, RPOSAC),
checkpoints, and a lane's independence of its neighbours.  5 lanes in the kernel tests (one full four-wave workgroup and a ragged
one), 16 in the trainer tests.  The host side: tests/test_scenario_bank.py."""
import functools

import numpy as np
import pytest
import torch

from rpo_amd import ops
from rpo_amd.env.electrical_grid.scenarios import Scenarios
from test_scenario_bank import bank_days
from test_scenarios_gpu import DEV, N, SEED, _actions, _days, _env, same
from test_train_step_golden import build_trainer

pytestmark = pytest.mark.gpu

BASE = 5                                                         # env_id_base of the kernel tests
STRIDE = 16                                                      # "the run's lane count" of the kernel tests
EP0 = (0, 3, 1, 0, 2)                                            # episode counters the lanes start from
LANES = 16                                                       # the trainer tests
TRAIN_SEED = 11                                                  # build_trainer's Philox seed
I32 = dict(dtype=torch.int32, device=DEV)


def device_days(ep_count, days, deal, stride=STRIDE, base=BASE, seed=SEED, n=N):
    out = torch.full((n,), -7, **I32)
    ops.evopf_bank_days(out, ep_count, days, deal, stride, seed, base)
    return out


def host_days(ep_count, days, deal, stride=STRIDE, base=BASE, seed=SEED, n=N):
    ep = np.zeros(n, dtype=np.int64) if ep_count is None else np.asarray(ep_count, dtype=np.int64) & 0xFFFFFFFF
    return bank_days(seed, base + np.arange(n), ep, days, deal, stride)


# ------------------------------------------------------------------------------------------------ 1. the deal
@pytest.mark.parametrize("deal", ["uniform", "cycle"])
def test_the_deal_equals_its_host_restatement(deal):
    for D in (1, 3, 7):
        for ep in (EP0, None, (-1, 2 ** 31 - 1, -2 ** 31, 65536, 7)):       # (the last: episode counters as the unsigned words they are)
            dev = device_days(None if ep is None else torch.tensor(ep, **I32), D, deal).cpu().numpy()
            assert dev.dtype == np.int32 and np.array_equal(dev.astype(np.int64), host_days(ep, D, deal)), (D, ep)
            if D == 1:
                assert (dev == 0).all()
    # more than one block of the one-thread-per-lane kernel, a ragged one at the end
    n = 2 * 256 + 3
    ep = torch.arange(n, **I32) % 5
    dev = device_days(ep, 731, deal, stride=n, base=1000, n=n).cpu().numpy()
    assert np.array_equal(dev.astype(np.int64), host_days(ep.cpu().numpy(), 731, deal, stride=n, base=1000, n=n))


# ------------------------------------------------------------------------------------------------ 2. + 3. the step
def _bank_vec(deal, ep0=EP0, n=N, base=BASE, max_episode_steps=None, table=None):
    env = _env()
    table = _days().table(DEV) if table is None else table
    v = env.make_vec(n, seed=SEED, env_id_base=base, max_episode_steps=max_episode_steps, bank=(table, deal, STRIDE))
    v.ep_count.copy_(torch.tensor(ep0, **I32))
    return v


def _fed_vec(day, max_episode_steps=None):
    """A table-fed env (``scenario=``) on day[i] of the same table, reset to hour 0."""
    v = _env().make_vec(N, seed=SEED, env_id_base=BASE, max_episode_steps=max_episode_steps, scenario=(_days().table(DEV), day))
    v.reset()
    return v


def _follow(deal, steps, max_episode_steps=None, auto_reset=True):
    """Steps a bank env beside table-fed envs: inside an episode everything is equal bit for bit; where an episode ends the bank
    lane is dealt the day of its next episode and goes on like a fresh table-fed env on that day."""
    D = len(_days())
    assert D == 3 < N                                            # fewer days than lanes
    bank = _bank_vec(deal, max_episode_steps=max_episode_steps)
    bank.reset()
    ep = np.array(EP0, dtype=np.int64)
    day = device_days(bank.ep_count, D, deal)
    assert np.array_equal(day.cpu().numpy(), host_days(ep, D, deal))
    fed = _fed_vec(day, max_episode_steps)
    rows_a, rows_b = (torch.full((N, _env().kernels.ring_floats), 7.0, device=DEV) for _ in range(2))
    for name in ("internal", "ep_len", "ep_ret"):
        assert same(getattr(bank, name), getattr(fed, name)), ("reset", name)
    assert float(bank.internal.abs().sum()) > 0
    actions = _actions(steps)
    length = min(24, max_episode_steps or 24)
    resets, pos = 0, 0
    for t in range(steps):
        bank.step(actions[t], rows=rows_a, cap_steps=1, auto_reset=auto_reset)
        fed.step(actions[t], rows=rows_b, cap_steps=1, auto_reset=False)
        pos += 1
        assert same(rows_a, rows_b), (t, "row")                  # the transition row, the episode's last one included
        assert float(rows_a[:, 158].sum()) == (N if pos == length or (not auto_reset and pos > length) else 0)
        if auto_reset and pos == length:                         # the end of an episode: the next deal
            ep += 1
            resets, pos = resets + 1, 0
            assert np.array_equal(bank.ep_count.cpu().numpy().astype(np.int64), ep)
            assert (bank.ep_len == 0).all() and (bank.ep_ret == 0).all()
            day = device_days(bank.ep_count, D, deal)
            assert np.array_equal(day.cpu().numpy(), host_days(ep, D, deal))
            fed = _fed_vec(day, max_episode_steps)               # evopf_reset_scenario on the new days
            assert same(bank.internal, fed.internal), (t, "the next deal")
        else:
            for name in ("internal", "ep_len", "ep_ret"):
                assert same(getattr(bank, name), getattr(fed, name)), (t, name)
    if not auto_reset:
        assert np.array_equal(bank.ep_count.cpu().numpy(), EP0) and int(bank.ep_len[0]) == steps
    assert int(bank.ctrl[ops.CONST["RPO_CTRL_NONFINITE"]]) == 0 and int(bank.ctrl[ops.CONST["RPO_CTRL_T"]]) == steps
    return resets


@pytest.mark.parametrize("deal", ["uniform", "cycle"])
def test_the_bank_step_is_the_table_fed_step_and_an_episodes_end_deals_the_next_day(deal):
    assert _follow(deal, 48) == 2                                # steps 1..23, the end at 24, 25..47 on the next deal, 48


@pytest.mark.parametrize("deal", ["uniform", "cycle"])
def test_an_episode_that_ends_before_its_day_is_dealt_the_next_day_too(deal):
    assert _follow(deal, 13, max_episode_steps=6) == 2


def test_without_auto_reset_the_bank_step_is_the_table_fed_step():
    assert _follow("uniform", 25, auto_reset=False) == 0


def test_the_days_of_one_bank_differ_between_the_lanes():
    """(what the comparisons above rest on: the three days are different days, and the lanes are not all on the same one)"""
    for deal in ("uniform", "cycle"):
        d = host_days(EP0, 3, deal)
        assert len(set(d.tolist())) > 1
    t = _days().table()
    assert not np.array_equal(t[0], t[1]) and not np.array_equal(t[1], t[2])


# ------------------------------------------------------------------------------------------------ 6. neighbours
@pytest.mark.parametrize("deal", ["uniform", "cycle"])
def test_a_lane_depends_on_its_global_id_only(deal):
    steps = 30
    actions = _actions(steps)
    together = _bank_vec(deal)
    together.reset()
    W = _env().kernels.ring_floats
    rows = torch.zeros(steps * N, W, device=DEV)
    for t in range(steps):
        together.step(actions[t], rows=rows, cap_steps=steps, auto_reset=True)
    rows = rows.view(steps, N, W)
    for i in range(N):
        alone = _bank_vec(deal, ep0=EP0[i:i + 1], n=1, base=BASE + i)
        alone.reset()
        mine = torch.zeros(steps, W, device=DEV)
        for t in range(steps):
            alone.step(actions[t, i:i + 1].contiguous(), rows=mine, cap_steps=steps, auto_reset=True)
        assert same(mine, rows[:, i]), i
        assert same(alone.internal[0], together.internal[i]) and int(alone.ep_count[0]) == int(together.ep_count[i]) == EP0[i] + 1


# ------------------------------------------------------------------------------------------------ 4. whole training runs
_SAC_KW = dict(lr_actor=1e-4, lr_critic=3e-4, grad_eps=0.1, init_lamb=0.0, init_nju=0.0, alpha=0.001,
               automatic_entropy_tuning=False, fixed=False)            # scripts/evopf_exp_sac.py:30-33


@functools.lru_cache(maxsize=None)
def _philox_bank():
    """The days the Philox streams deal 16 lanes under the trainer's seed in episodes 0..3, one after the other: with "cycle" and
    stride 16, lane i is dealt row i + 16 e in episode e -- exactly its Philox day."""
    return Scenarios.concat([_env().scenarios(LANES, TRAIN_SEED, episode=e) for e in range(4)])


def _train(algo, steps, use_graph, work_dir=None, **extra):
    torch.manual_seed(5)
    kw = dict(_SAC_KW) if algo == "sac" else {}
    kw.update(extra)
    tr = build_trainer(algo, "evopf256", ops, DEV, num_envs=LANES, use_graph=use_graph, **kw)
    assert tr.seed == TRAIN_SEED
    if work_dir is not None:
        tr.work_dir = work_dir
    if steps:
        tr.vec.reset()
        tr.run_steps(steps)
        torch.cuda.synchronize()
    return tr


def _assert_same_run(a, b, steps):
    assert torch.equal(a.agent.flat.data, b.agent.flat.data)
    for name in ("internal", "ep_count", "ep_len", "ep_ret"):
        assert torch.equal(getattr(a.vec, name), getattr(b.vec, name)), name
    filled = steps * LANES
    assert torch.equal(a.buffer.rows[:filled], b.buffer.rows[:filled]) and float(a.buffer.rows[:filled].abs().sum()) > 0
    assert int(a.vec.ctrl[0]) == int(b.vec.ctrl[0]) == steps


@pytest.mark.parametrize("algo,use_graph", [("ddpg", False), ("ddpg", True), ("sac", True)], ids=["ddpg_eager", "ddpg_graph", "sac_graph"])
def test_training_on_the_philox_days_as_a_bank_equals_plain_training(algo, use_graph, monkeypatch):
    monkeypatch.setenv("RPO_GRAPH_CYCLE", "4")
    monkeypatch.setenv("RPO_GRAPH_AUDIT", "1")
    steps = 60                                                   # every lane rolls over at steps 24 and 48
    plain = _train(algo, steps, use_graph)
    banked = _train(algo, steps, use_graph, scenarios=_philox_bank(), deal="cycle")
    assert plain.scenarios is None and plain.scenario_days() is None and len(banked.scenarios) == 64
    assert (plain.vec.ep_count == 2).all() and (plain.vec.ep_len == 12).all()
    _assert_same_run(plain, banked, steps)
    assert np.array_equal(banked.scenario_days(), 32 + np.arange(LANES))
    if use_graph:
        for tr in (plain, banked):
            kinds = [e.get("node_kinds") for e in tr._graphs.entries.values() if e["graph"] is not None]
            assert kinds and not tr._graphs.capture_failed
            for k in kinds:
                assert set(k) == {"kernel"}, k


def test_training_on_a_uniformly_dealt_bank():
    steps = 60
    S = _days()
    a = _train("ddpg", steps, True, scenarios=S)                 # deal="uniform" is the default
    b = _train("ddpg", steps, True, scenarios=S, deal="uniform")
    plain = _train("ddpg", steps, True)
    assert a.deal == "uniform" and a.vec.bank[1:] == ("uniform", LANES)
    assert bool(torch.isfinite(a.agent.flat.data).all()) and bool(torch.isfinite(a.vec.internal).all())
    assert bool(torch.isfinite(a.buffer.rows[:steps * LANES]).all())
    _assert_same_run(a, b, steps)                                # reproduces itself from the same seed
    assert not torch.equal(a.agent.flat.data, plain.agent.flat.data) and not torch.equal(a.vec.internal, plain.vec.internal)
    assert (a.vec.ep_count == 2).all()
    days = a.scenario_days()
    assert days.dtype == np.int64 and days.shape == (LANES,)
    assert np.array_equal(days, bank_days(TRAIN_SEED, np.arange(LANES), a.vec.ep_count.cpu().numpy(), 3, "uniform", LANES))
    # the lanes really are on those days: their price windows are the table's
    obs = a.vec.internal.cpu().numpy()
    for i in range(LANES):
        assert same(obs[i, 33:57], S.price[days[i], 12:36]), i


# ------------------------------------------------------------------------------------------------ 5. checkpoints
def test_resume_on_a_bank_is_exact_and_another_bank_is_refused(tmp_path):
    S = _days()
    d = str(tmp_path / "ckpt")
    whole = _train("ddpg", 60, True, work_dir=d, scenarios=S)
    first = _train("ddpg", 30, True, work_dir=d, scenarios=S)    # 30: six hours into the second episode
    first.save()
    st = torch.load(str(tmp_path / "ckpt" / "trainer_state.pth"), weights_only=False)
    assert st["bank"] == dict(days=3, deal="uniform", stride=LANES, digest=S.digest())
    second = _train("ddpg", 0, True, work_dir=d, scenarios=Scenarios.from_table(S.table()))   # the same days, another object
    second.load()
    assert np.array_equal(second.scenario_days(), first.scenario_days())
    second.run_steps(30)
    torch.cuda.synchronize()
    _assert_same_run(whole, second, 60)
    assert torch.equal(whole.agent.critic_target_flat, second.agent.critic_target_flat)
    # another bank, another deal, no bank: refused before anything is modified
    for extra in (dict(scenarios=S.scale_price(2.0)), dict(scenarios=S[:2]), dict(scenarios=S, deal="cycle"), {}):
        other = _train("ddpg", 0, True, work_dir=d, **extra)
        before = other.agent.flat.data.clone()
        with pytest.raises(ValueError, match="does not match this trainer"):
            other.load()
        assert torch.equal(before, other.agent.flat.data) and other._t == 0 and int(other.vec.ctrl[0]) == 0
    # and a checkpoint without a bank into a trainer with one
    plain = _train("ddpg", 4, True, work_dir=str(tmp_path / "plain"))
    plain.save()
    other = _train("ddpg", 0, True, work_dir=str(tmp_path / "plain"), scenarios=S)
    before = other.agent.flat.data.clone()
    with pytest.raises(ValueError, match="bank"):
        other.load()
    assert torch.equal(before, other.agent.flat.data)
