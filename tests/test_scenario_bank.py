"""Training on a scenario bank without a GPU: the header's view of the three entry points (rpo_evopf_reset_bank / _step_bank /
_bank_days), their argument refusals, the refusals of the bindings, of ``VecEnv(bank=)`` and of the trainers' ``scenarios=`` /
``deal=``, ``Scenarios.split``, and the host restatement of the two deal rules (``bank_days``), which tests/test_scenario_bank_gpu.py
holds the kernels to."""
import ctypes

import numpy as np
import pytest
import torch

import oracle_backend as ob
from oracle import philox
from rpo_amd import _lib, ops
from rpo_amd.env.electrical_grid.evopf import EVOPFEnv
from rpo_amd.env.electrical_grid.scenarios import Scenarios
from rpo_amd.env.vec import VecEnv
from test_scenarios import some_days
from test_train_step_golden import build_trainer

ARG, NULL = _lib.CONST["RPO_ERR_ARG"], _lib.CONST["RPO_ERR_NULL"]
CPU = torch.device("cpu")
STREAM_EVOPF_DAY = 8


# ------------------------------------------------------------------------------------------------ the deal, restated
def bank_days(seed, env_ids, episodes, days, deal, stride):
    """The bank row lane ``env_ids[i]`` plays in episode ``episodes[i]`` -> int64 [n].  "uniform": word 0 of Philox(seed; env id,
    episode, stream 8, 0) times ``days``, the high 32 bits of the 64-bit product; "cycle": (env id + episode * stride) mod days in
    unbounded integers.  Every index lies in [0, days)."""
    env_ids = np.asarray(env_ids, dtype=np.int64).reshape(-1)
    episodes = np.broadcast_to(np.asarray(episodes, dtype=np.int64), env_ids.shape)
    if deal == "uniform":
        w = philox.draw(seed, env_ids, episodes, STREAM_EVOPF_DAY, 0)[:, 0]
        out = np.array([(int(x) * int(days)) >> 32 for x in w], dtype=np.int64)
    elif deal == "cycle":
        out = np.array([(int(i) + int(e) * int(stride)) % int(days) for i, e in zip(env_ids, episodes)], dtype=np.int64)
    else:
        raise ValueError(deal)
    assert ((out >= 0) & (out < days)).all()
    return out


def test_the_restated_deals_stay_inside_the_bank_and_the_cycle_is_fair():
    ids = np.arange(5, 5 + 64)
    for days in (1, 3, 7, 731):
        for deal in ("uniform", "cycle"):
            for ep in (0, 1, 2 ** 31 - 1, 2 ** 32 - 1):           # (the restatement asserts 0 <= day < days itself)
                d = bank_days(77, ids, ep, days, deal, 64)
                assert d.shape == (64,) and d.dtype == np.int64
            assert (bank_days(77, ids, 3, 1, deal, 64) == 0).all()
    # cycle, stride and days coprime: over `days` consecutive episodes one lane visits every day exactly once
    for days, stride in ((7, 16), (3, 16), (731, 1024), (9, 16)):
        assert np.gcd(days, stride) == 1
        for lane in (0, 5, 1023):
            seen = bank_days(0, np.full(days, lane), np.arange(days), days, "cycle", stride)
            assert np.array_equal(np.sort(seen), np.arange(days)), (days, stride, lane)
            again = bank_days(0, np.full(3 * days, lane), np.arange(3 * days), days, "cycle", stride)
            assert (np.bincount(again, minlength=days) == 3).all()
    # cycle on a bank of stride * E days: lane i plays day i + e * stride in episode e < E (the bank of whole training runs)
    assert np.array_equal(bank_days(0, np.arange(16), 2, 64, "cycle", 16), 32 + np.arange(16))
    # uniform: keyed by the seed, the lane and the episode, and spread over the bank
    u = bank_days(77, np.arange(4096), 0, 7, "uniform", 4096)
    assert (np.bincount(u, minlength=7) > 4096 // 7 - 120).all()             # (6 sigma of a binomial(4096, 1/7) is 134)
    assert not np.array_equal(u, bank_days(78, np.arange(4096), 0, 7, "uniform", 4096))
    assert not np.array_equal(u, bank_days(77, np.arange(4096), 1, 7, "uniform", 4096))
    assert np.array_equal(u[5:10], bank_days(77, np.arange(5, 10), 0, 7, "uniform", 1))       # a lane's global id alone


# ------------------------------------------------------------------------------------------------ header and C ABI
def test_header_declares_the_entry_points_and_the_abi_stays():
    protos, consts = _lib.parse_header()
    assert consts["RPO_ABI_VERSION"] == 6 and consts["RPO_STREAM_EVOPF_DAY"] == STREAM_EVOPF_DAY == ops.STREAM_EVOPF_DAY
    assert consts["RPO_EVOPF_DEAL_UNIFORM"] == 0 and consts["RPO_EVOPF_DEAL_CYCLE"] == 1
    assert ops.DEALS == dict(uniform=0, cycle=1)
    taken = {k: v for k, v in consts.items() if k.startswith("RPO_STREAM_")}
    assert len(set(taken.values())) == len(taken)                # stream 8 is nobody else's
    P, I, U, L, F, Q = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint, ctypes.c_longlong, ctypes.c_float, ctypes.c_ulonglong
    step = list(protos["rpo_evopf_step"])
    assert step == [I, P, P, P, P, P, P, L, P, I, P, I, I, F, P, Q, U, P]
    # rpo_evopf_step's whole argument list (auto_reset, seed, env_id_base included), plus table, days, deal, stride
    assert protos["rpo_evopf_step_bank"] == step[:-1] + [P, I, I, I, P]
    assert protos["rpo_evopf_reset_bank"] == [I, P, P, P, P, P, I, I, I, Q, U, P]
    assert protos["rpo_evopf_bank_days"] == [I, P, I, I, I, Q, U, P, P]
    lib = _lib.load()
    assert lib.rpo_abi_version() == 6
    for name in ("rpo_evopf_reset_bank", "rpo_evopf_step_bank", "rpo_evopf_bank_days"):
        assert hasattr(lib, name)


def test_argument_refusals_return_their_codes_without_a_gpu():
    """Every call below is refused before any launch (none is complete): the pointers are never followed."""
    lib = _lib.load()
    p = ctypes.c_void_p(4096)                                    # stands for a device pointer
    days = lib.rpo_evopf_bank_days
    good = [5, p, 3, 1, 16, 77, 5, p, None]
    for k, v in ((0, 0), (0, -2), (2, 0), (2, -1), (3, -1), (3, 2), (4, 0), (4, -5)):    # n, days, deal, stride (cycle)
        args = list(good)
        args[k] = v
        assert days(*args) == ARG, (k, v)
    args = list(good)
    args[7] = None
    assert days(*args) == NULL
    assert days(5, None, 3, 0, 0, 77, 5, None, None) == NULL     # (ep_count may be NULL, and the uniform deal takes any stride)
    reset = lib.rpo_evopf_reset_bank
    good = [5, p, p, p, p, p, 3, 1, 16, 77, 5, None]
    for k, v in ((0, 0), (6, 0), (6, -1), (7, 2), (7, -1), (8, 0)):
        args = list(good)
        args[k] = v
        assert reset(*args) == ARG, (k, v)
    for k in (1, 2, 3, 5):                                       # state, ep_len, ep_ret, table
        args = list(good)
        args[k] = None
        assert reset(*args) == NULL, k
    step = lib.rpo_evopf_step_bank
    good = [5, p, p, p, p, p, p, 1, p, 2, p, 24, 1, 1e-3, p, 77, 5, p, 3, 1, 16, None]
    for k, v in ((0, 0), (0, -1), (18, 0), (18, -2), (19, 2), (19, -1), (20, 0), (11, 0), (7, 0), (9, 0)):
        args = list(good)
        args[k] = v
        assert step(*args) == ARG, (k, v)
    for k in (1, 2, 3, 4, 5, 14, 17):                            # state, action, ep_len, ep_ret, ep_count, consts, table
        args = list(good)
        args[k] = None
        assert step(*args) == NULL, k


def test_bindings_are_backend_functions_with_the_scenario_refusals():
    for name in ("evopf_reset_bank", "evopf_step_bank", "evopf_bank_days"):
        assert callable(getattr(ops, name)) and not hasattr(ops.EvopfKernels, name) and not hasattr(ob, name)
    k = EVOPFEnv(device="cpu").kernels
    z = torch.zeros
    i32 = dict(dtype=torch.int32)

    def reset(table, deal="cycle", stride=2, ep_count=None):
        ops.evopf_reset_bank(k, z(2, 57), z(2, **i32), z(2), z(2, **i32) if ep_count is None else ep_count, 0, 0, table, deal, stride)

    def step(table, deal="cycle", stride=2, ep_count=None):
        ops.evopf_step_bank(k, z(2, 57), z(2, 43), z(2, **i32), z(2), z(2, **i32) if ep_count is None else ep_count, None, 1, None,
                            None, 24, True, 1e-3, 0, 0, table, deal, stride)

    for fn in (reset, step):
        for table in (z(3, 719), z(0, 720), z(3, 720, dtype=torch.float64), z(720), z(720, 3).t(), None):
            with pytest.raises(_lib.RpoHipError, match="table"):
                fn(table)
        for deal in ("round-robin", 2, -1, None, True, 1.0):
            with pytest.raises(_lib.RpoHipError, match="deal"):
                fn(z(3, 720), deal=deal)
        for stride in (0, -4, 2 ** 31):
            with pytest.raises(_lib.RpoHipError, match="stride"):
                fn(z(3, 720), stride=stride)
        for ep_count in (z(3, **i32), z(2, dtype=torch.int64), z(2)):
            with pytest.raises(_lib.RpoHipError, match="ep_count"):
                fn(z(3, 720), ep_count=ep_count)
        with pytest.raises(_lib.RpoHipError, match="GPU"):      # CPU tensors are refused like by every other op
            fn(z(3, 720))
    for out, ep in ((z(2), None), (z(2, dtype=torch.int64), None), (z(0, **i32), None), (z(2, 2, **i32), None), (None, None),
                    (z(2, **i32), z(3, **i32)), (z(2, **i32), z(2, dtype=torch.int64))):
        with pytest.raises(_lib.RpoHipError):
            ops.evopf_bank_days(out, ep, 3, "cycle", 2, 0, 0)
    for days, deal, stride in ((0, "cycle", 2), (-1, "uniform", 2), (3, "shuffle", 2), (3, 5, 2), (3, "cycle", 0)):
        with pytest.raises(_lib.RpoHipError):
            ops.evopf_bank_days(z(2, **i32), None, days, deal, stride, 0, 0)
    with pytest.raises(_lib.RpoHipError, match="GPU"):
        ops.evopf_bank_days(z(2, **i32), None, 3, "uniform", 2, 0, 0)


# ------------------------------------------------------------------------------------------------ the public interface
def test_vec_env_takes_a_bank_or_a_scenario():
    k = EVOPFEnv(device="cpu").kernels
    table, day = torch.zeros(3, 720), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError, match="not both"):
        VecEnv(k, 2, CPU, scenario=(table, day), bank=(table, "cycle", 2))
    with pytest.raises(NotImplementedError, match="EVOPF-v0"):   # another env's kernels take no bank
        VecEnv(EVOPFEnv(backend=ob, device="cpu").kernels, 2, CPU, bank=(table, "cycle", 2))
    with pytest.raises(ValueError):
        VecEnv(k, 2, CPU, bank=(table, "cycle"))
    v = VecEnv(k, 2, CPU, bank=(table, "cycle", 2))
    assert v.scenario is None and v.bank[1:] == ("cycle", 2)
    assert VecEnv(k, 2, CPU).bank is None and VecEnv(k, 2, CPU, scenario=(table, day)).bank is None
    with pytest.raises(_lib.RpoHipError, match="GPU"):          # the bank's reset and step are the HIP kernels: no CPU path
        v.reset()
    with pytest.raises(_lib.RpoHipError, match="GPU"):
        v.step(v.action, auto_reset=False)


def test_constructor_refusals():
    S = Scenarios(*some_days(3))
    torch.manual_seed(0)
    kw = dict(fused=False, num_envs=2, use_graph=False, capacity=32)
    for algo in ("ddpg", "sac"):
        with pytest.raises(NotImplementedError, match="EVOPF-v0"):           # another env
            build_trainer(algo, "cart", ob, CPU, scenarios=S, **kw)
        with pytest.raises(NotImplementedError, match="EVOPF-v0"):           # EVOPF-v0 on the oracle backend
            build_trainer(algo, "evopf", ob, CPU, scenarios=S, **kw)
        with pytest.raises(NotImplementedError, match="EVOPF-v0"):           # the HIP kernels, but a CPU device
            build_trainer(algo, "evopf", ops, CPU, scenarios=S, **kw)
        for bad in (S.table(), (S.demand, S.price), "days.npz", 3):
            with pytest.raises(TypeError, match="Scenarios"):
                build_trainer(algo, "evopf", ob, CPU, scenarios=bad, **kw)
        for deal in ("round-robin", 1, None):
            with pytest.raises(ValueError, match="deal"):
                build_trainer(algo, "evopf", ob, CPU, scenarios=S, deal=deal, **kw)
    tr = build_trainer("ddpg", "cart", ob, CPU, **kw)            # without scenarios nothing changes
    assert tr.scenarios is None and tr.scenario_days() is None and tr.vec.bank is None
    for algo in ("ddpgla", "sacla"):                             # the Lagrangian baselines do not get the keyword
        with pytest.raises(TypeError):
            build_trainer(algo, "cart", ob, CPU, scenarios=S, num_envs=2, capacity=32)


def test_a_checkpoint_without_a_bank_has_no_bank_entry(tmp_path):
    torch.manual_seed(0)
    tr = build_trainer("ddpg", "cart", ob, CPU, fused=False, num_envs=2, use_graph=False, capacity=32)
    tr.work_dir = str(tmp_path / "ckpt")
    tr.vec.reset()
    tr.run_steps(2)
    tr.save()
    st = torch.load(str(tmp_path / "ckpt" / "trainer_state.pth"), weights_only=False)
    assert "bank" not in st
    tr.load()                                                    # and loads as before


# ------------------------------------------------------------------------------------------------ Scenarios.split
def test_split_is_disjoint_covering_and_reproducible():
    S = Scenarios(*some_days(10))
    a, b = S.split(0.7, seed=3)
    assert len(a) == 7 and len(b) == 3
    rows = {S.table()[i].tobytes(): i for i in range(10)}
    ia, ib = [rows[r.tobytes()] for r in a.table()], [rows[r.tobytes()] for r in b.table()]
    assert not set(ia) & set(ib) and sorted(ia + ib) == list(range(10))
    assert ia == sorted(ia) and ib == sorted(ib)                 # each part in the order of the source
    a2, b2 = S.split(0.7, seed=3)
    assert np.array_equal(a.table(), a2.table()) and np.array_equal(b.table(), b2.table())
    d0 = S.split(0.7)
    assert np.array_equal(d0[0].table(), S.split(0.7, seed=0)[0].table())
    assert any(not np.array_equal(S.split(0.7, seed=s)[1].table(), b.table()) for s in range(4, 9))
    assert [len(x) for x in S.split(0.5)] == [5, 5] and [len(x) for x in Scenarios(*some_days(2)).split(0.5)] == [1, 1]
    assert isinstance(a, Scenarios) and S.demand.shape[0] == 10  # the source is untouched


def test_split_refuses_an_empty_part():
    S = Scenarios(*some_days(10))
    for frac in (0.0, 1.0, -0.1, 1.5, 0.01, 0.99, float("nan"), "half", None, True):
        with pytest.raises(ValueError):
            S.split(frac)
    with pytest.raises(ValueError):
        Scenarios(*some_days(1)).split(0.5)


def test_digest_is_of_the_table_bytes():
    import hashlib
    S = Scenarios(*some_days(3))
    assert S.digest() == hashlib.sha1(S.table().astype(np.float32).tobytes()).hexdigest()
    assert S.digest() == Scenarios.from_table(S.table()).digest() != S.scale_price(2.0).digest()
    assert S.digest() != S[[1, 0, 2]].digest()
