"""Scenarios of EVOPF-v0 without a GPU: the ``Scenarios`` container (refusals, padding, save / load, indexing, scaling, the table
layout), ``Scenarios.from_system_days`` on the 8 days of tests/golden/evopf_days.npz (tests/golden/make_evopf_days.py), the header
and the argument refusals of the three C-ABI entry points, and the NotImplementedErrors of the public interface.  The kernels:
tests/test_scenarios_gpu.py."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import oracle_backend as ob
from rpo_amd import _lib, ops
from rpo_amd.algo import evaluate_opf
from rpo_amd.env.electrical_grid import case14
from rpo_amd.env.electrical_grid.evopf import EVOPFEnv
from rpo_amd.env.electrical_grid.scenarios import MAX_PF, MIN_PF, Scenarios
from test_train_step_golden import build_trainer

ARG, NULL = _lib.CONST["RPO_ERR_ARG"], _lib.CONST["RPO_ERR_NULL"]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "evopf_days.npz")
CPU = torch.device("cpu")


@functools.lru_cache(maxsize=None)
def fixture_days():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def some_days(D, seed=0):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.0, 1.0, size=(D, 24, 28)).astype(np.float32), rng.uniform(-1.0, 3.0, size=(D, 48)).astype(np.float32)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


# ------------------------------------------------------------------------------------------------ the container
def test_refusals():
    d, p = some_days(3)
    S = Scenarios(d, p)
    assert len(S) == 3 and S.demand.dtype == np.float32 and S.price.dtype == np.float32
    for bad_d, bad_p in ((d[:, :23], p), (d[:, :, :27], p), (d[0], p), (d, p[:2]), (d, p[:, :47]), (d, p[:, :25]), (d, p[0]),
                         (d[:0], p[:0])):
        with pytest.raises(ValueError):
            Scenarios(bad_d, bad_p)
    for value in (np.nan, np.inf, -np.inf, 1e39):                # (1e39: finite in float64, not in float32)
        for which in (0, 1):
            dd, pp = d.astype(np.float64), p.astype(np.float64)
            (dd if which == 0 else pp).reshape(-1)[5] = value
            with pytest.raises(ValueError, match="finite"):
                Scenarios(dd, pp)
    for bad in (d.astype(bool), d.astype(np.complex64), d.astype(str)):
        with pytest.raises(TypeError):
            Scenarios(bad, p)
    with pytest.raises(TypeError):
        Scenarios(d, p.astype(object))
    # the arrays are copies, and nobody writes to them
    d[0, 0, 0] = 99.0
    assert S.demand[0, 0, 0] != 99.0
    with pytest.raises(ValueError):
        S.demand[0, 0, 0] = 1.0
    assert np.array_equal(Scenarios(torch.tensor(d), torch.tensor(p)).price, p)        # tensors and integers are numbers too
    assert Scenarios(np.ones((1, 24, 28), dtype=np.int64), np.ones((1, 24), dtype=np.int32)).demand.dtype == np.float32


def test_a_24_hour_price_is_padded_with_exact_zeros():
    d, p = some_days(4)
    S = Scenarios(d, p[:, :24])
    assert S.price.shape == (4, 48) and same_bits(S.price[:, :24], p[:, :24])
    assert np.array_equal(S.price[:, 24:].view(np.int32), np.zeros((4, 24), dtype=np.int32))     # +0.0, bit for bit


def test_save_and_load_round_trip_bit_for_bit(tmp_path):
    d, p = some_days(5, seed=1)
    d[1, 2, 3], p[2, 40] = -0.0, np.float32(1e-42)               # a negative zero and a denormal survive
    S = Scenarios(d, p)
    path = str(tmp_path / "days.npz")
    S.save(path)
    assert os.path.exists(path)
    L = Scenarios.load(path)
    assert same_bits(L.demand, S.demand) and same_bits(L.price, S.price) and same_bits(L.table(), S.table())


def test_indexing_and_concat():
    d, p = some_days(6, seed=2)
    S = Scenarios(d, p)
    one = S[4]
    assert isinstance(one, Scenarios) and len(one) == 1 and same_bits(one.demand[0], d[4]) and same_bits(one.price[0], p[4])
    assert same_bits(S[-1].demand[0], d[5])
    part = S[1:5:2]
    assert len(part) == 2 and same_bits(part.demand, d[1:5:2]) and same_bits(part.price, p[1:5:2])
    idx = np.array([5, 0, 0, 3])
    pick = S[idx]
    assert len(pick) == 4 and same_bits(pick.demand, d[idx]) and same_bits(pick.price, p[idx])
    assert same_bits(S[[2, 1]].price, p[[2, 1]])
    with pytest.raises(IndexError):
        S[6]
    with pytest.raises(IndexError):
        S[2:2]
    for bad in (1.5, np.array([True] * 6), "a", np.zeros((2, 2), dtype=np.int64)):
        with pytest.raises((TypeError, IndexError)):
            S[bad]
    both = Scenarios.concat([S[:2], S[4], S[2:4]])
    assert len(both) == 5 and same_bits(both.demand, d[[0, 1, 4, 2, 3]]) and same_bits(both.price, p[[0, 1, 4, 2, 3]])
    for bad in ([], [S, d], d):
        with pytest.raises(TypeError):
            Scenarios.concat(bad)
    assert same_bits(Scenarios.concat(S).demand, d)              # (a Scenarios iterates over its days)


def test_scaling_returns_new_objects_and_leaves_the_source_untouched():
    d, p = some_days(3, seed=3)
    S = Scenarios(d, p)
    d0, p0 = S.demand.copy(), S.price.copy()
    a = S.scale_demand(1.1)
    assert a is not S and same_bits(a.demand, d * np.float32(1.1)) and same_bits(a.price, p)
    per_day = np.array([1.0, 2.0, 0.5], dtype=np.float32)
    assert same_bits(S.scale_demand(per_day).demand, d * per_day[:, None, None])
    per_hour = np.linspace(0.5, 1.5, 24).astype(np.float32)
    assert same_bits(S.scale_demand(per_hour).demand, d * per_hour[None, :, None])
    b = S.scale_price(3)
    assert same_bits(b.price, p * np.float32(3)) and same_bits(b.demand, d)
    assert same_bits(S.scale_price(per_day).price, p * per_day[:, None])
    assert same_bits(S.scale_price(per_hour).price, p * np.tile(per_hour, 2)[None, :])          # hour h + 24 takes hour h's factor
    assert same_bits(S.demand, d0) and same_bits(S.price, p0)
    for bad in (np.ones(5), np.ones((3, 24)), np.nan, "x"):
        with pytest.raises((ValueError, TypeError)):
            S.scale_demand(bad)
        with pytest.raises((ValueError, TypeError)):
            S.scale_price(bad)
    with pytest.raises(ValueError, match="ambiguous"):           # 24 days: [24] could be either
        Scenarios(*some_days(24)).scale_demand(np.ones(24))


def test_table_places_every_element_where_the_layout_says():
    D = 3
    table = np.arange(D * 720, dtype=np.float32).reshape(D, 720)  # distinct integers, exact in float32
    assert _lib.CONST["RPO_EVOPF_SCEN_DAY"] == 720 == 48 + 24 * 28 and (720 * 4) % 16 == 0
    S = Scenarios.from_table(table)
    for day in range(D):
        for h in range(48):
            assert S.price[day, h] == table[day, h]
        for t in range(24):
            for j in range(14):
                assert S.demand[day, t, j] == table[day, 48 + 28 * t + j]                   # pd
                assert S.demand[day, t, 14 + j] == table[day, 48 + 28 * t + 14 + j]         # qd
    out = S.table()
    assert out.dtype == np.float32 and out.flags["C_CONTIGUOUS"] and same_bits(out, table)
    # built the other way round: demand and price given, the table read
    d, p = some_days(2, seed=4)
    t2 = Scenarios(d, p).table()
    assert t2.shape == (2, 720) and same_bits(t2[:, :48], p) and same_bits(t2[:, 48:].reshape(2, 24, 28), d)
    dev = Scenarios(d, p)
    assert dev.table(CPU) is dev.table("cpu") and same_bits(dev.table(CPU).numpy(), t2)        # the device copy is made once
    with pytest.raises(ValueError):
        Scenarios.from_table(table[:, :719])


# ------------------------------------------------------------------------------------------------ from_system_days
def ulp32(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def test_from_system_days_on_the_fixture():
    z = fixture_days()
    load, price = z["load"], z["price"]
    assert load.shape == (8, 24) and price.shape == (8, 48) and price.min() < 0      # the fixture holds the data's negative-price day
    env = EVOPFEnv(backend=ob, device="cpu")
    S = Scenarios.from_system_days(env, load, price, seed=0)
    assert len(S) == 8 and S.demand.shape == (8, 24, 28) and S.price.shape == (8, 48)
    pd, qd = S.demand[:, :, :14].astype(np.float64), S.demand[:, :, 14:].astype(np.float64)
    bus_pd, bus_qd = case14.BUS[:, case14.PD], case14.BUS[:, case14.QD]
    p_total = bus_pd.sum() * 24
    want = load / load.sum(axis=1, keepdims=True) * p_total / env.baseMVA
    # 11 load buses, each rounded to float32 once (half an ulp of itself, at most half an ulp of the sum): 5.5 ulps of the sum
    assert (np.abs(pd.sum(axis=2) - want) <= 6 * ulp32(want)).all(), np.abs((pd.sum(axis=2) - want) / ulp32(want)).max()
    assert (pd >= 0).all() and (pd[:, :, bus_pd == 0] == 0).all() and (pd[:, :, bus_pd != 0] > 0).all()
    # the split: (1 - rho) * the nominal share + rho * a Dirichlet draw -> every load bus keeps at least (1 - rho) of its share
    share = pd / pd.sum(axis=2, keepdims=True)
    assert (share[:, :, bus_pd != 0] >= (1 - case14.RHO) * (bus_pd / bus_pd.sum())[bus_pd != 0] * (1 - 1e-6)).all()
    # |qd| = pd tan(acos(pf)) with pf in [min_pf, max_pf]: tan(acos(pf)) in [0, tan(acos(min_pf))]; the sign is the case's
    on = bus_pd != 0
    ratio = np.abs(qd[:, :, on]) / pd[:, :, on]
    pf = np.cos(np.arctan(ratio))
    assert (pf >= MIN_PF - 1e-6).all() and (pf <= MAX_PF).all() and pf.std() > 0.01     # (float32 rounding of pd and qd: ~1e-7)
    assert (np.sign(qd) == np.sign(bus_qd) * (qd != 0)).all() and (qd[:, :, bus_qd == 0] == 0).all()
    assert (np.sign(qd[:, :, on & (bus_qd != 0)]) == np.sign(bus_qd[on & (bus_qd != 0)])).mean() > 0.99   # (pf = 1 exactly: qd = 0)
    # the price in the observation's units, the negative hours kept
    assert same_bits(S.price, (price / env.baseMVA).astype(np.float32)) and S.price.min() < 0
    assert np.array_equal(S.price < 0, price < 0)
    # seeds
    again = Scenarios.from_system_days(env, load, price, seed=0)
    other = Scenarios.from_system_days(env, load, price, seed=1)
    assert same_bits(again.demand, S.demand) and same_bits(again.price, S.price)
    assert not np.array_equal(other.demand, S.demand) and same_bits(other.price, S.price)
    assert np.allclose(other.demand[:, :, :14].sum(axis=2), pd.sum(axis=2), rtol=1e-6)
    # a 24-hour price is padded, bad curves are refused
    assert (Scenarios.from_system_days(env, load, price[:, :24]).price[:, 24:] == 0).all()
    for bad in (load[:, :23], -load, np.zeros_like(load), np.where(np.arange(24) == 3, np.nan, load)):
        with pytest.raises(ValueError):
            Scenarios.from_system_days(env, bad, price)


# ------------------------------------------------------------------------------------------------ header and C ABI
def test_header_declares_the_entry_points_and_the_abi_stays():
    protos, consts = _lib.parse_header()
    assert consts["RPO_EVOPF_SCEN_DAY"] == 720 and consts["RPO_ABI_VERSION"] == 6 and ops.SCEN_DAY == 720
    P, I, U, L, F, Q = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint, ctypes.c_longlong, ctypes.c_float, ctypes.c_ulonglong
    assert protos["rpo_evopf_scenario_table"] == [I, P, P, P, Q, U, P]
    assert protos["rpo_evopf_reset_scenario"] == [I, P, P, P, P, I, P, P, P]
    # rpo_evopf_step's arguments without auto_reset, seed, env_id_base, plus table, days, day
    step = list(protos["rpo_evopf_step"])
    assert step == [I, P, P, P, P, P, P, L, P, I, P, I, I, F, P, Q, U, P]
    assert protos["rpo_evopf_step_scenario"] == step[:12] + step[13:15] + [P, I, P, P]
    lib = _lib.load()
    assert lib.rpo_abi_version() == 6
    for name in ("rpo_evopf_scenario_table", "rpo_evopf_reset_scenario", "rpo_evopf_step_scenario"):
        assert hasattr(lib, name)


def test_bindings_are_backend_functions():
    for name in ("evopf_scenario_table", "evopf_reset_scenario", "evopf_step_scenario"):
        assert callable(getattr(ops, name)) and not hasattr(ops.EvopfKernels, name) and not hasattr(ob, name)
    k = EVOPFEnv(device="cpu").kernels
    with pytest.raises(_lib.RpoHipError):                        # CPU tensors are refused like by every other op
        ops.evopf_scenario_table(k, torch.zeros(2, 720), None, 0, 0)
    with pytest.raises(_lib.RpoHipError):
        ops.evopf_scenario_table(k, torch.zeros(2, 719), None, 0, 0)
    z = torch.zeros
    for table, day in ((z(3, 719), z(2, dtype=torch.int32)), (z(0, 720), z(2, dtype=torch.int32)), (z(3, 720), z(3, dtype=torch.int32)),
                       (z(3, 720), z(2, dtype=torch.int64)), (z(3, 720, dtype=torch.float64), z(2, dtype=torch.int32)), (None, None)):
        with pytest.raises(_lib.RpoHipError):
            ops.evopf_reset_scenario(k, z(2, 57), z(2, dtype=torch.int32), z(2), table, day)
        with pytest.raises(_lib.RpoHipError):
            ops.evopf_step_scenario(k, z(2, 57), z(2, 43), z(2, dtype=torch.int32), z(2), z(2, dtype=torch.int32), None, 1, None, None,
                                    24, 1e-3, table, day)


def test_argument_refusals_return_their_codes_without_a_gpu():
    """Every call below is refused before any launch (none is complete): the pointers are never followed."""
    lib = _lib.load()
    p = ctypes.c_void_p(4096)                                    # stands for a device pointer
    table = lib.rpo_evopf_scenario_table
    assert table(0, p, None, p, 1, 0, None) == ARG and table(-3, p, p, p, 1, 0, None) == ARG
    assert table(5, None, None, p, 1, 0, None) == NULL and table(5, p, None, None, 1, 0, None) == NULL
    reset = lib.rpo_evopf_reset_scenario
    assert reset(0, p, p, p, p, 3, p, p, None) == ARG and reset(5, p, p, p, p, 0, p, p, None) == ARG
    assert reset(5, p, p, p, p, -1, p, p, None) == ARG
    good = [5, p, p, p, p, 3, p, p, None]
    for k in (1, 2, 3, 4, 6, 7):                                 # state, ep_len, ep_ret, table, day, consts
        args = list(good)
        args[k] = None
        assert reset(*args) == NULL, k
    step = lib.rpo_evopf_step_scenario
    good = [5, p, p, p, p, p, p, 1, p, 2, p, 24, 1e-3, p, p, 3, p, None]
    for k, v in ((0, 0), (0, -1), (15, 0), (15, -2), (11, 0), (7, 0), (9, 0)):      # n, days, max_episode_steps, cap_steps, stats_cap
        args = list(good)
        args[k] = v
        assert step(*args) == ARG, (k, v)
    for k in (1, 2, 3, 4, 5, 13, 14, 16):                        # state, action, ep_len, ep_ret, ep_count, consts, table, day
        args = list(good)
        args[k] = None
        assert step(*args) == NULL, k


# ------------------------------------------------------------------------------------------------ the public interface
def test_evaluate_with_scenarios_names_evopf_on_another_env():
    S = Scenarios(*some_days(2))
    torch.manual_seed(0)
    tr = build_trainer("ddpg", "cart", ob, CPU, fused=False, num_envs=2, use_graph=False, capacity=32)
    with pytest.raises(NotImplementedError, match="EVOPF-v0"):
        tr.evaluate(2, scenarios=S)
    with pytest.raises(NotImplementedError, match="EVOPF-v0"):
        evaluate_opf(tr, 2, scenarios=S)
    # EVOPF-v0 itself, where no HIP step kernel runs: the oracle backend on the CPU
    ev = build_trainer("ddpg", "evopf", ob, CPU, fused=False, num_envs=2, use_graph=False, capacity=32)
    with pytest.raises(NotImplementedError, match="EVOPF-v0"):
        ev.evaluate(2, scenarios=S)
    res = ev.evaluate(2, horizon=2, seed=1)
    assert res.days is None and res.path == "stepwise"


def test_env_scenarios_needs_the_kernel():
    with pytest.raises(NotImplementedError, match="evopf_scenario_table"):
        EVOPFEnv(backend=ob, device="cpu").scenarios(5, seed=1)
    with pytest.raises(NotImplementedError, match="GPU"):
        EVOPFEnv(device="cpu").scenarios(5, seed=1)


def test_vec_env_with_a_scenario_never_auto_resets():
    from rpo_amd.env.vec import VecEnv
    k = EVOPFEnv(device="cpu").kernels
    v = VecEnv(k, 2, CPU, scenario=(torch.zeros(1, 720), torch.zeros(2, dtype=torch.int32)))
    with pytest.raises(ValueError, match="auto"):
        v.step(v.action)
    with pytest.raises(ValueError, match="auto"):
        v.step(v.action, auto_reset=True)
    with pytest.raises(NotImplementedError):                     # another env's kernels take no scenario
        VecEnv(EVOPFEnv(backend=ob, device="cpu").kernels, 2, CPU, scenario=v.scenario)
