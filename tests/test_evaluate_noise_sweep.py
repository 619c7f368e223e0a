"""trainer.evaluate_noise() on the CPU: the "sweep" path driven by the oracle backend, the host side of ``NoiseSweep`` on
synthetic accumulator rows, the refusals, and the header's view of the two new entry points.

The definition is the yardstick: group g of a sweep is ``evaluate(obs_noise=levels[g])`` with the shared seed, bit for bit --
accumulator rows (every ``EvalResult`` field) and the ``ConstraintReport``.  ``evaluate()`` keys episode i's draw by (seed, i,
step, column), so the groups share their z.  Every bit-for-bit test first asserts that the levels matter
(``assert_levels_matter``): a sweep that ignored its level would give equal groups and a vacuous comparison.
test_evaluate_noise_sweep_gpu.py imports the helpers below."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import oracle_backend as ob
from rpo_amd import _lib
from rpo_amd.algo.evaluation import MAX_NOISE_LEVELS, EvalResult, NoiseSweep, Paired, PolicySweep, ResultSweep
from test_act import SHIFT, _shifted
from test_evaluate_budgets import _Allocations, _rows
from test_evaluate_constraints import _cpu_trainer, assert_reports_equal, initial_obs
from test_train_step_golden import build_trainer

H = 12
CASES = [("ddpg", "cart"), ("sac", "pendulum")]


# ------------------------------------------------------------------------------------------------ shared helpers
def levels_of(tr):
    """[clean, a number, a vector with zero columns, a larger number]: the four levels of the bit-for-bit tests."""
    vec = [0.03 * (q + 1) for q in range(tr.kernels.obs_dim)]
    vec[1] = vec[3] = 0.0
    return [0, 0.05, vec, 0.2]


def widened(tr, levels):
    """float32 [S, obs_dim]: None -> zeros, a number broadcast, a vector as it is."""
    out = np.zeros((len(levels), tr.kernels.obs_dim), dtype=np.float32)
    for g, lv in enumerate(levels):
        if lv is not None:
            out[g] = np.asarray(lv, dtype=np.float32)
    return out


def assert_group_is(res, want, level):
    """Every EvalResult field and the report of one group against the definition's, bit for bit (NaN-safe); ``level``: the
    float32 sigma vector the group carries (the definition's own ``obs_noise`` is None for an all-zero level)."""
    for f in EvalResult.FIELDS:
        x, y = getattr(res, f), getattr(want, f)
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), f
    assert res.seed == want.seed and res.horizon == want.horizon
    assert (res.constraints is None) == (want.constraints is None) and res.trajectory is None
    if want.constraints is not None:
        assert_reports_equal(res.constraints, want.constraints)
    assert res.obs_noise.dtype == np.float32 and res.obs_noise.tobytes() == np.asarray(level, np.float32).tobytes()
    if want.obs_noise is None:
        assert not np.any(level)
    elif want.obs_noise is not level:
        assert want.obs_noise.tobytes() == res.obs_noise.tobytes()


def assert_levels_matter(s):
    """The precondition of every bit-for-bit comparison: the groups differ in some per-episode array."""
    groups = {b"".join(getattr(s, f)[g].tobytes() for f in EvalResult.FIELDS) for g in range(len(s))}
    assert len(groups) >= 2, "every group has the same results"


def assert_sweep_is_the_definition(tr, s, levels, **kw):
    want = widened(tr, levels)
    assert len(s) == len(levels) and s.levels.dtype == np.float32 and s.levels.tobytes() == want.tobytes()
    for g in range(len(levels)):
        assert_group_is(s[g], tr.evaluate(obs_noise=want[g], **kw), want[g])


@functools.lru_cache(maxsize=None)
def _trainer(algo, envname):
    return _cpu_trainer(algo, envname)


# ------------------------------------------------------------------------------------------------ the sweep path
@pytest.mark.parametrize("algo,envname", CASES)
def test_sweep_equals_the_calls(algo, envname):
    tr = _trainer(algo, envname)
    levels = levels_of(tr)
    with _shifted(tr, SHIFT[envname]):                           # (the projection iterates and steps are violated)
        for constraints in (False, True):
            kw = dict(episodes=7, horizon=H, seed=21, constraints=constraints)
            s = tr.evaluate_noise(obs_noise=levels, **kw)
            assert isinstance(s, NoiseSweep) and s.path == "sweep" and s.seed == 21 and s.horizon == H and s.episodes == 7
            assert all(r.path == "stepwise" for r in s.results)
            assert_levels_matter(s)
            assert_sweep_is_the_definition(tr, s, levels, **kw)
            assert_group_is(s[0], tr.evaluate(**kw), np.zeros(tr.kernels.obs_dim, np.float32))   # level 0: the clean evaluation
        if envname == "cart":                                    # init_states are shared by all levels
            kw = dict(episodes=7, horizon=H, seed=21, init_states=initial_obs(tr, 7, 5))
            s = tr.evaluate_noise(obs_noise=[None, 0.1, 0.1], **kw)
            assert_levels_matter(s)
            assert_sweep_is_the_definition(tr, s, [None, 0.1, 0.1], **kw)
            assert_group_is(s[1], s[2], s.levels[1])             # the same level twice: the same z, the same bits


def test_sweep_equals_the_calls_on_evopf_and_on_a_baseline():
    tr = _cpu_trainer("ddpg", "evopf")
    kw = dict(episodes=2, horizon=2, seed=3, constraints=True)
    s = tr.evaluate_noise(obs_noise=[0, 1e-3], **kw)
    assert s.path == "sweep" and s[0].path == "stepwise"
    assert_sweep_is_the_definition(tr, s, [0, 1e-3], **kw)
    torch.manual_seed(5)                                         # no projection: evaluate() takes it, so the sweep does
    la = build_trainer("ddpgla", "cart", ob, torch.device("cpu"), num_envs=4, fused=False)
    kw = dict(episodes=5, horizon=H, seed=4)
    s = la.evaluate_noise(obs_noise=[0, 0.3], **kw)
    assert s.path == "sweep"
    assert_levels_matter(s)
    assert_sweep_is_the_definition(la, s, [0, 0.3], **kw)


def test_one_seed_and_one_tick_of_the_call_counter():
    tr = _trainer("ddpg", "cart")
    calls = getattr(tr, "_evaluate_calls", 0)
    try:
        s = tr.evaluate_noise(3, obs_noise=[0, 0.1, 0.2], horizon=2)
        assert tr._evaluate_calls == calls + 1 and s.seed == s[0].seed == s[1].seed == s[2].seed
        tr._evaluate_calls = calls                               # the seed is the one evaluate() draws at the same count
        assert tr.evaluate(3, horizon=2).seed == s.seed
        tr.evaluate_noise(3, obs_noise=[0.1], horizon=2, seed=1)
        assert tr._evaluate_calls == calls + 1                   # (an explicit seed: no tick)
    finally:
        tr._evaluate_calls = calls


# ------------------------------------------------------------------------------------------------ NoiseSweep on synthetic rows
def _sweep(viols, n=5, seed=0, lengths=8, obs_dim=6):
    """A NoiseSweep over made-up accumulator rows: ``viols[g]`` violating steps per episode of level g, every episode
    ``lengths`` steps long, level g = 0.1 g in every column."""
    rng = np.random.RandomState(seed)
    results = []
    for v in viols:
        acc, _ = _rows(rng, n, v)
        acc[:, 7] = (np.full(n, lengths, np.int32) << 2).view(np.float32)
        results.append(EvalResult(acc, "fused", 10, 42))
    levels = np.repeat(0.1 * np.arange(len(viols), dtype=np.float32)[:, None], obs_dim, axis=1)
    return NoiseSweep(results, levels, "fused")


def test_noise_sweep_arrays_levels_and_paired():
    s = _sweep([[0, 0, 0, 0, 0], [2, 1, 0, 3, 1], [0, 1, 0, 0, 0]])
    assert isinstance(s, ResultSweep) and len(s) == 3 and s.episodes == 5 and s.path == "fused" and s.seed == 42 and s.horizon == 10
    assert s.levels.dtype == np.float32 and s.levels.shape == (3, 6)
    for f in EvalResult.FIELDS + ("iters",):
        x = getattr(s, f)
        assert x.shape == (3, 5), f
        for g in range(3):
            row = getattr(s[g], "proj_iters" if f == "iters" else f)
            assert s[g] is s.results[g] and np.shares_memory(x[g], row) and x[g].tobytes() == row.tobytes(), f
    for g in range(3):
        assert s[g].obs_noise.dtype == np.float32 and s[g].obs_noise.tobytes() == s.levels[g].tobytes()
    np.testing.assert_array_equal(s.violation_rate(), [r.violation_rate() for r in s.results])
    np.testing.assert_array_equal(s.ret_mean(), [r.ret.mean() for r in s.results])
    for a, b in ((0, 1), (1, 0), (2, 2), (0, 2)):
        d = s.ret[a] - s.ret[b]
        got = s.paired(a, b)
        assert isinstance(got, Paired) and got == (d.mean(), d.std(ddof=1) / np.sqrt(5), 5)
    # PolicySweep.paired is the same definition: the same bits on the same rows
    p = PolicySweep(_sweep([[0, 0, 0, 0, 0], [2, 1, 0, 3, 1], [0, 1, 0, 0, 0]]).results, ["a", "b", "c"], "fused")
    assert p.ret.tobytes() == s.ret.tobytes() and p.paired(0, 1) == s.paired(0, 1) and p.paired(2, 1) == s.paired(2, 1)
    one = _sweep([[0], [1]], n=1)
    got = one.paired(0, 1)
    assert got.n == 1 and got.mean == float(one.ret[0, 0] - one.ret[1, 0]) and np.isnan(got.stderr)
    assert "NoiseSweep" in repr(s) and "fused" in repr(s)
    with pytest.raises(ValueError):
        NoiseSweep(s.results, s.levels[:2], "fused")
    with pytest.raises(ValueError):
        NoiseSweep([], np.zeros((0, 6), np.float32), "fused")


@pytest.mark.parametrize("name,viols,max_rate,want", [
    ("every level is safe: the last one", [[0] * 5] * 4, 0.0, 3),
    ("the prefix ends at the first failing level", [[0] * 5, [0] * 5, [1] * 5, [2] * 5], 0.0, 1),
    ("non-monotone: a safe level behind a failing one does not count", [[0] * 5, [1] * 5, [0] * 5, [0] * 5], 0.0, 0),
    ("level 0 already fails", [[1, 0, 0, 0, 0], [0] * 5, [0] * 5], 0.0, -1),
    ("max_rate lets a violating level through", [[0] * 5, [1] * 5, [4] * 5, [1] * 5], 0.125, 1),
    ("max_rate, non-monotone", [[1] * 5, [2] * 5, [1] * 5], 0.125, 0),
    ("one level, safe", [[0] * 5], 0.0, 0),
    ("one level, unsafe", [[3] * 5], 0.0, -1),
])
def test_tolerance_is_the_longest_safe_prefix(name, viols, max_rate, want):
    s = _sweep(viols)                                            # 8 steps per episode: [1] * 5 is a rate of exactly 0.125
    got = s.tolerance(max_rate)
    assert got == want and isinstance(got, int), name
    if max_rate == 0.0:
        assert s.tolerance() == want
    rate = s.violation_rate()
    assert all(rate[g] <= max_rate for g in range(got + 1)) and (got + 1 == len(s) or rate[got + 1] > max_rate)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_allocate_nothing(monkeypatch):
    tr = _trainer("ddpg", "cart")
    calls = getattr(tr, "_evaluate_calls", 0)
    nan, inf = float("nan"), float("inf")
    bad_calls = [dict(obs_noise=[]), dict(obs_noise=()), dict(obs_noise=None), dict(obs_noise=0.1), dict(obs_noise="0.1"),
                 dict(obs_noise=[0.0] * (MAX_NOISE_LEVELS + 1)), dict(obs_noise=np.float32(0.1)),
                 dict(obs_noise=[0, [0.1] * 5]), dict(obs_noise=[0, [0.1] * 7]), dict(obs_noise=[[]]),
                 dict(obs_noise=[0, -1e-3]), dict(obs_noise=[0, nan]), dict(obs_noise=[inf]), dict(obs_noise=[0, [0.1, 0, 0, 0, 0, -1]]),
                 dict(obs_noise=[True]), dict(obs_noise=[0, "0.1"]), dict(obs_noise=[0, 1e39]),
                 dict(obs_noise=[0.1], episodes=0), dict(obs_noise=[0.1], episodes=True), dict(obs_noise=[0.1], episodes=2.5),
                 dict(obs_noise=[0.1], horizon=0), dict(obs_noise=[0.1], horizon=1 << 24), dict(obs_noise=[0.1], constraints=1),
                 dict(obs_noise=[0.1], episodes=3, init_states=np.zeros((2, 6), np.float32)),
                 dict(obs_noise=[0.1], episodes=3, init_states=np.zeros((3, 5), np.float32))]
    with _Allocations(tr, monkeypatch) as spy:
        for kw in bad_calls:
            with pytest.raises(ValueError):
                tr.evaluate_noise(**kw)
        for g, bad in ((0, -1.0), (2, nan), (1, [0.1] * 5)):    # the error names the offending index
            lv = [0.0, 0.0, 0.0]
            lv[g] = bad
            with pytest.raises(ValueError, match=r"obs_noise\[%d\]" % g):
                tr.evaluate_noise(obs_noise=lv)
        for kw in (dict(record=True), dict(eval_steps=3), dict(eval_lr=0.1)):    # not part of this entry point
            with pytest.raises(TypeError):
                tr.evaluate_noise(2, obs_noise=[0.1], **kw)
        assert spy.seen == []
    assert getattr(tr, "_evaluate_calls", 0) == calls            # a refused call draws no seed
    s = tr.evaluate_noise(2, obs_noise=[0.01] * MAX_NOISE_LEVELS, horizon=1, seed=1)    # S = 64 is allowed
    assert len(s) == MAX_NOISE_LEVELS and s.levels.shape == (MAX_NOISE_LEVELS, 6)
    s = tr.evaluate_noise(2, obs_noise=np.array([[0.0] * 6, [0.1] * 6], np.float32), horizon=1, seed=1)    # an [S, obs_dim] array
    assert s.levels.tobytes() == np.array([[0.0] * 6, [0.1] * 6], np.float32).tobytes()
    s = tr.evaluate_noise(2, obs_noise=torch.tensor([0.0, 0.1]), horizon=1, seed=1)    # S numbers in a tensor
    assert s.levels.tobytes() == np.array([[0.0] * 6, [0.1] * 6], np.float32).tobytes()


# ------------------------------------------------------------------------------------------------ the header
def test_the_header_declares_the_two_entry_points():
    P = _lib.PROTOTYPES
    tail = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_ulonglong, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    for env, other in (("cartsafe", "policies"), ("pendulum", "policies")):
        name = "rpo_%s_evaluate_noise_sweep" % env
        assert name in P
        pol = P["rpo_%s_evaluate_%s" % (env, other)]
        # the arguments of the policy sweep up to con, then sigma_table, noise_seed, group_lanes, episodes, stream
        assert P[name][:-6] == pol[:-5] and P[name][-6:] == tail, name
        con = P["rpo_%s_evaluate_constraints" % env]             # = the _constraints arguments without the trace
        assert P[name][:-6] == con[:-5] and con[-5:-2] == [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    assert len(P["rpo_cartsafe_evaluate_noise_sweep"]) == len(P["rpo_pendulum_evaluate_noise_sweep"]) + 1
    assert _lib.CONST["RPO_ABI_VERSION"] == 6                    # entry points were added, none changed


def test_entry_points_validate_the_groups_before_any_hip_call():
    """NULL table -> RPO_ERR_NULL; a misaligned table, group_lanes that is no positive multiple of 64, episodes outside
    [1, group_lanes], n_envs that is no whole number of groups -> RPO_ERR_ARG.  The env pointers are host memory and the actor is
    empty, so a call that got past this validation would not return these codes (an empty actor is RPO_ERR_ARG: the last line)."""
    from rpo_amd import ops as hip_ops
    lib = _lib.load()
    ARG, NULL = _lib.CONST["RPO_ERR_ARG"], _lib.CONST["RPO_ERR_NULL"]
    net = hip_ops._MlpStruct()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    head = (ctypes.byref(net), 0, 1.0, 0.0)
    cart = lambda n: head + (n,) + (p,) * 7 + (0, 1, -1.0, 1.0, 1, 0.1, 1e-5, 0.0, None, 1, 200, 1e-3)      # noqa: E731
    pend = lambda n: head + (n,) + (p,) * 8 + (0, 1, -1.0, 1.0, 1, 0.1, 1e-5, 0.0, 200, 1e-3)               # noqa: E731
    for fn, args in ((lib.rpo_cartsafe_evaluate_noise_sweep, cart), (lib.rpo_pendulum_evaluate_noise_sweep, pend)):
        for con in (None, p):
            assert fn(*args(128), con, None, 3, 64, 40, None) == NULL
            assert fn(*args(128), con, ctypes.c_void_p(p.value + 2), 3, 64, 40, None) == ARG
            for lanes, episodes in ((32, 32), (96, 40), (40, 40), (0, 1), (-64, 1), (64, 65), (64, 0), (64, -1), (256, 40)):
                assert fn(*args(128), con, p, 3, lanes, episodes, None) == ARG, (lanes, episodes)
            assert fn(*args(96), con, p, 3, 64, 40, None) == ARG
        assert fn(None, *args(128)[1:], None, p, 3, 64, 40, None) == NULL
        assert fn(*args(128), None, p, 3, 64, 40, None) == ARG   # the groups pass: the empty actor is next
