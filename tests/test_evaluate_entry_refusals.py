"""The host-side validation of the 14 ``rpo_<env>_evaluate*`` entry points: which return code a refused call gets, that is, which
check comes first.  No GPU: every call of the table hands over an empty actor (``RPO_ERR_ARG`` before any launch, the last check
of the ladder) and host memory as "device" pointers, so no call can reach a launch.

The expected codes are the ones the library returned BEFORE the entry points were folded onto one validation ladder,
recorded once by ``tests/golden/make_eval_entry_refusals.py`` into ``tests/golden/eval_entry_refusals.json``.  Every variant
tail (record, report, sigma, per-lane budgets, policy groups, noise groups) is crossed with the common-argument cases: valid-
looking pointers, all env pointers NULL, n = 0, steps = 0, a NULL actor, and n = 96 (no whole number of 64-lane groups)."""
import ctypes
import json
import os

from rpo_amd import _lib
from rpo_amd import ops as hip_ops

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_entry_refusals.json")
N = 128

_RAW = (ctypes.c_char * 1024)()                                  # a 64-byte aligned host buffer stands in for device memory
P = ctypes.c_void_p((ctypes.addressof(_RAW) + 63) // 64 * 64)
OFF4 = ctypes.c_void_p(P.value + 4)                              # float-aligned, not 16-byte aligned (trace, con)
OFF2 = ctypes.c_void_p(P.value + 2)                              # not float-aligned (lanes, the sigma table)
_NET = hip_ops._MlpStruct()                                      # an empty actor
_SIGMA = {}                                                      # host sigma vectors, kept alive


def _sigma(*values):
    arr = (ctypes.c_float * len(values))(*values)
    _SIGMA[len(_SIGMA)] = arr
    return ctypes.cast(arr, ctypes.c_void_p), len(values)


# group geometry (group_lanes, episodes) at n = 128: the cases of test_evaluate_noise_sweep.py, then good ones
GEOMETRY = [(32, 32), (96, 40), (40, 40), (0, 1), (-64, 1), (64, 65), (64, 0), (64, -1), (256, 40), (64, 40), (128, 128)]
TRACES = {"none": (None, 0, 0), "set": (P, 4, 12), "null_rows": (None, 4, 12), "rows0": (P, 0, 12), "rows>n": (P, N + 1, 12),
          "steps0": (P, 4, 0), "misaligned": (OFF4, 4, 12)}
CONS = {"none": None, "set": P, "misaligned": OFF4}


def tails(obs_dim):
    """variant -> {case: the arguments between viol_thresh and stream}"""
    good, longer, negative = _sigma(*[0.1] * obs_dim), _sigma(*[0.1] * (obs_dim + 1)), _sigma(*[0.1] * (obs_dim - 1) + [-0.1])
    out = {"": {"plain": ()}}
    out["_record"] = {"trace=" + k: TRACES[k] for k in ("set", "null_rows", "rows0", "rows>n", "steps0", "misaligned")}
    out["_constraints"] = {"trace=%s,con=%s" % (t, c): TRACES[t] + (CONS[c],)
                           for t in ("none", "set", "rows0") for c in ("none", "set", "misaligned")}
    sig = {"null": (None, obs_dim), "good": good, "longer": longer, "negative": negative}
    out["_noisy"] = {"trace=%s,con=%s,sigma=%s" % (t, c, s): TRACES[t] + (CONS[c],) + sig[s] + (7,)
                     for t in ("none", "set", "rows0") for c in ("none", "set") for s in sig}
    lanes = {"null": (None, None), "set": (P, P), "steps_null": (None, P), "lr_null": (P, None), "misaligned": (P, OFF2)}
    out["_budgets"] = {"trace=%s,con=%s,lanes=%s" % (t, c, ln): TRACES[t] + (CONS[c],) + lanes[ln]
                       for t in ("none", "set", "null_rows") for c in ("none", "set", "misaligned") for ln in lanes}
    out["_policies"] = {"con=%s,stride=%d,lanes=%d,episodes=%d" % (c, st, gl, ep): (CONS[c], st, gl, ep)
                        for c in ("none", "set") for st, (gl, ep) in
                        [(8, g) for g in GEOMETRY] + [(6, (64, 40)), (0, (64, 40)), (-4, (64, 40)), (2, (32, 32))]}
    tables = {"null": None, "set": P, "misaligned": OFF2}
    out["_noise_sweep"] = {"con=%s,table=%s,lanes=%d,episodes=%d" % (c, tb, gl, ep): (CONS[c], tables[tb], 3, gl, ep)
                           for c in ("none", "set") for tb, (gl, ep) in
                           [("set", g) for g in GEOMETRY] + [("null", (64, 40)), ("misaligned", (64, 40)), ("null", (32, 32))]}
    return out


def common(env_pointers, consts):
    """case -> (actor, the arguments from gauss to viol_thresh): n_envs, the env's pointers, acc, t0, steps, the projection,
    the env's constants, max_episode_steps, viol_thresh"""
    def args(n, steps, p):
        return (0, 1.0, 0.0, n) + (p,) * env_pointers + (0, steps, -1.0, 1.0, 1, 0.1, 1e-5, 0.0) + consts + (200, 1e-3)
    net = ctypes.byref(_NET)
    return {"ok": (net, args(N, 1, P)), "env_null": (net, args(N, 1, None)), "n0": (net, args(0, 1, P)),
            "steps0": (net, args(N, 0, P)), "actor_null": (None, args(N, 1, P)), "n96": (net, args(96, 1, P))}


def table():
    """[(id, symbol, arguments)]: every symbol x every tail of its variant x every common case."""
    rows = []
    for env, obs_dim, env_pointers, consts in (("cartsafe", 6, 7, (P, 1)), ("pendulum", 5, 8, ())):
        for variant, cases in tails(obs_dim).items():
            symbol = "rpo_%s_evaluate%s" % (env, variant)
            for case, tail in cases.items():
                for name, (actor, args) in common(env_pointers, consts).items():
                    rows.append(("%s[%s][%s]" % (symbol, case, name), symbol, (actor,) + args + tail + (None,)))
    return rows


def run_table():
    """id -> the code the loaded library returns."""
    lib = _lib.load()
    return {rid: int(getattr(lib, symbol)(*args)) for rid, symbol, args in table()}


def test_every_refusal_returns_the_recorded_code():
    with open(FIXTURE) as f:
        want = json.load(f)
    got = run_table()
    assert sorted(got) == sorted(want)                           # the table is the fixture's
    wrong = {rid: (got[rid], want[rid]) for rid in got if got[rid] != want[rid]}
    assert not wrong, "%d calls return another code (got, recorded): %s" % (len(wrong), dict(list(wrong.items())[:10]))


def test_the_fixture_holds_refusals_of_both_kinds_for_every_symbol():
    ARG, NULL = _lib.CONST["RPO_ERR_ARG"], _lib.CONST["RPO_ERR_NULL"]
    with open(FIXTURE) as f:
        want = json.load(f)
    assert all(code != 0 for code in want.values())
    symbols = sorted(set(symbol for _, symbol, _ in table()))
    assert len(symbols) == 14 and all(s in _lib.PROTOTYPES for s in symbols)
    for symbol in symbols:
        codes = set(code for rid, code in want.items() if rid.startswith(symbol + "["))
        assert codes == {ARG, NULL}, (symbol, codes)

