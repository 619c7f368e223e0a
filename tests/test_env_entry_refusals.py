"""The host-side validation of the 32 stand-alone env entry points -- csrc/cartsafe.hip (7), pendulum.hip (8), evopf.hip (11)
and act.hip (6): which return code a refused call gets, that is, which check comes first.  No GPU, and none allowed: a call the
library accepts goes on to a launch -- harmless without a device (a HIP error), a kernel on host addresses with one.  The test
therefore skips where ``/dev/kfd`` exists, and it only makes the calls the fixture names, all of which are refusals.

The expected codes are the ones the library returned BEFORE these entry points were put on the shared launch helper and the
shared checks, recorded once by ``tests/golden/make_env_entry_refusals.py`` into ``tests/golden/env_entry_refusals.json`` (the
encoding of ``split_entry_refusals.json``).

For every symbol the table starts from a good call built from the header's prototype (every pointer a 128-byte aligned host
buffer, the actor struct of ``*_policy_act*`` fully populated) and applies
  * one defect (``defects``): every pointer argument NULL in turn, the scalar defects of ``SCALARS`` (``stride-1``: the row stride
    one below the env's width), ``explicit without noise``, a misaligned action / ineq_resid / profile and the actor defects of
    ``*_policy_act*``;
  * every pair (ARG defect, NULL defect) of the single defects the recorded library refused with RPO_ERR_ARG and with
    RPO_ERR_NULL: only such a pair shows which of two checks comes first;
  * the call with every argument NULL.
"""
import ctypes

import pytest

from rpo_amd import _lib
from rpo_amd import ops as hip_ops
from test_fused_entry_refusals import CODE, HAS_GPU_NODE, LETTER, P, _CONSTS, _arg, _field, _params, fixture_rows  # noqa: F401
import test_split_entry_refusals as split_refusals

FIXTURE = split_refusals.FIXTURE.replace("split_entry", "env_entry")
ENV_OBS = dict(cartsafe=6, pendulum=5, evopf=_lib.CONST["RPO_EVOPF_STATE"])
SYMBOLS = sorted(["rpo_%s_%s" % (env, m) for env in ("cartsafe", "pendulum", "evopf")
                  for m in ("reset", "step", "act_project", "complete_bwd", "resid", "ineq_partial_grad", "lagrangian")] +
                 ["rpo_pendulum_project_batchref"] +
                 ["rpo_evopf_%s" % m for m in ("tanh_box_bwd", "gauss_head", "gauss_head_bwd", "eq_vjp")] +
                 ["rpo_%s_%s" % (env, m) for env in ("cartsafe", "pendulum") for m in ("policy_act", "policy_act_profile", "project_profile")])
PARAMS = {s: _params(s) for s in SYMBOLS}
NET_FIELDS = hip_ops.MlpDesc.FIELDS
GOOD_INT = dict(n=64, n_envs=64, cap_steps=1000, stats_cap=8, noise_mode=_lib.CONST["RPO_NOISE_PHILOX"], max_steps=5, partial=1,
                max_episode_steps=200, auto_reset=1, newton_max_iters=50)
STRIDES = ("obs_stride", "state_stride")


def env_of(symbol):
    return symbol.split("_")[1]


class Call(object):
    """One call's arguments: the good call of a symbol and its actor struct."""

    def __init__(self, symbol):
        self.symbol, self.args, self.structs = symbol, {}, {}
        obs = ENV_OBS[env_of(symbol)]
        for name, kind in PARAMS[symbol]:
            if kind == "net":
                net = self.structs[name] = hip_ops._MlpStruct()
                for f in NET_FIELDS:
                    setattr(net, f, P)
                net.S, net.A, net.E, net.H, net.n_out, net.cat, net.head_dim = obs, 0, 128, 256, 1, 0, 1
            elif kind == "ptr":
                self.args[name] = None if name == "stream" else ctypes.addressof(_CONSTS) if name == "consts_host" else P
            elif kind in (ctypes.c_float, ctypes.c_double):
                self.args[name] = 0.5
            elif name in STRIDES:
                self.args[name] = obs
            else:
                self.args[name] = GOOD_INT.get(name, 1 if kind in (ctypes.c_uint, ctypes.c_ulonglong) else 0)

    def run(self, lib):
        args = [ctypes.addressof(self.structs[n]) if self.structs.get(n) is not None else self.args.get(n) for n, _ in PARAMS[self.symbol]]
        return int(getattr(lib, self.symbol)(*args))


SCALARS = dict([("%s=0" % n, {n: 0}) for n in ("n", "n_envs", "max_episode_steps", "cap_steps", "stats_cap", "newton_max_iters")] +
               [("max_steps=-1", {"max_steps": -1}), ("noise_mode=-1", {"noise_mode": -1}),
                ("noise_mode=%d" % (_lib.CONST["RPO_NOISE_CLIP_ONLY"] + 1), {"noise_mode": _lib.CONST["RPO_NOISE_CLIP_ONLY"] + 1}),
                ("noise_mode=explicit,noise=NULL", {"noise_mode": _lib.CONST["RPO_NOISE_EXPLICIT"], "noise": None}),
                ("partial=2", {"partial": 2}), ("form=-1", {"form": -1}), ("form=4", {"form": 4}),
                ("profile+4", {"profile": P + 4})])


def defects(symbol):
    """name -> the edit of a good Call, in the order of the module's docstring"""
    kinds = dict(PARAMS[symbol])
    nets = [n for n, k in PARAMS[symbol] if k == "net"]
    d = {"%s=NULL" % n: _arg(**{n: None}) for n, k in PARAMS[symbol] if k == "ptr" and n != "stream"}
    d.update(("%s=NULL" % n, (lambda c, n=n: c.structs.__setitem__(n, None))) for n in nets)
    d.update((name, _arg(**values)) for name, values in SCALARS.items() if all(k in kinds for k in values))
    d.update(("%s-1" % n, _arg(**{n: ENV_OBS[env_of(symbol)] - 1})) for n in STRIDES if n in kinds)
    if symbol == "rpo_pendulum_project_batchref":
        d["n=1025"] = _arg(n=1025)
    if nets:                                                     # *_policy_act*: 8-byte stores of the action and residual rows
        d["action+4"], d["ineq_resid+4"] = _arg(action=P + 4), _arg(ineq_resid=P + 4)
    for n in nets:
        d["%s.S+1" % n] = lambda c, n=n: setattr(c.structs[n], "S", c.structs[n].S + 1)
        d["%s.A=2" % n], d["%s.H=128" % n], d["%s.E=256" % n] = _field([n], A=2), _field([n], H=128), _field([n], E=256)
        d["%s.n_out=2" % n], d["%s.cat=1" % n], d["%s.head_dim=2" % n] = _field([n], n_out=2), _field([n], cat=1), _field([n], head_dim=2)
        d.update(("%s.%s=NULL" % (n, f), _field([n], **{f: None})) for f in ("Ws", "bs", "W0", "b0", "W1", "b1"))
    return d


def run_rows(rows_of):
    """rows_of(symbol, names of the single defects) -> the rows to run, each one a tuple of one or two defect names (a pair is
    applied ARG defect first).  -> {symbol: {row: code}}"""
    lib, out = _lib.load(), {}
    for symbol in SYMBOLS:
        d = defects(symbol)
        out[symbol] = {}
        for row in rows_of(symbol, list(d)):
            c = Call(symbol)
            for name in row:
                d[name](c)
            out[symbol][row] = c.run(lib)
    return out


def all_null(lib, symbol):
    """every pointer NULL, every scalar zero"""
    return int(getattr(lib, symbol)(*[None if k in ("net", "ptr") else 0 for _, k in PARAMS[symbol]]))


def load_fixture():
    import json
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.skipif(HAS_GPU_NODE, reason="an accepted call would launch a kernel on host addresses")
def test_every_refusal_returns_the_recorded_code():
    want = load_fixture()
    lib = _lib.load()
    assert sorted(want["all_null"]) == SYMBOLS
    assert {s: all_null(lib, s) for s in SYMBOLS} == want["all_null"]
    rows = {key: fixture_rows(entry) for key, entry in want["combos"].items()}
    got = run_rows(lambda key, names: rows[key])
    wrong = {(key, row): (got[key][row], code) for key in rows for row, code in rows[key].items() if got[key][row] != code}
    assert not wrong, "%d calls return another code (got, recorded): %s" % (len(wrong), dict(list(wrong.items())[:10]))


def test_every_fixture_row_is_in_the_table():
    want = load_fixture()
    assert sorted(want["combos"]) == SYMBOLS
    for symbol in SYMBOLS:
        names, entry = set(defects(symbol)), want["combos"][symbol]
        assert set(entry["arg"]) <= names and set(entry["null"]) <= names and not set(entry["arg"]) & set(entry["null"])
        assert set(entry["pairs"]) == set(entry["arg"])          # no pair is dropped: one letter per NULL defect, checked on load


def test_the_fixture_holds_refusals_of_both_kinds_for_every_symbol():
    """Every one of the 32 symbols tests a scalar and a pointer, so every one has both kinds."""
    want = load_fixture()
    assert len(SYMBOLS) == 32 and all(s in _lib.PROTOTYPES for s in SYMBOLS)
    assert all(code in LETTER for code in want["all_null"].values())
    for symbol in SYMBOLS:
        e = want["combos"][symbol]
        assert e["arg"] and e["null"], symbol
        assert all(e["pairs"][a].strip(".") for a in e["arg"]), symbol   # at least one pair for every ARG defect the symbol checks
