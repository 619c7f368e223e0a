"""The host-side validation of the 12 entry points of csrc/fused.hip (the rollouts, the critic forwards / fronts / backs, the actor
pipelines): which return code a refused call gets, that is, which check comes first.  No GPU, and none allowed: a call the
library accepts goes on to a launch -- harmless without a device (a HIP error), a kernel on host addresses with one.  The test
therefore skips where ``/dev/kfd`` exists, and it only makes the calls the fixture names, all of which are refusals.

The expected codes are the ones the library returned BEFORE the entry points were folded onto one body per family, recorded
once by ``tests/golden/make_fused_entry_refusals.py`` into ``tests/golden/fused_entry_refusals.json`` (the encoding of
``split_entry_refusals.json``).

For every symbol -- the four ``rpo_{ddpg,sac}_actor_*`` with env in {0, 1}, the two rollouts with gauss in {0, 1} -- the table
starts from a good call built from the header's prototype (every pointer a 128-byte aligned host buffer, every network and
gradient struct fully populated with the right S / A / E = 128 / H = 256 / n_out) and applies
  * one defect (``defects``): every pointer argument and every network / gradient struct pointer NULL in turn; per network S, A,
    H = 128, E = 64, E = 256 (alone: differing from the other networks of the call; and on all of them), n_out, cat = 1,
    head_dim = 2 and Ws / W0 / W1 / W1b NULL inside the struct; every field of the gradient struct NULL and splitk_scratch at
    +4 bytes; the scalar defects of ``SCALARS``;
  * every pair (ARG defect, NULL defect) of the single defects the recorded library refused with RPO_ERR_ARG and with
    RPO_ERR_NULL: only such a pair shows which of two checks comes first;
  * the call with every argument NULL.
"""
import ctypes
import re

import pytest

from rpo_amd import _lib
from rpo_amd import ops as hip_ops
from test_split_entry_refusals import CODE, HAS_GPU_NODE, LETTER, P, _CONSTS, fixture_rows  # noqa: F401
import test_split_entry_refusals as split_refusals

FIXTURE = split_refusals.FIXTURE.replace("split_entry", "fused_entry")
SYMBOLS = sorted(["rpo_cartsafe_rollout", "rpo_pendulum_rollout", "rpo_cartsafe_ddpg_critic_forward", "rpo_cartsafe_sac_critic_forward",
                  "rpo_pendulum_ddpg_critic_front", "rpo_pendulum_ddpg_critic_back", "rpo_pendulum_sac_critic_front",
                  "rpo_pendulum_sac_critic_back", "rpo_ddpg_actor_forward", "rpo_ddpg_actor_backward", "rpo_sac_actor_forward",
                  "rpo_sac_actor_backward"])
NET_FIELDS, GRAD_FIELDS = hip_ops.MlpDesc.FIELDS, hip_ops.MlpDesc.FIELDS + ("splitk_scratch",)


def _params(symbol):
    """[(name, kind)] of the header's prototype: kind net | grad | ptr, or the ctypes scalar type of _lib.PROTOTYPES"""
    text = re.sub(r"/\*.*?\*/", " ", open(_lib.HEADER).read(), flags=re.S)
    decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % symbol, text).group(1).split(",")
    assert len(decl) == len(_lib.PROTOTYPES[symbol])
    out = []
    for d, t in zip(decl, _lib.PROTOTYPES[symbol]):
        kind = "grad" if "rpo_mlp_grad" in d else "net" if "rpo_mlp" in d else "ptr" if t is ctypes.c_void_p else t
        out.append((d.split()[-1].lstrip("*"), kind))
    return out


PARAMS = {s: _params(s) for s in SYMBOLS}


def variants(symbol):
    """the crossed argument of a symbol: [(key suffix, {argument: value})]"""
    name = "env" if symbol.startswith(("rpo_ddpg_actor", "rpo_sac_actor")) else "gauss" if symbol.endswith("_rollout") else None
    return [("/%s=%d" % (name, v), {name: v}) for v in (0, 1)] if name else [("", {})]


COMBOS = [(symbol, suffix, fixed) for symbol in SYMBOLS for suffix, fixed in variants(symbol)]
GOOD_INT = dict(n_envs=64, batch=256, batch_size=256, cap_steps=1000, stats_cap=8, noise_mode=_lib.CONST["RPO_NOISE_PHILOX"], max_steps=5,
                partial=1, max_episode_steps=200, auto_reset=1)


class Call(object):
    """One call's arguments: the good call of (symbol, env or gauss), its network and gradient structs."""

    def __init__(self, symbol, fixed):
        self.symbol, self.args, self.structs = symbol, {}, {}
        obs = 5 if "pendulum" in symbol or fixed.get("env") == 1 else 6
        twin = fixed.get("gauss", 1 if "_sac_" in symbol else 0)
        for name, kind in PARAMS[symbol]:
            if kind == "net":
                net = self.structs[name] = hip_ops._MlpStruct()
                for f in NET_FIELDS:
                    setattr(net, f, P)
                net.S, net.E, net.H, net.cat, net.head_dim = obs, 128, 256, 0, 1
                net.A, net.n_out = (0, 1 + twin) if name.startswith("actor") else (2, 1)
            elif kind == "grad":
                g = self.structs[name] = hip_ops._MlpGradStruct()
                for f in GRAD_FIELDS:
                    setattr(g, f, P)
            elif kind == "ptr":
                self.args[name] = None if name == "stream" else ctypes.addressof(_CONSTS) if name == "consts_host" else P
            elif kind in (ctypes.c_float, ctypes.c_double):
                self.args[name] = 0.5
            else:
                self.args[name] = fixed.get(name, GOOD_INT.get(name, 1 if kind in (ctypes.c_uint, ctypes.c_ulonglong) else 0))

    def run(self, lib):
        args = [ctypes.addressof(self.structs[n]) if self.structs.get(n) is not None else self.args.get(n) for n, _ in PARAMS[self.symbol]]
        return int(getattr(lib, self.symbol)(*args))


def _arg(**values):
    return lambda c: c.args.update(values)


def _field(names, **values):
    def apply(c):
        for n in names:
            for k, v in values.items():
                setattr(c.structs[n], k, v)
    return apply


SCALARS = dict([("%s=0" % n, {n: 0}) for n in ("batch", "batch_size", "cap_steps", "n_envs", "max_episode_steps", "stats_cap")] +
               [("max_steps=-1", {"max_steps": -1}), ("noise_mode=explicit", {"noise_mode": _lib.CONST["RPO_NOISE_EXPLICIT"]}),
                ("env=2", {"env": 2}), ("partial=2", {"partial": 2})])


def defects(symbol):
    """name -> the edit of a good Call, in the order of the module's docstring"""
    kinds = dict(PARAMS[symbol])
    nets, grads = [n for n, k in PARAMS[symbol] if k == "net"], [n for n, k in PARAMS[symbol] if k == "grad"]
    d = {"%s=NULL" % n: _arg(**{n: None}) for n, k in PARAMS[symbol] if k == "ptr" and n != "stream"}
    d.update(("%s=NULL" % n, (lambda c, n=n: c.structs.__setitem__(n, None))) for n in nets + grads)
    for n in nets:
        actor = n.startswith("actor")
        d["%s.S+1" % n] = lambda c, n=n: setattr(c.structs[n], "S", c.structs[n].S + 1)
        d["%s.A=%d" % (n, 2 if actor else 0)] = _field([n], A=2 if actor else 0)
        d["%s.H=128" % n], d["%s.E=64" % n], d["%s.E=256" % n] = _field([n], H=128), _field([n], E=64), _field([n], E=256)
        d["%s.n_out" % n] = lambda c, n=n: setattr(c.structs[n], "n_out", 3 - c.structs[n].n_out)
        d["%s.cat=1" % n], d["%s.head_dim=2" % n] = _field([n], cat=1), _field([n], head_dim=2)
        d.update(("%s.%s=NULL" % (n, f), _field([n], **{f: None})) for f in ("Ws", "W0", "W1", "W1b"))
    d["nets.E=64"], d["nets.E=256"] = _field(nets, E=64), _field(nets, E=256)
    for g in grads:
        d.update(("%s.%s=NULL" % (g, f), _field([g], **{f: None})) for f in GRAD_FIELDS)
        d["%s.splitk_scratch+4" % g] = _field([g], splitk_scratch=P + 4)
    d.update((name, _arg(**values)) for name, values in SCALARS.items() if all(kinds.get(k) not in (None, "ptr") for k in values))
    return d


def run_rows(rows_of):
    """rows_of(key, names of the single defects) -> the rows to run, each one a tuple of one or two defect names (a pair is applied
    ARG defect first).  -> {key: {row: code}}"""
    lib, out = _lib.load(), {}
    for symbol, suffix, fixed in COMBOS:
        key, d = symbol + suffix, defects(symbol)
        out[key] = {}
        for row in rows_of(key, list(d)):
            c = Call(symbol, fixed)
            for name in row:
                d[name](c)
            out[key][row] = c.run(lib)
    return out


def all_null(lib, symbol):
    """every pointer NULL, every scalar zero"""
    return int(getattr(lib, symbol)(*[None if k in ("net", "grad", "ptr") else 0 for _, k in PARAMS[symbol]]))


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
    assert sorted(want["combos"]) == sorted(symbol + suffix for symbol, suffix, _ in COMBOS)
    for symbol, suffix, _ in COMBOS:
        names, entry = set(defects(symbol)), want["combos"][symbol + suffix]
        assert set(entry["arg"]) <= names and set(entry["null"]) <= names and not set(entry["arg"]) & set(entry["null"])
        assert set(entry["pairs"]) == set(entry["arg"])          # no pair is dropped: one letter per NULL defect, checked on load


def test_the_fixture_holds_refusals_of_both_kinds_for_every_symbol():
    want = load_fixture()
    assert len(SYMBOLS) == 12 and all(s in _lib.PROTOTYPES for s in SYMBOLS)
    assert all(code in LETTER for code in want["all_null"].values())
    for symbol in SYMBOLS:
        entries = [want["combos"][s + suffix] for s, suffix, _ in COMBOS if s == symbol]
        assert all(e["arg"] and e["null"] for e in entries), symbol
        for e in entries:                                        # at least one pair for every ARG defect the symbol checks
            assert all(e["pairs"][a].strip(".") for a in e["arg"]), symbol
