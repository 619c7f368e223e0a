"""The host-side validation of the 25 ``rpo_split_*`` entry points: which return code a refused call gets, that is, which check
comes first.  No GPU, and none allowed: the stages have no common last check that every row fails, so a call the library
accepts goes on to a launch -- harmless without a device (a HIP error), a kernel on host addresses with one.  The test
therefore skips where ``/dev/kfd`` exists, and it only makes the calls the fixture names, all of which are refusals.

The expected codes are the ones the library returned BEFORE the entry points were folded onto one body per stage family,
recorded once by ``tests/golden/make_split_entry_refusals.py`` into ``tests/golden/split_entry_refusals.json``.

For every symbol, env in {0, 1} and twin in {0, 1} the table starts from a fully populated struct (``Call``) and applies
  * one defect: every pointer field / network / gradient struct NULL in turn, the scalar defects of ``scalar_defects`` and, for
    the ``_ride`` symbols, the rider defects of ``rider_defects``;
  * every pair (ARG defect, NULL defect) of the single defects the recorded library refused with RPO_ERR_ARG and with
    RPO_ERR_NULL: only such a pair shows which of two checks comes first;
  * the call with every argument NULL.
"""
import ctypes
import json
import os

import pytest

from rpo_amd import _lib
from rpo_amd import ops as hip_ops

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "split_entry_refusals.json")
HAS_GPU_NODE = os.path.exists("/dev/kfd")

_RAW = (ctypes.c_char * 4096)()                                  # a 128-byte aligned host buffer stands in for device memory
P = (ctypes.addressof(_RAW) + 127) // 128 * 128
_CONSTS = (ctypes.c_float * 64)(*[0.5] * 64)                     # consts_host: read on the host by every CartSafe stage

NETS = ("actor", "actor_target", "critic1", "critic2", "critic_target1", "critic_target2")
CRITICS = NETS[2:]
GRADS = ("critic1_grad", "critic2_grad", "actor_grad")
SYMBOLS = sorted(s for s in _lib.PROTOTYPES if s.startswith("rpo_split_"))
COMBOS = [(symbol, env, twin) for symbol in SYMBOLS for env in (0, 1) for twin in (0, 1)]
CODE = {"A": _lib.CONST["RPO_ERR_ARG"], "N": _lib.CONST["RPO_ERR_NULL"]}
LETTER = {v: k for k, v in CODE.items()}


def _pointer_fields(struct, skip=()):
    return [n for n, t in struct._fields_ if t is ctypes.c_void_p and n not in skip]


U_POINTERS = _pointer_fields(hip_ops._SplitUpdateStruct, NETS + GRADS + ("consts_host",))
R_POINTERS = _pointer_fields(hip_ops._RolloutRiderStruct)


def rides(symbol):
    return len(_lib.PROTOTYPES[symbol]) == 3


class Call(object):
    """One call's arguments: the good struct of (env, twin), its six networks, three gradient structs and a good rider."""

    def __init__(self, env, twin):
        u = self.u = hip_ops._SplitUpdateStruct()
        for name in U_POINTERS:
            setattr(u, name, P)
        for j in range(3):
            u.prep2_step[j] = P
        u.env, u.twin, u.batch, u.cap_steps, u.n_envs, u.max_steps = env, twin, 256, 1000, 64, 5
        u.rollout_stats_cap, u.proj_store_mode = 8, 1
        u.consts_host, u.partial = ctypes.addressof(_CONSTS), 1
        self.nets, self.grads = {}, {}
        for name in NETS:
            net = self.nets[name] = hip_ops._MlpStruct()
            for f in hip_ops.MlpDesc.FIELDS:
                setattr(net, f, P)
            net.S, net.E, net.H, net.cat, net.head_dim = (6 if env == 0 else 5), 128, 256, 0, 1
            net.A, net.n_out = (2, 1) if name in CRITICS else (0, 1 + twin)
        for name in GRADS:
            g = self.grads[name] = hip_ops._MlpGradStruct()
            for f in hip_ops.MlpDesc.FIELDS + ("splitk_scratch",):
                setattr(g, f, P)
        r = self.r = hip_ops._RolloutRiderStruct()
        for name in R_POINTERS:
            setattr(r, name, P)
        r.n_envs, r.gauss, r.cap_steps, r.stats_cap, r.noise_mode = 64, twin, 1000, 8, _lib.CONST["RPO_NOISE_PHILOX"]
        r.max_steps, r.max_episode_steps, r.lane_begin, r.lane_end = 5, 200, 0, 64
        self.rider_null = False
        self._link()

    def _link(self):
        for name, s in list(self.nets.items()) + list(self.grads.items()):
            setattr(self.u, name, ctypes.addressof(s))

    def copy(self):
        def dup(s):
            return type(s).from_buffer_copy(s)
        c = Call.__new__(Call)
        c.u, c.r, c.rider_null = dup(self.u), dup(self.r), self.rider_null
        c.nets, c.grads = {k: dup(v) for k, v in self.nets.items()}, {k: dup(v) for k, v in self.grads.items()}
        c._link()
        return c

    def run(self, lib, symbol):
        rider = ((None if self.rider_null else ctypes.byref(self.r)),) if rides(symbol) else ()
        args = (ctypes.byref(self.u),) + rider + (None,)
        return int(getattr(lib, symbol)(*args))


def _set(target, **values):
    def apply(c):
        s = getattr(c, target) if target in ("u", "r") else c.nets[target]
        for k, v in values.items():
            setattr(s, k, v)
    return apply


def _other_env(c):
    """the good struct of the other env (front, mid and pfront serve one env only)"""
    c.u.env = 1 - c.u.env
    for net in c.nets.values():
        net.S = 6 if c.u.env == 0 else 5


def scalar_defects(twin):
    d = {"batch=%d" % b: _set("u", batch=b) for b in (0, 257, 1025)}
    d["env=2"], d["env=other"] = _set("u", env=2), _other_env
    d.update(("%s.H=128" % n, _set(n, H=128)) for n in NETS)
    d.update(("%s.A=0" % n, _set(n, A=0)) for n in CRITICS)
    d["partial=2"], d["consts_host=NULL"] = _set("u", partial=2), _set("u", consts_host=None)
    d["max_steps=-1"], d["max_steps=31"] = _set("u", max_steps=-1), _set("u", max_steps=31)
    d["cap_steps=0"], d["n_envs=0"], d["rollout_stats_cap=0"] = _set("u", cap_steps=0), _set("u", n_envs=0), _set("u", rollout_stats_cap=0)
    d["shared_embedding=1"] = _set("u", shared_embedding=1)
    d["proj_ws+64"], d["proj_store_mode=3"] = _set("u", proj_ws=P + 64), _set("u", proj_store_mode=3)
    return d


def rider_defects(twin):
    d = {"r=NULL": lambda c: setattr(c, "rider_null", True)}
    d.update(("r.%s=NULL" % n, _set("r", **{n: None})) for n in R_POINTERS)
    d["r.n_envs=0"], d["r.max_episode_steps=0"], d["r.max_steps=-1"] = _set("r", n_envs=0), _set("r", max_episode_steps=0), _set("r", max_steps=-1)
    d["r.noise_mode=explicit"] = _set("r", noise_mode=_lib.CONST["RPO_NOISE_EXPLICIT"])
    d["r.gauss!=twin"] = _set("r", gauss=1 - twin)
    d["r.cap_steps=0"], d["r.stats_cap=0"] = _set("r", cap_steps=0), _set("r", stats_cap=0)
    d["r.lane_begin=-16"], d["r.lane_begin=8"] = _set("r", lane_begin=-16), _set("r", lane_begin=8)
    d["r.lane_end<lane_begin"] = _set("r", lane_begin=32, lane_end=16)
    d["r.lane_end>n_envs"], d["r.lane_end=24"] = _set("r", lane_end=80), _set("r", lane_end=24)
    return d


def defects(symbol, twin):
    """name -> the edit of a good Call, in the order of the module's docstring"""
    d = {"%s=NULL" % n: _set("u", **{n: None}) for n in U_POINTERS + list(NETS + GRADS)}
    d.update(("prep2_step[%d]=NULL" % j, (lambda c, j=j: c.u.prep2_step.__setitem__(j, None))) for j in range(3))
    d.update(scalar_defects(twin))
    if rides(symbol):
        d.update(rider_defects(twin))
    return d


def combo_key(symbol, env, twin):
    return "%s/env=%d/twin=%d" % (symbol, env, twin)


def run_rows(rows_of):
    """rows_of(key, names of the single defects) -> the rows to run, each one a tuple of one or two defect names (a pair is applied
    ARG defect first).  -> {key: {row: code}}"""
    lib, out = _lib.load(), {}
    for symbol, env, twin in COMBOS:
        key, good, d = combo_key(symbol, env, twin), Call(env, twin), defects(symbol, twin)
        out[key] = {}
        for row in rows_of(key, list(d)):
            c = good.copy()
            for name in row:
                d[name](c)
            out[key][row] = c.run(lib, symbol)
    return out


def all_null(lib, symbol):
    return int(getattr(lib, symbol)(*[None] * len(_lib.PROTOTYPES[symbol])))


def fixture_rows(entry):
    """the rows of one fixture entry {"arg": [...], "null": [...], "pairs": {arg defect: a letter per NULL defect}} -> {row: code}"""
    rows = {(n,): CODE["A"] for n in entry["arg"]}
    rows.update(((n,), CODE["N"]) for n in entry["null"])
    for a, letters in entry["pairs"].items():
        assert len(letters) == len(entry["null"])
        rows.update(((a, n), CODE[ch]) for n, ch in zip(entry["null"], letters) if ch != ".")
    return rows


def load_fixture():
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
    assert sorted(want["combos"]) == sorted(combo_key(*c) for c in COMBOS)
    for symbol, env, twin in COMBOS:
        names, entry = set(defects(symbol, twin)), want["combos"][combo_key(symbol, env, twin)]
        assert set(entry["arg"]) <= names and set(entry["null"]) <= names and not set(entry["arg"]) & set(entry["null"])
        assert set(entry["pairs"]) <= set(entry["arg"])


def test_the_fixture_holds_refusals_of_both_kinds_for_every_symbol():
    want = load_fixture()
    assert len(SYMBOLS) == 25
    assert all(code in LETTER for code in want["all_null"].values())
    for symbol in SYMBOLS:
        entries = [want["combos"][combo_key(s, env, twin)] for s, env, twin in COMBOS if s == symbol]
        assert any(e["arg"] for e in entries) and any(e["null"] for e in entries), symbol
        for e in entries:                                        # at least one pair for every ARG defect the symbol checks
            assert not e["null"] or all(e["pairs"].get(a, "").strip(".") for a in e["arg"]), symbol
