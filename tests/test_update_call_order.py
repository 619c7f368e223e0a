"""What the trainers hand to the backend and to the env kernels, call by call, over a few iterations: the ordered list of every
backend / kernels call with its arguments.  No GPU: the trainers run on the CPU through ``tests/oracle_backend.py`` behind a
recording proxy that is handed in as ``backend=`` at construction (so the fused nets, the env kernels, the replay ring and the
optimisers all hold it) and that wraps the kernels object the env builds.

The expected lists are the ones the trainers made BEFORE the update skeleton of ``RPODDPG`` / ``RPOSAC`` was hoisted into
``RPOTrainerBase``, recorded once by ``tests/golden/make_update_call_order.py`` into ``tests/golden/update_call_order.json``.

Per call: the callable's name (``k.<method>`` on the kernels object) and one token per argument -- a tensor becomes
``t<index of first appearance of its storage>:<shape>:<dtype>`` (every recorded tensor is kept alive until the case ends, so an
index names one storage), a descriptor its name in ``fused.descs``, a scalar its value, None stays None, an object a recorded
constructor made (``Td``) the index of that call.

Cases: num_envs=2, warmup=0, ``2 * policy_fre`` iterations through ``run_steps``, then one ``train(t)`` on a policy step.
"""
import inspect
import json
import os

import numpy as np
import pytest
import torch

import oracle_backend as ob
from test_train_step_golden import build_trainer

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "update_call_order.json")

#: name -> (algo, env, fused, extra constructor arguments)
CASES = {}
for _algo in ("ddpg", "sac"):
    for _env in ("cart", "pendulum", "evopf256"):
        # (EVOPF: batch 16 -- the oracle's batched projection of 256 rows takes a second per update; same calls, smaller shapes)
        CASES["%s-%s-fused" % (_algo, _env)] = (_algo, _env, True, dict(batch_size=16) if _env == "evopf256" else {})
CASES.update({
    "ddpg-cart-torch": ("ddpg", "cart", False, {}),
    "sac-pendulum-torch": ("sac", "pendulum", False, {}),
    "ddpgla-cart": ("ddpgla", "cart", False, {}),
    "sacla-pendulum": ("sacla", "pendulum", False, {}),
    "ddpg-pendulum-fused-updates2": ("ddpg", "pendulum", True, dict(updates_per_step=2)),
    "ddpg-cart-fused-fixed": ("ddpg", "cart", True, dict(fixed=True)),
    "sac-cart-fused-auto_alpha": ("sac", "cart", True, dict(automatic_entropy_tuning=True)),
})
#: what `_host_state` adds to the declared names
HOST_EXTRA = {"steps_host", "su", "rider"}


class Recorder(object):
    """Forwards to `inner` (the backend module, or a kernels object under `prefix`) and books every call."""

    def __init__(self, inner, calls, prefix=""):
        self.__dict__.update(_inner=inner, _calls=calls, _prefix=prefix)

    def __getattr__(self, name):
        x = getattr(self._inner, name)                          # (AttributeError: `hasattr` answers as for the backend itself)
        if not (inspect.isroutine(x) or inspect.isclass(x)):
            return x

        def call(*args, **kwargs):
            entry = [self._prefix + name, args, kwargs, None]
            self._calls.append(entry)
            out = x(*args, **kwargs)
            if inspect.isclass(x):                              # (kept: an object handed on later is named by the call that made it)
                entry[3] = out
            return Recorder(out, self._calls, "k.") if inspect.isclass(x) and name.endswith("Kernels") else out
        return call

    def __setattr__(self, name, value):
        setattr(self._inner, name, value)


def tokens(calls, descs):
    """[[name, args, kwargs, object made]] -> ["name(token, ..., key=token)"]"""
    storages, desc_names = {}, {id(d): n for n, d in descs.items()}
    made = {id(c[3]): i for i, c in enumerate(calls) if c[3] is not None}

    def token(a):
        if a is None or isinstance(a, (bool, int, float, str)):
            return repr(a)
        if isinstance(a, torch.Tensor):
            i = storages.setdefault(a.untyped_storage().data_ptr() if a.numel() else ("empty", id(a)), len(storages))
            return "t%d:%s:%s" % (i, "x".join(map(str, a.shape)), str(a.dtype)[6:])
        if id(a) in desc_names:
            return "desc:" + desc_names[id(a)]
        if isinstance(a, np.generic):
            return repr(a.item())
        if isinstance(a, np.ndarray):
            return "ndarray:%s:%s" % ("x".join(map(str, a.shape)), a.dtype)
        if isinstance(a, (list, tuple)):
            return "[%s]" % ",".join(token(x) for x in a)
        if isinstance(a, dict):
            return "{%s}" % ",".join("%s=%s" % (k, token(v)) for k, v in sorted(a.items()))
        if isinstance(a, (torch.device, torch.dtype)):
            return str(a)
        if isinstance(a, Recorder):
            a = a._inner
        return "<%s%s>" % (type(a).__name__, ":call%d" % made[id(a)] if id(a) in made else "")

    return ["%s(%s)" % (name, ",".join([token(a) for a in args] + ["%s=%s" % (k, token(v)) for k, v in sorted(kwargs.items())]))
            for name, args, kwargs, _ in calls]                 # (kwargs by name: their order in the call is not pinned)


def run_case(name, after_construction=None, after_iteration=None):
    """-> the token list of one case; the two hooks see the trainer after construction and after the first iteration."""
    algo, envname, fused, extra = CASES[name]
    torch.set_num_threads(1)
    torch.manual_seed(123)
    calls = []
    tr = build_trainer(algo, envname, Recorder(ob, calls), torch.device("cpu"), fused=fused, num_envs=2, warmup=0,
                       use_graph=False, **extra)
    if after_construction is not None:
        after_construction(tr)
    tr.vec.reset()
    tr.run_steps(1)
    if after_iteration is not None:
        after_iteration(tr)
    tr.run_steps(2 * tr.policy_fre - 1)
    tr.train(2 * tr.policy_fre)
    return tokens(calls, tr.fused.descs if tr.fused is not None else {})


def pack(lists):
    """{case: [call]} -> the fixture: one table of the distinct calls and, per case, the indices into it"""
    table = sorted({c for calls in lists.values() for c in calls})
    at = {c: i for i, c in enumerate(table)}
    return {"table": table, "cases": {name: [at[c] for c in calls] for name, calls in lists.items()}}


def unpack(fixture):
    return {name: [fixture["table"][i] for i in order] for name, order in fixture["cases"].items()}


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return unpack(json.load(f))


def test_every_recorded_case_is_exercised(recorded):
    assert sorted(recorded) == sorted(CASES)
    assert all(len(calls) > 20 for calls in recorded.values())


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_trainers_make_the_recorded_calls(recorded, name):
    from rpo_amd.algo.trainer import RPOTrainerBase
    declared = set(RPOTrainerBase._HOST_STATE_DEFAULTS)
    assert declared == set(RPOTrainerBase._HOST_STATE)

    def host_state_is_the_declared_one(tr):
        assert set(tr._host_state()) - HOST_EXTRA == declared

    got = run_case(name, host_state_is_the_declared_one, host_state_is_the_declared_one)
    want = recorded[name]
    first = next((i for i, (g, w) in enumerate(zip(got, want)) if g != w), min(len(got), len(want)))
    assert got == want, "call %d of %d / %d differs (got, recorded): %s" % (
        first, len(got), len(want), (got[first:first + 1], want[first:first + 1]))
