"""What the env kernel classes of rpo_amd/ops.py (CartSafeKernels, EvopfKernels, PendulumKernels) hand to the library: for every
public method, the symbol called and its argument list.  No GPU and no library: the tensors are duck-typed fakes, ``ops._stream``
is patched and ``_lib.load`` is replaced by a recorder that returns 0.

The expected calls are the ones the classes made BEFORE their per-env method bodies were folded onto one base class, recorded once
by ``tests/golden/make_env_binding_calls.py`` into ``tests/golden/env_binding_calls.json``.

Every argument is normalised against the header's prototype: a pointer becomes the name of the buffer it came from (``NULL`` for
None; the host constant table by identity), a ``byref`` struct its field values, a scalar its value as the prototype's ctypes type
sees it.  An exception becomes its text (``RpoHipError``) or its type (any other).

Cases per (class, method) -- CartSafe once with partial 0 and once with 1:
  * ``all``: every parameter given; ``defaults``: the parameters with a default left out;
  * ``none:<p>``: tensor parameter p None, every one in turn; ``optional_none``: all those None together that the recorded classes
    accepted alone (the fixture names them);
  * ``obs:stride`` / ``obs:1row`` / ``obs:width``: obs a row view with a stride above its width, a 1-row view (every buffer one
    row), a view one column too wide;
  * ``bad:<p>``: a ring of the wrong width, a profile, an act output, an accumulator, a trace or a report of the wrong shape;
and the constructors with a bad constant table.
"""
import ctypes
import inspect
import json
import os

import numpy as np
import pytest
import torch

from rpo_amd import _lib
from rpo_amd import ops

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "env_binding_calls.json")
C = _lib.CONST


class FakeTensor(object):
    """What ops.py asks of a tensor, over an address that is never read"""
    is_cuda, device = True, "fake:0"

    def __init__(self, book, name, shape, dtype=torch.float32, strides=None, ptr=None):
        self.shape, self.dtype = tuple(shape), dtype
        if strides is None:
            strides = [1] * len(shape)
            for i in range(len(shape) - 2, -1, -1):
                strides[i] = strides[i + 1] * shape[i + 1]
        self._strides = tuple(strides)
        self._ptr = book.address(name) if ptr is None else ptr
        book.names[self._ptr] = name

    def dim(self):
        return len(self.shape)

    def numel(self):
        return int(np.prod(self.shape, dtype=np.int64))

    def stride(self, i=None):
        return self._strides if i is None else self._strides[i]

    def is_contiguous(self):
        return FakeTensor(Book(), "", self.shape)._strides == self._strides

    def data_ptr(self):
        return self._ptr


class Book(object):
    """address -> buffer name of one call"""

    def __init__(self):
        self.names, self.next = {}, 0x100000

    def address(self, name):
        self.next += 0x100000
        return self.next

    def name(self, value):
        if isinstance(value, ctypes.c_void_p):
            value = value.value
        return "NULL" if value is None else self.names.get(value, "0x%x" % value)


class FakeDesc(object):
    """An MlpDesc: its struct and -- for evaluate_policies -- its tensors, inside policy 0 of the bank"""

    def __init__(self, book, name, bank_ptr):
        self.tensors = {f: FakeTensor(book, "%s.%s" % (name, f), (4,), ptr=bank_ptr + 64 * (j + 1)) for j, f in enumerate(ops.MlpDesc.FIELDS)}

    def net_struct(self):
        return ops._MlpStruct(*[self.tensors[f].data_ptr() for f in ops.MlpDesc.FIELDS], 6, 0, 128, 256, 1, 0, 1)


DESCS = ("actor_desc", "actor", "actor_target", "critic", "critic_target", "critic1", "critic2", "critic_target1", "critic_target2")
I32, I64, B = torch.int32, torch.int64, 8
SCALARS = dict(gauss=1, scale=0.5, base=0.25, seed=11, env_id_base=3, cap_steps=16, max_episode_steps=200, auto_reset=True,
               viol_thresh=0.001, noise_mode=ops.NOISE_PHILOX, eps_start=0.9, eps_end=0.1, eps_decay=0.01, box_lo=-1.0, box_hi=1.0,
               max_steps=5, corr_lr=0.05, corr_eps=0.0001, corr_momentum=0.5, t0=2, steps=3, form=1, defer_clock=True, salt=5,
               sample_seed=7, sample_salt=9, noise_seed=13, noise_id_base=15, noise_salt=17, deterministic=True, autograd_sign=False,
               overwrite=True, ap_is_raw=True, store_mode=2, dlogp=0.125)


def tensor_shapes(k, n):
    """parameter name -> (shape, dtype) of the good call of n rows"""
    pd, ad = k.partial_dim, k.action_dim
    t = dict(internal=(n, k.internal_dim), obs=(n, k.obs_dim), action=(n, ad), ep_ret=(n,), rows=(16 * n, k.ring_floats),
             stats=(4, ops.STATS_SUB, ops.STATS_LEN), ap_raw=(n * pd,), noise=(n * pd,), proposal=(n, pd), eq_resid=(n, k.eq_num),
             ineq_resid=(n, k.ineq_num), profile=(SCALARS["max_steps"] + 1, n, 4), grad_action=(n, ad), grad_action2=(n, ad),
             grad_action_b=(n, ad), grad_ap=(n * pd,), eq_out=(n, k.eq_num), ineq_out=(n, k.ineq_num), step_out=(n, ad),
             nu=(k.ineq_num,), loss_out=(1,), grad_nu=(k.ineq_num,), acc=(n, ops.EVAL_LEN),
             trace=(3, 1, ops.trace_layout(k.obs_dim, pd, ad)[1]), con=(n, ops.con_width(k.ineq_num, k.eq_num)), lane_lr=(n,),
             bank=(2 - n % 2, 4096), sigma_table=(2 - n % 2, 8), batch_out=(B, k.row_floats), eps_in=(B,), q_out=(B,), qn_out=(B,),
             q1_out=(B,), q2_out=(B,), qn1_out=(B,), qn2_out=(B,), logp_out=(B,), ap_out=(B,), x0_save=(B, 256), h1_save=(B, 256),
             x0_save1=(B, 256), h1_save1=(B, 256), x0_save2=(B, 256), h1_save2=(B, 256), batch_rows=(B, k.row_floats),
             next_actions=(B, 2), ap=(n,), raw=(n, 2 * pd), eps=(n, pd), dap=(n, pd), dout=(n, pd), draw=(n, 2 * pd),
             grad_eq=(n, k.eq_num))
    t = {name: (shape, torch.float32) for name, shape in t.items()}
    t.update({name: ((n,), I32) for name in ("ep_len", "ep_count", "iters", "iters_out", "lane_steps")})
    t.update(ctrl=((ops.CTRL_LEN,), I64), idx_out=((B,), I64), idx_in=((B,), I64), ws=((ops.PROJ_WS_WORDS,), I64))
    return t


def kernel_sets():
    """[(key, class, constructor)]"""
    cart, evopf = np.full(C["RPO_CART_CONSTS_LEN"], 0.5, np.float32), np.full(C["RPO_EVOPF_CONSTS_LEN"], 0.5, np.float32)
    return [("CartSafeKernels/partial=0", ops.CartSafeKernels, lambda: ops.CartSafeKernels(cart, 0)),
            ("CartSafeKernels/partial=1", ops.CartSafeKernels, lambda: ops.CartSafeKernels(cart, 1)),
            ("EvopfKernels", ops.EvopfKernels, lambda: ops.EvopfKernels(evopf)),
            ("PendulumKernels", ops.PendulumKernels, lambda: ops.PendulumKernels())]


def public_methods(cls):
    return sorted(m for m in dir(cls) if not m.startswith("_") and inspect.isfunction(getattr(cls, m)))


def is_tensor(method, p):
    """(evaluate's noise is a (sigma, seed) pair, the other methods' a tensor)"""
    return not (method == "evaluate" and p == "noise") and p not in SCALARS and p not in DESCS and p not in ("n_envs", "group_lanes", "episodes")


class Recorder(object):
    """Stands in for the library: every symbol records its call and answers 0"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, symbol):
        return lambda *args: self.calls.append((symbol, args)) or 0


def normalise(book, symbol, args):
    types = _lib.PROTOTYPES[symbol]
    if len(args) != len(types):
        return ["%d arguments for %d parameters" % (len(args), len(types))]
    out = []
    for a, t in zip(args, types):
        if t is not ctypes.c_void_p:
            try:
                out.append("%s=%r" % (t.__name__, t(a).value))
            except TypeError:
                out.append("%s<-%s" % (t.__name__, type(a).__name__))
        elif hasattr(a, "_obj"):                                 # byref(struct)
            s = a._obj
            out.append("{%s}" % ",".join("%s=%s" % (f, book.name(getattr(s, f)) if ft is ctypes.c_void_p else getattr(s, f))
                                         for f, ft in s._fields_))
        elif a is None or isinstance(a, (int, ctypes.c_void_p)):
            out.append(book.name(a))
        else:
            out.append("?%s" % type(a).__name__)
    return out


def run_case(make, method, case, nulled=()):
    """One call of one case -> {"calls": [[symbol, arguments]]} or {"error": text}"""
    n = 1 if case == "obs:1row" else 8
    book, rec, k = Book(), Recorder(), make()
    book.names[k.consts.ctypes.data if hasattr(k, "consts") else -1] = "consts_host"
    if hasattr(k, "_dev"):
        k._dev[FakeTensor.device] = FakeTensor(book, "consts_dev", (k.consts.size,))
    shapes = tensor_shapes(k, n)
    bank_ptr = book.address("bank")
    sigma = np.full(k.obs_dim, 0.25, np.float32)
    book.names[sigma.ctypes.data] = "sigma_host"
    kwargs = {}
    for p, par in inspect.signature(getattr(k, method)).parameters.items():
        if case == "defaults" and par.default is not inspect.Parameter.empty:
            continue
        if p in DESCS:
            kwargs[p] = FakeDesc(book, p, bank_ptr)
        elif method == "evaluate" and p == "noise":
            kwargs[p] = (sigma, 21)
        elif p in SCALARS:
            kwargs[p] = SCALARS[p]
        elif p in ("n_envs", "group_lanes", "episodes"):
            kwargs[p] = dict(n_envs=n, group_lanes=n // (2 - n % 2), episodes=max(1, n // (2 - n % 2) - 1))[p]
        else:
            shape, dtype = shapes[p]
            strides = None
            if p == "obs" and case == "obs:stride":
                strides = (shape[1] + 3, 1)
            elif p == "obs" and case == "obs:1row":
                strides = (99, 1)
            elif p == "obs" and case == "obs:width":
                shape = (shape[0], shape[1] + 1)
            elif case == "bad:" + p:
                shape = (shape[0] + 1,) + shape[1:] if p != "rows" and p != "trace" else shape[:-1] + (shape[-1] + 1,)
            kwargs[p] = FakeTensor(book, p, shape, dtype, strides, ptr=bank_ptr if p == "bank" else None)
    for p in ([case[5:]] if case.startswith("none:") else nulled):
        kwargs[p] = None
    saved = ops._lib.load, ops._stream
    ops._lib.load, ops._stream = (lambda: rec), (lambda: None)
    try:
        getattr(k, method)(**kwargs)
    except ops.RpoHipError as e:
        return {"error": "RpoHipError: %s" % e}
    except Exception as e:  # noqa: BLE001 -- what a None in place of a tensor the method measures raises: its type is the record
        return {"error": type(e).__name__}
    finally:
        ops._lib.load, ops._stream = saved
    return {"calls": [[symbol, normalise(book, symbol, args)] for symbol, args in rec.calls]}


BAD = ("rows", "profile", "action", "proposal", "iters", "eq_resid", "ineq_resid", "acc", "trace", "con", "lane_steps", "bank",
       "sigma_table")


def cases(cls, method):
    """the case names of a method, ``optional_none`` apart"""
    params = inspect.signature(getattr(cls, method)).parameters
    tensors = [p for p in params if p != "self" and is_tensor(method, p)]
    out = ["all", "defaults"] + ["none:" + p for p in tensors]
    if "obs" in params:
        out += ["obs:stride", "obs:1row", "obs:width"]
    acts = method.startswith("policy_act")
    out += ["bad:" + p for p in tensors if p in BAD and (acts or p not in ("action", "proposal", "iters", "eq_resid", "ineq_resid"))]
    return out


def constructor_errors():
    out = {}
    for name, make in (("CartSafeKernels", lambda t: ops.CartSafeKernels(t, 0)), ("EvopfKernels", lambda t: ops.EvopfKernels(t))):
        for what, table in (("short", np.zeros(3, np.float32)), ("2d", np.zeros((2, 40), np.float32))):
            try:
                make(table)
                out["%s/%s" % (name, what)] = "accepted"
            except ops.RpoHipError as e:
                out["%s/%s" % (name, what)] = "RpoHipError: %s" % e
    return out


def record(optional_of):
    """optional_of(key, method, {case: result}) -> the parameters ``optional_none`` sets to None.  -> the fixture's content"""
    out = {"constructors": constructor_errors(), "methods": {}}
    for key, cls, make in kernel_sets():
        out["methods"][key] = {}
        for method in public_methods(cls):
            got = {case: run_case(make, method, case) for case in cases(cls, method)}
            nulled = optional_of(key, method, got)
            got["optional_none"] = dict(run_case(make, method, "optional_none", nulled), nulled=nulled)
            out["methods"][key][method] = got
    return out


def load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def test_the_classes_make_the_recorded_calls():
    want = load_fixture()
    got = record(lambda key, method, results: want["methods"][key][method]["optional_none"]["nulled"])
    assert got["constructors"] == want["constructors"]
    assert sorted(got["methods"]) == sorted(want["methods"])
    wrong = []
    for key, methods in want["methods"].items():
        assert sorted(got["methods"][key]) == sorted(methods), key      # the public methods of the class: none more, none fewer
        for method, results in methods.items():
            assert sorted(got["methods"][key][method]) == sorted(results), (key, method)
            wrong += [(key, method, case, got["methods"][key][method][case], r) for case, r in results.items()
                      if got["methods"][key][method][case] != r]
    assert not wrong, "%d cases differ (class, method, case, got, recorded): %s" % (len(wrong), wrong[:3])


def test_the_fixture_covers_every_method_both_ways_and_the_refusals():
    want = load_fixture()
    assert sorted(want["methods"]) == sorted(k for k, _, _ in kernel_sets())
    errors = set()
    for key, cls, _ in kernel_sets():
        assert sorted(want["methods"][key]) == public_methods(cls), key
        for method, results in want["methods"][key].items():
            assert "calls" in results["all"] and "calls" in results["optional_none"], (key, method)
            assert all(len(r["calls"]) == 1 for r in results.values() if "calls" in r), (key, method)
            errors |= {r["error"].split(",")[0][:40] for r in results.values() if "error" in r}
    for text in ("RpoHipError: replay ring must be", "RpoHipError: profile must be", "RpoHipError: policy_act: ", "RpoHipError: required tensor is None",
                 "RpoHipError: expected a [n"):
        assert any(e.startswith(text) for e in errors), text
    assert all(v.startswith("RpoHipError: bad ") for v in want["constructors"].values())


def test_the_attributes_the_trainer_reads_stay():
    for key, cls, make in kernel_sets():
        k = make()
        assert all(hasattr(k, a) for a in ("name", "cols", "row_floats", "ring_floats", "partial")), key
        assert hasattr(k, "fused_adds") == (cls is ops.EvopfKernels), key
