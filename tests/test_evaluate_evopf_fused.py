"""The host side of the fused EVOPF-v0 evaluation (schedule ``fused_eval_evopf``), without a GPU: the schedule key, the routing
predicate ``fused_evopf_ok`` on stand-in trainers, the oracle backend staying on the stepwise path, and the refusals of
``rpo_evopf_evaluate`` -- host memory as "device" pointers and actors that no call can launch with, so every call returns
before any HIP call."""
import ctypes
import types

import numpy as np
import torch

import oracle_backend as ob
from rpo_amd import _lib
from rpo_amd import ops as hip_ops
from rpo_amd.algo import evaluation
from rpo_amd.algo.trainer import SCHEDULE_DEFAULTS, parse_schedule
from test_train_step_golden import build_trainer


# ------------------------------------------------------------------------------------------------ schedule
def test_schedule_key_defaults_to_off(monkeypatch):
    monkeypatch.delenv("RPO_SCHEDULE", raising=False)
    assert SCHEDULE_DEFAULTS["fused_eval_evopf"] == 0 and parse_schedule()["fused_eval_evopf"] == 0
    assert parse_schedule(dict(fused_eval_evopf=1))["fused_eval_evopf"] == 1
    monkeypatch.setenv("RPO_SCHEDULE", "fused_eval_evopf=1")
    s = parse_schedule()
    assert s["fused_eval_evopf"] == 1 and s["fused_eval"] == 1
    # a constant of its own, whole rounds of the 1024 lanes the chip runs at once under the kernel's geometry
    assert hip_ops.EVOPF_EVAL_LANE_STEPS % 1024 == 0 and 1024 <= hip_ops.EVOPF_EVAL_LANE_STEPS < hip_ops.EVAL_LANE_STEPS


# ------------------------------------------------------------------------------------------------ routing
def _stand_in(**over):
    """What ``fused_evopf_ok`` reads of a trainer, in the state in which it holds."""
    tr = types.SimpleNamespace(schedule=parse_schedule(dict(fused_eval_evopf=1)), device=torch.device("cuda"),
                               fused=types.SimpleNamespace(descs={"actor": types.SimpleNamespace(E=256, H=256)}),
                               backend=hip_ops, kernels=hip_ops.EvopfKernels, _box_affine=None)
    for k, v in over.items():
        setattr(tr, k, v)
    return tr


def test_predicate_holds_and_declines(monkeypatch):
    monkeypatch.delenv("RPO_SCHEDULE", raising=False)
    ok = evaluation.fused_evopf_ok
    assert ok(_stand_in(), 16384) is True
    assert not ok(_stand_in(schedule=parse_schedule()), 10)                                  # the switch is off by default
    assert not ok(_stand_in(schedule=parse_schedule(dict(fused_eval_evopf=1, fused_eval=0))), 10)
    assert not ok(_stand_in(device=torch.device("cpu")), 10)
    assert not ok(_stand_in(), 16385)                              # FusedNets.forward leaves the layer-by-layer launches
    assert not ok(_stand_in(_deterministic=True), 10)              # a Lagrangian baseline: no projection
    assert not ok(_stand_in(fused=None), 10)
    assert not ok(_stand_in(fused=types.SimpleNamespace(descs={"actor": types.SimpleNamespace(E=64, H=64)})), 10)
    assert not ok(_stand_in(kernels=hip_ops.CartSafeKernels, _box_affine=(1.0, 0.0)), 10)
    assert not ok(_stand_in(backend=ob), 10)                       # a backend without `evopf_evaluate`
    assert not ok(_stand_in(), 10, record=2)
    assert not ok(_stand_in(), 10, sigma=np.full(57, 1e-3, np.float32))
    for key in ("mlp_gemm", "gemm_ksplit"):
        with hip_ops.tuning(**{key: 0}):
            assert not ok(_stand_in(), 10)
        assert ok(_stand_in(), 10)
    assert not evaluation.fused_ok(_stand_in())                    # curve mode's predicate does not pick EVOPF up


def test_oracle_backend_stays_stepwise():
    torch.set_num_threads(1)
    torch.manual_seed(5)
    tr = build_trainer("ddpg", "evopf", ob, torch.device("cpu"), num_envs=4, fused=False, use_graph=False)
    assert tr.schedule["fused_eval_evopf"] == 0
    off = tr.evaluate(2, seed=3, horizon=3)
    tr.schedule["fused_eval_evopf"] = 1
    on = tr.evaluate(2, seed=3, horizon=3)
    assert off.path == on.path == "stepwise"
    for f in on.FIELDS:
        np.testing.assert_array_equal(getattr(on, f), getattr(off, f), err_msg=f)


# ------------------------------------------------------------------------------------------------ entry refusals
_RAW = (ctypes.c_char * 1024)()                                  # a 64-byte aligned host buffer stands in for device memory
P = ctypes.c_void_p((ctypes.addressof(_RAW) + 63) // 64 * 64)
OFF4 = ctypes.c_void_p(P.value + 4)                              # float-aligned, not 16-byte aligned
EMPTY = hip_ops._MlpStruct()
NARROW = hip_ops._MlpStruct(*[P.value] * 10, 57, 0, 128, 256, 1, 0, 14)      # a whole actor, but E = 128
ONE_HEAD = hip_ops._MlpStruct(*[P.value] * 10, 57, 0, 256, 256, 1, 0, 14)    # RPODDPG's actor, handed over as gauss = 1


def _call(actor=EMPTY, gauss=0, n=8, p=P, t0=0, steps=1, max_steps=5, newton_iters=50, max_episode_steps=200, con=None):
    return int(_lib.load().rpo_evopf_evaluate(None if actor is None else ctypes.byref(actor), gauss, n, p, p, p, p, p, None, p, t0,
                                              steps, max_steps, 1e-4, 1e-4, 0.0, 1e-5, newton_iters, p, max_episode_steps, 1e-3, 7,
                                              0, con, None))


def test_entry_refusals():
    """The ladder of the evaluation entry points (csrc/evaluate.hip evaluate_entry, csrc/host_glue.h), in its order: "a NULL
    actor_host (RPO_ERR_NULL); n_envs <= 0, steps <= 0, t0 < 0, max_episode_steps <= 0, max_steps < 0, newton_max_iters <= 0
    (RPO_ERR_ARG); a NULL state, action, ep_len, ep_ret, ep_count, acc or consts_dev (RPO_ERR_NULL); a con that is not 16-byte
    aligned (RPO_ERR_ARG); an actor that is not S = 57, E = H = 256 with 14 outputs per head, one head (gauss = 0) or two
    (RPO_ERR_ARG)" (include/rpo_hip.h, rpo_evopf_evaluate).  The actor's shape is the last check, so a call with an empty
    actor and otherwise good arguments is refused there, and none of these calls reaches a launch."""
    ARG, NULL = _lib.CONST["RPO_ERR_ARG"], _lib.CONST["RPO_ERR_NULL"]
    assert "rpo_evopf_evaluate" in _lib.PROTOTYPES
    assert _call(actor=None) == NULL
    assert _call(actor=None, n=0) == NULL                          # the actor comes first
    assert _call(n=0) == ARG and _call(n=-4) == ARG
    assert _call(steps=0) == ARG
    assert _call(t0=-1) == ARG
    assert _call(max_episode_steps=0) == ARG
    assert _call(max_steps=-1) == ARG
    assert _call(newton_iters=0) == ARG
    assert _call(t0=(1 << 24) - 1, steps=2) == ARG                 # step indices stay exact in the float32 row
    assert _call(p=None) == NULL                                   # all env pointers NULL
    assert _call(p=None, n=0) == ARG                               # ... behind the range
    assert _call(con=OFF4) == ARG and _call(actor=ONE_HEAD, con=OFF4) == ARG   # a misaligned report, whatever the actor
    assert _call() == ARG and _call(con=P) == ARG                  # an empty actor
    assert _call(actor=NARROW) == ARG
    assert _call(actor=ONE_HEAD, gauss=1) == ARG
