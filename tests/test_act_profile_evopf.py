"""The host side of the one-launch projection profile of EVOPF-v0 (schedule ``profile_evopf``), without a GPU: the schedule key,
the C-ABI entry point ``rpo_evopf_project_profile`` and its refusals, the binding, and the routing of ``act(profile=True)`` on
the oracle backend, which sweeps whatever the switch says.  The kernel itself: tests/test_act_profile_evopf_gpu.py."""
import ctypes
import inspect

import pytest
import torch

import oracle_backend as ob
from rpo_amd import _lib, ops
from rpo_amd.algo.trainer import SCHEDULE_DEFAULTS, parse_schedule
from test_train_step_golden import build_trainer

ARG, NULL = _lib.CONST["RPO_ERR_ARG"], _lib.CONST["RPO_ERR_NULL"]


def test_schedule_key(monkeypatch):
    assert SCHEDULE_DEFAULTS["profile_evopf"] == 0 and parse_schedule()["profile_evopf"] == 0
    assert parse_schedule(dict(profile_evopf=1))["profile_evopf"] == 1
    monkeypatch.setenv("RPO_SCHEDULE", "profile_evopf=1")
    s = parse_schedule()
    assert s["profile_evopf"] == 1 and s["fused_act"] == 1
    monkeypatch.delenv("RPO_SCHEDULE")
    with pytest.raises(ValueError):
        parse_schedule(dict(profile_evopfs=1))
    monkeypatch.setenv("RPO_SCHEDULE", "profile_evopfs=1")
    with pytest.raises(ValueError):
        parse_schedule()


def test_header_declares_the_entry_point_and_the_binding_exists():
    proto = _lib.PROTOTYPES["rpo_evopf_project_profile"]
    assert len(proto) == 16
    assert proto[0] is ctypes.c_int and proto[1] is ctypes.c_void_p and proto[4] is ctypes.c_int and proto[14] is ctypes.c_void_p
    assert _lib.CONST["RPO_ABI_VERSION"] == 6
    # the binding: a function of the backend behind the trainer's EvopfKernels, like ops.evopf_evaluate -- the public methods of the
    # env kernel classes are pinned by tests/test_env_binding_calls.py and stay as they are
    assert callable(ops.evopf_project_profile) and not hasattr(ops.EvopfKernels, "project_profile")
    assert list(inspect.signature(ops.evopf_project_profile).parameters) == [
        "kernels", "obs", "ap_raw", "action", "iters", "max_steps", "corr_lr", "corr_eps", "corr_momentum", "profile", "ap_is_raw"]
    assert list(inspect.signature(ops.PendulumKernels.project_profile).parameters)[1:] == list(
        inspect.signature(ops.evopf_project_profile).parameters)[1:-1]
    assert not hasattr(ob, "evopf_project_profile")              # (the oracle backend has no profile kernel: it sweeps)


def test_routing_on_stand_ins():
    """``acting.profile_kernel``: the kernels' own method wherever there is one, whatever the switch says; on EVOPF-v0 the backend's
    function under the switch only; never on CPU tensors or on a backend without the function."""
    import types
    from rpo_amd.algo.acting import profile_kernel
    evopf = types.SimpleNamespace(name="EVOPF-v0")
    pend = types.SimpleNamespace(name="SpringPendulum-v0", project_profile=lambda *a, **k: "method")
    calls = []
    hip = types.SimpleNamespace(evopf_project_profile=lambda *a, **k: calls.append((a, k)))

    def tr(kernels, on, device="cuda", backend=hip):
        return types.SimpleNamespace(kernels=kernels, schedule=parse_schedule(dict(profile_evopf=on)), device=torch.device(device),
                                     backend=backend)
    assert profile_kernel(tr(evopf, 0)) is None and profile_kernel(tr(evopf, 1, device="cpu")) is None
    assert profile_kernel(tr(evopf, 1, backend=ob)) is None
    assert profile_kernel(tr(pend, 0)) is pend.project_profile and profile_kernel(tr(pend, 1)) is pend.project_profile
    assert profile_kernel(tr(pend, 1, device="cpu")) is None
    fn = profile_kernel(tr(evopf, 1))
    fn("obs", "ap", ap_is_raw=True)
    assert calls == [((evopf, "obs", "ap"), dict(ap_is_raw=True))]


def test_refusals_before_any_hip_call():
    """Host addresses stand in for the device pointers (nothing is dereferenced by a refusal), so never where a GPU is visible.
    A call that got as far as a launch would answer a HIP error code here, neither RPO_ERR_ARG nor RPO_ERR_NULL."""
    if torch.cuda.device_count() != 0:
        pytest.skip("host stand-ins for device pointers: only where no GPU is visible")
    lib = _lib.load()
    buf = (ctypes.c_float * 1024)()
    base = (ctypes.addressof(buf) + 15) // 16 * 16
    r = ctypes.c_void_p(base)
    good = dict(n=4, state=r, state_stride=57, ap_raw=r, ap_is_raw=0, action=r, iters=None, max_steps=2, corr_lr=1e-4,
                corr_eps=1e-5, corr_momentum=0.0, newton_tol=1e-5, newton_max_iters=50, consts_dev=r, profile=r, stream=None)

    def call(**kw):
        return lib.rpo_evopf_project_profile(*dict(good, **kw).values())
    assert call(n=0) == ARG
    assert call(n=-3) == ARG
    assert call(max_steps=-1) == ARG
    assert call(newton_max_iters=0) == ARG
    assert call(state_stride=56) == ARG
    assert call(state=None) == NULL
    assert call(ap_raw=None) == NULL
    assert call(action=None) == NULL
    assert call(consts_dev=None) == NULL
    assert call(profile=None) == NULL
    assert call(profile=ctypes.c_void_p(base + 4)) == ARG        # not 16-byte aligned
    assert call(profile=ctypes.c_void_p(base + 8)) == ARG
    cap = _lib.CONST["RPO_TRACE_MAX_BYTES"]
    assert call(n=cap // (16 * 3) + 1) == ARG                    # one row too many at K = 2
    assert call(n=1 << 28, max_steps=15) == ARG                  # 2^36 bytes: 0 in 32-bit arithmetic
    assert call(n=1, max_steps=(1 << 31) - 1) == ARG             # K + 1 itself must not wrap
    # the arguments are refused in the order the header states: sizes before pointers
    assert call(n=0, state=None) == ARG and call(state=None, profile=ctypes.c_void_p(base + 4)) == NULL


def test_the_oracle_backend_sweeps_whatever_the_switch_says():
    """EVOPF-v0 on the oracle backend (n = 4, K = 2) with ``profile_evopf=1``: the sweep, and the planes of the switch at 0."""
    torch.set_num_threads(1)
    torch.manual_seed(5)
    tr = build_trainer("ddpg", "evopf", ob, torch.device("cpu"), use_graph=False, num_envs=4, fused=False,
                       schedule=dict(profile_evopf=1))
    assert tr.schedule["profile_evopf"] == 1
    tr.vec.reset()
    tr.run_steps(2)
    x = tr.vec.obs[:4].clone()
    on = tr.act(x, profile=True, eval_steps=2)
    assert on.path == "sweep" and on.form is None and tuple(on.profile.data.shape) == (3, 4, 4)
    tr.schedule["profile_evopf"] = 0
    try:
        off = tr.act(x, profile=True, eval_steps=2)
    finally:
        tr.schedule["profile_evopf"] = 1
    assert off.path == "sweep" and torch.equal(on.profile.data, off.profile.data) and torch.equal(on.profile.iters, off.profile.iters)
    for f in on.FIELDS:
        assert torch.equal(getattr(on, f), getattr(off, f)), f
    r = tr.act(x, eval_steps=2)
    assert r.path == "stepwise" and torch.equal(on.action, r.action) and torch.equal(on.profile.action(2), r.action[:, :2])
