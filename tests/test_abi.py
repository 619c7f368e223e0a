"""The C-ABI library loads and exports every symbol include/rpo_hip.h declares (no GPU needed, no compute calls)."""
import ctypes
import os
import subprocess
import sys

import pytest

from rpo_amd import _lib, ops


def test_header_parses():
    protos, consts = _lib.parse_header()
    assert len(protos) >= 20
    for must in ("rpo_cartsafe_step", "rpo_cartsafe_act_project", "rpo_pendulum_step", "rpo_replay_sample_gather",
                 "rpo_td_huber", "rpo_adam_step", "rpo_cartsafe_lagrangian", "rpo_abi_version"):
        assert must in protos
    assert consts["RPO_CART_ROW"] == 24 and consts["RPO_PEND_ROW"] == 16 and consts["RPO_CART_RING"] == 32 and consts["RPO_PEND_RING"] == 16 and consts["RPO_ERR_ARG"] == -1
    # spot-check the type mapping
    assert protos["rpo_polyak"] == [ctypes.c_longlong, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p]


def test_library_exports_every_declared_symbol():
    if not os.path.exists(_lib.LIBRARY):
        from rpo_amd.csrc import build
        build.build(verbose=False)
    lib = _lib.load()
    for name in _lib.PROTOTYPES:
        assert hasattr(lib, name), name
    assert lib.rpo_abi_version() == _lib.CONST["RPO_ABI_VERSION"]
    # nothing torch-typed in the dynamic symbol table: the boundary is plain C
    syms = subprocess.run(["nm", "-D", "--defined-only", _lib.LIBRARY], capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in syms.splitlines() if " T " in line}
    assert set(_lib.PROTOTYPES) <= exported
    # ... and nothing else: the dynamic symbol table IS the header (internal cross-unit functions are visibility("hidden"))
    assert exported == set(_lib.PROTOTYPES), sorted(exported - set(_lib.PROTOTYPES))


def test_argument_validation_without_gpu():
    """Argument checks run before any HIP call, so they can be exercised on a CPU-only box."""
    lib = _lib.load()
    assert lib.rpo_polyak(0, None, None, 0.5, None) == _lib.CONST["RPO_ERR_ARG"]
    assert lib.rpo_polyak(4, None, None, 0.5, None) == _lib.CONST["RPO_ERR_NULL"]
    assert lib.rpo_replay_gather(None, 32, 23, 4, None, None, None) == _lib.CONST["RPO_ERR_ARG"]   # row not 16-B multiple
    assert lib.rpo_replay_gather(None, 16, 24, 4, None, None, None) == _lib.CONST["RPO_ERR_ARG"]   # ring stride < row
    with pytest.raises(_lib.RpoHipError):
        _lib.check(-1, "x")


def test_ops_refuse_cpu_tensors():
    import torch
    from rpo_amd import ops
    with pytest.raises(_lib.RpoHipError):
        ops.polyak(torch.zeros(4), torch.zeros(4), 0.5)


def test_struct_layouts_match_the_compiler(tmp_path):
    """The ctypes mirrors of the header's structs (rpo_split_update, rpo_adam_seg, rpo_mlp, rpo_td) have the compiler's
    size and field offsets: a C program that includes include/rpo_hip.h prints them, gcc only."""
    import torch  # noqa: F401  (rpo_amd.ops imports it)
    from rpo_amd import ops
    structs = {"rpo_split_update": ops._SplitUpdateStruct, "rpo_adam_seg": ops._AdamSegStruct, "rpo_mlp": ops._MlpStruct,
               "rpo_mlp_grad": ops._MlpGradStruct, "rpo_td": ops._TdStruct, "rpo_rollout_rider": ops._RolloutRiderStruct}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % _lib.HEADER, "int main(void) {"]
    for cname, st in structs.items():
        lines.append('printf("%s size %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in st._fields_:
            lines.append('printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines += ["return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    seen = 0
    for line in out.splitlines():
        cname, field, value = line.split()
        st = structs[cname]
        if field == "size":
            assert ctypes.sizeof(st) == int(value), (cname, ctypes.sizeof(st), value)
        else:
            assert getattr(st, field).offset == int(value), (cname, field)
        seen += 1
    assert seen > 120


def test_split_update_stages_validate_arguments():
    lib = _lib.load()
    stages, ride_stages = ops.SplitUpdate.STAGES, ops.SplitUpdate.RIDE_STAGES
    exported = {n: len(a) for n, a in _lib.PROTOTYPES.items() if n.startswith("rpo_split_")}      # (u, stream) | (u, rider, stream)
    assert sorted("rpo_split_" + s for s in stages) == sorted(n for n, k in exported.items() if k == 2)
    assert sorted("rpo_split_" + s + "_ride" for s in ride_stages) == sorted(n for n, k in exported.items() if k == 3)
    for stage in stages:
        assert getattr(lib, "rpo_split_" + stage)(None, None) == _lib.CONST["RPO_ERR_NULL"]
    assert lib.rpo_xcc_probe(8, 16, 4, 256, None, None) == _lib.CONST["RPO_ERR_NULL"]
    assert lib.rpo_xcc_probe(0, 16, 4, 256, None, None) == _lib.CONST["RPO_ERR_ARG"]
    for stage in ride_stages:                                        # the riding rollout halves: both structs are required
        assert getattr(lib, "rpo_split_" + stage + "_ride")(None, None, None) == _lib.CONST["RPO_ERR_NULL"]
    assert _lib.CONST["RPO_ABI_VERSION"] == 6


def test_every_entry_point_survives_null_arguments():
    """Every `int rpo_*(...)` of the header called (a) with all-zero arguments and (b) with sizes = 4, scalars = 1 and NULL
    pointers: the validation in front of every launch must answer RPO_ERR_ARG / RPO_ERR_NULL (or, at worst, a HIP error code
    from a launch attempt on a box without a GPU) -- never dereference a NULL host pointer.  Run under ASan + UBSan by
    tests/test_sanitizers.py."""
    lib = _lib.load()
    skip = {"rpo_abi_version", "rpo_tuning", "rpo_mlp_supported", "rpo_mlp_split_supported"}    # (predicates: 0 = "no")
    assert lib.rpo_mlp_supported(0, 0, 0) == 0 and lib.rpo_mlp_split_supported(None) == 0
    bad = {}
    for name, argtypes in _lib.PROTOTYPES.items():
        if name in skip:
            continue
        fn = getattr(lib, name)
        for fill in (0, 4):
            args = []
            for t in argtypes:
                if t is ctypes.c_void_p:
                    args.append(None)
                elif t is ctypes.c_float:
                    args.append(float(fill and 1.0))
                else:
                    args.append(fill)
            rc = fn(*args)
            if rc == 0:
                bad[(name, fill)] = rc
    assert not bad, "entry points that report success on NULL / empty arguments: %s" % bad
    # the switch table: unknown keys are refused, a query does not change the value
    assert lib.rpo_tuning(-1, 1) == _lib.CONST["RPO_ERR_ARG"] and lib.rpo_tuning(_lib.CONST["RPO_TUNE_COUNT"], 1) == _lib.CONST["RPO_ERR_ARG"]
    was = lib.rpo_tuning(_lib.CONST["RPO_TUNE_BWD_ONEPASS"], -1)
    assert lib.rpo_tuning(_lib.CONST["RPO_TUNE_BWD_ONEPASS"], 0) == was and lib.rpo_tuning(_lib.CONST["RPO_TUNE_BWD_ONEPASS"], was) == 0
    assert lib.rpo_tuning(_lib.CONST["RPO_TUNE_BWD_ONEPASS"], -1) == was



_MISALIGNED_CHILD = r"""
import ctypes, sys
import torch
from rpo_amd import _lib, ops
if torch.cuda.device_count() != 0:                # (host addresses stand in for device pointers: never where a GPU is visible)
    sys.exit(3)
lib = _lib.load()
S, A, E, H, n = 6, 2, 128, 256, 20000
buf = (ctypes.c_float * (1 << 16))()
base = (ctypes.addressof(buf) + 15) // 16 * 16
p = [base + 4096 * i for i in range(10)]        # (distinct, 16-byte aligned host addresses; nothing is dereferenced)
critic = ops._MlpStruct(p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], None, None, S, A, E, H, 1, 0, 1)
actor = ops._MlpStruct(p[0], p[1], None, None, p[4], p[5], p[6], p[7], None, None, S, 0, E, H, 1, 0, 1)
gactor = ops._MlpStruct(p[0], p[1], None, None, p[4], p[5], p[6], p[7], p[8], p[9], S, 0, E, H, 2, 0, 1)
bad = ops._MlpGradStruct(*p[:8], p[8], p[9], base + 4, 1 << 24)
good = ops._MlpGradStruct(*p[:8], p[8], p[9], base + 16, 1 << 24)
r = ctypes.c_void_p(base)
res = {}
one = (n, r, 16, r, 16, r, r, r, r, r, None)
pair = (n, r, 16, r, 16, r, r, r, r, r, None, r, r, r, r, r, None)
# default switches, and the rows pass + split-K weights pass, whose rows kernel is launched BEFORE the scratch is zeroed: only
# a refusal in the argument validation answers RPO_ERR_ARG there -- a launch on this GPU-less process answers a HIP error
for key, tune in (("default", {}), ("two_pass", dict(bwd_stream=0, bwd_onepass=0))):
    with ops.tuning(**tune):
        res["backward_" + key] = lib.rpo_mlp_backward(ctypes.byref(critic), ctypes.byref(bad), *one, 1, 0, None, None, None)
        res["pair_" + key] = lib.rpo_mlp_backward_pair(ctypes.byref(critic), ctypes.byref(bad), ctypes.byref(critic),
                                                       ctypes.byref(bad), *pair, 1, 0, None, None, None, None)
        res["pair_second_" + key] = lib.rpo_mlp_backward_pair(ctypes.byref(critic), ctypes.byref(good), ctypes.byref(critic),
                                                              ctypes.byref(bad), *pair, 1, 0, None, None, None, None)
# the fused actor backward entry points (their weights pass is launched after the actor kernel)
res["ddpg_actor"] = lib.rpo_ddpg_actor_backward(0, ctypes.byref(actor), ctypes.byref(bad), ctypes.byref(critic), 0, r, n, r, r, r,
                                                r, r, 1.0, 1.0, 0.0, -1.0, 1.0, 1.0, 0.0, r, r, 1, r, r, r, r, r, r, r, r, r,
                                                r, r, r, r, None, None)
res["sac_actor"] = lib.rpo_sac_actor_backward(0, ctypes.byref(gactor), ctypes.byref(bad), ctypes.byref(critic), ctypes.byref(critic),
                                              0, r, n, r, r, r, r, r, r, r, 0.1, -1.0, 1.0, 1.0, 0.0, r, 1, r, r, r, r, r, r, r,
                                              r, r, r, r, r, r, r, r, r, r, r, None, None)
print(res)
sys.exit(0 if all(v == _lib.CONST["RPO_ERR_ARG"] for v in res.values()) else 1)
"""


def test_misaligned_splitk_scratch_is_refused_before_any_launch():
    """rpo_mlp_grad.splitk_scratch must be 16-byte aligned (it is zeroed with float4 stores; a hipMemsetAsync fallback would put
    a memset node into a captured window).  rpo_mlp_backward, rpo_mlp_backward_pair (either network) and the fused
    rpo_ddpg_actor_backward / rpo_sac_actor_backward answer RPO_ERR_ARG in their argument validation, before any launch.
    Host buffers stand in for the device pointers, so the calls run in a child process that sees no GPU: a launch there
    fails with a HIP error instead of touching memory, and that error is what a missing up-front check would return."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _MISALIGNED_CHILD], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
