"""The opt-in switch of the 3 x bf16 split-precision streaming forward (include/rpo_hip.h: RPO_TUNE_FWD_BF16X3): the key exists,
is off by default, and sets and restores like every other tuning key.  No GPU: rpo_tuning is host code."""
from rpo_amd import _lib, ops


def test_fwd_bf16x3_key_exists_defaults_to_off_and_restores():
    assert ops.TUNE["fwd_bf16x3"] == _lib.CONST["RPO_TUNE_FWD_BF16X3"] == 9
    assert _lib.CONST["RPO_TUNE_COUNT"] == 10
    lib = _lib.load()
    key = ops.TUNE["fwd_bf16x3"]
    assert lib.rpo_tuning(key, -1) == 0                          # the default: the exact-f32 form
    assert lib.rpo_tuning(key, 1) == 0 and lib.rpo_tuning(key, -1) == 1
    assert lib.rpo_tuning(key, 0) == 1 and lib.rpo_tuning(key, -1) == 0
    with ops.tuning(fwd_bf16x3=1):
        assert ops.tuning.get("fwd_bf16x3") == 1
        assert ops.tuning.get("fwd_stream") == 1                 # (no other key moves)
    assert ops.tuning.get("fwd_bf16x3") == 0
