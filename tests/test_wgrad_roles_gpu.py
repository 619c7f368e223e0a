"""The all-rows launches of the column-split update (rpo_split_critic_bwd_b, rpo_split_policy_e) with their hidden-vector
blocks staged in LDS (``rpo_tuning(RPO_TUNE_WGRAD_STAGED, 1)``, the default) against the form that fetches the operands with one
wave (key 0): the same chains over the same rows in the same order, so every bit the update leaves must be the same.  Needs an MI355X.

Per case the trainer is built twice from the same seeds (64 lanes, five iterations first so that a policy step has happened and
the ring holds data), once under each value of the key, and one eager update is cut open (update_f64.run_update):
``flat.grad`` after the critic half and after the policy half (which holds ``nju.weight.grad``, asserted on its own slice too), both
losses and both gradmax slots are ``torch.equal`` / ``==`` between the two builds, and the staged build passes
update_f64.check_update (every element within its float64 bound).

Batch sizes: the smallest shapes at which the staging can go wrong -- 1 (three of the four batch ranges are empty), 3, 17 (ragged
against the 16-row tile), 100, 255 and 256 (the edge of one staging pass of 64 rows per range), 257 and 272 (a second pass with an
almost empty tail), 1024 (four passes, the largest batch the stages take).  No batch is skipped for any case: the trainer chooses
the front launches by itself where the dispatcher's placement allows them (ops.front_launch_ok) and one launch per stage elsewhere.

One more case runs 20 iterations in hipGraph windows (RPO_GRAPH_CYCLE=8) under each value of the key: the parameters and the replay
ring are bit-identical (RPODDPG with the shared embedding: the plain launches; RPOSAC: K = 2 and the two-head pol_e, with the
rollout riding on the critic update's launches -- rpo_split_critic_bwd_b_ride itself keeps the one-wave form under either value).
"""
import pytest
import torch

import update_f64 as uf
from test_train_step_golden import build_trainer

pytestmark = pytest.mark.gpu

CASES = [("ddpg", "cart", {}), ("ddpg", "cart", dict(shared_param=False)), ("sac", "cart", {}), ("sac", "pendulum", {})]
BATCHES = (1, 3, 17, 100, 255, 256, 257, 272, 1024)
MATRIX = [(a, e, kw, b) for a, e, kw in CASES for b in BATCHES]
IDS = ["-".join([a, e] + ["%s=%s" % kv for kv in sorted(kw.items())] + ["B=%d" % b]) for a, e, kw, b in MATRIX]


@pytest.fixture(scope="module")
def hip():
    from rpo_amd import ops
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    assert ops.TUNE["wgrad_staged"] == 11 and ops.tuning.get("wgrad_staged") == 1
    return ops


def _snapshot(hip, algo, envname, kw, batch, staged):
    with hip.tuning(wgrad_staged=staged):
        torch.manual_seed(5)
        tr = build_trainer(algo, envname, hip, torch.device("cuda"), fused=True, num_envs=64, use_graph=False, batch_size=batch, **dict(kw))
        tr.vec.reset()
        tr.run_steps(5)
        torch.cuda.synchronize()
        snap = uf.run_update(tr)
        torch.cuda.synchronize()
    assert snap["path"] == ("split", "split"), snap["path"]
    return tr, snap


@pytest.mark.parametrize("algo,envname,kw,batch", MATRIX, ids=IDS)
def test_staged_roles_leave_the_same_bits(hip, algo, envname, kw, batch):
    tr0, s0 = _snapshot(hip, algo, envname, kw, batch, 0)
    tr1, s1 = _snapshot(hip, algo, envname, kw, batch, 1)
    for x, y in zip(s0["cols"], s1["cols"]):
        assert torch.equal(x, y), "the two builds sampled different batches"
    for k in ("grad_c", "grad_a"):
        assert torch.equal(s0[k], s1[k]), (k, float((s0[k] - s1[k]).abs().max()))
    lo, hi = s1["nu_off"]
    assert torch.equal(s0["grad_a"][lo:hi], s1["grad_a"][lo:hi])
    assert torch.equal(uf._cpu(tr0.agent.nju.weight.grad), uf._cpu(tr1.agent.nju.weight.grad))
    assert s0["loss_c"] == s1["loss_c"] and s0["loss_a"] == s1["loss_a"], (s0["loss_c"], s1["loss_c"], s0["loss_a"], s1["loss_a"])
    assert torch.equal(s0["parts_c"], s1["parts_c"])
    assert s0["gradmax_c"] == s1["gradmax_c"] and s0["gradmax_a"] == s1["gradmax_a"]
    assert s1["gradmax_c"] is not None and s1["gradmax_a"] is not None
    worst, _ = uf.check_update(tr1, s1)
    uf.report("%s %s %s B=%d staged" % (algo, envname, kw, batch), worst)
    assert max(worst.values()) <= 1.0


@pytest.mark.parametrize("algo,kw", [("ddpg", {}), ("sac", {})], ids=["ddpg-shared", "sac-ride"])
def test_graph_windows_leave_the_same_parameters_and_ring(hip, monkeypatch, algo, kw):
    monkeypatch.setenv("RPO_GRAPH_CYCLE", "8")
    out = []
    for staged in (1, 0):
        with hip.tuning(wgrad_staged=staged):
            torch.manual_seed(5)
            tr = build_trainer(algo, "cart", hip, torch.device("cuda"), fused=True, num_envs=64, use_graph=True, **dict(kw))
            tr.vec.reset()
            tr.run_steps(20)
            torch.cuda.synchronize()
            assert tr._split_state() is not None
            out.append((tr.agent.flat.data.clone(), tr.buffer.rows.clone()))
    assert torch.equal(out[0][0], out[1][0]), float((out[0][0] - out[1][0]).abs().max())
    assert torch.equal(out[0][1], out[1][1])
