"""``agent.flat.grad`` between the backward launches and the optimiser step, on every update path of the trainers, against the
float64 chain of tests/update_f64.py.  Needs an MI355X.

One eager update with a policy step is cut open (update_f64.run_update: 64 lanes, five iterations first so that one policy step
has happened and the ring holds data): flat.grad.zero_() and _critic_update | read | _critic_step(True) | _actor_update | read.
Per case (update_f64.check_update): every element of the critic, shared and actor slices and of nju.weight.grad within its bound
(FlatParams.offset), padding floats and the other optimiser's private slice exactly 0, last_losses within theirs, gradmax equal to
max |slice| where the backward left it, the launches' intermediates (x0 / h1 / q / qn / dq, ap_det or the Gaussian heads and log pi,
the completed actions, g_act; RPOSAC's log pi(a'|s') on every path, on EVOPF-v0 the sampled ap' as well) layer-locally within
float64, ambiguous rows (relu(g), clip seams, min(Q1, Q2)) under AMBIG_CAP.

Paths, chosen with RPO_SCHEDULE and asserted per case: the generic launches, the row-tile pipelines (fused.hip), the column-split
stages (nsplit.hip) with the front launches and with one launch per stage.  CartSafe's row-tile pipelines and split stages complete
and project the next actions inside the launch that evaluates the target critics and do not export them (SpringPendulum's hand
them over through memory: wrapped _project_batch, split.next_actions): their qn is judged against the target chain recomputed in
float64 (update_f64.cart_target_chain; the TD chain runs from that value and bound), and their q / qn are held bit for bit to the
generic launches' on the same parameters, ring and draws as well; the split stages with and without front launches leave the same
bits in flat.grad after each half.  The 256-wide networks: tests/test_embed256_f64_gpu.py.

Worst |err| / bound measured on an MI355X, per group (every case prints its own under -s; the gradient bounds are worst-case
chains over B + 20 additions, so a correct kernel sits far inside them -- the planted errors of test_update_f64.py, 0.4 % of a
gradient, land at 13 to 580):
    CartSafe, generic launches       critic slice 0.0002, shared slice 0.0002, actor slice 0.0006, losses 0.0014, log_alpha 0.01
    CartSafe, row-tile pipelines     critic 0.026, shared 0.0002, actor 0.0006, losses 0.024 (the TD chain from the launch's own qn, which
                                     is judged against the target chain: 0.0005; from qn64 and its bound: critic 0.001, losses 0.0001)
    CartSafe, split, front / none    critic 0.026, shared 0.0002, actor 0.0004, losses 0.023, log_alpha 0.01
    SpringPendulum, every path       critic 0.00006, actor 0.0004 (split 0.0003), d nu 0.05, losses 0.0009
    *_viol, row-tile and split       critic 0.025 / 0.007, actor 0.0011 / 0.0026, d nu 0.0026 / 0.0013 (cart / pendulum)
    EVOPF-v0 RPODDPG, generic chain  critic 0.00002, actor 0.0009, d nu 0.028, losses 0.0004 (64 rows and 50)
    EVOPF-v0 RPOSAC, generic chain   critic 0.00003, actor 0.0015 (alpha = 0.2: 0.019, the log-std head), d nu 0.05, losses 0.0035
                                     (alpha = 0.2: 0.010), log_alpha 0.01; log pi and log pi(a'|s') 0.06, the sampled ap and ap' 0.056,
                                     g_act 0.26 (50 rows), the basic components of the completed actions equal to the head's ap.
                                     At alpha = 0.2 every row's TD error lies beyond the Huber clamp (alpha log pi(a'|s') is about 10,
                                     the rewards -1 to -3): dq is +-1 / B exactly, and the critic slices do not depend on log pi there;
                                     at the script's alpha = 0.001 they do
    layer-local intermediates        x0 0.63, RPOSAC's sampled ap 0.28, completed actions 0.26, g_act 0.23, dq 0.21, log pi 0.18,
                                     log pi(a'|s') of the pipelines 0.0008 (its bound carries the heads' forward bound), the rest below 0.05
Ambiguous rows per comparison: none for relu(g) and the clip seams, at most 0.4 % (one row of 256) for min(Q1, Q2); none left out.
102 cases, 6.3 s; the slowest case 0.6 s.
"""
import pytest
import torch

import update_f64 as uf
from test_train_step_golden import build_trainer

pytestmark = pytest.mark.gpu

PATHS = {"generic": "fused_critic=0,fused_actor=0", "row-tile": "split=0", "split": "", "split-nofront": "front=0"}
_SNAPS = {}


@pytest.fixture(scope="module")
def hip():
    from rpo_amd import ops
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return ops


def _build(hip, monkeypatch, algo, envname, path, kw, steps=5):
    monkeypatch.setenv("RPO_SCHEDULE", PATHS[path])
    torch.manual_seed(5)
    tr = build_trainer(algo, envname, hip, torch.device("cuda"), fused=True, num_envs=64, use_graph=False, **dict(kw))
    tr.vec.reset()
    tr.run_steps(steps)
    torch.cuda.synchronize()
    return tr


def _assert_path(hip, tr, snap, path):
    """Which launches ran: the trainers' own switches, and what the harness saw."""
    su = tr._split_state()
    want = {"generic": ("generic", "generic"), "row-tile": ("row-tile", "row-tile")}.get(path, ("split", "split"))
    assert snap["path"] == want, (path, snap["path"])
    if path == "generic":
        assert not tr._pipelines and not tr._actor_pipeline
    elif path == "row-tile":
        assert tr._pipelines and tr._actor_pipeline and su is None
    else:
        assert tr._pipelines and tr._actor_pipeline and su is not None and int(su.st.batch) == tr.batch_size
        front = bool(tr._front_ok())
        assert front == (path == "split" and hip.front_launch_ok(tr.batch_size, tr.sac)), (path, front)


def _case(hip, monkeypatch, algo, envname, path, kw):
    """Snapshot and verdict of one case, computed once (the front / no-front equality reads the same snapshots)."""
    key = (algo, envname, path, tuple(sorted(kw.items())))
    if key not in _SNAPS:
        tr = _build(hip, monkeypatch, algo, envname, path, kw)
        snap = uf.run_update(tr)
        _assert_path(hip, tr, snap, path)
        worst, info = uf.check_update(tr, snap)
        keep = {k: snap[k] for k in ("grad_c", "grad_a", "loss_c", "loss_a", "log_alpha_grad", "nu_off", "path")}
        _SNAPS[key] = (keep, worst, info)
    return _SNAPS[key]


def _ids(cases):
    return ["-".join([c[0], c[1], c[2]] + ["%s=%s" % kv for kv in sorted(c[3].items())]) for c in cases]


CART = [("ddpg", "cart", {}), ("ddpg", "cart", dict(shared_param=False)), ("sac", "cart", {})]
PEND = [("ddpg", "pendulum", {}), ("sac", "pendulum", {})]
MATRIX = [(a, e, p, dict(kw, batch_size=b)) for a, e, kw in CART for p in PATHS for b in (256, 250, 100)] + \
         [(a, e, p, dict(kw, batch_size=b)) for a, e, kw in PEND for p in PATHS for b in (256, 250)] + \
         [(a, e, p, dict(kw, batch_size=272)) for a, e, kw in PEND for p in ("split", "split-nofront")]


@pytest.mark.parametrize("algo,envname,path,kw", MATRIX, ids=_ids(MATRIX))
def test_flat_gradient_matches_float64(hip, monkeypatch, algo, envname, path, kw):
    """RPODDPG on CartSafe with the shared embedding (the headline) and with separate ones, RPOSAC on CartSafe, both on
    SpringPendulum with the reference's batched projection; generic launches, row-tile pipelines, split stages with and without
    front launches; batches of 256, 250 and 100 rows (ragged against the 16-row tile; SpringPendulum: 256 and 250) and, on the
    split stages, 272 (17 tiles: the one-workgroup form of the batch projection)."""
    snap, worst, info = _case(hip, monkeypatch, algo, envname, path, kw)
    uf.report("%s %s %s B=%d" % (algo, envname, path, kw["batch_size"]), worst)
    assert max(worst.values()) <= 1.0


VIOL = [(a, e, p, {}) for a, e in (("ddpg", "cart_viol"), ("ddpg", "pendulum_viol")) for p in ("row-tile", "split")]


@pytest.mark.parametrize("algo,envname,path,kw", VIOL, ids=_ids(VIOL))
def test_flat_gradient_with_violated_constraints(hip, monkeypatch, algo, envname, path, kw):
    """The ``*_viol`` hyper-parameters of test_train_step_golden.HP (large exploration noise, non-zero initial multipliers):
    the Lagrangian's d/d action and d/d nu are not zero -- at least one and not all rows of the batch violate."""
    snap, worst, info = _case(hip, monkeypatch, algo, envname, path, kw)
    uf.report("%s %s %s" % (algo, envname, path), worst)
    viol = info["violating"]
    assert 0 < int(viol.sum()) < viol.size
    assert float(abs(info["gnu"]).max()) > 0.0
    off = snap["nu_off"]
    assert float(snap["grad_a"][off[0]:off[1]].abs().max()) > 0.0
    assert max(worst.values()) <= 1.0


@pytest.mark.parametrize("path", ["generic", "split"])
def test_log_alpha_gradient(hip, monkeypatch, path):
    """RPOSAC on CartSafe with automatic_entropy_tuning: log_alpha.grad = -(mean log pi + H_target) beside the other slices."""
    snap, worst, info = _case(hip, monkeypatch, "sac", "cart", path, dict(automatic_entropy_tuning=True))
    uf.report("sac cart %s automatic_entropy_tuning" % path, worst)
    assert "log_alpha" in worst and snap["log_alpha_grad"] != 0.0
    assert max(worst.values()) <= 1.0


def _kw_id(kw):
    return "-".join("%s=%s" % kv for kv in sorted(kw.items()))


@pytest.mark.parametrize("kw", [dict(batch_size=64), dict(batch_size=50)], ids=_kw_id)
def test_evopf_flat_gradient_matches_float64(hip, monkeypatch, kw):
    """RPODDPG on EVOPF-v0 at the script's network sizes (256 -> 256, a concatenating critic, a 14-wide actor head): the generic
    chain with the kernels' fused adds (rpo_evopf_lagrangian overwrites, rpo_evopf_complete_bwd adds the Lagrangian's d/d action),
    a batch of 64 and one of 50 (ragged against the 16 rows per workgroup of the head kernels and the row tile of mlp_gemm)."""
    snap, worst, info = _case(hip, monkeypatch, "ddpg", "evopf256", "generic", kw)
    uf.report("ddpg evopf256 generic B=%d" % kw["batch_size"], worst)
    assert getattr(hip.EvopfKernels, "fused_adds", False)
    assert 0 < int(info["violating"].sum()) and float(abs(info["gnu"]).max()) > 0.0
    assert max(worst.values()) <= 1.0


# (the cases of tests/test_update_f64.py, which runs them on the oracle backend first: the ambiguous shares are known there)
NJU = dict(batch_size=64, init_nju=0.1)
EVOPF_SAC = [NJU, dict(batch_size=50, init_nju=0.1), dict(NJU, alpha=0.2), dict(NJU, automatic_entropy_tuning=True),
             dict(batch_size=64), dict(batch_size=64, init_nju=0.0)]


@pytest.mark.parametrize("kw", EVOPF_SAC, ids=_kw_id)
def test_evopf_sac_flat_gradient_matches_float64(hip, monkeypatch, kw):
    """RPOSAC on EVOPF-v0 (scripts/evopf_exp_sac.py's sizes: 256 -> 256, two concatenating critics, two 14-wide actor heads) on
    the generic chain, as the trainer composes it: the squashed-Gaussian head in the state-dependent box, log pi summed over 14
    components into the TD prologue of both critics, rpo_min_q_bwd's split of -1 / B between the two mlp_gemm backward passes,
    the three-way add (da1 + da2) + g_act inside rpo_evopf_complete_bwd, the head's backward with alpha / B.  Non-zero
    multipliers (the Lagrangian's d/d action and d/d nu are not zero: asserted), 64 rows and a ragged 50, alpha = 0.2 beside
    the script's 0.001 (where alpha / B d log pi is 1e-6 of the other terms), automatic_entropy_tuning, and multipliers of zero."""
    snap, worst, info = _case(hip, monkeypatch, "sac", "evopf256", "generic", kw)
    uf.report("sac evopf256 generic %s" % _kw_id(kw), worst)
    assert getattr(hip.EvopfKernels, "fused_adds", False)
    for key in ("ambiguous min", "ambiguous seam", "ambiguous relu(g)"):
        assert worst[key] <= uf.AMBIG_CAP, (key, worst[key])
    if kw.get("init_nju"):
        off = snap["nu_off"]
        assert int(info["violating"].sum()) > 0 and float(abs(info["gnu"]).max()) > 0.0 and info["g_act"] > 0.0
        assert float(snap["grad_a"][off[0]:off[1]].abs().max()) > 0.0
    if kw.get("automatic_entropy_tuning"):
        assert "log_alpha" in worst and snap["log_alpha_grad"] != 0.0
    assert max(worst.values()) <= 1.0


FRONT = [(a, e, dict(kw, batch_size=256)) for a, e, kw in CART + PEND]


@pytest.mark.parametrize("algo,envname,kw", FRONT, ids=["-".join([c[0], c[1]] + ["%s=%s" % kv for kv in sorted(c[2].items())]) for c in FRONT])
def test_front_launches_leave_the_same_gradient_bits(hip, monkeypatch, algo, envname, kw):
    """The split stages with the front launches against one launch per stage (front=0): flat.grad bit for bit after the critic
    half and after the policy half -- the equality test_trainer_gpu.py states on the parameters after Adam, on the gradient."""
    assert hip.front_launch_ok(256, algo == "sac")
    a = _case(hip, monkeypatch, algo, envname, "split", kw)[0]
    b = _case(hip, monkeypatch, algo, envname, "split-nofront", kw)[0]
    assert torch.equal(a["grad_c"], b["grad_c"]), float((a["grad_c"] - b["grad_c"]).abs().max())
    assert torch.equal(a["grad_a"], b["grad_a"]), float((a["grad_a"] - b["grad_a"]).abs().max())
    assert a["loss_c"] == b["loss_c"] and a["loss_a"] == b["loss_a"]


EQUAL = [(a, dict(kw, batch_size=b)) for a, _, kw in CART for b in (256, 250, 100)]


@pytest.mark.parametrize("algo,kw", EQUAL, ids=["-".join([c[0]] + ["%s=%s" % kv for kv in sorted(c[1].items())]) for c in EQUAL])
@pytest.mark.parametrize("path", ["row-tile", "split", "split-nofront"])
def test_cart_targets_equal_the_generic_launches(hip, monkeypatch, path, algo, kw):
    """CartSafe's row-tile critic pipeline and its split stages keep the next actions inside the launch, so their qn cannot be held
    against float64 at them (above it is held against the recomputed target chain, whose bound carries the proposal's interval).
    Beside that: q and qn (and dq, and RPOSAC's log pi(a'|s')) of those launches are bit for bit those of the
    generic launches -- whose next actions and qn ARE held against float64 above -- on the same parameters, targets and ring
    (copied over) and the same Philox draws (same seed and clock: the sampled batch is asserted equal); every CartSafe case of
    the matrix above: shared and separate embeddings, RPOSAC, 256 / 250 / 100 rows."""
    a = _build(hip, monkeypatch, algo, "cart", path, kw)
    b = _build(hip, monkeypatch, algo, "cart", "generic", kw)
    b.agent.flat.data.copy_(a.agent.flat.data)
    b.agent.critic_target_flat.copy_(a.agent.critic_target_flat)
    if a.agent.actor_target_flat is not None:
        b.agent.actor_target_flat.copy_(a.agent.actor_target_flat)
    b.buffer.rows.copy_(a.buffer.rows)
    assert torch.equal(a.vec.ctrl, b.vec.ctrl) and torch.equal(a._uctrl, b._uctrl)
    sa, sb = uf.run_update(a, critic_only=True), uf.run_update(b, critic_only=True)
    assert sa["path"][0] == path.split("-nofront")[0] and sb["path"][0] == "generic"
    for x, y in zip(sa["cols"], sb["cols"]):
        assert torch.equal(x, y), "the two paths sampled different batches"
    if algo == "sac":
        assert torch.equal(sa["rec"]["logp_next"], sb["rec"]["logp_next"]) and torch.equal(sa["rec"]["eps_next"], sb["rec"]["eps_next"])
    for ca, cb in zip(sa["critic"], sb["critic"]):
        for k in ("q", "qn", "dq"):
            assert torch.equal(ca[k], cb[k]), (k, float((ca[k] - cb[k]).abs().max()))
