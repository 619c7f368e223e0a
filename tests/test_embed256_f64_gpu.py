"""The 256-wide instantiations -- ``embed_dim = hidden_dim = 256``, what ``RPODDPG(...)`` / ``RPOSAC(...)`` build by default --
against float64.  Needs an MI355X.

At this width CartSafe and SpringPendulum run rollout_kernel<ENV, 256, 256, 1>, the critic pipelines
cart_{ddpg,sac}_critic_forward_kernel<256, 256> / pend_{ddpg,sac}_critic_front_kernel<256, 256> / pend_critic_back_kernel<256, 256, K>
(fused.hip) and everything else layer by layer through mlp_gemm.h; neither the column-split stages nor the actor pipelines apply.
tests/test_trainer_gpu.py holds the two forms of the rollout and of the critic update to each other within twice what a parent
commit measured; here each is held to float64 on its own.

The update (test_flat_gradient_at_256).  tests/update_f64.py's harness as in tests/test_update_f64_gpu.py -- 64 lanes, five
iterations first, one eager update cut open, everything check_update judges: every element of the critic, shared and actor slices
of flat.grad and of nju.weight.grad, padding exactly 0, the losses, gradmax, x0 / h1 / q / dq layer-locally, RPOSAC's log pi(a'|s')
-- on the generic launches and on the default schedule (critic half: row-tile pipelines; policy half: generic launches, i.e.
gemm_backward_rows and rpo_mlp_backward_pair, whose gradient bound gamma_L |A||B| with the batch chain n + 20 holds for any order of
the sums: mlp_f64.batch_chain), asserted per case.  RPODDPG on CartSafe with the shared embedding and with separate ones, RPOSAC on
CartSafe, both on SpringPendulum; batches of 256, 250 and 100 (SpringPendulum: 256 and 250), and on the default schedule 17 (one
full tile and one row) and 1: the smallest shapes at which the gather, the saved activations and the TD prologue of a ragged tile can
go wrong.  CartSafe's pipelines keep the next actions to themselves: their qn is judged against the target chain recomputed in
float64, pi_targ(s') -> box / Gaussian head -> Complete -> Proj -> Q_targ (update_f64.cart_target_chain: the proposal's interval
carried through the projection at three points and along that path through the target critics), and the TD chain runs from that
value and bound.  SpringPendulum hands its next actions over through memory (_project_batch): qn at them, as at 128.

The rollout (test_rollout_at_256).  rpo_<env>_rollout called on buffers the test owns (sentinels behind every buffer, in every
other ring slot and statistics row), from the state of a trainer three vector steps after reset: RPOSAC on both envs, RPODDPG on
CartSafe, 1 / 17 / 100 lanes, ring slot 3 of 8, and 17 lanes at a ring of 2 steps that has wrapped (slot 1).  Lanes 3 and n - 1
stand one step before the time limit, so the launch resets them.  Judged: the stored actions against float64 from the observation
the launch read (update_f64.rollout_actions: actor -> tanh box + eps_t x the Philox draw, or the Gaussian head at the Philox
draw -> Complete -> Proj, three points); the step layer-locally from the launch's own float32 action (envs_f64.check_cart_step /
check_pend_step: next state, reward, done, the violations of the ring row), the episode words and the auto-reset against the Philox
oracle exactly; the statistics row as a function of the stored rows (check_stats of tests/test_envs_f64_gpu.py); ring rows outside
the step's slot, everything behind a buffer's end and the other statistics rows untouched (the next row: untouched or zero).

Ambiguous rows (a clip, stop or mask decision of the projection that differs over the proposal's interval, or a mask within its
guard): at most AMBIG_CAP (2 %) per comparison, printed per case; tests/test_update_f64.py holds the oracle backend to the cap at
the same seeds, lanes and batches on the CPU.

Worst |err| / bound measured on an MI355X, per group (every case prints its own under -s; the gradient bounds are worst-case
chains over B + 20 additions and the target chain's carries the proposal's interval, so a correct kernel sits far inside them --
the planted errors of tests/test_update_f64.py land at 1.7 to 690 on qn and at 52 on a rollout action):
    CartSafe, generic launches        critic slice 0.00008, shared slice 0.0008, actor slice 0.0003, losses 0.0035, qn 0.00003, dq 0.00006
    CartSafe, default schedule        qn against the target chain 0.00024; from the launch's own qn: critic 0.15 (B = 1; 0.03 at the
                                      larger batches), losses 0.037, dq 0.17; from qn64 and its bound: critic 0.0004, losses 0.00015,
                                      dq 0.0004; shared 0.0021, actor 0.0007
    SpringPendulum, generic / default critic 0.0050 / 0.0054, actor 0.00014 / 0.00027, losses 0.0004, qn 0.00004 / 0.00006, dq 0.17 / 0.20
    layer-local intermediates         x0 0.54, RPOSAC's sampled ap 0.31, completed actions 0.27, log pi 0.18, h1 0.02, q 0.007,
                                      log pi(a'|s') of the pipelines 0.0004, d nu and g_act 0 (no row violates at these seeds)
    rollout                           actions 0.026 (SpringPendulum; CartSafe 0.00012); step: CartSafe violations 0.25, next state 0.25,
                                      accelerations 0.14; SpringPendulum next 0.18, reward 0.17, cos / sin 0.12, violations 0.07 -- of
                                      the limit 4 * C_REF_*
Ambiguous rows per comparison: none in any case.  48 cases, 5.0 s.
"""
import numpy as np
import pytest
import torch

import envs_f64 as ef
import update_f64 as uf
from oracle import philox
from test_envs_f64_gpu import SENT, Buf, bits, check_stats
from test_train_step_golden import build_trainer
from test_update_f64_gpu import _build

pytestmark = pytest.mark.gpu

E256 = dict(embed_dim=256, hidden_dim=256)
PATHS = {"generic": "generic", "row-tile": "split"}          # -> the RPO_SCHEDULE of test_update_f64_gpu.PATHS ("split": the default)
WORST = {}


@pytest.fixture(scope="module")
def hip():
    from rpo_amd import ops
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    yield ops
    print("\nworst |err| / bound over the module:", {k: float("%.3g" % v) for k, v in sorted(WORST.items())})


def _note(worst):
    for k, v in worst.items():
        WORST[k] = max(WORST.get(k, 0.0), float(v))


# ====================================================================================================================== update
CART = [("ddpg", "cart", {}), ("ddpg", "cart", dict(shared_param=False)), ("sac", "cart", {})]
PEND = [("ddpg", "pendulum", {}), ("sac", "pendulum", {})]
MATRIX = [(a, e, p, dict(kw, batch_size=b)) for a, e, kw in CART for p in PATHS for b in (256, 250, 100)] + \
         [(a, e, p, dict(kw, batch_size=b)) for a, e, kw in PEND for p in PATHS for b in (256, 250)] + \
         [(a, e, "row-tile", dict(kw, batch_size=b)) for a, e, kw in CART + PEND for b in (17, 1)]


def _assert_path(tr, snap, path):
    """Which launches ran at this width: the trainers' own switches, and what the harness saw."""
    assert tr.fused.descs["actor"].E == 256 and tr._split_state() is None and not tr._actor_pipeline
    if path == "generic":
        assert snap["path"] == ("generic", "generic") and not tr._pipelines
    else:
        assert snap["path"] == ("row-tile", "generic") and tr._pipelines and tr._rollout_pipeline


@pytest.mark.parametrize("algo,envname,path,kw", MATRIX,
                         ids=["-".join([c[0], c[1], c[2]] + ["%s=%s" % kv for kv in sorted(c[3].items())]) for c in MATRIX])
def test_flat_gradient_at_256(hip, monkeypatch, algo, envname, path, kw):
    tr = _build(hip, monkeypatch, algo, envname, PATHS[path], dict(E256, **kw))
    snap = uf.run_update(tr)
    _assert_path(tr, snap, path)
    worst, info = uf.check_update(tr, snap)
    uf.report("256 wide %s %s %s B=%d" % (algo, envname, path, kw["batch_size"]), worst)
    _note(worst)
    kept = envname == "cart" and path == "row-tile"              # the launch keeps the next actions: qn against the target chain
    assert ("qn target chain" in worst) == kept and ("qn" in worst) == (not kept)
    assert max(worst.values()) <= 1.0


# ===================================================================================================================== rollout
ROLL = [(a, e, n, 8) for a, e in (("sac", "cart"), ("sac", "pendulum"), ("ddpg", "cart")) for n in (1, 17, 100)] + \
       [(a, e, 17, 2) for a, e in (("sac", "cart"), ("sac", "pendulum"), ("ddpg", "cart"))]
STATS_CAP = 8


def _limit(worst, group, value):
    worst[group] = float(value) / ef.tol_c(group)


@pytest.mark.parametrize("algo,envname,n,cap", ROLL, ids=["%s-%s-%d-ring%d" % c for c in ROLL])
def test_rollout_at_256(hip, monkeypatch, algo, envname, n, cap):
    monkeypatch.setenv("RPO_SCHEDULE", "")
    torch.manual_seed(5)
    tr = build_trainer(algo, envname, hip, torch.device("cuda"), fused=True, num_envs=n, use_graph=False, batch_size=16, **E256)
    tr.vec.reset()
    tr.run_steps(3)
    torch.cuda.synchronize()
    assert tr._rollout_pipeline and tr.fused.descs["actor"].E == 256 and tr.fused.descs["actor"].H == 256
    v, k = tr.vec, tr.kernels
    cart = envname == "cart"
    t = int(v.ctrl[0])
    assert t == 3 and t % cap != 0                               # the slot is not 0; a ring of 2 steps has wrapped
    params = uf.read_params(tr)
    st = v.internal.cpu().numpy()
    obs0 = st if cart else v.obs.cpu().numpy()
    max_steps = v.max_episode_steps
    ep_len, ep_ret, ep_count = v.ep_len.cpu().numpy().copy(), v.ep_ret.cpu().numpy(), v.ep_count.cpu().numpy()
    forced = np.zeros(n, bool)
    if n >= 17:
        forced[[3, n - 1]] = True                                # one step before the time limit: the launch resets these lanes
        ep_len[forced] = max_steps - 1
    S, A = Buf(st), Buf(np.full((n, 2), SENT, np.float32))
    O = None if cart else Buf(obs0)
    L, R, C = Buf(ep_len, torch.int32), Buf(ep_ret), Buf(ep_count, torch.int32)
    ring = Buf(np.full((cap * n, k.ring_floats), SENT, np.float32))
    stats = hip.new_stats(STATS_CAP, "cuda")
    stats.fill_(SENT)
    stats[t % STATS_CAP].zero_()
    ctrl = v.ctrl.clone()
    scale, base = tr._box_affine
    k.rollout(tr.fused.descs["actor"], tr._gauss_policy, scale, base, S.view, None if cart else O.view, A.view, L.view, R.view, C.view,
              ring.view, cap, stats, ctrl, hip.NOISE_NONE if tr._gauss_policy else hip.NOISE_PHILOX, tr.eps_start, tr.eps, tr.decay_value,
              tr._box_lo, tr._box_hi, tr.max_steps, tr.corr_lr, tr.corr_eps, tr.corr_momentum, max_steps, True, v.viol_thresh, tr.seed,
              v.env_id_base)
    torch.cuda.synchronize()
    worst = {}
    act, after = A.get(), S.get()                                # (Buf.get: nothing behind the buffer's end was written)
    # ---- actions: float64 from the observation the launch read
    res = uf.rollout_actions(tr, params, torch.from_numpy(obs0), act, t, int(ctrl[2]), v.env_id_base)
    worst["actions"] = res["ratio"]
    worst["ambiguous proj"] = float(res["ambiguous"].mean())
    # ---- the step, layer-locally from the launch's own action
    slot = (t % cap) * n
    allring = ring.get()
    rows = allring[slot:slot + n]
    assert np.all(np.delete(allring, np.s_[slot:slot + n], axis=0) == np.float32(SENT)), "a ring row outside the step's slot was written"
    nlen = ep_len + 1
    if cart:
        table = np.asarray(k.consts, np.float32)
        r, amb = ef.check_cart_step(st, act, table, int(k.partial), rows)
        assert amb.mean() <= ef.AMBIG_CAP
        for g, val in r.items():
            _limit(worst, g, val.max())
        assert np.array_equal(bits(rows[:, 0:6]), bits(st)) and np.array_equal(bits(rows[:, 6:8]), bits(act))
        assert np.all(rows[:, 14] == 1.0) and np.all(rows[:, 23] == 0.0)
        pad = rows[:, 24:]
        assert np.all((pad == 0.0) | (pad == np.float32(SENT)))
        term = ef.cart_terminated_f32(rows[:, 8:14])
        np.testing.assert_array_equal(term, ef.cart_terminated_ref(rows[:, 8:14]))
        done = term | (nlen >= max_steps)
        np.testing.assert_array_equal(rows[:, 15], done.astype(np.float32))
        reward = rows[:, 14]
        fresh = philox.cart_reset(tr.seed, np.arange(n) + v.env_id_base, ep_count + 1)
        assert np.array_equal(bits(after[~done]), bits(rows[~done, 8:14])) and np.array_equal(bits(after[done]), bits(fresh[done]))
        max_ineq, max_eq = np.fmax.reduce(rows[:, 17:23], axis=1), np.abs(rows[:, 16])
    else:
        ref = ef.pend_step(ef.B64, st, act)
        nint = np.stack([ref["nth"].v] + [ref["next"][j].v for j in (2, 3, 4)], axis=1).astype(np.float32)
        # (a done lane's next theta is not stored: its termination from float64, every other lane's from the stored state)
        assert np.all((rows[:, 13] == 0.0) | (rows[:, 13] == 1.0))
        done = rows[:, 13] == 1.0
        term = done & ef.pend_terminated_f32(nint)
        assert not ef.pend_terminated_f32(after[~done]).any() and np.all(nlen[~done] < max_steps)
        assert np.all(((nlen >= max_steps) | term)[done])
        for sel, nth in ((~done, after[~done, 0]), (done, None)):
            if sel.any():
                for g, val in ef.check_pend_step(st[sel], act[sel], rows[sel], nth).items():
                    worst[g] = max(worst.get(g, 0.0), float(val.max()) / ef.tol_c(g))
        assert np.array_equal(bits(rows[:, 2:5]), bits(st[:, 1:4])) and np.array_equal(bits(rows[:, 5:7]), bits(act))
        obs1 = O.get()
        assert np.array_equal(bits(after[~done, 1:]), bits(rows[~done, 9:12]))
        assert np.array_equal(bits(obs1[~done, :2]), bits(rows[~done, 7:9])) and np.array_equal(bits(obs1[:, 2:]), bits(after[:, 1:]))
        reward = rows[:, 12]
        fresh = philox.pendulum_reset(tr.seed, np.arange(n) + v.env_id_base, ep_count + 1)
        assert np.array_equal(bits(after[done]), bits(fresh[done]))
        max_ineq, max_eq = rows[:, 15], np.abs(rows[:, 14])
    assert bool(done[forced].all())
    ret = ep_ret + reward
    np.testing.assert_array_equal(L.get(), np.where(done, 0, nlen))
    assert np.array_equal(bits(R.get()), bits(np.where(done, np.float32(0), ret)))
    np.testing.assert_array_equal(C.get(), ep_count + done)
    # ---- statistics and the control words
    check_stats(hip, stats[t % STATS_CAP], reward, done, term, ret[done], nlen[done], max_ineq, max_eq, v.viol_thresh)
    for row in range(STATS_CAP):
        if row != t % STATS_CAP:
            s = stats[row]
            assert bool((s == SENT).all()) or (row == (t + 1) % STATS_CAP and bool((s == 0).all())), "statistics row %d written" % row
    c = ctrl.cpu().numpy()
    assert c[hip.CONST["RPO_CTRL_T"]] == t + 1 and c[hip.CONST["RPO_CTRL_NONFINITE"]] == 0
    print("rollout 256 wide %s %s n=%d ring=%d: %s" % (algo, envname, n, cap, ", ".join("%s %.3g" % kv for kv in sorted(worst.items()))))
    _note({"rollout " + key: val for key, val in worst.items()})
    assert worst.pop("ambiguous proj") <= ef.AMBIG_CAP
    assert max(worst.values()) <= 1.0
