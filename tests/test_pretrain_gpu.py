"""trainer.pretrain() on an MI355X: the cloning head (rpo_bc_head / rpo_evopf_bc_head) against the float64 restatement of
tests/bc_f64.py, the loop against its five launches issued by hand, one step's gradient against float64 autograd, what the call
leaves alone, graph windows against eager launches, and the whole path on the demonstrations of evaluate_opf().

Tolerance of every comparison with float64: MARGIN (4) * C_REF_* * eps32 * magnitude sum (bc_f64.py), C_REF_* measured on the CPU
(test_pretrain.py).  Every such test prints its worst ratio to that tolerance.  Output buffers are 64 elements too long and
pre-filled; the tail must come back untouched.
"""
import numpy as np
import pytest
import torch

import bc_f64 as bf
from rpo_amd.algo import Demonstrations
from rpo_amd.algo import pretrain as pt
from rpo_amd.algo.agent.flat import FusedAdam
from test_pretrain import chain_inputs, chain_reference
from test_train_step_golden import build_trainer

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
PAD, SENTINEL = 64, -12345.0
SIZES = (1, 15, 16, 17, 257)


@pytest.fixture(scope="module")
def ops():
    from rpo_amd import ops as _ops
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return _ops


@pytest.fixture(scope="module")
def evopf(ops):
    from rpo_amd.env import EVOPFEnv
    return EVOPFEnv(device=DEV).kernels


def dev(x, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).to(DEV)


def strided(x, extra=3):
    """A [n, w] device row view with rows w + extra floats apart (what a column block of a gathered batch is)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    wide = torch.full((x.shape[0], x.shape[1] + extra), SENTINEL, device=DEV)
    wide[:, :x.shape[1]] = dev(x)
    return wide[:, :x.shape[1]]


VARIANTS = [(name, len(lo), bf.const_lohi(lo, hi), lo, hi) for name, (lo, hi) in bf.CONST_BOXES.items()] + \
    [("evopf", 14, bf.evopf_lohi, None, None)]


def run_head(ops, evopf, variant, raw, tgt, st, weights, heads, contiguous=False):
    """One launch of the variant's head -> (draw [n, heads * P], loss_parts [G]) on the CPU; the buffers' tails are checked."""
    name, P, _, lo, hi = variant
    n = tgt.shape[0]
    G = (n + 15) // 16
    dbuf = torch.full((n * heads * P + PAD,), SENTINEL, device=DEV)
    pbuf = torch.full((G + PAD,), SENTINEL, device=DEV)
    draw, parts = dbuf[:n * heads * P].view(n, heads * P), pbuf[:G]
    t = dev(tgt) if contiguous else strided(tgt)
    if name == "evopf":
        ops.evopf_bc_head(evopf, dev(st) if contiguous else strided(st), dev(raw), t, weights, bf.CLIP, draw, parts)
    else:
        ops.bc_head(dev(raw), t, lo, hi, weights, bf.CLIP, draw, parts)
    torch.cuda.synchronize()
    assert bool((dbuf[n * heads * P:] == SENTINEL).all()) and bool((pbuf[G:] == SENTINEL).all()), "wrote past the end of an output"
    return draw.cpu(), parts.cpu()


def box64_of(variant, st):
    name, P, _, lo, hi = variant
    return bf.evopf_box(st) if name == "evopf" else bf.const_box(lo, hi, st.shape[0])


def check_against_f64(tag, variant, raw, tgt, st, weights, heads, draw, parts):
    P = variant[1]
    box = box64_of(variant, st)
    ref = bf.bc_loss(raw, tgt, box[0], box[1], weights, bf.CLIP, heads)
    mags = bf.bc_mags(raw, tgt, box, weights, bf.CLIP)
    rg = bf.worst(draw[:, :P], ref["draw"][:, :P], mags["draw"]) / (bf.MARGIN * bf.C_REF_BC_GRAD)
    rp = bf.worst(parts, ref["parts"], mags["parts"]) / (bf.MARGIN * bf.C_REF_BC_LOSS)
    rl = bf.worst(parts.to(torch.float64).sum(), ref["loss"], mags["loss"]) / (bf.MARGIN * bf.C_REF_BC_LOSS)
    print("%s n=%d: draw %.3f, parts %.3f, loss %.3f of the tolerance" % (tag, tgt.shape[0], rg, rp, rl))
    assert rg <= 1.0 and rp <= 1.0 and rl <= 1.0, (tag, rg, rp, rl)
    if heads == 2:
        assert bool((draw[:, P:] == 0).all()), tag                                        # the log-std half: exactly 0
    dead = ~ref["live"]
    assert bool((draw[:, :P][dead] == 0).all()), tag                                      # empty boxes: exactly 0
    return ref


# ================================================================================================== 1. the head kernels
@pytest.mark.parametrize("heads", (1, 2))
@pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: v[0])
def test_head_against_float64(ops, evopf, variant, heads):
    name, P, box_of = variant[:3]
    raw, tgt, st = bf.all_rows(P, heads, box_of)
    for weights in bf.WEIGHT_SETS[P]:
        tag = "%s/h%d/%s" % (name, heads, "w1" if weights is None else "wz")
        draw, parts = run_head(ops, evopf, variant, raw, tgt, st, weights, heads)
        ref = check_against_f64(tag, variant, raw, tgt, st, weights, heads, draw, parts)
        if name == "evopf":
            assert bool((~ref["live"]).any())                                             # the out-of-band rows are among them
        if weights is not None:
            zero = np.asarray(weights) == 0
            assert bool((draw[:, :P][:, zero] == 0).all())
        again = run_head(ops, evopf, variant, raw, tgt, st, weights, heads)                # the same launch twice: the same bits
        assert torch.equal(draw, again[0]) and torch.equal(parts, again[1])
        dense = run_head(ops, evopf, variant, raw, tgt, st, weights, heads, contiguous=True)   # strides change nothing
        assert torch.equal(draw, dense[0]) and torch.equal(parts, dense[1])
    perm = np.random.RandomState(7).permutation(raw.shape[0])
    for n in SIZES:                                              # ragged groups, one group, several workgroups
        pick = perm[:n]
        d, p = run_head(ops, evopf, variant, raw[pick], tgt[pick], st[pick], None, heads)
        check_against_f64("%s/h%d" % (name, heads), variant, raw[pick], tgt[pick], st[pick], None, heads, d, p)
        assert p.shape == ((n + 15) // 16,)


@pytest.mark.parametrize("variant", [VARIANTS[0], VARIANTS[3]], ids=lambda v: v[0])
def test_head_rows_do_not_see_their_neighbours(ops, evopf, variant):
    name, P, box_of = variant[:3]
    raw, tgt, st = bf.all_rows(P, 1, box_of)
    n = 257
    raw, tgt, st = raw[:n].copy(), tgt[:n].copy(), st[:n].copy()
    draw, parts = run_head(ops, evopf, variant, raw, tgt, st, None, 1)
    keep = np.array([0, 15, 16, 100, 256])
    other = np.ones(n, dtype=bool)
    other[keep] = False
    rng = np.random.RandomState(1)
    raw2, tgt2, st2 = raw.copy(), tgt.copy(), st.copy()
    raw2[other] = rng.randn(int(other.sum()), P).astype(np.float32)                        # every other row is somebody else
    tgt2[other] = tgt[other][::-1]
    st2[other] = st[other][::-1]
    draw2, _ = run_head(ops, evopf, variant, raw2, tgt2, st2, None, 1)
    assert torch.equal(draw[keep], draw2[keep]) and not torch.equal(draw[other], draw2[other])
    # ... and alone: 1 / (n P) of a batch of 16 is 1 / 16 of that of a batch of 1, exactly, so the row's gradient is too
    d16, p16 = run_head(ops, evopf, variant, raw[:16], tgt[:16], st[:16], None, 1)
    for i in (0, 7, 15):
        d1, p1 = run_head(ops, evopf, variant, raw[i:i + 1], tgt[i:i + 1], st[i:i + 1], None, 1)
        assert torch.equal(d1 * (1.0 / 16.0), d16[i:i + 1]), i


def test_head_keeps_a_nan_and_strides_over_many_groups(ops, evopf):
    variant = VARIANTS[3]
    raw, tgt, st = bf.all_rows(14, 2, bf.evopf_lohi)
    raw, tgt, st = raw[:40].copy(), tgt[:40].copy(), st[:40].copy()
    live = bf.bc_loss(raw, tgt, *bf.evopf_box(st)[:2], heads=2)["live"]
    i = int(np.flatnonzero(live.all(dim=1).numpy())[3])
    clean = run_head(ops, evopf, variant, raw, tgt, st, None, 2)
    raw[i, 2] = np.nan
    draw, parts = run_head(ops, evopf, variant, raw, tgt, st, None, 2)
    assert bool(torch.isnan(draw[i, 2])) and bool(torch.isnan(parts[i // 16]))             # not clipped away
    mask = torch.ones_like(draw, dtype=torch.bool)
    mask[i, 2] = False
    assert torch.equal(draw[mask], clean[0][mask]) and int(torch.isnan(parts).sum()) == 1  # ... and nowhere else
    # more groups than the widest grid (2048 workgroups): the second pass of the grid-stride loop
    variant = VARIANTS[0]
    n = 16 * 2048 + 40
    rng = np.random.RandomState(5)
    raw = (1.5 * rng.randn(n, 1)).astype(np.float32)
    tgt = rng.uniform(-1.2, 1.2, (n, 1)).astype(np.float32)
    st = np.zeros((n, 57), dtype=np.float32)
    draw, parts = run_head(ops, evopf, variant, raw, tgt, st, None, 1)
    check_against_f64("unit/h1/big", variant, raw, tgt, st, None, 1, draw, parts)


# ================================================================================================== helpers of the loop tests
def trainer(algo, envname, **kw):
    torch.manual_seed(123)
    kw.setdefault("num_envs", 16)
    kw.setdefault("use_graph", False)
    from rpo_amd import ops as _ops
    tr = build_trainer(algo, envname, _ops, DEV, **kw)
    tr.vec.reset()
    return tr


def demos_for(tr, N, seed=0):
    k = tr.kernels
    if k.partial_dim == 14:
        _, tgt, obs = bf.random_rows(N, 14, 1, bf.evopf_lohi, seed)
    else:
        lo, hi = (np.asarray(v, np.float32).reshape(-1) for v in tr.base_env.box_constraint_partial)
        _, tgt, _ = bf.random_rows(N, k.partial_dim, 1, bf.const_lohi(lo, hi), seed)
        obs = np.random.RandomState(seed + 3).randn(N, k.obs_dim).astype(np.float32)
    return Demonstrations(obs, tgt)


def actor_slice(tr):
    fl = tr.agent.flat
    return fl.param(fl.actor_range)


def by_hand(tr, d, steps, B, lr, idx=None, seed=None, weights=None, clip=0.98):
    """The launches of ``pretrain`` issued one by one through ops / trainer.fused -> the per-step partials [steps, G]."""
    ops, f, ag, k = tr.backend, tr.fused, tr.agent, tr.kernels
    fl = ag.flat
    O, P = k.obs_dim, k.partial_dim
    heads = f.descs["actor"].n_out
    table = d.table(DEV)
    batch = torch.zeros(B, table.shape[1], device=DEV)
    raw = torch.zeros(B, heads * P, device=DEV)
    draw = torch.zeros_like(raw)
    parts = torch.zeros(steps, (B + 15) // 16, device=DEV)
    ctrl = torch.zeros(ops.CTRL_LEN, dtype=torch.int64, device=DEV)
    ctrl[0] = 1
    opt = FusedAdam(ops, fl.param(fl.actor_range), fl.gradient(fl.actor_range), lr, ag.reg, ag.actor_optim.clip_thres)
    opt.zero_grad_after = True
    assert opt.clip_thres > 0
    fl.gradient(fl.actor_range).zero_()
    for s in range(steps):
        if idx is not None:
            ops.replay_gather(table, idx[s], batch)
        else:
            ops.replay_sample_gather(table, 1, len(d), batch, None, seed, pt._SALT_BC, ctrl)
        obs, tgt = batch[:, :O], batch[:, O:O + P]
        f.forward("actor", obs, None, raw, save=True)
        if P == 14:
            ops.evopf_bc_head(k, obs, raw, tgt, weights, clip, draw, parts[s])
        else:
            lo, hi = tr.base_env.box_constraint_partial
            ops.bc_head(raw, tgt, lo, hi, weights, clip, draw, parts[s])
        f.backward("actor", obs, None, draw, gradmax=opt.gradmax)
        opt.step(gradmax_ready=True, clock=ctrl)
    torch.cuda.synchronize()
    assert int(ctrl[0]) == 1 + steps
    return parts.cpu().numpy()


# ================================================================================================== 2. the loop is its launches
@pytest.mark.parametrize("algo,envname,N,B,steps", [("ddpg", "evopf256", 37, 16, 4), ("ddpg", "evopf256", 37, 48, 4),
                                                    ("sac", "evopf256", 37, 16, 4), ("sac", "evopf256", 37, 48, 4),
                                                    ("ddpg", "cart", 5, 16, 3), ("sac", "pendulum", 5, 16, 3)])
def test_the_loop_is_its_launches(algo, envname, N, B, steps):
    a, b = trainer(algo, envname), trainer(algo, envname)
    assert torch.equal(a.agent.flat.data, b.agent.flat.data)
    d = demos_for(a, N)
    idx = torch.from_numpy(np.random.RandomState(3).randint(0, N, size=(steps, B)).astype(np.int64))
    w = None if envname != "evopf256" else bf.WEIGHT_SETS[14][1]
    before = actor_slice(a).clone()
    r = a.pretrain(d, steps=steps, batch_size=B, lr=1e-3, idx=idx, weights=w, sync_targets=False)
    parts = by_hand(b, d, steps, B, 1e-3, idx=idx.to(DEV), weights=w)
    assert torch.equal(actor_slice(a), actor_slice(b)) and not torch.equal(actor_slice(a), before)
    np.testing.assert_array_equal(r.loss, pt.sum_parts(parts))
    assert r.loss.dtype == np.float32 and r.loss.shape == (steps,) and np.all(np.isfinite(r.loss)) and np.all(r.loss > 0)
    assert (r.steps, r.batch_size, r.lr, r.seed, r.rows) == (steps, B, 1e-3, None, N)
    # the drawn form: the same launches with the table's own sampler, keyed by (seed, step)
    r2 = a.pretrain(d, steps=steps, batch_size=B, lr=1e-3, seed=5, weights=w, sync_targets=False)
    parts2 = by_hand(b, d, steps, B, 1e-3, seed=5, weights=w)
    assert torch.equal(actor_slice(a), actor_slice(b)) and r2.seed == 5
    np.testing.assert_array_equal(r2.loss, pt.sum_parts(parts2))


# ================================================================================================== 3. gradient against float64
@pytest.mark.parametrize("algo,envname", [("ddpg", "evopf256"), ("sac", "evopf256"), ("ddpg", "cart")])
def test_gradient_against_float64(algo, envname):
    tr = trainer(algo, envname)
    ops, f, k = tr.backend, tr.fused, tr.kernels
    fl = tr.agent.flat
    desc = f.descs["actor"]
    obs, tgt, box64, _ = chain_inputs(tr)
    loss, grads, mags, _, _ = chain_reference(desc, obs, tgt, box64)
    n, P, heads = obs.shape[0], k.partial_dim, desc.n_out
    o, t = dev(obs), dev(tgt)
    raw = torch.zeros(n, heads * P, device=DEV)
    draw, parts = torch.zeros_like(raw), torch.zeros(1, device=DEV)
    fl.grad.zero_()
    f.forward("actor", o, None, raw, save=True)
    if P == 14:
        ops.evopf_bc_head(k, o, raw, t, None, 0.98, draw, parts)
    else:
        lo, hi = tr.base_env.box_constraint_partial
        ops.bc_head(raw, t, lo, hi, None, 0.98, draw, parts)
    f.backward("actor", o, None, draw)
    torch.cuda.synchronize()
    worst = {key: bf.worst(desc.tensors[key].grad.cpu(), grads[key], mags[key]) / (bf.MARGIN * bf.C_REF_BC_CHAIN) for key in mags}
    print("%s %s: worst ratio to the tolerance per tensor %s; loss %.6g vs %.6g"
          % (algo, envname, {key: round(v, 3) for key, v in worst.items()}, float(parts[0]), float(loss)))
    assert max(worst.values()) <= 1.0, worst
    outside = torch.ones_like(fl.grad, dtype=torch.bool)
    outside[fl.actor_range[0]:fl.actor_range[1]] = False
    assert bool((fl.grad[outside] == 0).all())                   # the backward writes the actor's range alone


# ================================================================================================== 4. isolation
def snapshot(tr):
    ag, v = tr.agent, tr.vec
    fl = ag.flat
    c = fl.actor_range[0]
    s = dict(critic_only=fl.data[:c], behind_actor=fl.data[fl.actor_range[1]:], grad=fl.grad, nju=ag.nju.weight.data,
             lamb=ag.lamb.weight.data, ctrl=v.ctrl, uctrl=tr._uctrl, internal=v.internal, obs=v.obs, ep_len=v.ep_len,
             ep_ret=v.ep_ret, ep_count=v.ep_count, action=v.action, rows=tr.buffer.rows, critic_target=ag.critic_target_flat)
    if ag.actor_target_flat is not None:
        s["actor_target"] = ag.actor_target_flat
    opts = dict(critic=ag.critic_optim, actor=ag.actor_optim, nju=ag.nju_optim, lamb=ag.lamb_optim)
    if getattr(ag, "alpha_optim", None) is not None:
        opts["alpha"] = ag.alpha_optim
    for name, o in opts.items():
        s.update({name + ".exp_avg": o.exp_avg, name + ".exp_avg_sq": o.exp_avg_sq, name + ".step": o.step_dev,
                  name + ".gradmax": o.gradmax})
    torch.cuda.synchronize()
    return {key: t.detach().clone() for key, t in s.items()}


def same(a, b, skip=()):
    return [key for key in a if key not in skip and not torch.equal(a[key].view(torch.uint8) if a[key].dtype.is_floating_point else a[key],
                                                                     b[key].view(torch.uint8) if b[key].dtype.is_floating_point else b[key])]


@pytest.mark.parametrize("algo,envname", [("ddpg", "cart"), ("ddpg", "evopf256"), ("sac", "pendulum")])
def test_pretrain_leaves_everything_else_alone(algo, envname):
    tr = trainer(algo, envname)
    tr.run_steps(8)                                              # moments, counters, replay rows and a gradient buffer worth comparing
    fl, ag = tr.agent.flat, tr.agent
    fl.grad.copy_(torch.randn_like(fl.grad))                     # (the steps leave it zero: make "restored bit for bit" visible)
    d = demos_for(tr, 37)
    calls = getattr(tr, "_evaluate_calls", 0)
    s0, actor0 = snapshot(tr), actor_slice(tr).clone()
    r = tr.pretrain(d, steps=8, batch_size=16, sync_targets=False)
    s1 = snapshot(tr)
    assert same(s0, s1) == [] and not torch.equal(actor0, actor_slice(tr))
    assert r.lr == ag.lr_actor and r.batch_size == 16 and getattr(tr, "_evaluate_calls", 0) == calls
    tr.pretrain(d, steps=8, batch_size=16)                       # sync_targets=True
    s2 = snapshot(tr)
    c = fl.actor_range[0]
    sh = fl.critic_range[1] - c if fl.sizes[1] > 0 else 0
    assert same(s1, s2, skip=("actor_target", "critic_target")) == []
    if ag.actor_target_flat is not None:
        assert torch.equal(ag.actor_target_flat, actor_slice(tr)) and not torch.equal(s1["actor_target"], s2["actor_target"])
    assert torch.equal(s1["critic_target"][:c], s2["critic_target"][:c])                   # the critic-only part of the target stays
    if sh:
        assert envname == "cart"                                 # (shared_param=True)
        assert torch.equal(ag.critic_target_flat[c:c + sh], fl.data[c:c + sh]) and not torch.equal(s1["critic_target"], s2["critic_target"])
    else:
        assert torch.equal(s1["critic_target"], s2["critic_target"])


def test_a_no_op_pretrain_does_not_disturb_training():
    a, b = trainer("ddpg", "cart"), trainer("ddpg", "cart")
    r = a.pretrain(demos_for(a, 5), steps=0, batch_size=16)
    assert r.loss.shape == (0,) and r.steps == 0
    a.run_steps(8)
    b.run_steps(8)
    torch.cuda.synchronize()
    assert same(snapshot(a), snapshot(b)) == [] and torch.equal(a.agent.flat.data, b.agent.flat.data)


# ================================================================================================== 5. graph == eager
def test_graph_windows_equal_eager_launches(monkeypatch):
    monkeypatch.setenv("RPO_GRAPH_AUDIT", "1")
    g, e = trainer("ddpg", "evopf256", use_graph=True), trainer("ddpg", "evopf256", use_graph=False)
    d = demos_for(g, 37)
    start = actor_slice(g).clone()
    rg = g.pretrain(d, steps=40, batch_size=16, seed=3, lr=1e-3)
    re_ = e.pretrain(d, steps=40, batch_size=16, seed=3, lr=1e-3)
    assert torch.equal(actor_slice(g), actor_slice(e)) and not torch.equal(actor_slice(g), start)
    np.testing.assert_array_equal(rg.loss, re_.loss)
    assert rg.graph_node_kinds and re_.graph_node_kinds == []    # a window was captured, and replayed
    for kinds in rg.graph_node_kinds:
        assert set(kinds) == {"kernel"} and kinds["kernel"] >= 5 * 16, kinds
    # the same call on the same initial weights: the same bits; another seed: other minibatches
    end = actor_slice(g).clone()
    for tr in (g, e):
        actor_slice(tr).copy_(start)
    again = g.pretrain(d, steps=40, batch_size=16, seed=3, lr=1e-3)
    other = e.pretrain(d, steps=40, batch_size=16, seed=4, lr=1e-3)
    assert torch.equal(actor_slice(g), end) and not torch.equal(actor_slice(e), end)
    np.testing.assert_array_equal(again.loss, rg.loss)
    assert not np.array_equal(other.loss, rg.loss)
    ops = g.backend
    table, ctrl = d.table(DEV), torch.zeros(ops.CTRL_LEN, dtype=torch.int64, device=DEV)
    ctrl[0] = 1
    drawn = []
    for seed in (3, 4):
        idx = torch.zeros(16, dtype=torch.int64, device=DEV)
        ops.replay_sample_gather(table, 1, 37, torch.zeros(16, table.shape[1], device=DEV), idx, seed, pt._SALT_BC, ctrl)
        drawn.append(idx.cpu())
    assert not torch.equal(drawn[0], drawn[1]) and all(0 <= int(i.min()) and int(i.max()) < 37 for i in drawn)
    # seed=None: a fresh seed per call, from a counter of pretrain's own
    s1 = g.pretrain(d, steps=1, batch_size=16).seed
    s2 = g.pretrain(d, steps=1, batch_size=16).seed
    assert s1 != s2 and s1 == pt.fresh_seed(type("T", (), {"seed": g.seed})())


# ================================================================================================== 6. it learns
def test_it_learns_from_the_opf_controller():
    """The condition is: the mean of the last 20 losses is below the mean of the first 20.  Observed on an MI355X: 382
    demonstrations (2 of the 384 steps dropped), loss 0.36978 -> 0.00874, a ratio of 0.0236."""
    tr = trainer("ddpg", "evopf256")
    b = tr.evaluate_opf(16, seed=1, record=True)
    t = b.trajectory
    d = Demonstrations.from_trajectory(t, tr.base_env, mask=b.opf_converged)
    unconverged = int((t.valid & ~b.opf_converged).sum())
    assert len(d) >= 200 and d.dropped >= unconverged
    kept = np.zeros(t.valid.size, dtype=bool)
    kept[d.index] = True
    assert not bool((kept.reshape(t.valid.shape) & ~b.opf_converged).any())                # every unconverged step is dropped
    np.testing.assert_array_equal(d.target, t.action[kept.reshape(t.valid.shape)][:, tr.base_env.partial_actions])
    r = tr.pretrain(d, steps=200, batch_size=64, lr=1e-3, seed=0)
    first, last = float(r.loss[:20].mean()), float(r.loss[-20:].mean())
    print("pretrain on %d OPF demonstrations (%d dropped): loss %.5f -> %.5f (ratio %.4f)" % (len(d), d.dropped, first, last, last / first))
    assert np.all(np.isfinite(r.loss)) and last < first
    out = tr.act(d.obs[:37])
    torch.cuda.synchronize()
    from rpo_amd import _lib
    assert bool(torch.isfinite(out.action).all()) and bool(torch.isfinite(out.proposal).all())
    assert int(tr.vec.ctrl[_lib.CONST["RPO_CTRL_NONFINITE"]]) == 0
    # the relabelling step on the record's own observations gives the record's targets
    lab = Demonstrations.label(tr.base_env, d.obs)
    assert len(lab) >= 200 and lab.index is not None
    np.testing.assert_array_equal(lab.target, d.target[lab.index])
    np.testing.assert_array_equal(lab.obs, d.obs[lab.index])
