#!/usr/bin/env python
"""Benchmark of the RPO hot path on MI355X: env-steps/s of RPODDPG on CartSafe-v0 with 4096 vectorised envs per GPU
(BASELINE.json configs[1]), one constrained policy update of batch 256 per vector step (the reference's cadence,
rpo/algo/rpo_ddpg.py:160-161).

    python bench.py [--gpus N --steps K --warmup W] [--full]          # N > 1: starts N ranks itself (torch.distributed.run)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

A "step" is one vector step: actor forward on N lanes -> noise + equation solver + GRG projection -> fused env step +
violation bookkeeping + replay scatter -> sample/gather 256 transitions -> critic (and every 4th step actor + dual)
update.  Rank 0 prints ONE JSON line; everything else goes to stderr.

A plain run does only what the headline needs: set up, warm up, time the steps, --dump-outputs, print the line.  --full
adds everything else: the CPU baseline, the cart_sac leg, the vector-cadence and num_envs = 1 violation rates, the lanes
sweep, the rollout-only / UTD-matched / large-batch legs and the kernel clinics (roofline); --no-cpu-baseline, --no-clinic,
--no-extras, --n1-seeds and --lanes trim a --full run.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ENVS_PER_GPU = 4096
HBM_PEAK_GBS = 8000.0                      # MI355X HBM3E spec peak, /opt/skills/guides/MI355X_MICROARCH.md
HBM_ACHIEVABLE_GBS = 6290.0                # what a device-to-device copy reaches on this part (same guide; measured here too)
LLC_BYTES = 256 * 2 ** 20                  # Infinity Cache: a working set below this is served from the LLC, not from HBM
MFMA_F32_PEAK_TFLOPS = 157.3               # v_mfma_f32_16x16x4_f32 == the f32 vector peak (MI355X_MICROARCH.md)
HP = dict(batch_size=256, max_steps=10, warmup=0, lr_dual=0.2, corr_lr=2e-2, eps=1.0, eps_start=1.0, lr_actor=1e-4,
          lr_critic=3e-4, eps_epoch=20000, eval_lr=2e-2, eval_steps=50, grad_eps=0.1, corr_momentum=0.0, policy_fre=4,
          capacity=20000, shared_param=True, value_type="add", clip_thres=0.2, embed_dim=128,
          hidden_dim=256)        # scripts/cart_exp.py:26-28


def log(*a):
    print(*a, file=sys.stderr, flush=True)


# the other scripts' hyper-parameters, for --workload
WORKLOADS = {
    "cart_ddpg": ("cart", "ddpg", {}),
    "cart_sac": ("cart", "sac", dict(eps=5e-3, eps_start=5e-3, shared_param=False, alpha=0.1, automatic_entropy_tuning=False)),
    "pen_ddpg": ("pen", "ddpg", dict(lr_dual=0.01, corr_lr=2e-3, eval_lr=2e-3, eps=0.5, eps_start=0.5, shared_param=False)),
    "pen_sac": ("pen", "sac", dict(lr_dual=0.01, corr_lr=2e-3, eval_lr=2e-3, eps=1e-2, eps_start=1e-2, shared_param=False,
                                   alpha=0.01, automatic_entropy_tuning=False)),
    # BASELINE.json configs[4]: EVOPF-v0, RPODDPG, 1024 envs on one MI355X (scripts/evopf_exp.py:29-31)
    "evopf_ddpg": ("evopf", "ddpg", None),
    # scripts/evopf_exp_sac.py:30-33
    "evopf_sac": ("evopf", "sac", dict(lr_actor=1e-4, lr_critic=3e-4, grad_eps=0.1, fixed=False, init_lamb=0.0, init_nju=0.0,
                                       alpha=0.001, automatic_entropy_tuning=False)),
}
EVOPF_HP = dict(batch_size=256, max_steps=10, warmup=0, lr_dual=2e-2, corr_lr=1e-4, eps=0.0001, eps_start=0.0001,
                eps_epoch=20000, eval_lr=1e-4, eval_steps=50, grad_eps=0.02, corr_momentum=0.0, policy_fre=4,
                ex_action_dim=1, gamma=0.95, capacity=20000, clip_thres=0.2, shared_param=False, value_type="cat")
DESCRIBE = {
    "cart_ddpg": "CartSafe-v0 RPODDPG (scripts/cart_exp.py)", "cart_sac": "CartSafe-v0 RPOSAC (scripts/cart_exp_sac.py)",
    "pen_ddpg": "SpringPendulum-v0 RPODDPG (scripts/pen_exp.py)", "pen_sac": "SpringPendulum-v0 RPOSAC (scripts/pen_exp_sac.py)",
    "evopf_ddpg": "EVOPF-v0 RPODDPG (scripts/evopf_exp.py)", "evopf_sac": "EVOPF-v0 RPOSAC (scripts/evopf_exp_sac.py)"}


def envs_per_gpu(workload):
    return 1024 if workload.startswith("evopf") else ENVS_PER_GPU


def workload_hp(workload):
    envname, algo, over = WORKLOADS[workload]
    if envname == "evopf":
        hp = dict(EVOPF_HP)
        if over:
            hp.update(over)
            hp.pop("gamma", None)                     # evopf_exp_sac.py keeps RPOSAC's default discount
    else:
        hp = dict(HP)
        hp.update(over)
    return envname, algo, hp


def make_trainer(n_envs, device, max_epochs, capacity=None, workload="cart_ddpg", updates_per_step=None, backend=None,
                 torch_seed=123, **extra):
    from rpo_amd import gym_shim
    from rpo_amd.algo import RPODDPG, RPOSAC
    from rpo_amd.env import CartSafeEnv, EVOPFEnv, SpringPendulumEnv
    np.random.seed(123)
    torch.manual_seed(torch_seed)           # identical replicas on every rank (the trainer broadcasts rank 0's anyway)
    envname, algo, hp = workload_hp(workload)
    kw = {} if backend is None else dict(backend=backend, device=device)
    if envname == "evopf":
        env = EVOPFEnv(**kw)
    else:
        env = gym_shim.TimeLimit(CartSafeEnv(**kw) if envname == "cart" else SpringPendulumEnv(**kw), 200)
    if capacity is not None:
        hp["capacity"] = capacity
    hp.update(extra)
    cls = RPODDPG if algo == "ddpg" else RPOSAC
    return cls(env, "/tmp/rpo_bench", name="bench", logger=None, max_epochs=max_epochs, device=device,
               num_envs=n_envs, updates_per_step=updates_per_step, backend=backend, **hp)


def spin_up(device, seconds=1.5):
    """Untimed: keep the GPU busy for a moment before anything is measured, so that a fresh box has left its idle
    power state (one in ~10 fresh boxes otherwise measured the first window ~40 % slow)."""
    x = torch.randn(4096, 4096, device=device)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        for _ in range(10):
            x = torch.mm(x, x).clamp_(-1.0, 1.0)
        torch.cuda.synchronize()


def time_kernel(fn, reps=100):
    """Average duration (us) of one launch: `reps` back-to-back launches captured in a hipGraph and bracketed by ONE pair
    of HIP events on the replay stream (an event pair around a single launch has a ~13 us floor on this stack, far above
    these kernels).  The figure includes the ~1.5 us dependent-launch boundary between consecutive kernels."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    g.replay()
    torch.cuda.synchronize()
    times = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3 / reps)
    return float(np.median(times)), float(np.mean(times))


# ------------------------------------------------------------------------------------------------ kernel clinic

class LaunchRecorder(object):
    """Records every call that goes through the C ABI wrappers (rpo_amd.ops functions and the env's kernel set) during
    a few eager iterations, so that each launch of the iteration can afterwards be replayed and timed on its own with
    the very arguments the trainer uses (static device buffers)."""

    def __init__(self, tr):
        from rpo_amd import ops
        self.tr, self.ops, self.calls, self._undo = tr, ops, [], []
        skip = ("new_stats", "reduce_stats", "mlp_supported", "check")
        for name, fn in list(vars(ops).items()):
            if callable(fn) and not name.startswith("_") and not isinstance(fn, type) and name not in skip \
                    and getattr(fn, "__module__", None) == ops.__name__:
                self._wrap(ops, name, fn)
        if hasattr(ops, "SplitUpdate"):                           # stages of the column-split update: one launch each
            orig_run = ops.SplitUpdate.run
            rec = self

            def run(su, stage, rider=None):
                kw = {} if rider is None else dict(rider=rider)
                rec.calls.append(("split_" + stage + ("" if rider is None else "_ride"), orig_run, (su, stage), kw))
                return orig_run(su, stage, **kw)
            self._undo.append((ops.SplitUpdate, "run", orig_run, True))
            ops.SplitUpdate.run = run
        k = tr.kernels
        for name in dir(k):
            fn = getattr(k, name)
            if callable(fn) and not name.startswith("_") and hasattr(fn, "__self__"):
                self._wrap(k, name, fn, prefix=type(k).__name__ + ".")

    def _wrap(self, owner, name, fn, prefix=""):
        rec = self

        def wrapped(*a, **kw):
            rec.calls.append((prefix + name, fn, a, kw))
            return fn(*a, **kw)
        had = name in vars(owner)
        self._undo.append((owner, name, vars(owner).get(name), had))
        setattr(owner, name, wrapped)

    def close(self):
        for owner, name, old, had in reversed(self._undo):
            if had:
                setattr(owner, name, old)
            else:
                delattr(owner, name)


def mlp_flops(d):
    """Forward flops per row of one rpo_mlp network (2 x multiply-adds of its three layers)."""
    return 2 * (d.S * d.E + d.A * d.E + d.ein * d.H + d.H * d.outs)


def launch_models(tr, workload):
    """Algorithmic work per launch for the launches of one iteration: name -> (bound, units, per unit).
    HBM-bound kernels are priced in bytes, the MLP pipelines in flops (forward x1, backward x2)."""
    k, f, B, n = tr.kernels, tr.fused, tr.batch_size, tr.n_local
    S, A, P, E_, I_ = k.obs_dim, k.action_dim, k.partial_dim, k.eq_num, k.ineq_num
    row = 4 * (2 * S + A + 1 + E_ + I_) + 1                     # the reference's transition (rpo/utils/buffer.py:3-20)
    step_bytes = 4 * S + 4 * A + 4 * S + row                     # cart: 145 B, pendulum: 109 B, EVOPF: 1605 B
    d = f.descs if f is not None else {}
    fa = mlp_flops(d["actor"]) if "actor" in d else 0
    crit = d.get("critic", d.get("critic1"))
    fc = mlp_flops(crit) if crit is not None else 0
    twin = 2 if "critic1" in d else 1
    kn = type(k).__name__ + "."
    m = {
        kn + "rollout": ("mfma", n, fa), kn + "step": ("hbm", n, step_bytes),
        # units = rows of the call.  EVOPF: one wavefront per lane solves a 22 x 22 Newton system (~5 iterations) and
        # eliminates a 28 x 43 Jacobian per GRG iteration (10): ~5.2e5 flops per lane, priced against the f32
        # peak (VALU == MFMA rate for f32); the classic-control projections are a few dozen flops on 40 bytes: HBM-priced
        kn + "act_project": ("mfma", None, 520000) if workload.startswith("evopf") else ("hbm", None, 4 * S + 4 * P + 4 * A + 4),
        "replay_sample_gather": ("hbm", B, 2 * row + 4),
        kn + "ddpg_critic_forward": ("mfma", B, fa + 2 * fc), kn + "sac_critic_forward": ("mfma", B, 2 * fa + 4 * fc),
        kn + "ddpg_critic_front": ("mfma", B, fa), kn + "sac_critic_front": ("mfma", B, fa),
        kn + "ddpg_critic_back": ("mfma", B, 2 * fc), kn + "sac_critic_back": ("mfma", B, 4 * fc),
        kn + "project_batchref": ("hbm", B, 4 * S + 4 * P + 4 * A + 4),
        "mlp_backward": ("mfma", B, 2 * fc), "mlp_backward_pair": ("mfma", B, 4 * fc),
        "mlp_forward_multi": ("mfma", B, 2 * twin * fc), "mlp_forward": ("mfma", None, None),
        "ddpg_actor_forward": ("mfma", B, fa + fc), "ddpg_actor_backward": ("mfma", B, 2 * (fa + fc)),
        "sac_actor_forward": ("mfma", B, 2 * fa + 2 * fc), "sac_actor_backward": ("mfma", B, 2 * (fa + 2 * fc)),
        "adam_step": ("hbm", None, 36), "adam_step_multi": ("hbm", None, 36), "absmax": ("hbm", None, 4),
        # column-split update stages (rpo_amd/csrc/nsplit.hip)
        "split_critic_fwd_a": ("mfma", B, fa + twin * fc), "split_critic_fwd_b": ("mfma", B, twin * fc),
        "split_pend_head_project": ("hbm", B, 4 * S + 4 * P + 4 * A + 4),
        # bwd_a: dQ -> dh1 -> dx0 through W1 and W0: one forward's worth of flops per critic.  bwd_b: every parameter gradient:
        # dW0 (H x Ein outer products: 2 B H Ein = 16.8 MFLOP at batch 256), the first-layer matrices, the head
        "split_critic_bwd_a": ("mfma", B, twin * fc),
        "split_critic_bwd_b": ("mfma", B, twin * (2 * (crit.H * crit.ein if crit is not None else 0) + 2 * 128 * (S + A + 2))),
        # ... with the next vector step riding along: the stage's own flops + the actor forward of half the lanes
        # each (fwd_a / fwd_b); bwd_b + the step of every lane is priced by the step's bytes
        "split_critic_fwd_a_ride": ("mfma", n, (B * (fa + twin * fc) + (n // 2) * fa) / float(n)),
        "split_critic_fwd_b_ride": ("mfma", n, (B * twin * fc + (n - n // 2) * fa) / float(n)),
        "split_critic_bwd_b_ride": ("hbm", n, step_bytes),
        # fused front (fwd_a + fwd_b + bwd_a in one launch; SpringPendulum "mid": fwd_b + bwd_a), with pol_a / the whole actor
        # forward of the next step as extra planes
        # front = fwd_a (pi_targ + Q_k) + fwd_b (Q_targ,k) + bwd_a (one forward's worth per critic): fa + 3 twin fc
        "split_critic_front": ("mfma", B, fa + 3 * twin * fc), "split_critic_front_pol": ("mfma", B, 2 * fa + 3 * twin * fc),
        "split_critic_front_ride": ("mfma", n, (B * (fa + 3 * twin * fc) + n * fa) / float(n)),
        "split_critic_mid": ("mfma", B, 2 * twin * fc), "split_critic_mid_pol": ("mfma", B, fa + 2 * twin * fc),
        "split_critic_mid_ride": ("mfma", n, (B * 2 * twin * fc + (n - n // 2) * fa) / float(n)),
        # SpringPendulum fused front: fwd_a + the batch-coupled projection (one workgroup per row tile) + fwd_b + bwd_a
        "split_critic_pfront": ("mfma", B, fa + 3 * twin * fc), "split_critic_pfront_pol": ("mfma", B, 2 * fa + 3 * twin * fc),
        "split_critic_pfront_ride": ("mfma", n, (B * (fa + 3 * twin * fc) + n * fa) / float(n)),
    }
    return m


def hbm_regime(working_set_bytes, rate_gbs):
    """Labels of an HBM-priced launch.  `working_set_bytes` = the distinct bytes the back-to-back replays of the clinic keep
    touching (NOT the bytes of one launch: a step kernel writes a different ring slot every launch, an act_project launch
    re-reads the same observations).  Below the 256 MiB Infinity Cache the launch is served from the LLC and its bytes / time
    is NOT an HBM bandwidth (it can exceed what HBM delivers); a streaming launch is also priced against the 6.29 TB/s a
    device copy achieves."""
    if working_set_bytes < LLC_BYTES:
        return dict(regime="LLC-resident (working set %.1f MB < 256 MiB Infinity Cache): bytes / time, not an HBM bandwidth"
                           % (working_set_bytes / 1e6), frac_of_achievable=None)
    return dict(regime="HBM streaming (working set %.0f MB)" % (working_set_bytes / 1e6),
                frac_of_achievable=min(rate_gbs / HBM_ACHIEVABLE_GBS, 1.0), achievable_peak=HBM_ACHIEVABLE_GBS)


def kernel_clinic(tr, workload):
    """Per-launch durations of every launch of one policy_fre period of the iteration (at the bench size), each priced
    against its roofline; for the headline also the streaming kernels at 1M lanes."""
    from rpo_amd import ops
    out = {}
    models = launch_models(tr, workload)
    graphs_on = tr._graphs.enabled
    tr._graphs.enabled = False
    tr._flush_tail()
    rec = LaunchRecorder(tr)
    try:
        t0 = tr._t
        if getattr(tr, "_ride_ok", lambda d: False)(True):
            # the launches of one policy_fre period as the graph windows issue them: the rollout rides on the critic update's
            # launches except behind the policy step
            tr._sync_uclock(rollout_pending=True)
            tr._uclock_ok = True
            tr._ridden_window(t0, tr.policy_fre)
            for i in range(tr.policy_fre):
                tr._advance_host(t0 + i + 1)
            tr._updates += tr.policy_fre
        else:
            for i in range(tr.policy_fre):
                tr._iteration(False, True, (t0 + i + 1) % tr.policy_fre == 0)
                tr._advance_host(t0 + i + 1)
                tr._updates += 1
    finally:
        rec.close()
        tr._graphs.enabled = graphs_on
    torch.cuda.synchronize()
    seen = {}
    for name, fn, a, kw in rec.calls:
        # one entry per distinct (entry point, row count): the first occurrence is timed
        rows = None
        if name.endswith("act_project"):
            rows = a[3].shape[0]
        elif name == "mlp_forward":
            rows = a[3].shape[0]
        elif name in ("adam_step", "absmax"):
            rows = a[0].numel()
        elif name == "adam_step_multi":
            rows = sum(g["param"].numel() for g in a[0])
        key = name if rows is None else "%s[%d]" % (name, rows)
        if key in seen:
            seen[key]["count"] += 1
            continue
        seen[key] = dict(name=name, fn=fn, a=a, kw=kw, rows=rows, count=1)
    for key, c in seen.items():
        us = time_kernel(lambda c=c: c["fn"](*c["a"], **c["kw"]))[0]
        bound, units, per = models.get(c["name"], (None, None, None))
        if c["name"] == "mlp_forward":
            per, units = mlp_flops(c["a"][0]), c["rows"]
        elif units is None:
            units = c["rows"]
        e = dict(us=us, launches_per_period=c["count"])
        if bound is not None and per:
            work = per * units
            rate, peak, unit = (work / us * 1e-3, HBM_PEAK_GBS, "GB/s") if bound == "hbm" else \
                (work / us * 1e-6, MFMA_F32_PEAK_TFLOPS, "TFLOP/s")
            e.update(bound=bound, n=units, work=work, rate=rate, unit=unit, peak=peak, frac=rate / peak)
            if bound == "hbm":
                e.update(hbm_regime(work, rate))
        out[key] = e
    if workload == "cart_ddpg":
        out.update(streaming_clinic(tr))
    for name, e in sorted(out.items(), key=lambda kv: -kv[1]["us"]):
        if "rate" in e:
            llc = str(e.get("regime", "")).startswith("LLC")
            log("  %-46s n=%-8d %9.2f us x%d  %9.2f %-8s (%s)" % (
                name, e["n"], e["us"], e.get("launches_per_period", 0), e["rate"], e["unit"],
                "LLC-resident working set: not an HBM bandwidth" if llc else "%.2f%% of the %s peak" % (100 * e["frac"], e["bound"])))
        else:
            log("  %-46s %20.2f us x%d" % (name, e["us"], e.get("launches_per_period", 0)))
    return out


def streaming_clinic(tr, sizes=((1 << 20, "1M"), (65536, "64K"))):
    """The HBM-bound CartSafe kernels and the one-launch rollout at SURVEY 8d's large micro-benchmark sizes, 2^20 lanes (where
    the streaming regime is actually reached) and 65 536 (round 6: the mid point)."""
    from rpo_amd import ops
    from rpo_amd.env.vec import VecEnv
    out = {}
    k, f = tr.kernels, tr.fused
    scale, base = tr._box_affine
    dev = tr.vec.device
    for big_n, tag in sizes:
        big = VecEnv(k, big_n, dev, seed=3, stats_cap=64)
        big.reset()
        rows = torch.zeros(8 * big_n, k.ring_floats, device=dev)
        big_ap = torch.zeros(big_n, device=dev)
        big_batch = torch.zeros(big_n, k.row_floats, device=dev)
        ring_bytes = rows.numel() * 4                            # 8 slots x n rows x 128 B (1.07 GB at 2^20: cycled through, never cached)
        reps = 20 if big_n > 200000 else 50

        def hbm(name, us, per, working_set):
            r = per * big_n / us * 1e-3
            out[name] = dict(n=big_n, us=us, bound="hbm", work=per * big_n, rate=r, unit="GB/s", peak=HBM_PEAK_GBS,
                             frac=r / HBM_PEAK_GBS, **hbm_regime(working_set, r))
        hbm("cartsafe_step_kernel@" + tag, time_kernel(lambda: k.step(
            big.internal, big.obs, big.action, big.ep_len, big.ep_ret, big.ep_count, rows, 8, big.stats, big.ctrl, 200, True,
            1e-3, big.seed, big.env_id_base), reps=reps)[0], 145, ring_bytes)   # SURVEY 8d's algorithmic 145 B; the launch MOVES
        # 208 B per lane: s 24 + a 8 + bookkeeping 12 read; s' 24 + bookkeeping 12 + a whole 128-byte ring line written
        out["cartsafe_step_kernel@" + tag]["moved_bytes_per_lane"] = 4 * 6 + 4 * 2 + 12 + 4 * 6 + 12 + 4 * k.ring_floats
        hbm("cartsafe_act_project_kernel@" + tag, time_kernel(lambda: k.act_project(
            big.obs, big_ap, None, big.action, None, ops.NOISE_PHILOX, 1.0, 1.0, 0.0, -10.0, 10.0, 10, 2e-2, 1e-5, 0.0,
            big.seed, big.env_id_base, big.ctrl, big.stats), reps=reps)[0], 40, 40 * big_n)      # the same buffers every launch: LLC
        hbm("replay_sample_gather_kernel@" + tag, time_kernel(lambda: ops.replay_sample_gather(
            rows, 8, big_n, big_batch, None, 1, 0, big.ctrl), reps=reps)[0], 178 + 4, ring_bytes)   # 2 x 89 B + index
        # what the launch moves since the 128-byte ring rows: one 128-byte line read + a 96-byte batch row written (+ 4 B index)
        out["replay_sample_gather_kernel@" + tag]["moved_bytes_per_sample"] = 4 * k.ring_floats + 4 * k.row_floats + 4
        for e in (out["cartsafe_step_kernel@" + tag], out["replay_sample_gather_kernel@" + tag]):
            moved = e.get("moved_bytes_per_lane", e.get("moved_bytes_per_sample")) * big_n / e["us"] * 1e-3
            e["moved_rate_gbs"] = moved                          # (the launch's own HBM rate: both run AT the achievable 6.29 TB/s)
            e["moved_frac_of_achievable"] = moved / HBM_ACHIEVABLE_GBS
        us = time_kernel(lambda: k.rollout(
            f.descs["actor"], False, scale, base, big.internal, None, big.action, big.ep_len, big.ep_ret, big.ep_count, rows,
            8, big.stats, big.ctrl, ops.NOISE_PHILOX, 1.0, 1.0, 0.0, -10.0, 10.0, 10, 2e-2, 1e-5, 0.0, 200, True, 1e-3,
            big.seed, big.env_id_base), reps=5 if big_n > 200000 else 20)[0]
        fl = mlp_flops(f.descs["actor"])
        out["rollout_kernel<CartEnv>@" + tag] = dict(
            n=big_n, us=us, bound="mfma", work=fl * big_n, rate=fl * big_n / us * 1e-6, unit="TFLOP/s", peak=MFMA_F32_PEAK_TFLOPS,
            frac=fl * big_n / us * 1e-6 / MFMA_F32_PEAK_TFLOPS, env_steps_per_s=big_n / us * 1e6,
            kernel="rollout_stream_kernel<CartEnv, 1> (rollout_stream.hip: weights stationary in LDS, the env step as the epilogue)"
            if big_n >= 65536 else "rollout_kernel<CartEnv, 128, 256, 4>")
        del big, rows, big_batch, big_ap
        torch.cuda.empty_cache()
    return out


# the device-side kernel each recorded entry point launches (for matching with the rocprofv3 summaries in profiles/)
KERNEL_OF = {
    "CartSafeKernels.rollout": "rollout_kernel<CartEnv>", "PendulumKernels.rollout": "rollout_kernel<PendEnv>",
    "CartSafeKernels.ddpg_critic_forward": "cart_ddpg_critic_forward_kernel",
    "CartSafeKernels.sac_critic_forward": "cart_sac_critic_forward_kernel",
    "PendulumKernels.ddpg_critic_front": "pend_ddpg_critic_front_kernel",
    "PendulumKernels.sac_critic_front": "pend_sac_critic_front_kernel",
    "PendulumKernels.ddpg_critic_back": "pend_critic_back_kernel", "PendulumKernels.sac_critic_back": "pend_critic_back_kernel",
    "EvopfKernels.act_project": "evopf_act_project_kernel", "mlp_backward": "mlp_bwd_rows_kernel + mlp_bwd_weights_kernel",
    "mlp_backward_pair": "mlp_bwd_rows_kernel + mlp_bwd_weights_kernel (twin)",
    "split_critic_fwd_a": "split_critic_fwd_a_kernel", "split_critic_fwd_b": "split_critic_fwd_b_kernel",
    "split_critic_bwd_a": "split_critic_bwd_a_kernel", "split_critic_bwd_b": "split_critic_bwd_b_kernel",
    "split_pend_head_project": "split_pend_head_project_kernel",
    "split_critic_fwd_a_ride": "split_critic_fwd_a_ride_kernel", "split_critic_fwd_b_ride": "split_critic_fwd_b_ride_kernel",
    "split_critic_bwd_b_ride": "split_critic_bwd_b_ride_kernel",
    "split_critic_front": "split_critic_front_kernel", "split_critic_front_pol": "split_critic_front_kernel",
    "split_critic_front_ride": "split_critic_front_ride_kernel", "split_critic_mid": "split_critic_mid_kernel",
    "split_critic_mid_pol": "split_critic_mid_kernel", "split_critic_mid_ride": "split_critic_mid_ride_kernel",
    "split_critic_pfront": "split_critic_pfront_kernel", "split_critic_pfront_pol": "split_critic_pfront_kernel",
    "split_critic_pfront_ride": "split_critic_pfront_ride_kernel",
}


def pmc_traffic(kernel, lanes, workload="cart_ddpg"):
    """HBM bytes per launch from the committed rocprofv3 PMC collections (profiles/r0*_pmc_traffic*.json; recipe and the
    gfx950 FETCH_SIZE correction are described there): the workload's own table first (tools/kernel_probe.py
    window:<workload>), then the CartSafe tables of earlier rounds.  None when that (kernel, size) was not collected."""
    base = kernel.split("<")[0].split(" ")[0]
    names = ["r06_pmc_traffic_%s.json" % workload, "r05_pmc_traffic_%s.json" % workload, "r04_pmc_traffic_%s.json" % workload]
    if workload.startswith("cart"):
        names += ["r06_pmc_traffic.json", "r05_pmc_traffic.json", "r04_pmc_traffic.json", "r03_pmc_traffic.json", "r02_pmc_traffic.json", "r01_pmc_traffic.json"]
    for name in names:
        try:
            with open(os.path.join(ROOT, "profiles", name)) as f:
                table = json.load(f)["kernels"]
        except (OSError, KeyError, ValueError):
            continue
        for key, sizes in table.items():                        # (the tables key kernels with or without template arguments)
            if key.split("<")[0] != base or str(lanes) not in sizes:
                continue
            if "Pend" in kernel and "<" in key and "Pend" not in key:
                continue
            return sizes[str(lanes)]["traffic_bytes"]
    return None


# ------------------------------------------------------------------------------------------------ CPU baseline

def _oracle_loop(workload):
    """The oracle's single-env, per-step CPU loop for `workload` (reference cadence: one env step + one batch-256
    update per iteration): returns run(n_steps)."""
    envname, algo, hp = workload_hp(workload)
    if envname == "evopf":
        # no OracleRPO adapter for EVOPF: the shipped trainer's host loop driven by the oracle's kernels
        # (tests/oracle_backend.py -> oracle/evopf.py), 1 env, torch-CPU MLPs
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import oracle_backend as ob
        tr = make_trainer(1, torch.device("cpu"), 10 ** 9, workload=workload, backend=ob, capacity=2000, use_graph=False)
        tr.vec.reset()
        return lambda n: tr.run_steps(n)
    from oracle import rpo_loop
    np.random.seed(123)
    torch.manual_seed(123)
    drop = ("grad_eps", "value_type", "automatic_entropy_tuning")
    hp = {k: v for k, v in hp.items() if k not in drop}
    env = rpo_loop.CartAdapter(1, seed=0) if envname == "cart" else rpo_loop.PendulumAdapter(seed=0)
    tr = rpo_loop.OracleRPO(env, sac=(algo == "sac"), **hp)
    return lambda n: tr.run(n)


def _cpu_worker(workload, seconds, chunk, barrier, q):
    torch.set_num_threads(1)
    run = _oracle_loop(workload)
    run(max(2, chunk // 2))                  # page in
    if barrier is not None:
        barrier.wait()
    done, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        run(chunk)
        done += chunk
    q.put((done, time.perf_counter() - t0))


def physical_cores():
    """Physical cores this process may run on ((physical id, core id) pairs of /proc/cpuinfo within the affinity mask)."""
    allowed = os.sched_getaffinity(0) if hasattr(os, "sched_getaffinity") else set(range(os.cpu_count() or 1))
    cores, cur = set(), {}
    try:
        with open("/proc/cpuinfo") as f:
            for line in f.read().split("\n") + [""]:
                if not line.strip():
                    if "processor" in cur and int(cur["processor"]) in allowed:
                        cores.add((cur.get("physical id", "0"), cur.get("core id", cur["processor"])))
                    cur = {}
                elif ":" in line:
                    a, b = line.split(":", 1)
                    cur[a.strip()] = b.strip()
    except OSError:
        pass
    return max(1, len(cores)) if cores else max(1, len(allowed))


def cpu_quota():
    """CPUs the container may actually use at once (cgroup v2 cpu.max / v1 cfs quota); None when unlimited."""
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            q, p = f.read().split()[:2]
            return None if q == "max" else float(q) / float(p)
    except (OSError, ValueError):
        pass
    try:
        with open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us") as f:
            q = float(f.read())
        with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as f:
            p = float(f.read())
        return None if q <= 0 else q / p
    except (OSError, ValueError):
        return None


CPU_PROCS_AT_ONCE = 4        # + this process: every worker opens the GPU (torch.optim's step asks torch.cuda.is_available(),
                             # which initialises the HIP runtime), and a shared MI355X node ends a job that holds the GPU in
                             # more than 6 processes at once


def cpu_baseline(workload, seconds=12.0):
    """Reference-cadence CPU port timed on the host cores BEFORE this process touches the GPU (fork is safe then):
    (1) one single-thread process alone, (2) min(P, CPU_PROCS_AT_ONCE) single-thread processes at once, P = physical
    cores (bounded by memory: each worker holds its own torch state), their mean rate scaled to P -- the whole-node CPU
    number of SURVEY.md 8d.  `value` is the whole-node figure."""
    import multiprocessing as mp
    ctx = mp.get_context("fork")
    chunk = 4 if workload.startswith("evopf") else 100
    q = ctx.Queue()
    p = ctx.Process(target=_cpu_worker, args=(workload, seconds, chunk, None, q))
    p.start()
    done1, dt1 = q.get()
    p.join()
    solo = done1 / dt1
    P = phys = physical_cores()
    quota = cpu_quota()
    cap_note = ""
    if quota is not None and quota < P:
        P = max(1, int(quota))
        cap_note = " (%d physical cores visible, cgroup CPU quota %.1f)" % (phys, quota)
    try:
        with open("/proc/meminfo") as f:
            avail = [int(l.split()[1]) for l in f if l.startswith("MemAvailable")][0] / 1e6      # GB
        P_mem = max(1, int(avail / 0.75))
    except (OSError, IndexError):
        P_mem = P
    if P_mem < P:
        cap_note = " (%d physical cores visible, capped by available memory)" % phys
        P = P_mem
    K = min(P, CPU_PROCS_AT_ONCE)
    barrier = ctx.Barrier(K)
    procs = [ctx.Process(target=_cpu_worker, args=(workload, seconds, chunk, barrier, q)) for _ in range(K)]
    for pr in procs:
        pr.start()
    res = [q.get() for _ in procs]
    for pr in procs:
        pr.join()
    per_process = sum(d / t for d, t in res) / K
    node = per_process * P
    kind = "shipped trainer host loop on tests/oracle_backend.py (oracle/evopf.py kernels), torch-CPU MLPs" \
        if workload.startswith("evopf") else "oracle/rpo_loop.py OracleRPO"
    return dict(value=node, unit="env-steps/s", cores=P, kind="port", single_core_value=solo,
                per_process_under_load=per_process, processes_at_once=K,
                sample="%s, %s, 1 env per process, rollout + one batch-256 update per env step, 1 thread per process: "
                       "1 process alone %.1f s (%d steps) and %d processes at once %.1f s each (%d steps in total), their "
                       "mean rate x %d cores%s"
                       % (kind, DESCRIBE[workload], dt1, done1, K, seconds, sum(d for d, _ in res), P, cap_note))


# ------------------------------------------------------------------------------------------------ launch of N ranks

def self_launch(n, argv, backend="nccl"):
    """`python bench.py --gpus N` without a launcher: start N ranks as children of a process that has NOT touched the GPU
    (torch.cuda.device_count() does not initialise HIP on this image) and pass their output / exit code through.
    ``backend="gloo"`` (RPO_BENCH_BACKEND / --backend): the ranks may SHARE the visible GPUs (rank r on cuda:r mod #GPUs) --
    the control-flow check of the N > 1 path on a one-GPU box, never a scaling figure."""
    have = torch.cuda.device_count()
    if have < n and not (backend == "gloo" and have >= 1):
        log("bench.py: --gpus %d requested but only %d GPU(s) are visible; refusing to print a %d-GPU line" % (n, have, have))
        sys.exit(2)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")          # dmabuf IPC: RCCL peer buffers across processes
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + argv
    log("bench.py: starting %d ranks: %s" % (n, " ".join(cmd)))
    sys.exit(subprocess.run(cmd, env=env).returncode)


def timed_run(tr, steps, warmup, world, device):
    def fence():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
            torch.cuda.synchronize()
    tr.run_steps(warmup)
    # untimed, like the capture phase of prepared_trainer: the timed region starts on a policy_fre boundary (graph windows
    # start there), and a SHORT region (the driver's --steps 20) is rehearsed once so that the hipGraphs of exactly its
    # launch pattern (a 16-iteration window + a 4-iteration one) exist before the clock starts
    pf = tr.policy_fre
    tr.run_steps((-tr._t) % pf)
    if steps < 20 * max(tr._cycle, 1):
        for _ in range(tr._graphs.warm + 2):                   # (a hipGraph is captured on the call after `warm` eager ones)
            tr.run_steps(steps)
            tr.run_steps((-tr._t) % pf)
    if os.environ.get("RPO_BENCH_DEBUG"):    # extra untimed windows, to see drift / host stalls (stderr)
        for w in range(6):
            fence()
            tw = time.perf_counter()
            tr.run_steps(500)
            fence()
            log("debug window %d: %.4f ms/iter" % (w, (time.perf_counter() - tw) / 500 * 1e3))
    # The timed region is EXACTLY `steps` steps between two fences (max over ranks), timed once: `--steps` is the number of
    # steps measured, and the trainer's state after them does not depend on the clock (--dump-outputs).  A short region is a
    # single sample of a noisy quantity; ask for more steps to average over more.
    fence()
    t0 = time.perf_counter()
    tr.run_steps(steps)
    fence()
    dt = time.perf_counter() - t0
    if world > 1:
        tmax = torch.tensor([dt], device=device, dtype=torch.float64)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dt = float(tmax.item())
    return [dt]


DUMP_MAX_BYTES = 64 * 2 ** 20


def dump_outputs(tr, out_dir):
    """--dump-outputs: what the timed steps handed back in the last of them, one .npy per array -- the transitions the
    fused step scattered into the replay ring (`transition_<column>`, one row per env), the observations the next step
    starts from (`obs`), the parameters after the update (`params`: the flat buffer, critic | shared | actor | multipliers)
    and the target networks, all float32, and the last losses (`loss_<name>`, float64).  Every input comes from the seeds
    of make_trainer, so two builds run with the same arguments can be compared array for array."""
    torch.cuda.synchronize()
    buf, ag = tr.buffer, tr.agent
    n = buf.n_envs
    first = (buf.pointer - n) % (buf.capacity * n)              # the ring slot of the last vector step
    rows = buf.rows[first:first + n]
    arrays = {"transition_" + k: rows[:, lo:hi] for k, (lo, hi) in buf.cols.items()}
    arrays.update(obs=tr.vec.obs, params=ag.flat.data, critic_target=ag.critic_target_flat)
    if ag.actor_target_flat is not None:
        arrays["actor_target"] = ag.actor_target_flat
    arrays = {k: v.detach().float().cpu().numpy() for k, v in arrays.items()}
    arrays.update(("loss_" + k, np.float64(float(v))) for k, v in tr.last_losses.items())
    total = sum(np.asarray(v).nbytes for v in arrays.values())
    assert total <= DUMP_MAX_BYTES, "--dump-outputs: %d bytes" % total
    os.makedirs(out_dir, exist_ok=True)
    for k, v in arrays.items():
        np.save(os.path.join(out_dir, k + ".npy"), v)
    log("dumped %d arrays (%d bytes) of step %d to %s" % (len(arrays), total, tr._t, out_dir))


def region_stats(regions, steps):
    r = np.sort(np.asarray(regions, dtype=np.float64))
    return dict(median=float(np.median(r)), ms_per_step=float(np.median(r)) / steps * 1e3, ms_per_step_min=float(r[0]) / steps * 1e3,
                ms_per_step_max=float(r[-1]) / steps * 1e3, timed_regions=int(len(r)), timed_total_ms=float(r.sum()) * 1e3)


def prepared_trainer(n_total, device, workload):
    """Untimed pre-conditioning on a throw-away trainer (tiny replay ring) -- the first process on a fresh box otherwise
    pays for paging in the libraries and code paths of the iteration inside the timed window (measured: 0.14 instead of
    0.10 ms per iteration in 4 of 4 first-process runs) -- then the measured trainer with every hipGraph of the steady
    state captured (three eager passes + capture: single iterations with / without the policy step, and the
    multi-iteration window), like a compile step."""
    pre = make_trainer(n_total, device, 10 ** 9, capacity=64, workload=workload)
    pre.vec.reset()
    pre.run_steps(1500)
    pre._harvest(final=True)                # first use of the statistics path (gather / reduce / copy-out kernels)
    torch.cuda.synchronize()
    del pre
    tr = make_trainer(n_total, device, 10 ** 9, workload=workload)
    tr.vec.reset()
    tr.run_steps(5 * max(tr._cycle, 4))
    return tr


# SURVEY 8d / VERDICT r05 next 3: the LOOP (not only single kernels) at the sizes where the HBM / MFMA-bound regime is reached
ROLLOUT_FLOP_PER_LANE = 2 * (6 * 128 + 128 * 256 + 256 * 1)     # actor forward, SURVEY 8d: 67 584
ROLLOUT_BYTES_PER_LANE = 145 + 40                              # fused step 145 B + complete / project 40 B
UPDATE_FLOP_PER_SAMPLE = (67584 + 2 * 68096 + 136192) + (67584 + 68096 + 68096 + 135168) / 4.0   # critic update + a quarter policy step
UPDATE_BYTES = 256 * 182 + 36 * 34564 + (36 * 34177 + 256 * 178) / 4.0                          # gather + Adam/Polyak (+ policy / 4)


def lanes_sweep(device, sizes, workload="cart_ddpg"):
    """Whole-iteration figures of the headline workload at `sizes` lanes on ONE GPU: (i) rollout only, (ii) rollout + the
    reference-cadence update (one batch-256 update per vector step), each as env-steps/s and as fractions of the f32 MFMA
    peak (67 584 flop per lane + the update's flops) and of the HBM roofline (185 algorithmic bytes per lane + the update's
    bytes), in hipGraph windows like the headline.  From 65 536 lanes the rollout launch is the streaming form
    (rollout_stream.hip).  Replay capacity 8 vector steps per lane (1 GiB at 2^20 lanes), everything else as the headline."""
    out = []
    for n in sizes:
        row = {"lanes": int(n)}
        try:
            _lanes_row(row, int(n), device, workload)
        except Exception as e:                                  # noqa: BLE001  (an extra must never cost the line its headline)
            row["error"] = "%s: %s" % (type(e).__name__, str(e)[:200])
            log("lanes %d: %s" % (n, row["error"]))
            torch.cuda.empty_cache()
        out.append(row)
    torch.cuda.empty_cache()
    return {"workload": DESCRIBE[workload], "rows": out,
            "note": "whole iterations in hipGraph windows on one GPU; fractions = (lanes x %d flop [+ %.1f MFLOP of update]) / time "
                    "/ %.1f TFLOP/s and (lanes x %d B [+ %.2f MB of update]) / time / %.0f GB/s (SURVEY 8d's algorithmic figures)"
                    % (ROLLOUT_FLOP_PER_LANE, 256 * UPDATE_FLOP_PER_SAMPLE * 1e-6, MFMA_F32_PEAK_TFLOPS, ROLLOUT_BYTES_PER_LANE,
                       UPDATE_BYTES * 1e-6, HBM_PEAK_GBS)}


def _lanes_row(row, n, device, workload):
    for mode in ("rollout_only", "with_update"):
        torch.cuda.empty_cache()
        tr = make_trainer(int(n), device, 10 ** 9, capacity=8, workload=workload)
        tr.vec.reset()
        train = mode == "with_update"
        tr.run_steps(5 * max(tr._cycle, 4), train=train)          # eager passes + graph capture
        steps = int(max(2 * tr._cycle, min(2000, 2 ** 28 // n)))
        steps -= steps % max(tr._cycle, 1)
        regions = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.run_steps(steps, train=train)
            torch.cuda.synchronize()
            regions.append((time.perf_counter() - t0) / steps)
        dt = float(np.median(regions))
        flop = n * ROLLOUT_FLOP_PER_LANE + (256 * UPDATE_FLOP_PER_SAMPLE if train else 0.0)
        byts = n * ROLLOUT_BYTES_PER_LANE + (UPDATE_BYTES if train else 0.0)
        row[mode] = {"ms_per_step": dt * 1e3, "env_steps_per_s": n / dt, "steps_timed": steps,
                     "frac_of_f32_mfma_peak": flop / dt * 1e-12 / MFMA_F32_PEAK_TFLOPS,
                     "frac_of_hbm_roofline": byts / dt * 1e-9 / HBM_PEAK_GBS, "hip_graph_window": tr._cycle}
        tr._harvest(final=True)
        del tr
    ro, wu = row["rollout_only"], row["with_update"]
    log("lanes %8d: rollout only %9.1f M env-steps/s (%.3f of the f32 MFMA peak, %.4f of the HBM roofline); with the batch-256 "
        "update %9.1f M (%.3f / %.4f)" % (n, ro["env_steps_per_s"] * 1e-6, ro["frac_of_f32_mfma_peak"], ro["frac_of_hbm_roofline"],
                                         wu["env_steps_per_s"] * 1e-6, wu["frac_of_f32_mfma_peak"], wu["frac_of_hbm_roofline"]))


def main():
    os.environ.setdefault("RPO_VERBOSE", "0")
    if os.environ.get("RPO_BENCH_FAULT"):                       # debugging aid: every thread's stack to stderr after N seconds
        import faulthandler
        faulthandler.dump_traceback_later(int(os.environ["RPO_BENCH_FAULT"]), repeat=True, exit=False)
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--full", action="store_true",
                    help="besides the headline, run every other measurement: CPU baseline, extra legs, violation rates, lanes "
                         "sweep, kernel clinics (a plain run does none of them)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baseline")
    ap.add_argument("--no-clinic", action="store_true", help="--full without the kernel clinics")
    ap.add_argument("--no-extras", action="store_true", help="--full without the rollout-only / UTD-matched / cart_sac / n = 1 / "
                                                               "lanes legs")
    ap.add_argument("--workload", default="cart_ddpg", choices=sorted(WORKLOADS),
                    help="cart_ddpg is the headline (BASELINE.json configs[1]); the others are extra measurements")
    ap.add_argument("--force-dist", action="store_true",
                    help="one GPU: run the data-parallel code path over a ONE-rank RCCL group (the gradient all-reduce and the "
                         "rpo_absmax_slots launch inside the graph windows): the measured intercept of the 1 -> N expectation")
    ap.add_argument("--n1-seeds", type=int, default=384,
                    help="headline extras: seeds of the num_envs = 1 violation-rate figure (0: skip)")
    ap.add_argument("--n1-seed-base", type=int, default=None,
                    help="first seed of that sample (default: derived from this file's hash and the clock, so that every run is an "
                         "INDEPENDENT sample; printed in the line -- pass it back to reproduce a line)")
    ap.add_argument("--lanes", default="4096,65536,1048576", metavar="N[,N...]",
                    help="headline extras: whole-iteration figures (rollout only / rollout + batch-256 update) at these lane "
                         "counts on one GPU, with fractions of the f32 MFMA and HBM rooflines ('' or 0: skip); the headline "
                         "itself stays BASELINE.json's 4096 lanes")
    ap.add_argument("--backend", default=os.environ.get("RPO_BENCH_BACKEND", "nccl"), choices=("nccl", "gloo"),
                    help="collective backend of an N > 1 run.  nccl (= RCCL, one rank per GPU) is what is measured; gloo lets "
                         "the ranks share a GPU with host-driven collectives between hipGraph segments -- a control-flow check "
                         "of the N > 1 path on a one-GPU box, labelled as such in the line")
    ap.add_argument("--tuning", default="", metavar="KEY=VALUE[,...]",
                    help="A/B aid: library kernel-variant switches (rpo_tuning / ops.TUNE) set before the trainer is built; the "
                         "line reports them under config.tuning")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what their last step computed (transitions, observations, parameters, "
                         "losses of --workload's trainer; rank 0) as DIR/<name>.npy, to compare two builds on identical inputs")
    args = ap.parse_args()

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        os.environ["RPO_BENCH_BACKEND"] = args.backend           # (the ranks read it like the flag)
        self_launch(args.gpus, sys.argv[1:], args.backend)       # never returns
    # stdout carries ONE JSON line (rank 0's) and nothing else: whatever a library prints there (gloo announces its
    # connections on stdout from C++, from every rank) goes to stderr -- file descriptor 1 is pointed at 2 for the whole run
    # and the line is written to the saved descriptor at the end
    sys.stdout.flush()
    real_stdout = os.dup(1)
    os.dup2(2, 1)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    shared_gpu = False
    if args.backend == "gloo" and world > 1:
        have = torch.cuda.device_count()                         # (does not initialise HIP)
        shared_gpu = have < world
        local_rank = local_rank % max(1, have)
    if world != args.gpus:
        log("note: --gpus %d but WORLD_SIZE %d; using WORLD_SIZE" % (args.gpus, world))
    headline = args.workload == "cart_ddpg"
    extras = args.full and not args.no_extras
    clinic = args.full and not args.no_clinic

    # CPU leg first: forked single-thread workers, before this process initialises the GPU
    cpu = None
    if args.full and not args.no_cpu_baseline and world == 1:
        cpu = cpu_baseline(args.workload)
        log("cpu baseline: %.1f env-steps/s on %d cores (1 core alone: %.1f)" % (cpu["value"], cpu["cores"],
                                                                                cpu["single_core_value"]))

    assert torch.cuda.is_available(), "bench.py needs an MI355X (there is no CPU fallback)"
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    if world > 1 or args.force_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if world == 1:
            s0 = socket.socket()
            s0.bind(("127.0.0.1", 0))
            os.environ.setdefault("MASTER_PORT", str(s0.getsockname()[1]))
            s0.close()
            os.environ["RPO_SCHEDULE"] = ",".join(filter(None, [os.environ.get("RPO_SCHEDULE", ""), "force_dist=1"]))
            dist.init_process_group(backend="nccl", rank=0, world_size=1, device_id=device)
        elif args.backend == "gloo":
            dist.init_process_group(backend="gloo")              # host-driven collectives on GPU tensors; no device binding
        else:
            dist.init_process_group(backend="nccl", device_id=device)
        log("rank %d/%d on cuda:%d: process group up, backend %s%s, %d ranks" % (
            rank, world, local_rank, dist.get_backend(), " (RCCL)" if dist.get_backend() == "nccl" else
            " (host-driven%s)" % (", ranks share a GPU" if shared_gpu else ""), dist.get_world_size()))
    rccl_ranks = dist.get_world_size() if (dist.is_initialized() and dist.get_backend() == "nccl") else 0

    tuning = {k.strip(): int(v) for k, _, v in (item.partition("=") for item in args.tuning.split(",") if item.strip())}
    if tuning:
        from rpo_amd import ops as _ops
        _ops.tuning(**tuning).__enter__()                        # (for the life of the process)
    EPG = envs_per_gpu(args.workload)
    n_total = EPG * world
    spin_up(device)
    tr = prepared_trainer(n_total, device, args.workload)
    timing = region_stats(timed_run(tr, args.steps, args.warmup, world, device), args.steps)
    if args.dump_outputs and rank == 0:
        dump_outputs(tr, args.dump_outputs)
    elapsed = timing["median"]
    value = n_total * args.steps / elapsed
    # the violation rate needs a window of its own: over a few dozen vector steps it is noise (measured 0.325 over
    # 20 steps vs 0.023 over 2000).  --full continues the same run, untimed, to at least 1000 vector steps.
    if args.full and tr._t < 1000:
        tr.run_steps(1000 - tr._t)
    tr._harvest(final=True)
    # did EVERY rank replay captured hipGraphs (data-parallel: with the collectives inside them)?  A rank whose capture
    # fails takes all ranks to eager launches together (trainer._GraphCache.run), and the line says so.
    replayed_everywhere = tr.dist.replaying_everywhere(tr._graphs, device)

    result = {
        "metric": "env-steps/sec (whole node), %s, rollout + one batch-256 constrained policy update per vector step"
                  % ("SafeCartpole-v0 (CartSafe-v0) RPODDPG" if headline else args.workload),
        "value": value, "unit": "env-steps/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": timing["ms_per_step"], "ms_per_step_min": timing["ms_per_step_min"],
        "ms_per_step_max": timing["ms_per_step_max"], "timed_regions": timing["timed_regions"],
        "timed_total_ms": timing["timed_total_ms"],
        "timing_note": "value = steps x envs / the time of ONE region of exactly `steps` steps (barrier + synchronize on both "
                       "sides, max over ranks)",
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f32", "data": "synthetic",
        "config": {"workload": ("CartSafe-v0 RPODDPG, %d vectorised envs per MI355X, scripts/cart_exp.py "
                                "hyper-parameters, update batch 256 every vector step (reference cadence), replay "
                                "capacity 20000 per env" % EPG) if headline else
                               "%s, %d vectorised envs per MI355X (extra measurement, not the headline)" % (DESCRIBE[args.workload], EPG),
                   "envs_per_gpu": EPG, "global_envs": n_total, "update_batch": 256,
                   "parallelism": ("dp%d (env shards, one RCCL all-reduce of the flat gradient bucket per update, "
                                   "captured inside the iteration's hipGraph)" % world) if args.backend == "nccl" or world == 1 else
                                  ("dp%d (env shards, one gloo all-reduce of the flat gradient bucket per update, issued by the "
                                   "host between hipGraph segments)" % world),
                   "collective_backend": (dist.get_backend() if dist.is_initialized() else None),
                   "hip_graph": bool(tr._graphs.enabled), "graph_window_iterations": tr._cycle,
                   "training_batch_projection": tr.projection_mode,
                   **({"tuning": tuning} if tuning else {}),
                   # what RCCL saw (0: no process group -- the single-process run has no collective at all), and the
                   # collectives of the data-parallel iteration: one all-reduce of the critic's flat gradient slice per update,
                   # one more (actor slice + multipliers [+ log alpha] in one bucket) on every policy_fre-th
                   "rccl_ranks": rccl_ranks, "data_parallel_path": bool(tr.dist.on),
                   "collectives_per_update": (1.0 + 1.0 / tr.policy_fre) if tr.dist.on else 0.0,
                   "collectives_in_graph": bool(tr.dist.on and tr.dist.in_graph and replayed_everywhere),
                   "graphs_replayed_on_all_ranks": bool(replayed_everywhere),
                   "graph_capture_fell_back_to_eager": bool(tr._graphs.capture_failed),
                   "allreduce_bytes": {"critic_update": 4 * int(tr.agent.flat.gradient(tr.agent.flat.critic_range).numel()),
                                       "policy_step": 4 * int(sum(t.numel() for t in [tr.agent.flat.gradient(tr.agent.flat.policy_bucket)]))}
                   if tr.dist.on else None},
        **({"control_flow_check": "gloo%s: control-flow check of the N > 1 path, NOT a scaling figure (the measured "
                                  "configuration is one rank per GPU over RCCL)" % (", %d ranks time-slicing %d GPU(s)" % (
                                      world, torch.cuda.device_count()) if shared_gpu else "")}
           if (world > 1 and args.backend == "gloo") else {}),
    }
    if args.full:
        # NOT the reference's quantity: the fraction of (env, vector step) pairs with max(max_ineq, max_eq) > 1e-3 over the
        # first `constraint_violation_window` of THIS run, in which the policy receives one update per VECTOR step (1 / 4096 of
        # the reference's learning per env step) -- it mostly measures how early in training the window sits.  The figure that
        # is comparable with the reference's 3000-step single-env runs is constraint_violation_rate_n1 below (1536 + 1536 seeds
        # in profiles/r06_stat_rows_ddpg_cart.*: +0.12e-3 +- 0.27e-3); at matched UPDATES the vectorised cadence violates 2.2e-3
        # LESS than the reference (profiles/r06_cadence_learning.json).
        result.update({"constraint_violation_rate_vector_cadence": tr.viol_rate,
                       "constraint_violation_window": "%d vector steps x %d envs" % (tr._t, n_total),
                       "mean_projection_iters": tr.proj_iters_mean})

    if extras and headline:
        # config 4's algorithm (RPOSAC on CartSafe-v0, scripts/cart_exp_sac.py) on the same ranks, same protocol
        del tr
        torch.cuda.empty_cache()
        sac = prepared_trainer(n_total, device, "cart_sac")
        t2 = region_stats(timed_run(sac, args.steps, args.warmup, world, device), args.steps)
        result["cart_sac_env_steps_per_s"] = n_total * args.steps / t2["median"]
        result["cart_sac_ms_per_step"] = t2["ms_per_step"]
        result["cart_sac_ms_per_step_min_max"] = [t2["ms_per_step_min"], t2["ms_per_step_max"]]
        if clinic and world > 1 and sac.fused is not None:
            # config 4 IS this algorithm at N = 8: its own roofline on the N > 1 lines (every rank runs the clinic -- its recorded
            # iterations contain the collectives --, rank 0's figures are printed).  At N = 1 `--workload cart_sac` carries it.
            log("kernel clinic of the cart-SAC leg (config 4's algorithm):")
            result["cart_sac_roofline"] = roofline(kernel_clinic(sac, "cart_sac"), "cart_sac")
            result["cart_sac_roofline"]["note"] += "; rank 0's launches of the %d-rank run" % world
        del sac
        torch.cuda.empty_cache()
        tr = None

    if extras and headline and world == 1 and args.n1_seeds > 0:
        result.update(violation_rate_n1(device, args.n1_seeds, seed_base=args.n1_seed_base))
    lanes = [int(x) for x in args.lanes.split(",") if x.strip() and int(x) > 0]
    if extras and headline and world == 1 and rank == 0 and lanes:
        result["lanes_sweep"] = lanes_sweep(device, lanes)
    if clinic and world > 1:
        # every rank runs the clinic (its recorded iterations contain the collectives); rank 0's figures are printed
        if tr is None:
            tr = prepared_trainer(n_total, device, args.workload)
        if tr.fused is not None:
            result["roofline"] = roofline(kernel_clinic(tr, args.workload), args.workload)
            result["roofline"]["note"] += "; rank 0's launches of the %d-rank run" % world
    if rank == 0 and world == 1:
        if extras:
            # (i) rollout-only throughput next to the headline, so that the cadence is visible
            ro = make_trainer(EPG, device, 10 ** 9, capacity=64, workload=args.workload)
            ro.vec.reset()
            ro.run_steps(5 * max(ro._cycle, 4), train=False)      # eager passes + graph capture
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            ro.run_steps(1000, train=False)
            torch.cuda.synchronize()
            result["rollout_only_env_steps_per_s"] = EPG * 1000 / (time.perf_counter() - t1)
            del ro
            # (iii) UTD-matched: one batch-256 update per ENV step as in the reference, i.e. EPG updates per
            # vector step -- a bounded sample of vector steps
            utd = make_trainer(EPG, device, 10 ** 9, capacity=256, workload=args.workload, updates_per_step=EPG)
            utd.vec.reset()
            utd.run_steps(1)
            torch.cuda.synchronize()
            # median of three samples of four vector steps (16 384 sequential updates, ~0.47 s each): a single sample right
            # behind the trainer's construction read 29.0 - 31.9 us per update from box to box, three in a row 28.1 - 28.3
            samples = []
            for _ in range(3):
                t2 = time.perf_counter()
                utd.run_steps(4)
                torch.cuda.synchronize()
                samples.append(time.perf_counter() - t2)
            dt = float(np.median(samples))
            result["utd_matched_samples_us_per_update"] = [x / (EPG * 4) * 1e6 for x in samples]
            result["utd_matched_env_steps_per_s"] = EPG * 4 / dt
            result["utd_matched_updates_per_s"] = EPG * 4 / dt
            result["utd_matched_us_per_update"] = dt / (EPG * 4) * 1e6
            del utd
            if headline:
                # (iii') the same number of sampled transitions per env step as ONE large batch per vector step (SURVEY 8d-iii:
                # "batch 256 * N per vector step"): batch 256 * 4096 = 2^20 through the generic MLP kernels (64-row tiles,
                # split-K weights pass) -- one optimiser step per vector step instead of 4096 sequential ones, so it is an
                # EXTRA mode with other learning dynamics, not a replacement of the exact-cadence default
                torch.cuda.empty_cache()
                lb = make_trainer(EPG, device, 10 ** 9, capacity=64, workload=args.workload, batch_size=256 * EPG)
                lb.vec.reset()
                lb.run_steps(5 * max(lb._cycle, 4))
                torch.cuda.synchronize()
                t3 = time.perf_counter()
                lb.run_steps(2 * max(lb._cycle, 4))
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t3) / (2 * max(lb._cycle, 4))
                result["large_batch"] = {
                    "update_batch": 256 * EPG, "ms_per_step": dt * 1e3, "env_steps_per_s": EPG / dt,
                    "sampled_transitions_per_s": 256 * EPG / dt,
                    "over_utd_matched": (EPG / dt) / result["utd_matched_env_steps_per_s"],
                    "note": "one batch-%d update per vector step: 256 sampled transitions per env step like the reference, one "
                            "optimiser step per vector step (not %d)" % (256 * EPG, EPG),
                    # tools/cadence_learning.py, 32 (large batch) / 128 (batch 256) seeds x 3000 updates vs the reference's 1536 runs
                    # (profiles/r06_cadence_learning.json, tests/test_statistical_evidence.py; round 5's figures for this mode were
                    # collected with the hipGraph memset-node bug of DESIGN.md 4.5 and read 24.9 / 29.6)
                    "learning_at_matched_updates": "another optimiser regime (one step per vector step): at 3000 updates it reaches "
                            "return 27.4 +- 2.0 (second half 34.6 +- 3.1) where the reference reaches 28.9 +- 0.35 (35.5 +- 0.5) -- not "
                            "distinguishable at 32 seeds -- with HALF the violation rate (0.66e-2 +- 0.08e-2 vs 1.33e-2); the batch-256 "
                            "cadence of the headline is better than the reference on both at matched updates (33.4 +- 1.6 / 42.6 +- 2.3, "
                            "1.10e-2 +- 0.06e-2: sampling from 4096 independent histories; one lane reproduces the reference, "
                            "DESIGN.md 5)"}
                if clinic:
                    log("kernel clinic of the large-batch update:")
                    cl = kernel_clinic(lb, args.workload)
                    result["large_batch"]["kernels"] = {
                        k: {kk: vv for kk, vv in v.items() if kk in ("us", "rate", "unit", "frac", "bound", "n", "launches_per_period",
                                                                     "regime", "frac_of_achievable")}
                        for k, v in cl.items() if "@" not in k and v.get("n", 0) == 256 * EPG}
                del lb
                torch.cuda.empty_cache()
        if clinic:
            if tr is None:
                tr = prepared_trainer(n_total, device, args.workload)
            if tr.fused is not None:
                log("kernel clinic (hipGraph of back-to-back launches between two HIP events on the launch stream):")
                result["roofline"] = roofline(kernel_clinic(tr, args.workload), args.workload)
        if cpu is not None:
            result["cpu_baseline"] = cpu
            if "large_batch" in result:
                result["large_batch"]["over_cpu"] = result["large_batch"]["env_steps_per_s"] / cpu["value"]
                result["large_batch"]["over_cpu_single_core"] = result["large_batch"]["env_steps_per_s"] / cpu["single_core_value"]
            result["gpu_over_cpu"] = value / cpu["value"]
            result["gpu_over_cpu_single_core"] = value / cpu["single_core_value"]
            if "utd_matched_env_steps_per_s" in result:
                result["utd_matched_over_cpu"] = result["utd_matched_env_steps_per_s"] / cpu["value"]
                result["utd_matched_over_cpu_single_core"] = result["utd_matched_env_steps_per_s"] / cpu["single_core_value"]
    if rank == 0:
        sys.stdout.flush()
        os.write(real_stdout, (json.dumps(result) + "\n").encode())
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()


def bench_py_sha16():
    import hashlib
    with open(os.path.abspath(__file__), "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()[:16]


def violation_rate_n1(device, seeds, steps=3000, seed_base=None):
    """The constraint-violation rate in the REFERENCE's setting (rpo_ddpg.py:120-123,137; threshold cartpole.py:326-330):
    num_envs = 1, one update per env step, `steps` iterations of scripts/cart_exp.py per seed, averaged over `seeds` runs of
    the shipped trainer on the HIP kernels -- next to the same statistic of the unmodified reference's runs (384 seeds,
    tests/golden/training_stats_ddpg_cart.npz, recorded by tests/golden/make_golden.py stats).  north_star: |delta| <= 1e-3."""
    from rpo_amd.utils.logger import Logger
    # Every run of bench.py draws an INDEPENDENT sample (rounds 3-5 re-ran seeds 5000.. / 123.. and the
    # driver's figure carried no new information): the first seed comes from this file's hash and the clock, and is printed.
    sha16 = bench_py_sha16()
    if seed_base is None:
        seed_base = (int(sha16[:8], 16) ^ (int(time.time()) * 2654435761)) % (1 << 30)
    seed_base = int(seed_base)
    rates = []
    t0 = time.perf_counter()
    for seed in range(seeds):
        # (its own initial weights AND its own Philox seed per run, like tests/test_statistical_parity_gpu.py)
        tr = make_trainer(1, device, steps, capacity=steps, workload="cart_ddpg", torch_seed=seed_base + 123 + seed,
                          seed=seed_base + 5000 + seed)
        tr.logger = Logger(("epoch", "reward", "max_ineq", "max_eq"), times=1, epochs=steps)
        tr.run(eval=False)
        n = tr.logger.pointer
        mi, me = tr.logger.tracker["max_ineq"][:n], tr.logger.tracker["max_eq"][:n]
        rates.append(float((np.maximum(mi, me) > 1e-3).mean()))
        del tr
    rates = np.asarray(rates)
    out = {"constraint_violation_rate_n1": float(rates.mean()),
           "constraint_violation_rate_n1_se": float(rates.std(ddof=1) / np.sqrt(len(rates))),
           "constraint_violation_rate_n1_protocol": "%d seeds x %d iterations at num_envs = 1 (reference cadence), %.0f s" % (
               seeds, steps, time.perf_counter() - t0),
           "constraint_violation_rate_n1_seed_base": seed_base, "bench_py_sha16": sha16,
           "constraint_violation_rate_n1_seeds": int(seeds)}
    try:
        ref = np.load(os.path.join(ROOT, "tests", "golden", "training_stats_ddpg_cart.npz"))["stats"][:, 1]
        se = float(np.sqrt(ref.var(ddof=1) / len(ref) + rates.var(ddof=1) / len(rates)))
        out.update({"constraint_violation_rate_reference": float(ref.mean()),
                    "constraint_violation_rate_reference_se": float(ref.std(ddof=1) / np.sqrt(len(ref))),
                    "constraint_violation_rate_reference_seeds": int(len(ref)),
                    "constraint_violation_rate_n1_minus_reference": float(rates.mean() - ref.mean()),
                    "constraint_violation_rate_difference_se": se})
    except (OSError, KeyError):
        pass
    return out


def roofline(clinic, workload):
    """The dominant kernel of the iteration: the single launch with the largest share of one policy_fre period
    (duration x launches per period) among the priced launches at the bench size; the backward entries are PAIRS of
    launches (rows pass + weights pass) and are listed in all_kernels only."""
    in_iter = {k: v for k, v in clinic.items() if "rate" in v and "@" not in k and not k.startswith("mlp_backward")}
    dom = max(in_iter, key=lambda n: in_iter[n]["us"] * in_iter[n].get("launches_per_period", 1))
    d = in_iter[dom]
    kernel = KERNEL_OF.get(dom.split("[")[0], dom)
    r = {"bound": d["bound"], "kernel": kernel, "entry_point": dom, "achieved": d["rate"], "peak": d["peak"],
         "unit": d["unit"], "frac": d["frac"],
         # (PMC counters of this workload's own launches: profiles/r04_pmc_traffic_<workload>.json)
         "traffic": pmc_traffic(kernel, d["n"], workload), "launch_us": d["us"],
         "units_per_launch": d["n"],
         "algorithmic_%s_per_launch" % ("bytes" if d["bound"] == "hbm" else "flops"): d["work"],
         "note": "dominant launch of the iteration at the bench size (latency-bound: %d units per launch); "
                 "all_kernels lists every launch of one policy_fre period with its own roofline" % d["n"],
         "all_kernels": {k: {kk: vv for kk, vv in v.items() if kk in ("us", "rate", "unit", "frac", "bound", "n",
                                                                     "launches_per_period", "regime", "frac_of_achievable",
                                                                     "moved_bytes_per_lane", "moved_bytes_per_sample", "moved_rate_gbs",
                                                                     "moved_frac_of_achievable", "env_steps_per_s", "kernel")}
                         for k, v in clinic.items()}}
    st = clinic.get("cartsafe_step_kernel@1M")
    if st is not None:
        r["hbm_streaming"] = {"kernel": "cartsafe_step_kernel", "bound": "hbm", "units_per_launch": st["n"],
                              "launch_us": st["us"], "achieved": st["rate"], "peak": HBM_PEAK_GBS, "unit": "GB/s",
                              "frac": st["frac"], "frac_of_achievable": st.get("frac_of_achievable"),
                              "achievable_peak": HBM_ACHIEVABLE_GBS, "regime": st.get("regime"),
                              "traffic": pmc_traffic("cartsafe_step_kernel", st["n"]),
                              "algorithmic_bytes_per_launch": st["work"],
                              # the launch MOVES 208 B per lane (ring padding + episode bookkeeping are outside SURVEY's 145 B): its
                              # own HBM rate is the achievable one -- the fraction above is the ratio of algorithmic to moved bytes
                              "moved_bytes_per_launch": st.get("moved_bytes_per_lane", 0) * st["n"],
                              "moved_rate": st.get("moved_rate_gbs"), "moved_frac_of_achievable": st.get("moved_frac_of_achievable")}
    return r


if __name__ == "__main__":
    main()
