"""The float64 chain of the constrained policy update (tests/update_f64.py) and the harness that reads ``agent.flat.grad`` between
the backward launches and the optimiser step, on the CPU: the chain against torch autograd, the harness on the oracle backend
(tests/oracle_backend.py: the generic launches' call order), and planted errors that the post-Adam checks of the suite let pass.
At embed_dim = hidden_dim = 256, the trainers' default width: the harness again, the target chain of the launches that keep their
next actions (update_f64.cart_target_chain) and the rollout's actions (update_f64.rollout_actions) on the oracle backend at the
seeds of tests/test_embed256_f64_gpu.py, and errors planted into a float32 stand-in of that chain.
"""
import numpy as np
import pytest
import torch

import envs_f64 as ef
import heads_f64 as hf
import mlp_f64 as mf
import oracle_backend as ob
import update_f64 as uf
from oracle import pendulum as opd
from test_train_step_golden import build_trainer

F64 = torch.float64
CPU = torch.device("cpu")


# ============================================================================================== the chain against autograd
def _params(kind, S, A, seed, n_out=1):
    spec = ("net", kind, S, A, 128, n_out, 1)
    return {k: v.to(F64) for k, v in mf.make_params(spec, seed, zero_col=False).items()}, spec


class _Net(object):
    """The same network twice: an Mlp64 for the chain and plain torch float64 leaves for autograd (masks as constants)."""

    def __init__(self, kind, S, A, seed, n_out=1, shared_with=None, head_gain=1.0):
        p, spec = _params(kind, S, A, seed, n_out)
        p["W1"] = p["W1"] * head_gain
        if shared_with is not None:                              # one state embedding for both networks (agent/flat.py)
            p["Ws"], p["bs"] = shared_with.leaf["Ws"], shared_with.leaf["bs"]
        self.leaf = {k: (v if v.requires_grad else v.clone().requires_grad_(True)) for k, v in p.items()}
        self.ref = mf.mlp64_of(spec, {k: v.detach() for k, v in self.leaf.items()})

    def __call__(self, s, a, m0, m1):
        """Forward with the ReLU masks m0 / m1 passed in as constants."""
        p = self.leaf
        x0 = s @ p["Ws"].t() + p["bs"]
        if a is not None:
            x0 = x0 + a @ p["Wa"].t() + p["ba"]
        h = (x0 * m0) @ p["W0"].t() + p["b0"]
        hr = h * m1
        out = [hr @ p["W1"].t() + p["b1"]]
        if "W1b" in p:
            out.append(hr @ p["W1b"].t() + p["b1b"])
        return torch.cat(out, dim=1)

    def masks(self, s, a):
        _, x0, h1 = self.ref.forward(s, a)
        return x0, h1, (x0 > 0).to(F64), (h1 > 0).to(F64)


def _env(envname, partial):
    """(EnvRef, Complete as a torch function, g as a torch function, state [B, S]): the constraints restated in torch for
    autograd from the same float32 constants (cartpole.py:369-379, pendulum.py:256-311)."""
    g = torch.Generator().manual_seed(3)
    B = 64
    if envname == "cart":
        from oracle import cartsafe as ocs
        table = ocs.Constants(partial).as_array()
        env = uf.EnvRef("cart", table, partial)
        t = torch.from_numpy(np.asarray(table, np.float32).astype(np.float64))
        C_p, C_o_inv, b, G, d = t[2], t[3], t[4], t[5:17].view(6, 2), t[17:23]
        state = torch.randn(B, 6, generator=g).float()

        def complete(s, ap):
            ao = (b - ap * C_p) * C_o_inv
            return torch.stack([ap, ao] if partial == 0 else [ao, ap], dim=1)

        def ineq(a):
            return a @ G.t() - d
        return env, complete, ineq, state
    env = uf.EnvRef("pend")
    th = torch.rand(B, generator=g) * 2 - 1
    state = torch.stack([torch.cos(th), torch.sin(th), torch.randn(B, generator=g), 1 + 0.1 * torch.randn(B, generator=g),
                         0.1 * torch.randn(B, generator=g)], dim=1).float()

    def complete(s, ax):
        s = s.to(F64)
        cs, sn, thd, l, ld = (s[:, i] for i in range(5))
        bb = -opd.M_DT * ld - (l * opd.M * thd * thd - opd.K * (l - opd.L0) - opd.M * opd.G * cs)
        return torch.stack([ax, (bb - ax * sn) * (1.0 / cs)], dim=1)

    def ineq(a):
        return ((a * a).sum(dim=1) - opd.MAX_SUMMATION).view(-1, 1)
    return env, complete, ineq, state


def _rel(got, ref):
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-300))


AUTOGRAD_CASES = [("ddpg", "cart", 0, True), ("ddpg", "cart", 1, False), ("sac", "cart", 1, False), ("sac", "cart", 0, True),
                  ("ddpg", "pend", 0, False), ("ddpg", "pend", 0, True), ("sac", "pend", 0, False)]
AUTOGRAD_WORST = 4e-15          # 10 x the measured figure: see the docstring below


@pytest.mark.parametrize("algo,envname,partial,shared", AUTOGRAD_CASES,
                         ids=["%s-%s%d-%s" % (a, e, p, "shared" if s else "separate") for a, e, p, s in AUTOGRAD_CASES])
def test_chain_equals_autograd(algo, envname, partial, shared):
    """critic_chain / ddpg_actor_chain / sac_actor_chain against torch autograd of the losses written as plain float64 torch
    (the ReLU masks, the clip mask, relu(g)'s mask and the split of min(Q1, Q2) passed in as constants), from float64 values that
    are consistent with each other (``exact``: no float32 rounding between the stages): the hand-derived chain and the kernels
    cannot share a mistake that autograd does not make.  RPODDPG and RPOSAC, CartSafe (partial 0 and 1) and SpringPendulum,
    shared and separate embeddings.  Achieved: the worst |chain - autograd| / max |gradient| over the tensors of a case is 1.9e-16
    to 4.0e-16 (the largest: RPODDPG on SpringPendulum, separate embeddings); asserted at 10 x that: 4e-15."""
    env, complete, ineq, state = _env(envname, partial)
    S, B = state.shape[1], state.shape[0]
    sac = algo == "sac"
    g = torch.Generator().manual_seed(11)
    # (RPOSAC: a mean head wide enough for the squashed samples to reach the constraints)
    actor = _Net("gauss" if sac else "actor", S, 0, 21, n_out=2 if sac else 1, head_gain=8.0 if sac else 1.0)
    critics = [_Net("add", S, 2, 31 + k, shared_with=actor if shared else None) for k in range(2 if sac else 1)]
    targets = [_Net("add", S, 2, 41 + k) for k in range(len(critics))]
    s64 = state.to(F64)
    action = torch.randn(B, 2, generator=g, dtype=F64)
    next_state, next_actions = torch.randn(B, S, generator=g, dtype=F64), torch.randn(B, 2, generator=g, dtype=F64)
    reward, done = torch.randn(B, generator=g, dtype=F64) * 2, (torch.rand(B, generator=g) < 0.2).to(F64)
    logp_next = torch.randn(B, generator=g, dtype=F64) if sac else None
    gamma, alpha = 0.5, 0.25                                      # (float32-exact: mlp_f64.td rounds them as the kernels' arguments)
    worst = 0.0
    # ---- critic half
    qn = [t.ref.forward(next_state, next_actions)[0].view(-1) for t in targets]
    y = reward + gamma * (1 - done) * ((torch.minimum(qn[0], qn[1]) - alpha * logp_next) if sac else qn[0])
    loss = 0.0
    chain = []
    for c in critics:
        x0, h1, m0, m1 = c.masks(s64, action)
        q = c(s64, action, m0, m1).view(-1)
        loss = loss + torch.nn.functional.smooth_l1_loss(q, y)
        chain.append(uf.critic_chain(c.ref, s64, action, x0, h1, q.detach(), qn[0], None, reward, done, gamma,
                                     qn[1] if sac else None, logp_next, alpha if sac else 0.0))
    leaves = [(c, k) for c in critics for k in sorted(c.leaf)]
    grads = torch.autograd.grad(loss, [c.leaf[k] for c, k in leaves])
    assert abs(float(loss.detach()) - sum(ch[1][0] for ch in chain)) <= 1e-14 * abs(float(loss.detach()))
    for (c, k), gr in zip(leaves, grads):
        ref = chain[critics.index(c)][0][k][0]
        if shared and sac and k in ("Ws", "bs"):                # (one tensor under both critics: autograd adds the two)
            ref = sum(ch[0][k][0] for ch in chain)
        worst = max(worst, _rel(ref.reshape(gr.shape), gr))
    # ---- policy half
    nu = (np.array([0.3, 0.0, 1.5, 0.2, 0.7, 0.05], np.float32) if envname == "cart" else np.array([0.37], np.float32))
    nu_t = torch.from_numpy(nu.astype(np.float64)).requires_grad_(True)
    scale, base, lo, hi = (10.0, 0.0, -10.0, 10.0) if envname == "cart" else (6.0, 0.0, -6.0, 6.0)
    noise = torch.randn(B, generator=g, dtype=F64)
    eps_t = scale                                                # (large: about a third of the rows clips)
    x0a, h1a, ma0, ma1 = actor.masks(s64, None)
    out = actor(s64, None, ma0, ma1)
    if sac:
        ls = torch.clamp(out[:, 1] - 3, hf.LS_MIN, hf.LS_MAX)
        yv = torch.tanh(out[:, 0] + noise * ls.exp())
        logp = -0.5 * noise * noise - ls - hf.HALF_LOG_2PI - torch.log(scale * (1 - yv * yv) + 1e-6)
        pre = scale * yv + base
    else:
        pre = scale * torch.tanh(out[:, 0]) + base + eps_t * noise
    inside = ((pre >= lo) & (pre <= hi)).detach()
    ap = torch.where(inside, pre, pre.detach().clamp(lo, hi))
    actions = complete(state, ap)
    acts = actions.detach()
    saved = [c.masks(s64, acts) for c in critics]
    qs = [c(s64, actions, sv[2], sv[3]).view(-1) for c, sv in zip(critics, saved)]
    gv = ineq(actions)
    viol = (gv > 0).detach()
    lag = ((gv * viol) @ nu_t).mean()
    if sac:
        w1 = ((qs[0] < qs[1]).to(F64) + 0.5 * (qs[0] == qs[1]).to(F64)).detach()
        loss = (alpha * logp - (w1 * qs[0] + (1 - w1) * qs[1])).mean() + lag
        ch = uf.sac_actor_chain(env, actor.ref, [c.ref for c in critics], s64, x0a, h1a, out.detach(), noise, (scale, base, lo, hi),
                                acts, [(sv[0], sv[1]) for sv in saved], w1, nu, alpha, shared, exact=True)
    else:
        loss = (-qs[0]).mean() + lag
        ch = uf.ddpg_actor_chain(env, actor.ref, critics[0].ref, s64, x0a, h1a, noise, eps_t, (scale, base, lo, hi), acts,
                                 saved[0][0], saved[0][1], nu, shared, exact=True)
        assert bool((ch["clipped"] == ~inside).all()) and 0.05 < float((~inside).double().mean()) < 0.95
    assert 0 < int(viol.any(dim=1).sum()) < B
    keys = sorted(actor.leaf)
    grads = torch.autograd.grad(loss, [actor.leaf[k] for k in keys] + [nu_t])
    assert abs(float(loss.detach()) - ch["loss"][0]) <= 1e-13 * max(1.0, abs(float(loss.detach())))
    for k, gr in zip(keys, grads):
        worst = max(worst, _rel(ch["grads"][k][0].reshape(gr.shape), gr))
    worst = max(worst, _rel(torch.from_numpy(ch["gnu"][0]), grads[-1]))
    print("chain vs autograd %s %s partial=%d %s: worst relative difference %.3g" % (algo, envname, partial, "shared" if shared else
                                                                                    "separate", worst))
    assert worst <= AUTOGRAD_WORST


def test_exact_inputs_of_the_env_stages_change_nothing_on_float32_values():
    """``exact=True`` of envs_f64's Lagrangian and Complete-backward (float64 inputs taken as they are) gives the same values and
    the same magnitude sums as the float32 form on float32-representable inputs: the keyword adds an input form, no arithmetic."""
    from oracle import cartsafe as ocs
    rng = np.random.RandomState(0)
    a = (rng.randn(64, 2) * 5).astype(np.float32)
    nu = np.array([0.3, 0.0, 1.5, 0.2, 0.7, 0.05], np.float32)
    obs = ef.pend_obs32(ef.pend_rows(64, seed=1)[0])
    for partial in (0, 1):
        table = ocs.Constants(partial).as_array()
        for x, y in ((ef.cart_lagrangian(ef.B64, table, partial, a, nu, 0.25), ef.cart_lagrangian(ef.B64, table, partial, a, nu, 0.25, exact=True)),):
            for k in ("g0", "g1"):
                assert np.array_equal(x[k].v, y[k].v) and np.array_equal(ef.B64.mag(x[k]), ef.B64.mag(y[k]))
        x, y = ef.cart_complete_bwd(ef.B64, table, partial, a), ef.cart_complete_bwd(ef.B64, table, partial, a, exact=True)
        assert np.array_equal(x.v, y.v) and np.array_equal(ef.B64.mag(x), ef.B64.mag(y))
    x, y = ef.pend_lagrangian(ef.B64, a, 0.37, 0.25), ef.pend_lagrangian(ef.B64, a, 0.37, 0.25, exact=True)
    assert np.array_equal(x["g0"].v, y["g0"].v) and np.array_equal(ef.B64.mag(x["g1"]), ef.B64.mag(y["g1"]))
    x, y = ef.pend_complete_bwd(ef.B64, obs, a), ef.pend_complete_bwd(ef.B64, obs, a, exact=True)
    assert np.array_equal(x.v, y.v) and np.array_equal(ef.B64.mag(x), ef.B64.mag(y))


# ============================================================================================ the harness, oracle backend
def _trainer(algo, envname, backend=ob, seed=5, **kw):
    torch.set_num_threads(1)
    torch.manual_seed(seed)
    tr = build_trainer(algo, envname, backend, CPU, fused=True, num_envs=64, use_graph=False, **kw)
    tr.vec.reset()
    tr.run_steps(5)                                              # (one policy step has happened, the ring holds 320 transitions)
    return tr


# every case of the GPU matrix the oracle backend can run (its launches are the generic chain)
NJU = dict(batch_size=64, init_nju=0.1)
EVOPF_SAC = [NJU, dict(batch_size=50, init_nju=0.1), dict(NJU, alpha=0.2), dict(NJU, automatic_entropy_tuning=True),
             dict(batch_size=64), dict(batch_size=64, init_nju=0.0)]
HARNESS_CASES = [("ddpg", "evopf256", dict(batch_size=64)), ("ddpg", "evopf256", dict(batch_size=50))] + \
                [("sac", "evopf256", kw) for kw in EVOPF_SAC] + \
                [("ddpg", "cart", {}), ("ddpg", "cart", dict(shared_param=False)), ("sac", "cart", {}),
                 ("ddpg", "pendulum", {}), ("sac", "pendulum", {}), ("ddpg", "cart_viol", {}), ("ddpg", "pendulum_viol", {}),
                 ("sac", "cart", dict(automatic_entropy_tuning=True)),
                 ("ddpg", "cart", dict(batch_size=250)), ("ddpg", "cart", dict(batch_size=100)), ("sac", "cart", dict(batch_size=250)),
                 ("sac", "cart", dict(batch_size=100)), ("ddpg", "pendulum", dict(batch_size=250)), ("sac", "pendulum", dict(batch_size=250)),
                 ("ddpg", "pendulum", dict(batch_size=272)), ("sac", "pendulum", dict(batch_size=272)),
                 ("ddpg", "cart", dict(batch_size=250, shared_param=False)), ("ddpg", "cart", dict(batch_size=100, shared_param=False))]


def _case_id(c):
    return "-".join([c[0], c[1]] + ["%s=%s" % kv for kv in sorted(c[2].items())])


@pytest.mark.parametrize("algo,envname,kw", HARNESS_CASES, ids=[_case_id(c) for c in HARNESS_CASES])
def test_harness_on_the_oracle_backend(algo, envname, kw):
    """The shipped trainer on tests/oracle_backend.py (fused=True: the generic launches' call order), cut open by
    update_f64.run_update and judged by update_f64.check_update -- the code the GPU test uses: every element of the critic, shared
    and actor slices of flat.grad and of nju.weight.grad within its bound, padding and the other optimiser's slice exactly 0,
    last_losses within theirs, gradmax exact, the ambiguous rows of every comparison under AMBIG_CAP; the seeds are the GPU
    file's, so the cap is known to hold for them before a device is asked.  (The oracle backend's
    float32 is torch's on the CPU: the ratios say the harness is right, not how good a kernel is -- the worst gradient ratio of
    any case is 0.005, d/d nu 0.16, the worst layer-local one 0.44, x0.)

    EVOPF-v0: RPODDPG at 64 and at 50 rows (ragged against the 16 rows per workgroup of the head kernels and the row tile of
    mlp_gemm), and RPOSAC (update_f64.evopf_sac_actor_chain) with non-zero multipliers at 64 and 50 rows, at alpha = 0.2, with
    automatic_entropy_tuning, with build_trainer's own arguments (EVOPF_HP: init_nju = 0.1 as well) and with multipliers of
    zero.  With init_nju given, at least one row violates and g_act, d/d nu in float64 and nju.weight.grad are not zero (42 of
    50 rows violate after the five iterations at seed 5, the GPU file's).  Worst ratios there: gradients 0.03, d/d nu 0.04."""
    tr = _trainer(algo, envname, **kw)
    snap = uf.run_update(tr)
    assert snap["path"] == ("generic", "generic")
    worst, info = uf.check_update(tr, snap)
    uf.report("oracle backend %s" % _case_id((algo, envname, kw)), worst)
    assert max(worst.values()) <= 1.0
    viol = info["violating"]
    if envname.endswith("_viol"):
        assert 0 < int(viol.sum()) < viol.size and float(np.abs(info["gnu"]).max()) > 0 and float(snap["grad_a"].abs().max()) > 0
    if kw.get("automatic_entropy_tuning"):
        assert "log_alpha" in worst and snap["log_alpha_grad"] != 0.0
    if kw.get("init_nju"):
        assert_multipliers_act(snap, info)


def assert_multipliers_act(snap, info):
    """Non-zero multipliers and a violated constraint: the Lagrangian's d/d action and d/d nu are not zero, in float64 and in
    what the launches left."""
    off = snap["nu_off"]
    assert int(info["violating"].sum()) > 0 and float(np.abs(info["gnu"]).max()) > 0.0 and info["g_act"] > 0.0
    assert float(snap["grad_a"][off[0]:off[1]].abs().max()) > 0.0


# ================================================================================================================ planted errors
SCALE = 1.0 + 2.0 ** -8


class _Plant(object):
    """oracle_backend with ONE error planted into the launches of the update (never into the repository); everything else is
    forwarded.  The buffers the harness reads back stay as the unplanted launch leaves them, so only flat.grad can tell."""

    def __init__(self, what):
        self.what, self.tr = what, None
        inner_td = ob.Td
        plant = self

        class Td(inner_td):
            def apply(self):
                dout = inner_td.apply(self).clone()              # (dq_out itself stays right)
                n = dout.shape[0]
                if plant.what == "dq_row" and plant.armed:
                    dout[7] = 0.0
                if plant.what == "padded_batch" and plant.armed:
                    dout *= n / (16.0 * ((n + 15) // 16))
                if plant.what.startswith("logp_components") and plant.armed:
                    # log pi(a'|s') with one of its 14 components left out of the sum ("crit.logp", dq_out and the loss
                    # partials stay right: a second prologue on buffers of its own hands the backward its dq)
                    lost = inner_td(self.q, self.qn1, self.qn2, self.logp - plant.logp_component(3), self.reward, self.done,
                                    self.alpha, self.gamma, torch.zeros_like(self.dq_out), torch.zeros_like(self.loss_partial))
                    dout = inner_td.apply(lost).clone()
                return dout
        self.Td = Td
        self.armed = False

    def __getattr__(self, name):
        return getattr(ob, name)

    def mlp_backward(self, d, s, a, x0, h1, dout, dh, dx0, da=None, param_grads=True, first_layer_state_only=False, **kw):
        if self.armed and self.what == "shared_embedding" and first_layer_state_only:
            param_grads = False                                  # the critic's first-layer state gradient never reaches the shared slice
        if self.armed and self.what == "padded_batch" and kw.get("td") is None and da is not None:
            n = dout.shape[0]
            dout = dout * (n / (16.0 * ((n + 15) // 16)))        # d mean(-Q) / dQ with the padded batch's 1 / B
        return ob.mlp_backward(d, s, a, x0, h1, dout, dh, dx0, da, param_grads, first_layer_state_only, **kw)

    def gauss_head_bwd(self, raw, eps, dap, dlogp, *rest):
        return ob.gauss_head_bwd(raw, eps, dap, dlogp * (SCALE if self.armed and self.what == "alpha_over_b" else 1.0), *rest)

    def arm(self, tr):
        """Switch the error on (after the warm-up iterations, which both runs share bit for bit)."""
        self.armed, self.tr = True, tr
        B, k = tr.batch_size, tr.kernels
        if self.what in ("lagrangian_da", "lagrangian_da_3way", "twin_da"):
            inner = k.complete_bwd

            def complete_bwd(obs, grad_action, grad_ap, action=None):
                if self.what == "twin_da":                       # ((da1 + da2) + g_act: the second critic's share never arrives)
                    return inner(obs, grad_action - tr.fused.buf("da2", B, k.action_dim), grad_ap, action=action)
                g_act = tr.fused.buf("g_act", B, k.action_dim)
                return inner(obs, grad_action + (SCALE - 1.0) * g_act, grad_ap, action=action)   # (da + g_act: the Lagrangian's share scaled)
            k.complete_bwd = complete_bwd
        if self.what.startswith("alpha_over_b_evopf"):           # (the state-dependent box: the head's backward is the env's own)
            inner_head = k.gauss_head_bwd
            k.gauss_head_bwd = lambda obs, raw, eps, dap, dlogp, draw: inner_head(obs, raw, eps, dap, dlogp * SCALE, draw)

    def logp_component(self, j):
        """Component j of log pi(a'|s') of the critic update that is running, [B] float32: from the heads, the draw and the batch
        that launch read."""
        tr = self.tr
        B = tr.batch_size
        next_state = tr.buffer.split(tr._batch)["next_state"]
        head = uf.evopf_gauss(next_state, tr.fused.buf("crit.raw", B, 2 * tr.kernels.partial_dim), tr._noise_b)
        return head["fw"]["logp"][:, j].float()


PLANTS = [("dq_row", "ddpg", "cart", {}), ("lagrangian_da", "ddpg", "cart_viol", {}), ("shared_embedding", "ddpg", "cart", {}),
          ("padded_batch", "ddpg", "cart", dict(batch_size=250)), ("alpha_over_b", "sac", "cart", {})] + \
         [(w, "sac", "evopf256", dict(NJU, alpha=0.2)) for w in ("twin_da", "lagrangian_da_3way", "alpha_over_b_evopf")] + \
         [("logp_components", "sac", "evopf256", dict(NJU, alpha=0.2, gamma=0.05)), ("logp_components@0.01", "sac", "evopf256", dict(NJU, alpha=0.01))]
GRAD_KEYS = ("critic ", "actor ", "shared ", "nu")


def _grad_ratio(worst):
    return max(v for k, v in worst.items() if k.startswith(GRAD_KEYS))


@pytest.mark.parametrize("what,algo,envname,kw", PLANTS, ids=[p[0] for p in PLANTS])
def test_planted_errors_are_found_in_the_flat_gradient(what, algo, envname, kw):
    """Errors of the kind hand-written pipelines make, each planted into the backend proxy of an oracle-backend trainer
    behind the buffers the harness reads back, so that ONLY the flat-gradient check can see it -- and it must: the worst
    |err| / bound over the gradient slices goes above 1.  Beside it, the worst parameter shift after the optimiser steps of the
    same update against the unplanted run: what the post-Adam checks of the suite would have had to see, next to their
    tolerances (the four-update fixtures at atol 2e-6 on the CPU and 5e-6 on the GPU; the path-equality tests at 1e-7 to 2e-6).
    Printed, not asserted.  Measured (gradient ratio unplanted -> planted | post-Adam shift; the shift is that of ONE update six
    iterations after initialisation, where Adam's second moments are young and its steps at their largest -- the two errors
    that do move a parameter by more than the fixtures' tolerance here, a lost row and a lost embedding share, are 0.4 % and a
    few % of the gradient; the scaled Lagrangian and alpha / B sit under the GPU tests' 5e-6, the padded 1 / B under everything):

      dq_row            one batch row's dq zeroed before the critic backward        0.0007 -> 103 (critic dW0) | 4.5e-5
      lagrangian_da     the Lagrangian's d/d action scaled by 1 + 2^-8              0.0022 -> 32 (actor dW0) | 4.8e-6
      shared_embedding  the critic's share of the shared embedding left out         0.0007 -> 583 (shared dbs) | 1.6e-4
      padded_batch      1 / B taken as 1 / (16 ceil(B / 16)) at B = 250             0.0007 -> 49 (actor dW0) | 3.0e-8
      alpha_over_b      RPOSAC: alpha / B of the Gaussian head's backward x (1 + 2^-8)   0.0017 -> 13 (actor dW1b) | 4.4e-6

    RPOSAC on EVOPF-v0 (init_nju = 0.1, alpha = 0.2, 64 rows), the places where that update differs from everything above:

      twin_da             the second critic's d/d action dropped from complete_bwd     0.03 -> 300 (actor dW1) | 1.7e-4
      lagrangian_da_3way  the Lagrangian's share of the three-way add x (1 + 2^-8)      0.03 -> 5.1 (actor dW1) | 1.3e-5
      alpha_over_b_evopf  alpha / B of the 14-wide head's backward x (1 + 2^-8)         0.03 -> 546 (actor dW1b) | 1.3e-5
                          (printed beside it: the same error at the script's alpha = 0.001 lands at 0.022 -> 59, still found)
      logp_components     one of the 14 components left out of log pi(a'|s') before Td  0.04 -> 78 (critic dW0) | 3.9e-6
                          at gamma = 0.05.  At the trainer's default discount, 0.95, this error cannot be found by anything at
                          alpha = 0.2: alpha log pi(a'|s') is 8.5 to 10.4 (log pi 42 to 52, a component -1.3 to 5.0) against
                          rewards of -1 to -3 and q of -0.7, so every row's TD error is 8.6 to 11.7, beyond the Huber clamp, and
                          stays above 7.6 whichever component is left out: dq is +-1 / B whatever log pi is, and the critic
                          gradients of the planted and the unplanted run are equal bit for bit (printed beside it: 0.03 -> 0.03;
                          the device shows the same saturation, a dq ratio of 0 in tests/test_update_f64_gpu.py's
                          alpha = 0.2 case).  The plant needs rows inside the clamp, so this one trainer is built with
                          gamma = 0.05: gamma alpha log pi is then about 0.5, of the size of the rewards, alpha and the
                          multipliers as in the three above.
      logp_components@0.01  the same error at gamma = 0.95 and alpha = 0.01, where rows are inside the clamp   0.02 -> 4.0 (critic dW0)
                          (at the script's alpha = 0.001 it lands at 0.41: a 14th of alpha log pi is then 0.003 in a TD error
                          of 0.5 to 2, inside the bound of the chain)
    """
    runs = _planted_runs(what, algo, envname, kw)
    clean, bad = runs[False][0], runs[True][0]
    shift = float((runs[True][1] - runs[False][1]).abs().max())
    print("planted %-16s gradient ratio %.3g -> %.3g (%s) | worst post-Adam parameter shift %.3g"
          % (what, _grad_ratio(clean), _grad_ratio(bad), max((k for k in bad if k.startswith(GRAD_KEYS)), key=bad.get), shift))
    assert _grad_ratio(clean) <= 1.0 and not runs[False][2]
    # the buffer next to the planted stage is the unplanted launch's: only the gradient can tell
    near = dict(dq_row="dq", padded_batch="dq", shared_embedding="dq", lagrangian_da="g_act", alpha_over_b="logp", twin_da="g_act",
                lagrangian_da_3way="g_act", alpha_over_b_evopf="logp", logp_components="logp")[what.split("@")[0]]
    assert bad[near] == clean[near] <= 1.0, (near, bad[near], clean[near])
    if what.startswith("logp_components"):                       # (found by the critic slices; dq as the launch left it stays right)
        assert bad["dq"] == clean["dq"] <= 1.0
        critic = max(v for k, v in bad.items() if k.startswith("critic "))
        assert critic > 1.0, "log pi(a'|s') less one component stays inside the critic slices' bound: %.3g (see the docstring)" % critic
    assert _grad_ratio(bad) > 1.0, "the planted error stays inside the bound: %.3g" % _grad_ratio(bad)
    if what == "logp_components":                                # (printed only: the same error at the default discount)
        low = _planted_runs(what, algo, envname, {k: v for k, v in kw.items() if k != "gamma"})
        print("planted %-16s at gamma = 0.95: gradient ratio %.3g -> %.3g" % (what, _grad_ratio(low[False][0]), _grad_ratio(low[True][0])))
    if what == "alpha_over_b_evopf":                             # (printed only: the same error at the script's alpha)
        low = _planted_runs(what, algo, envname, dict(kw, alpha=0.001))
        print("planted %-16s at alpha = 0.001: gradient ratio %.3g -> %.3g" % (what, _grad_ratio(low[False][0]), _grad_ratio(low[True][0])))


def _planted_runs(what, algo, envname, kw):
    """{planted: (worst, parameters after the optimiser steps, fails)} of the same update without and with the error."""
    runs = {}
    for planted in (False, True):
        backend = _Plant(what)
        tr = _trainer(algo, envname, backend=backend, **kw)
        assert tr.fused.backend is backend and tr.backend is backend
        if planted:
            backend.arm(tr)
        snap = uf.run_update(tr)
        worst, info = uf.check_update(tr, snap, strict=False)
        tr._actor_step(snap["actor_out"])
        runs[planted] = (worst, torch.cat([tr.agent.flat.data.clone(), tr.agent.critic_target_flat.clone()]), info["fails"])
    return runs


# ================================================================================== the 256-wide networks (the default width)
E256 = dict(embed_dim=256, hidden_dim=256)
HARNESS_256 = [(a, e, dict(kw, batch_size=b)) for a, e, kw in (("ddpg", "cart", {}), ("sac", "cart", {}), ("sac", "pendulum", {}))
               for b in (100, 17)]


@pytest.mark.parametrize("algo,envname,kw", HARNESS_256, ids=[_case_id(c) for c in HARNESS_256])
def test_harness_on_the_oracle_backend_at_256(algo, envname, kw):
    """The harness at embed_dim = hidden_dim = 256, the trainers' default width, on the oracle backend (the generic chain): what
    test_harness_on_the_oracle_backend judges, and on CartSafe qn against the recomputed target chain as well
    (update_f64.cart_target_chain, the form in which the launches that keep their next actions are judged), with the TD chain
    run from it."""
    tr = _trainer(algo, envname, **dict(E256, **kw))
    assert tr.fused.descs["actor"].E == 256
    snap = uf.run_update(tr)
    assert snap["path"] == ("generic", "generic")
    worst, info = uf.check_update(tr, snap, target_chain=(envname == "cart"))
    uf.report("oracle backend, 256 wide, %s" % _case_id((algo, envname, kw)), worst)
    assert ("qn target chain" in worst) == (envname == "cart")
    assert max(worst.values()) <= 1.0


# the seeds, lanes, warm-up steps and batches of tests/test_embed256_f64_gpu.py: the reference alone must stay within AMBIG_CAP there
CAP_UPDATE = [(a, dict(kw, batch_size=b)) for a, kw in (("ddpg", {}), ("ddpg", dict(shared_param=False)), ("sac", {}))
              for b in (256, 250, 100, 17, 1)]


@pytest.mark.parametrize("algo,kw", CAP_UPDATE, ids=[_case_id((c[0], "cart", c[1])) for c in CAP_UPDATE])
def test_target_chain_ambiguity_on_the_oracle_backend(algo, kw):
    """CartSafe at 256: the share of rows whose target-chain projection is ambiguous (a clip, stop or mask decision that differs
    over ap +- delta) on the oracle backend at the GPU cases' seeds and batches, under AMBIG_CAP -- a condition on the reference
    and the seeds, known to hold before a device is asked -- and the oracle backend's own qn within the chain's bound."""
    tr = _trainer(algo, "cart", **dict(E256, **kw))
    snap = uf.run_update(tr, critic_only=True)
    chain = uf.cart_target_chain(tr, snap, uf.EnvRef.of(tr.kernels), uf.trainer_box(tr))
    share = float(chain["ambiguous"].double().mean())
    r = uf.target_qn_ratio(chain, [c["qn"] for c in snap["critic"]]) if share < 1.0 else 0.0
    print("target chain %s: ambiguous share %.3g (cap %.3g), iterations up to %d, qn ratio %.3g"
          % (_case_id((algo, "cart", kw)), share, uf.AMBIG_CAP, int(chain["iters"].max()), r))
    assert share <= uf.AMBIG_CAP and r <= 1.0


ROLL = [(a, e, n) for a, e in (("sac", "cart"), ("sac", "pendulum"), ("ddpg", "cart")) for n in (1, 17, 100)]


@pytest.mark.parametrize("algo,envname,n", ROLL, ids=["%s-%s-%d" % c for c in ROLL])
def test_rollout_actions_on_the_oracle_backend(algo, envname, n):
    """update_f64.rollout_actions on the oracle backend's vector step (the stepwise sequence) at 256, at the lanes and steps of
    the GPU cases: the stored actions within the bound, the ambiguous share within AMBIG_CAP."""
    tr = _rollout_trainer(algo, envname, n)
    obs, t, sub, params = tr.vec.obs.clone(), int(tr.vec.ctrl[0]), int(tr.vec.ctrl[2]), uf.read_params(tr)
    tr._rollout(False)
    res = uf.rollout_actions(tr, params, obs, tr.vec.action, t, sub, tr.vec.env_id_base)
    share = float(res["ambiguous"].mean())
    print("rollout %s %s n=%d t=%d: ratio %.3g, ambiguous share %.3g" % (algo, envname, n, t, res["ratio"], share))
    assert t >= 1 and share <= uf.AMBIG_CAP and res["ratio"] <= 1.0


def _rollout_trainer(algo, envname, n, steps=3):
    torch.set_num_threads(1)
    torch.manual_seed(5)
    tr = build_trainer(algo, envname, ob, CPU, fused=True, num_envs=n, use_graph=False, batch_size=16, **E256)
    tr.vec.reset()
    tr.run_steps(steps)
    return tr


def _mlp32(p, s, a=None, drop_rows=None, drop_cols=None):
    """A network in plain float32 torch (the stand-in of a launch).  drop_rows / drop_cols: the hidden layer of those rows leaves
    those embedding columns out -- one k-step of a tile lost."""
    x0 = s @ p["Ws"].t() + p["bs"]
    if a is not None:
        x0 = x0 + a @ p["Wa"].t() + p["ba"]
    r0 = torch.relu(x0)
    h1 = r0 @ p["W0"].t() + p["b0"]
    if drop_rows is not None:
        keep = torch.ones(r0.shape[1], dtype=torch.bool)
        keep[drop_cols] = False
        h1[drop_rows] = r0[drop_rows][:, keep] @ p["W0"][:, keep].t() + p["b0"]
    r1 = torch.relu(h1)
    out = [r1 @ p["W1"].view(1, -1).t() + p["b1"]]
    if p.get("W1b") is not None:
        out.append(r1 @ p["W1b"].view(1, -1).t() + p["b1b"])
    return torch.cat(out, dim=1)


def _proposal32(tr, p, obs, eps, box, plant, name):
    """The basic action in float32: the tanh box of the deterministic actor (+ the caller's exploration) or the Gaussian head at the
    draw ``eps``.  plant "ls_from_mean": the head reads its log-std from the mean's column."""
    scale, base, lo, hi = box
    raw = _mlp32(p[name], obs)
    if tr.sac:
        ls = raw[:, 0 if plant == "ls_from_mean" else 1]
        return hf.gauss_head(raw[:, 0], ls, eps, scale, base, lo, hi, dtype=torch.float32)["ap"].numpy()
    return (np.float32(scale) * torch.tanh(raw[:, 0]) + np.float32(base)).numpy()


def _target_qn32(tr, snap, plant=None):
    """The target chain pi(s') -> head -> Complete -> Proj -> Q_targ in float32 (plain torch and envs_f64.cart_project_f32: a
    stand-in of the launch that shares no code with the float64 chain), with ONE error planted:
      k_step        Q_targ's hidden layer leaves 4 of the 256 embedding columns out for the rows of the second tile
      uncompleted   the rows of the ragged last tile keep a' = (ap, 0): neither completed nor projected
      ls_from_mean  RPOSAC: the Gaussian head reads its log-std from the mean's column
      q_at_s        Q_targ is evaluated at (s, a') in place of (s', a')"""
    state, _, next_state = snap["cols"][:3]
    p0, env, box = snap["params0"], uf.EnvRef.of(tr.kernels), uf.trainer_box(tr)
    B, K = state.shape[0], int(tr.max_steps)
    ap = _proposal32(tr, p0, next_state, snap["rec"].get("eps_next"), box, plant, "actor" if tr.sac else "actor_target")
    planes, _ = ef.cart_project_f32(env.table, env.partial, ap, K, tr.corr_lr, tr.corr_eps, 0.0)
    a = planes[K][:, :2].copy()
    if plant == "uncompleted":
        last = np.arange(16 * (B // 16), B)
        assert 0 < last.size < 16
        a[last] = ef.cart_join(env.partial, ap[last], np.zeros(last.size, np.float32))
    a = torch.from_numpy(a)
    at = state if plant == "q_at_s" else next_state
    drop = dict(drop_rows=torch.arange(16, 32), drop_cols=torch.arange(128, 132)) if plant == "k_step" else {}
    return [_mlp32(p0[t], at, a, **drop).view(-1) for _, t in uf.critic_names(tr)]


TARGET_PLANTS = [("k_step", "ddpg"), ("uncompleted", "ddpg"), ("ls_from_mean", "sac"), ("q_at_s", "ddpg")]


@pytest.mark.parametrize("what,algo", TARGET_PLANTS, ids=[p[0] for p in TARGET_PLANTS])
def test_planted_errors_are_found_in_the_target_values(what, algo):
    """Four errors of the kind a row-tile pipeline makes in the chain it keeps to itself, planted into a float32 stand-in of the
    launch's qn (never into the repository's kernels) on CartSafe at 256 wide, 100 rows: each lands above 1 x the bound of
    update_f64.cart_target_chain while the unplanted stand-in -- and the oracle backend's own qn -- stay below it.
    Measured, worst |qn - float64| / bound, unplanted -> planted, under the four forms of the bound (update_f64.cart_target_chain):

                      "path" (asserted)     "corners"            "running"            "chain" (the first form)
      k_step          0.00014 -> 21         0.00009 -> 11        5.8e-7 -> 0.068      9.9e-8 -> 0.013
      uncompleted     0.00014 -> 1.7        0.00009 -> 0.93      5.8e-7 -> 0.0043     9.9e-8 -> 0.0007
      ls_from_mean    0.00019 -> 21         0.00014 -> 13        6.0e-7 -> 0.10       8.6e-8 -> 0.016
      q_at_s          0.00014 -> 690        0.00009 -> 369       5.8e-7 -> 1.4        9.9e-8 -> 0.29

    The chain form lets every one of them pass and the running form three: the sensitivity with every weight in absolute value,
    |W1| |W0| |Wa| delta_a, is some hundred times the network's response to delta_a.  The corners of the box a' +- delta_a leave
    the path Complete keeps a' on, and let the uncompleted rows pass (the critic of a fresh trainer hardly answers to a').  Hence
    "path".  The uncompleted rows stay the thinnest: 4 rows, an a' that is off by 0.1 to 0.3 where delta_a is 0.003 to 0.006."""
    tr = _trainer(algo, "cart", **dict(E256, batch_size=100))
    snap = uf.run_update(tr, critic_only=True)
    env, box = uf.EnvRef.of(tr.kernels), uf.trainer_box(tr)
    clean32, bad32 = _target_qn32(tr, snap), _target_qn32(tr, snap, what)
    line = []
    for bounds in ("path", "corners", "running", "chain"):
        chain = uf.cart_target_chain(tr, snap, env, box, bounds=bounds)
        assert float(chain["ambiguous"].double().mean()) <= uf.AMBIG_CAP
        own = uf.target_qn_ratio(chain, [c["qn"] for c in snap["critic"]])
        clean, bad = uf.target_qn_ratio(chain, clean32), uf.target_qn_ratio(chain, bad32)
        line.append("%s %.3g -> %.3g" % (bounds, clean, bad))
        assert own <= 1.0 and clean <= 1.0, (bounds, own, clean)
        if bounds == uf.TARGET_BOUNDS:
            assert bad > 1.0, "the planted error stays inside the bound: %.3g" % bad
    print("planted %-13s qn ratio unplanted -> planted: %s" % (what, " | ".join(line)))


def test_planted_log_std_column_is_found_in_the_rollout_actions():
    """RPOSAC's rollout on CartSafe at 256 wide, 17 lanes: a float32 stand-in of the vector step's policy whose Gaussian head reads
    its log-std from the mean's column lands above 1 x the bound of update_f64.rollout_actions, the unplanted stand-in and the
    oracle backend's own actions below it.  Measured: 0.00008 -> 52."""
    tr = _rollout_trainer("sac", "cart", 17)
    obs, t, sub, params = tr.vec.obs.clone(), int(tr.vec.ctrl[0]), int(tr.vec.ctrl[2]), uf.read_params(tr)
    tr._rollout(False)
    env, box = uf.EnvRef.of(tr.kernels), uf.trainer_box(tr)
    eps = uf.rollout_noise(tr, 17, t, sub, tr.vec.env_id_base)
    got = {}
    for plant in (None, "ls_from_mean"):
        ap = _proposal32(tr, params, obs, eps, box, plant, "actor")
        planes, _ = ef.cart_project_f32(env.table, env.partial, ap, int(tr.max_steps), tr.corr_lr, tr.corr_eps, 0.0)
        got[plant] = uf.rollout_actions(tr, params, obs, planes[int(tr.max_steps)][:, :2], t, sub, tr.vec.env_id_base)["ratio"]
    own = uf.rollout_actions(tr, params, obs, tr.vec.action, t, sub, tr.vec.env_id_base)["ratio"]
    print("planted ls_from_mean  rollout action ratio %.3g -> %.3g (the oracle backend's own %.3g)" % (got[None], got["ls_from_mean"], own))
    assert own <= 1.0 and got[None] <= 1.0 < got["ls_from_mean"]


# ============================================================================================================ EVOPF-v0
def test_evopf_chain_equals_autograd_around_the_oracle_completion():
    """evopf_actor_chain (RPODDPG on EVOPF-v0) against torch autograd of mean(-Q(s, a)) + the Lagrangian term in a, the backward of
    Complete taken from oracle/evopf.py (complete_partial_bwd: other code than evopf_f64.complete_bwd_ref, held to the reference's
    autograd by the oracle's own tests), and autograd again through clip and tanh box into the actor -- Newton's completion is an
    implicit function, autograd cannot run through it.  Actions and states are float32 values (what the chain reads); the oracle's
    backward is given the Jacobian of the float32 table (evopf_f64.dense_jac, equal to oracle/evopf.py's eq_jac up to the table's
    rounding, asserted) and the Lagrangian the table's bounds, so both sides state the same problem.  Achieved: actor gradients
    agree to 7.3e-16 of max |gradient| (two solves of the 22 x 22 system), asserted at 10 x that; d/d nu is equal to the last bit
    (the same sums of the same float64 terms), asserted within two float64 roundings."""
    import evopf_f64 as vf
    from oracle import evopf as oe
    B, g = 32, torch.Generator().manual_seed(2)
    s32 = oe.reset(7, np.arange(B), np.zeros(B, np.int64)).astype(np.float32)
    s64 = torch.from_numpy(s32.astype(np.float64))
    actor = _Net("actor", 57, 0, 51)
    hd = 14                                                     # a 14-wide head on the 128-wide test network
    u = lambda *shape: (torch.rand(*shape, generator=g, dtype=F64) * 2 - 1) / 16      # noqa: E731
    actor.leaf["W1"], actor.leaf["b1"] = u(hd, 256).requires_grad_(True), u(hd).requires_grad_(True)
    actor.ref = mf.Mlp64({k: v.detach() for k, v in actor.leaf.items()}, 57, 0, 128, 256, head_dim=hd)
    cp = {k: v.to(F64) for k, v in mf.make_params(("c", "cat", 57, 43, 128, 1, 1), 52, zero_col=False).items()}
    critic = mf.Mlp64(cp, 57, 43, 128, 256, cat=True)
    lo, hi, scale, base, _, _ = hf.evopf_box(s32)
    noise = torch.randn(B, 14, generator=g, dtype=F64).float()
    eps_t = 0.5
    x0a, h1a, m0, m1 = actor.masks(s64, None)
    raw = actor(s64, None, m0, m1)
    pre = scale * torch.tanh(raw) + base + eps_t * noise.to(F64)
    inside = ((pre >= lo) & (pre <= hi)).detach()
    ap = torch.where(inside, pre, pre.detach().clamp(lo, hi))
    assert 0.02 < float((~inside).double().mean()) < 0.98
    acts = oe.project(s32.astype(np.float64), ap.detach().numpy(), 0, 0.0, 1e-5, 0.0)[0].astype(np.float32)
    a_var = torch.from_numpy(acts.astype(np.float64)).requires_grad_(True)
    nu = (0.05 + 0.2 * torch.rand(58, generator=g)).float().numpy()
    nu_t = torch.from_numpy(nu.astype(np.float64)).requires_grad_(True)
    J = torch.from_numpy(oe.ineq_jac())
    # (constraint bounds and admittances from the float32 table the kernels read, on both sides: the oracle's float64 case data
    #  would differ from it by half an eps32)
    tab = vf.Tab(vf.B64E, vf.consts_table())
    resid = vf.val(vf.B64E, vf.ineq_resid(vf.B64E, tab, vf.cols(vf.B64E, s32), vf.cols(vf.B64E, acts)))
    const = torch.from_numpy(resid) - a_var.detach() @ J.t()
    gv = a_var @ J.t() + const
    viol = (gv > 0).detach()
    assert 0 < int(viol.any(dim=1).sum())
    x0c = torch.cat([s64 @ cp["Ws"].t() + cp["bs"], a_var @ cp["Wa"].t() + cp["ba"]], dim=1)
    h1c = torch.relu(x0c) @ cp["W0"].t() + cp["b0"]
    q = torch.relu(h1c) @ cp["W1"].t() + cp["b1"]
    loss = (-q).mean() + ((gv * viol) @ nu_t).mean()
    dl, dnu = torch.autograd.grad(loss, [a_var, nu_t])
    jac = vf.dense_jac(vf.consts_table(), acts)[0]
    np.testing.assert_allclose(jac, oe.eq_jac(acts.astype(np.float64)), rtol=0, atol=1e-5)      # (the same Jacobian, table rounding apart)
    jn = jac[:, oe.GRID.keep_constr][:, :, oe.GRID.newton_vars]
    dz = torch.from_numpy(oe.complete_partial_bwd(dl.numpy(), jac, jn))
    keys = sorted(actor.leaf)
    grads = torch.autograd.grad(ap, [actor.leaf[k] for k in keys], grad_outputs=dz)
    ch = uf.evopf_actor_chain(vf.consts_table(), actor.ref, critic, s64, x0a, h1a, raw.detach(), noise, eps_t, torch.from_numpy(acts),
                              x0c.detach(), h1c.detach(), nu)
    assert bool((ch["clipped"] == ~inside).all())
    worst = max(_rel(ch["grads"][k][0].reshape(gr.shape), gr) for k, gr in zip(keys, grads))
    wnu = _rel(torch.from_numpy(ch["gnu"][0]), dnu)
    print("evopf chain vs autograd around the oracle's completion: actor gradients %.3g, d/d nu %.3g" % (worst, wnu))
    assert worst <= 8e-15 and wnu <= 2 * 2.0 ** -52


def test_evopf_sac_chain_equals_autograd_around_the_oracle_completion():
    """evopf_sac_actor_chain (RPOSAC on EVOPF-v0) against torch autograd of mean(alpha log pi - min(Q1, Q2)) + the Lagrangian term:
    the SAC twin of the test above.  The squashed Gaussian is written out here in plain torch (14 components in the
    state-dependent box, log pi summed over them), the two concatenating critics and the Lagrangian are differentiated by
    autograd in the action, Complete's backward is oracle/evopf.py's (complete_partial_bwd), and autograd runs again from the
    sampled ap and from log pi into the actor's two 14-wide heads.  alpha = 0.25 and B = 32, so alpha / B is a float32 value (the
    chain rounds it as the kernel's argument).  Achieved: the actor gradients agree to 2.6e-16 of max |gradient|; asserted at the
    tolerance of the test above (8e-15: the same two solves of the 22 x 22 system), d/d nu within two float64 roundings."""
    import evopf_f64 as vf
    from oracle import evopf as oe
    B, g, alpha, hd = 32, torch.Generator().manual_seed(4), 0.25, 14
    s32 = oe.reset(7, np.arange(B), np.zeros(B, np.int64)).astype(np.float32)
    s64 = torch.from_numpy(s32.astype(np.float64))
    actor = _Net("gauss", 57, 0, 61, n_out=2)
    u = lambda *shape: (torch.rand(*shape, generator=g, dtype=F64) * 2 - 1) / 16      # noqa: E731
    for w, b in (("W1", "b1"), ("W1b", "b1b")):
        actor.leaf[w], actor.leaf[b] = u(hd, 256).requires_grad_(True), u(hd).requires_grad_(True)
    b1b = actor.leaf["b1b"].detach() - 0.5                      # (log-stds around -3.5: a visible sample spread ...)
    b1b[:2] += 2.5                                              # (... and two components beyond the upper clamp at -2)
    actor.leaf["b1b"] = b1b.requires_grad_(True)
    actor.ref = mf.Mlp64({k: v.detach() for k, v in actor.leaf.items()}, 57, 0, 128, 256, n_out=2, head_dim=hd)
    cps = [{k: v.to(F64) for k, v in mf.make_params(("c", "cat", 57, 43, 128, 1, 1), 62 + k, zero_col=False).items()} for k in range(2)]
    critics = [mf.Mlp64(cp, 57, 43, 128, 256, cat=True) for cp in cps]
    lo, hi, scale, base, _, _ = hf.evopf_box(s32)
    noise = torch.randn(B, hd, generator=g, dtype=F64).float()
    x0a, h1a, m0, m1 = actor.masks(s64, None)
    raw = actor(s64, None, m0, m1)
    e = noise.to(F64)
    lsr = raw[:, hd:] - 3.0
    ls = torch.clamp(lsr, hf.LS_MIN, hf.LS_MAX)
    assert 0 < int((lsr > hf.LS_MAX).sum()) < lsr.numel()
    y = torch.tanh(raw[:, :hd] + e * ls.exp())
    logp = (-0.5 * e * e - ls - hf.HALF_LOG_2PI - torch.log(scale * (1 - y * y) + 1e-6)).sum(1)
    ap = torch.clamp(scale * y + base, min=lo, max=hi)
    acts = oe.project(s32.astype(np.float64), ap.detach().numpy(), 0, 0.0, 1e-5, 0.0)[0].astype(np.float32)
    a_var = torch.from_numpy(acts.astype(np.float64)).requires_grad_(True)
    nu = (0.05 + 0.2 * torch.rand(58, generator=g)).float().numpy()
    nu_t = torch.from_numpy(nu.astype(np.float64)).requires_grad_(True)
    J = torch.from_numpy(oe.ineq_jac())
    tab = vf.Tab(vf.B64E, vf.consts_table())                    # (the float32 table's bounds on both sides, as above)
    resid = vf.val(vf.B64E, vf.ineq_resid(vf.B64E, tab, vf.cols(vf.B64E, s32), vf.cols(vf.B64E, acts)))
    gv = a_var @ J.t() + (torch.from_numpy(resid) - a_var.detach() @ J.t())
    viol = (gv > 0).detach()
    assert 0 < int(viol.any(dim=1).sum())
    qs, saved = [], []
    for cp in cps:
        x0c = torch.cat([s64 @ cp["Ws"].t() + cp["bs"], a_var @ cp["Wa"].t() + cp["ba"]], dim=1)
        h1c = torch.relu(x0c) @ cp["W0"].t() + cp["b0"]
        qs.append((torch.relu(h1c) @ cp["W1"].t() + cp["b1"]).view(-1))
        saved.append((x0c.detach(), h1c.detach()))
    w1 = ((qs[0] < qs[1]).to(F64) + 0.5 * (qs[0] == qs[1]).to(F64)).detach()
    assert 0 < int(w1.sum()) < B                                # (both critics take rows)
    lag = ((gv * viol) @ nu_t).mean()
    ent = (alpha * logp).mean()
    dl, dnu = torch.autograd.grad((-(w1 * qs[0] + (1 - w1) * qs[1])).mean() + lag, [a_var, nu_t])
    jac = vf.dense_jac(vf.consts_table(), acts)[0]
    jn = jac[:, oe.GRID.keep_constr][:, :, oe.GRID.newton_vars]
    dz = torch.from_numpy(oe.complete_partial_bwd(dl.numpy(), jac, jn))
    keys = sorted(actor.leaf)
    grads = torch.autograd.grad([ap, ent], [actor.leaf[k] for k in keys], grad_outputs=[dz, torch.ones((), dtype=F64)])
    ch = uf.evopf_sac_actor_chain(vf.consts_table(), actor.ref, critics, s64, x0a, h1a, raw.detach(), noise, torch.from_numpy(acts),
                                  saved, w1, nu, alpha)
    loss = float((ent + (-(w1 * qs[0] + (1 - w1) * qs[1])).mean() + lag).detach())
    assert abs(loss - ch["loss"][0]) <= 1e-13 * max(1.0, abs(loss))
    assert float((ch["logp"][0] - logp.detach()).abs().max()) <= 1e-12 and float((ch["ap"][0] - ap.detach()).abs().max()) <= 1e-14
    worst = max(_rel(ch["grads"][k][0].reshape(gr.shape), gr) for k, gr in zip(keys, grads))
    wnu = _rel(torch.from_numpy(ch["gnu"][0]), dnu)
    print("evopf sac chain vs autograd around the oracle's completion: actor gradients %.3g, d/d nu %.3g" % (worst, wnu))
    assert worst <= 8e-15 and wnu <= 2 * 2.0 ** -52
