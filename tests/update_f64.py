"""The constrained policy update as ONE float64 chain: what ``agent.flat.grad`` must hold between the backward launches and the
optimiser step, with a bound beside every element.  Not collected; used by test_update_f64.py (CPU: the chain against autograd,
the harness on the oracle backend, planted errors), test_update_f64_gpu.py (every update path of the trainers on the device) and
test_embed256_f64_gpu.py (the 256-wide networks; the rollout's actions through policy_proposal and envs_f64.project_interval).

Nothing here is new arithmetic.  The chain composes the restatements the kernel tests already use, stage by stage:

    critic   Mlp64.first_layer / hidden / head (layer-local forward checks), Mlp64.forward_bound (the target networks at the
             launches' own next actions), mlp_f64.td (TD target + Huber: dq, the loss), Mlp64.backward
    actor    DDPG: Mlp64.head -> heads_f64.tanh_box (ap_det, the exploration clip) -> the env's Complete (envs_f64.check_explore)
             -> Mlp64 forward of the critic at the completed actions -> envs_f64.*_lagrangian (loss term, d/d action, d/d nu)
             -> Mlp64.backward of the critic (da; with a shared embedding also the state part of its first layer)
             -> envs_f64.*_complete_bwd -> heads_f64.tanh_box (backward) -> Mlp64.backward of the actor
             SAC: the same with heads_f64.gauss_head (forward and backward, alpha / B on log pi) and min(Q1, Q2)
             EVOPF-v0 (DDPG): evopf_f64.lagrangian, evopf_f64.complete_bwd_ref at the float64 Jacobian of the stored action,
             heads_f64.tanh_box on heads_f64.evopf_box
             EVOPF-v0 (SAC): heads_f64.gauss_head on heads_f64.evopf_box (14 components, log pi their sum), min(Q1, Q2) of two
             concatenating critics, (da1 + da2) + g in the kernel's association, the same completion backward, alpha / B

The losses are the reference's (rpo_ddpg.py:307-337, rpo_sac.py:321-353):
    critic   mean Huber(Q(s, a) - (r + gamma (1 - d) Q_targ(s', a')))           SAC: min of the twin targets - alpha log pi(a'|s'),
                                                                                the two Huber terms added
    actor    DDPG  mean(-Q(s, Complete(clip(pi(s) + eps_t noise)))) + mean_b sum_j nu_j relu(g_j)
             SAC   mean(alpha log pi - min(Q1, Q2)) + the same Lagrangian term;   d/d nu_j = mean_b relu(g_j)
             shared state embedding: the gradient through the critic's first layer is added into the shared slice
             automatic_entropy_tuning: log_alpha.grad = -(mean log pi + H_target)

Two rules (tests/test_large_batch_f64_gpu.py::test_large_batch_critic_update_matches_float64):

  * No decision is re-made in float64.  The ReLU masks of both networks come from the launches' saved x0 / h1 (Mlp64.backward
    reads them), relu(g_j) from the mask under which the launch's g_act agrees with float64 (envs_f64's enumeration of ambiguous
    predicates), the exploration clip from the stored action (strictly inside the box or on it), the split of min(Q1, Q2) from
    the launch's dq.  clamp / smooth-L1 of the TD error and min() of the targets are continuous with bounded slope: there the
    float64 value stands with its bound (mlp_f64.td).  Every such value is first held against float64 layer-locally (log pi(a'|s')
    of the pipelines, whose heads stay inside the launch, from the float64 actor at s' and the reproduced draw); at most
    AMBIG_CAP of the rows of a comparison may be ambiguous, and none is left out.
  * Every stage returns (value, bound): its own rounding bound -- gamma_L |A||B| for the MLP stages (mlp_f64.bound), MARGIN *
    C_REF_* * eps32 * magnitude sum for the head and env stages (heads_f64.C_REF_*, envs_f64.tol_c) -- plus its linear map, in
    absolute value, applied to the bound it was handed (the gradients are linear in dout: a second backward with dout = the bound).
"""
import numpy as np
import torch

import envs_f64 as ef
import heads_f64 as hf
import mlp_f64 as mf

F64 = torch.float64
U = mf.U
AMBIG_CAP = ef.AMBIG_CAP


def t64(x):
    return (x.detach() if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))).to("cpu", F64)


def n64(x):
    return t64(x).numpy()


# ================================================================================================================= the envs
class EnvRef(object):
    """Complete's backward and the Lagrangian term of one env from envs_f64, as (value, bound) stages on numpy float64."""

    def __init__(self, kind, table=None, partial=None):
        self.kind, self.table, self.partial = kind, table, partial
        self.p = int(partial) if kind == "cart" else 0           # column of the basic action

    @classmethod
    def of(cls, kernels):
        """From a trainer's kernel set (rpo_amd.ops or tests/oracle_backend.py)."""
        if kernels.name.startswith("CartSafe"):
            table = kernels.consts if hasattr(kernels, "consts") else kernels.c.as_array()
            return cls("cart", np.asarray(table, np.float32), int(kernels.partial))
        assert kernels.name.startswith("SpringPendulum"), kernels.name
        return cls("pend")

    def _lag(self, actions, nu, scale, mask, exact):
        if self.kind == "cart":
            l = ef.cart_lagrangian(ef.B64, self.table, self.partial, actions, nu, scale, mask, exact=exact)
            return l, l["margins"], l["dist"]
        l = ef.pend_lagrangian(ef.B64, actions, nu[0], scale, None if mask is None else mask[:, 0], exact=exact)
        return l, [l["margin"]], [l["dist"]]

    def lagrangian(self, actions, nu, scale, got=None, exact=False):
        """mean_b nu . relu(g(a_b)) from the launch's float32 actions (``exact``: float64 ones as they are): dict(g (value,
        bound) [n,2], gnu (value, bound) [J], loss (value, bound), ambiguous [n], violating [n], ratio [n]).  ``got``: the launch's
        g_act -- a row with ambiguous predicates g_j > 0 takes the mask under which ``got`` agrees best (the launch's decision)."""
        actions, nu = np.asarray(actions), np.asarray(nu, np.float32).reshape(-1)
        with np.errstate(all="ignore"):
            ref, margins, dist = self._lag(actions, nu, scale, None, exact)
            base = np.stack([m.v > 0 for m in margins], axis=1)
            ambm = np.zeros_like(base) if exact else np.stack([ef.ambiguous(m, self.kind + "_resid") for m in margins], axis=1)
            assert not (ambm.sum(axis=1) > ef.MAX_ENUM).any(), "rows with more ambiguous predicates than the enumeration takes"
            gv = np.stack([ref["g0"].v, ref["g1"].v], axis=1)
            gm = np.stack([ef.B64.mag(ref["g0"]), ef.B64.mag(ref["g1"])], axis=1)
            ratio = np.zeros(actions.shape[0])
            if got is not None:
                got = np.asarray(got, np.float32)
                best = np.full(actions.shape[0], np.inf)
                for mask in ef._mask_choices(base, ambm):
                    l = self._lag(actions, nu, scale, mask, exact)[0]
                    r = np.maximum(ef.ratio(got[:, 0], l["g0"]), ef.ratio(got[:, 1], l["g1"]))
                    take = r < best
                    best = np.where(take, r, best)
                    gv[take] = np.stack([l["g0"].v, l["g1"].v], axis=1)[take]
                    gm[take] = np.stack([ef.B64.mag(l["g0"]), ef.B64.mag(l["g1"])], axis=1)[take]
                ratio = best
            tol = ef.tol_c(self.kind + "_lag") * ef.EPS32
            dv = np.stack([d.v for d in dist], axis=1)
            dm = np.stack([ef.B64.mag(d) for d in dist], axis=1)
            n, s32 = actions.shape[0], float(np.float32(scale))
            # (the bound of rpo_*_lagrangian's d/d nu and loss words: tests/test_envs_f64_gpu.py)
            gnu = s32 * dv.sum(axis=0)
            gnu_b = s32 * ((n + 8) * ef.EPS32 * np.abs(dv).sum(axis=0) + tol * dm.sum(axis=0)) + ef.TINY
            nu64 = nu.astype(np.float64)
            return dict(g=(gv, tol * gm + ef.TINY), gnu=(gnu, gnu_b), loss=(float(gnu @ nu64), float(gnu_b @ np.abs(nu64)) * 2 + ef.TINY),
                        ambiguous=ambm.any(axis=1), violating=base.any(axis=1), ratio=ratio)

    def complete_bwd(self, state, ga, ga_bound):
        """d/d ap through Complete of a float64 d/d action [n,2] and its bound -> (value, bound) [n]: the stage's own rounding
        bound plus |J| applied to the incoming one (J: the map itself applied to the unit vectors)."""
        def run(g):
            if self.kind == "cart":
                return ef.cart_complete_bwd(ef.B64, self.table, self.partial, g, exact=True)
            return ef.pend_complete_bwd(ef.B64, state, g, exact=True)
        with np.errstate(all="ignore"):
            ga = np.asarray(ga, np.float64)
            out = run(ga)
            e0, e1 = np.zeros_like(ga), np.zeros_like(ga)
            e0[:, 0], e1[:, 1] = 1.0, 1.0
            j0, j1 = np.abs(run(e0).v), np.abs(run(e1).v)
            m = np.broadcast_to(out.m, out.v.shape)
            own = ef.tol_c(self.kind + "_cbwd") * ef.EPS32 * m + ef.TINY
            return np.array(out.v), own + j0 * ga_bound[:, 0] + j1 * ga_bound[:, 1]

    def check_actions(self, actions, ap_in, noise, eps_t, lo, hi, state):
        """The launch's completed actions against float64 from the proposal it was given (envs_f64.check_explore), in units of the
        stage's tolerance."""
        r = ef.check_explore(self.kind, actions, ap_in, noise, eps_t, lo, hi, table=self.table, partial=self.partial, obs=state)
        return float(np.max(r)) / ef.tol_c(self.kind + "_act")


# ================================================================================================================ MLP stages
def param_allowed(res, res_b, name, rows, extra=0):
    """(ref, allowed) of one parameter gradient: gamma_(L + batch chain) |A||B| plus |A||B| of the backward run on the incoming
    bound (the gradient is linear in dout)."""
    ref, absval, L = res[name]
    L = L + mf.batch_chain(rows) + extra
    return ref, mf.bound(absval, L) + res_b[name][1] * (1.0 + 2 * L * U)


def forward_checks(net, s, a, x0, h1, out, worst, tag):
    """x0 / h1 / out of one launch, layer by layer from the launch's own input to each layer (mlp_f64.check_forward; gamma_L |A||B|
    holds for ANY order of the K products' sum, so head partials summed over column groups need no extra term)."""
    r, ab, L = net.first_layer(s, a)
    mf.check(tag + " x0", x0, r, ab, L, worst)
    r, ab, L = net.hidden(x0)
    mf.check(tag + " h1", h1, r, ab, L, worst)
    if out is not None:
        r, ab, L = net.head(h1)
        mf.check(tag + " out", out, r, ab, L, worst)


def critic_chain(net, state, action, x0, h1, q, qn, qn_err, reward, done, gamma, qn2=None, logp=None, alpha=0.0):
    """One critic's half of the update from the launches' x0 / h1 / q: {field: (ref, allowed)}, (loss, bound), (dq, bound).
    qn / qn2: float64 target values with ``qn_err`` = a bound on what the launch read instead (mlp_f64.td)."""
    dq, dq_b, loss, loss_b, _ = mf.td(q, qn, reward, done, gamma, qn2, logp, alpha, qn_err=qn_err)
    res = net.backward(state, action, x0, h1, dq.view(-1, 1))
    res_b = net.backward(state, action, x0, h1, dq_b.view(-1, 1))
    rows = dq.numel()
    grads = {k: param_allowed(res, res_b, k, rows) for k in mf.FIELDS if k in res}
    return grads, (loss, loss_b), (dq, dq_b)


TARGET_BOUNDS = "path"


def _forward(net, obs, bounds, a=None):
    """(out, bound) of a float32 forward against float64: Mlp64.forward_bound ("chain": gamma of the whole chain on the |.|
    expression pushed through every layer) or Mlp64.forward_running (the running bound, layer by layer)."""
    if bounds == "chain":
        out, absval, L = net.forward_bound(obs, a)
        return out, mf.bound(absval, L)
    return net.forward_running(obs, a)


def _spread(net, obs, centre, points):
    """max over ``points`` of |Q64(obs, point) - centre|, per row."""
    out = torch.zeros_like(centre)
    for pt in points:
        out = torch.maximum(out, (net.forward(obs, pt)[0] - centre).abs())
    return out


def policy_proposal(tr, params, box, obs, eps=None, target=True, det_noise=None, eps_t=0.0, bounds=None):
    """The basic action the policy proposes at ``obs`` in float64 and a bound on the launch's float32 one: (ap, delta, heads).
    RPODDPG: the target actor (``target``) or the live one through the tanh box, heads_f64.C_REF_BOX_FWD on the box and |scale|
    times the forward bound of the head (tanh is 1-Lipschitz), plus eps_t x ``det_noise`` (the rollout's exploration: its product
    and its sum round once each).  RPOSAC: the live actor through the Gaussian head at the draw ``eps``, heads_f64.C_REF_AP on the
    head and |d ap / d heads| (autograd of heads_f64.gauss_head) on the forward bound of the two heads -- the sensitivity
    check_update's "log pi(a'|s')" branch uses.  The clip to the box is left to the caller (envs_f64.project_interval:
    continuous, its seam a predicate)."""
    scale, base, lo, hi = box
    n = obs.shape[0]
    bounds = TARGET_BOUNDS if bounds is None else bounds
    if tr.sac:
        out, rb = _forward(net64(tr, params, "actor"), obs, bounds)
        fw = hf.gauss_head(out[:, 0], out[:, 1], eps, scale, base, -1e30, 1e30, dap=torch.ones(n, dtype=F64), dlogp=0.0)
        mg = hf.gauss_mags(out[:, 0], out[:, 1], eps, scale, base)
        delta = hf.MARGIN * hf.C_REF_AP * hf.EPS32 * mg["ap"] + fw["g_mean"].abs() * rb[:, 0] + fw["g_ls"].abs() * rb[:, 1] + mf.TINY
        return fw["ap"], delta, out
    out, o_b = _forward(net64(tr, params, "actor_target" if target else "actor"), obs, bounds)
    o, o_b = out.view(-1), o_b.view(-1)
    ap = scale * torch.tanh(o) + base
    delta = hf.MARGIN * hf.C_REF_BOX_FWD * hf.EPS32 * hf.tanh_box_fwd_mags(o, scale, base) + abs(scale) * o_b + mf.TINY
    if det_noise is not None:
        nz = t64(det_noise).view(-1) * hf.f32(eps_t)
        delta = delta + hf.EPS32 * (ap.abs() + 2 * nz.abs())
        ap = ap + nz
    return ap, delta, out


def cart_target_chain(tr, snap, env, box, bounds=None):
    """qn of the launches that keep the next actions to themselves (CartSafe's row-tile critic pipelines and split stages),
    recomputed in float64 from the gathered batch, the parameters before the update and, for RPOSAC, the reproduced draw:

        pi_targ(s') (RPOSAC: pi(s') at eps_next) -> box / Gaussian head      policy_proposal: (ap, delta)
        -> Complete -> Proj                                                  envs_f64.project_interval at ap - delta, ap, ap + delta:
                                                                             (a', delta_a), ambiguous rows
        -> Q_targ(s', a')                                                    its forward bound + its response to the interval

    ``bounds`` (default TARGET_BOUNDS; tests/test_update_f64.py::test_planted_errors_are_found_in_the_target_values measures
    what each form lets pass):
      "chain"    Mlp64.forward_bound for both networks and the sensitivity |W1| |W0| |Wa| delta_a, every weight in absolute value:
                 valid through the relu, which is 1-Lipschitz (a first-order gradient at a' is not a bound).  At 256 -> 256 it allows
                 qn some units (delta = 0.05 on a proposal of size 1, 3.7 on a qn of 0.4 where the float32 error is 2e-7) and hides
                 every planted error: kept as the yardstick the tighter forms are shown against.
      "running"  Mlp64.forward_running for both (the running bound layer by layer: the same inequalities, no looser step) with
                 delta_a handed to it as the error of the action input -- still every weight in absolute value; hides three of four.
      "corners"  forward_running for the networks' own rounding, and for delta_a the spread of Q_targ64 over the four corners
                 a' +- delta_a about the centre, doubled (the map is piecewise linear in a' with relu kinks: the factor covers a
                 kink inside the box, as project_interval's covers curvature).  The corners leave the line Complete keeps a' on.
      "path"     the proposal is one scalar per row, so the propagation is one-dimensional: the spread of Q_targ64 over the two
                 end points a'(ap - delta), a'(ap + delta) about a'(ap), doubled, and the float32 loop's own (ulp-sized) share of
                 delta_a through forward_running in absolute value.
    Returns dict(qn [(value, bound)] per target critic, ambiguous [n], next_actions (a', delta_a), ap (ap, delta), iters [n])."""
    bounds = TARGET_BOUNDS if bounds is None else bounds
    next_state = snap["cols"][2]
    p0, rec = snap["params0"], snap["rec"]
    ap, delta, _ = policy_proposal(tr, p0, box, next_state, eps=rec.get("eps_next"), bounds=bounds)
    a, a_b, amb, iters, path = ef.project_interval(env.kind, ap.numpy(), delta.numpy(), int(tr.max_steps), tr.corr_lr, tr.corr_eps, box[2],
                                                   box[3], table=env.table, partial=env.partial, obs=n64(next_state))
    a, a_b = torch.from_numpy(a), torch.from_numpy(a_b)
    qn = []
    for _, tname in critic_names(tr):
        net = net64(tr, p0, tname)
        if bounds == "chain":
            out, own = _forward(net, next_state, bounds, a)
            ws, _ = net._heads()
            b = own + (((a_b @ net.p["Wa"].abs().t()) @ net.p["W0"].abs().t()) @ ws[0].abs().t()) * (1.0 + 4 * U)
        elif bounds == "running":
            out, b = net.forward_running(next_state, a, a_err=a_b)
        elif bounds == "corners":
            out, own = net.forward_running(next_state, a)
            b = own + 2.0 * _spread(net, next_state, out, [a + a_b * torch.tensor([s0, s1], dtype=F64) for s0 in (-1.0, 1.0) for s1 in (-1.0, 1.0)])
        else:
            # along the path: the two end points of the proposal's interval, and around each of the three points the corners of
            # the float32 loop's own (ulp-sized) box
            pown = torch.from_numpy(path["own"])
            out, own = net.forward_running(next_state, a, a_err=pown)
            b = own + 2.0 * _spread(net, next_state, out, [torch.from_numpy(e) for e in path["ends"]])
        qn.append((out.view(-1), b.view(-1)))
    return dict(qn=qn, ambiguous=torch.from_numpy(amb), next_actions=(a, a_b), ap=(ap, delta), iters=iters)


def trainer_box(tr):
    """(scale, base, lo, hi) of the constant action box, as the float32 arguments the launches receive."""
    return (hf.f32(tr._box_affine[0]), hf.f32(tr._box_affine[1]), hf.f32(tr._box_lo), hf.f32(tr._box_hi))


def rollout_noise(tr, n, t, sub=0, env_id_base=0):
    """The draw of one vector step at clock ``t``, from the Philox oracle at the launch's key: RPODDPG's exploration noise
    (STREAM_ACT, index t) or RPOSAC's sample (STREAM_POLICY, index t + salt 0, sub-stream ctrl[RPO_CTRL_UPDATES])."""
    from oracle import philox
    ids = np.arange(n) + int(env_id_base)
    if tr.sac:
        r = philox.draw(tr.seed, ids, int(t) & 0xFFFFFFFF, philox.STREAM_POLICY, int(sub))
    else:
        r = philox.draw(tr.seed, ids, int(t), philox.STREAM_ACT)
    return torch.from_numpy(np.asarray(philox.normal(r[:, 0], r[:, 1]), np.float32))


def rollout_actions(tr, params, obs, actions, t, sub=0, env_id_base=0, bounds=None):
    """The actions of one vector step against float64 from the observation the launch read: actor(obs) -> tanh box + eps_t x the
    Philox draw and the clip (RPODDPG) or the Gaussian head at the Philox draw (RPOSAC) -> Complete -> Proj, by the three-point
    scheme of cart_target_chain (policy_proposal, envs_f64.project_interval).  Returns dict(ratio: worst |action - float64| /
    bound over the rows that are not ambiguous, ambiguous [n], ref (a, bound), iters [n])."""
    env, box = EnvRef.of(tr.kernels), trainer_box(tr)
    obs = t64(obs)
    n = obs.shape[0]
    noise = rollout_noise(tr, n, t, sub, env_id_base)
    if tr.sac:
        ap, delta, _ = policy_proposal(tr, params, box, obs, eps=noise, bounds=bounds)
    else:
        eps_t = hf.eps_schedule(tr.eps_start, tr.eps, tr.decay_value, t)
        ap, delta, _ = policy_proposal(tr, params, box, obs, target=False, det_noise=noise, eps_t=eps_t, bounds=bounds)
    a, a_b, amb, iters, _ = ef.project_interval(env.kind, ap.numpy(), delta.numpy(), int(tr.max_steps), tr.corr_lr, tr.corr_eps, box[2], box[3],
                                                table=env.table, partial=env.partial, obs=obs.numpy())
    got = n64(actions).reshape(n, 2)
    assert np.isfinite(got).all(), "rollout actions: non-finite"
    r = np.abs(got - a) / a_b
    keep = ~amb
    return dict(ratio=float(r[keep].max()) if keep.any() else 0.0, ambiguous=amb, ref=(a, a_b), iters=iters, noise=noise)


def target_qn_ratio(chain, got):
    """Worst |qn - float64| / bound of the launch's target values ``got`` (one [n] tensor per target critic) over the rows whose
    projection is not ambiguous."""
    keep = ~chain["ambiguous"]
    return max(float(((t64(g).view(-1) - ref).abs() / b)[keep].max()) for g, (ref, b) in zip(got, chain["qn"]))


def _critic_da(critics, state, actions, dqs, shared, rows):
    """d(loss)/d action through the critic(s) at the policy's actions, and (shared embedding) the state part of their first
    layers: (da, bound) [n,2] and {field: (ref, allowed)} of the shared slice.  critics: [(net, x0, h1)]; dqs: [(dq, bound)]."""
    da, da_b, grads = 0.0, 0.0, {}
    for (net, x0, h1), (dq, dq_b) in zip(critics, dqs):
        res = net.backward(state, actions, x0, h1, dq.view(-1, 1), param_grads=shared, first_layer_state_only=True)
        res_b = net.backward(state, actions, x0, h1, dq_b.view(-1, 1), param_grads=shared, first_layer_state_only=True)
        ref, absval, L = res["da"]
        da = da + ref
        da_b = da_b + mf.bound(absval, L) + res_b["da"][1] * (1.0 + 2 * L * U)
        if shared:
            for k in ("Ws", "bs"):
                r, al = param_allowed(res, res_b, k, rows, extra=1)
                grads[k] = (grads[k][0] + r, grads[k][1] + al) if k in grads else (r, al)
    return da, da_b, grads


def _add_shared(grads, shared_grads):
    """The critic's contribution to the shared embedding added onto the actor's own (one more rounding of the sum)."""
    for k, (r, al) in shared_grads.items():
        r0, al0 = grads[k]
        grads[k] = (r0 + r, al0 + al + 2 * U * (r0.abs() + r.abs()))
    return grads


def ddpg_actor_chain(env, actor, critic, state, x0a, h1a, noise, eps_t, box, actions, x0c, h1c, nu, shared, g_act=None,
                     exact=False):
    """RPODDPG's policy step from the launches' saved activations, noise and completed actions -> dict(grads {field: (ref,
    allowed)} of the actor (shared fields summed), gnu (ref, bound), loss (ref, bound), lag (the env stage's dict), o, ap_det
    (ref, bound), clip rows).  box = (scale, base, lo, hi)."""
    scale, base, lo, hi = box
    B = state.shape[0]
    o, o_abs, Lo = actor.head(h1a)
    o, o_b = o.view(-1), mf.bound(o_abs, Lo).view(-1)
    fw = hf.tanh_box(o, noise, eps_t, scale, base, lo, hi)
    ap_b = hf.MARGIN * hf.C_REF_BOX_FWD * hf.EPS32 * hf.tanh_box_fwd_mags(o, scale, base) + abs(scale) * o_b + mf.TINY
    ap = t64(actions)[:, env.p]
    inside = (ap > lo) & (ap < hi)                               # the launch's clip decision, from the action it stored
    seam = hf.near_seam(fw["pre"], lo, hi)
    lag = env.lagrangian(n64(actions), nu, 1.0 / B, got=g_act, exact=exact)
    q, q_abs, Lq = critic.head(h1c)
    dq = torch.full((B,), -1.0 / B, dtype=F64)
    da, da_b, sh = _critic_da([(critic, x0c, h1c)], state, actions, [(dq, U * dq.abs())], shared, B)
    tot = da + torch.from_numpy(lag["g"][0])
    tot_b = da_b + torch.from_numpy(lag["g"][1]) + 2 * U * tot.abs()
    dap, dap_b = env.complete_bwd(n64(state), tot.numpy(), tot_b.numpy())
    dap, dap_b = torch.from_numpy(dap), torch.from_numpy(dap_b)
    y = torch.tanh(o)
    slope = abs(scale) * (1 - y * y)
    do = hf.tanh_box(o, None, 0.0, scale, base, lo, hi, dap=dap)["g"] * inside
    do_b = (hf.MARGIN * hf.C_REF_BOX_BWD * hf.EPS32 * hf.tanh_box_mags(o, scale, dap) + slope * dap_b
            + dap.abs() * 2 * y.abs() * slope * o_b) * inside + mf.TINY
    res = actor.backward(state, None, x0a, h1a, do.view(-1, 1))
    res_b = actor.backward(state, None, x0a, h1a, do_b.view(-1, 1))
    grads = {k: param_allowed(res, res_b, k, B, extra=1 if shared and k in ("Ws", "bs") else 0) for k in mf.FIELDS if k in res}
    if shared:
        grads = _add_shared(grads, sh)
    qb = mf.bound(q_abs, Lq).view(-1)
    loss = lag["loss"][0] - float(q.mean())
    loss_b = lag["loss"][1] + float(qb.mean()) + float(mf.bound(q.abs().mean(), B + 16))
    return dict(grads=grads, gnu=lag["gnu"], loss=(loss, loss_b), lag=lag, o=(o, o_b), ap_det=(fw["ap_det"], ap_b), do=(do, do_b),
                seam=seam, clipped=~inside, q=(q.view(-1), qb))


def sac_actor_chain(env, actor, critics, state, x0a, h1a, raw, noise, box, actions, saved, w1, nu, alpha, shared, g_act=None,
                    exact=False):
    """RPOSAC's policy step.  critics: [critic1, critic2] (Mlp64); saved: [(x0, h1)] of both at the policy's actions; raw: the
    launch's two head outputs [n,2]; w1: the share of d(-min(Q1, Q2)) that critic 1 takes per row (1, 0, or 0.5 on a tie), read
    from the launch's dq.  Returns ddpg_actor_chain's dict with logp (ref, bound) and the min() ambiguity."""
    scale, base, lo, hi = box
    B = state.shape[0]
    raw = t64(raw)
    a32 = hf.f32(alpha)
    dlogp = hf.f32(a32 / B) if not exact else alpha / B
    fw = hf.gauss_head(raw[:, 0], raw[:, 1], noise, scale, base, lo, hi)
    mags = hf.gauss_mags(raw[:, 0], raw[:, 1], noise, scale, base)
    logp_b = hf.MARGIN * hf.C_REF_LOGP * hf.EPS32 * mags["logp"] + mf.TINY
    lag = env.lagrangian(n64(actions), nu, 1.0 / B, got=g_act, exact=exact)
    w1 = t64(w1).view(-1)
    qs = [c.head(h1) for c, (x0, h1) in zip(critics, saved)]
    qv = [q[0].view(-1) for q in qs]
    qb = [mf.bound(q[1], q[2]).view(-1) for q in qs]
    tie = (qv[0] - qv[1]).abs() <= qb[0] + qb[1]                 # min(Q1, Q2): either critic may have been the smaller one
    dqs = [(w * (-1.0 / B), U * (w * (-1.0 / B)).abs()) for w in (w1, 1.0 - w1)]
    da, da_b, sh = _critic_da([(c, x0, h1) for c, (x0, h1) in zip(critics, saved)], state, actions, dqs, shared, B)
    tot = da + torch.from_numpy(lag["g"][0])
    tot_b = da_b + torch.from_numpy(lag["g"][1]) + 3 * U * tot.abs()
    dap, dap_b = env.complete_bwd(n64(state), tot.numpy(), tot_b.numpy())
    dap, dap_b = torch.from_numpy(dap), torch.from_numpy(dap_b)
    bw = hf.gauss_head(raw[:, 0], raw[:, 1], noise, scale, base, lo, hi, dap=dap, dlogp=dlogp)
    bmag = hf.gauss_mags(raw[:, 0], raw[:, 1], noise, scale, base, dap=dap, dlogp=dlogp)
    lin = hf.gauss_head(raw[:, 0], raw[:, 1], noise, scale, base, lo, hi, dap=dap_b, dlogp=0.0)     # |map| on the incoming bound
    draw = torch.stack([bw["g_mean"], bw["g_ls"]], dim=1)
    draw_b = torch.stack([hf.MARGIN * hf.C_REF_G_MEAN * hf.EPS32 * bmag["g_mean"] + lin["g_mean"].abs(),
                          hf.MARGIN * hf.C_REF_G_LS * hf.EPS32 * bmag["g_ls"] + lin["g_ls"].abs()], dim=1) + mf.TINY
    res = actor.backward(state, None, x0a, h1a, draw)
    res_b = actor.backward(state, None, x0a, h1a, draw_b)
    grads = {k: param_allowed(res, res_b, k, B, extra=1 if shared and k in ("Ws", "bs") else 0) for k in mf.FIELDS if k in res}
    if shared:
        grads = _add_shared(grads, sh)
    qmin = torch.minimum(qv[0], qv[1])
    term = a32 * fw["logp"] - qmin
    term_b = abs(a32) * logp_b + torch.maximum(qb[0], qb[1]) + 2 * U * (abs(a32) * fw["logp"].abs() + qmin.abs())
    loss = lag["loss"][0] + float(term.mean())
    loss_b = lag["loss"][1] + float(term_b.mean()) + float(mf.bound(term.abs().mean(), B + 16))
    a_seam = hf.near_seam(scale * torch.tanh(raw[:, 0] + noise_t(noise) * torch.clamp(raw[:, 1] - 3, hf.LS_MIN, hf.LS_MAX).exp())
                          + base, lo, hi)
    ls = raw[:, 1] - 3.0
    ls_seam = ((ls - hf.LS_MIN).abs() <= 8 * hf.EPS32 * 23) | ((ls - hf.LS_MAX).abs() <= 8 * hf.EPS32 * 3)
    return dict(grads=grads, gnu=lag["gnu"], loss=(loss, loss_b), lag=lag, logp=(fw["logp"], logp_b), draw=(draw, draw_b),
                seam=a_seam | ls_seam, tie=tie, q=list(zip(qv, qb)),
                ap=(fw["ap"], hf.MARGIN * hf.C_REF_AP * hf.EPS32 * mags["ap"] + mf.TINY))


def _evopf_lagrangian(consts, s32, a32, nu, g_act=None):
    """EVOPF-v0's Lagrangian term mean_b nu . relu(g(a_b)) at the launch's float32 states and completed actions
    (evopf_f64.lagrangian): EnvRef.lagrangian's dict -- g (value, bound) [n,43], gnu (value, bound) [58], loss (value, bound),
    ambiguous [n], violating [n], ratio [n] (the launch's ``g_act`` in units of the "lag_grad" tolerance).  A row with ambiguous
    predicates takes the mask under which ``g_act`` agrees best (either value of an ambiguous mask: the launch's decision)."""
    import evopf_f64 as vf
    B = s32.shape[0]
    with np.errstate(all="ignore"):
        c = vf.Tab(vf.B64E, consts)
        S, Ac = vf.cols(vf.B64E, s32), vf.cols(vf.B64E, a32)
        zero = np.zeros(nu.size, np.float32)
        r = vf.lagrangian(vf.B64E, c, S, Ac, nu, 1.0 / B, 0.0, zero, True)
        mv, mm = vf.val(vf.B64E, r["margins"]), vf.mag(vf.B64E, r["margins"])
        amb = (mm > 0) & (np.abs(mv) <= vf.tol_c("resid_ineq") * ef.EPS32 * mm)
        gv, gm = vf.val(vf.B64E, r["grad"]), vf.mag(vf.B64E, r["grad"])
        ratio = np.zeros(B)
        if g_act is not None:
            got = np.asarray(t64(g_act).numpy(), np.float32)
            ratio = vf.ratios("lag_grad", got, gv, gm).max(axis=1)
            if amb.any():                                        # (either value of an ambiguous mask: the launch's decision)
                up = np.array([u for _, u in vf.INEQ_ROWS])
                for flip in (amb & up[None], amb & ~up[None], amb):
                    alt = vf.lagrangian(vf.B64E, c, S, Ac, nu, 1.0 / B, 0.0, zero, True, mask=(mv > 0) ^ flip)
                    av, am = vf.val(vf.B64E, alt["grad"]), vf.mag(vf.B64E, alt["grad"])
                    ra = vf.ratios("lag_grad", got, av, am).max(axis=1)
                    take = ra < ratio
                    gv[take], gm[take], ratio[take] = av[take], am[take], ra[take]
        g_b = vf.tol_c("lag_grad") * ef.EPS32 * gm + ef.TINY
        gnu = np.array([float(x.v) for x in r["grad_nu"]])
        gnu_b = vf.tol_c("lag_sum") * ef.EPS32 * np.array([float(x.m) for x in r["grad_nu"]]) + ef.TINY
        return dict(g=(gv, g_b), gnu=(gnu, gnu_b), ambiguous=amb.any(axis=1), violating=(mv > 0).any(axis=1), ratio=ratio,
                    loss=(float(r["loss"].v), vf.tol_c("lag_sum") * ef.EPS32 * float(r["loss"].m) + ef.TINY))


def _evopf_complete_bwd(consts, a32, dl, dlm):
    """evopf_f64.complete_bwd_ref row by row at the float64 Jacobian of the stored actions (evopf_f64.dense_jac): dl [n,43] the
    summed d/d action, dlm its running bound in units of tol_c("cbwd") * eps32 -> (dap, bound) [n,14] as torch float64."""
    import evopf_f64 as vf
    n = a32.shape[0]
    jv, jm = vf.dense_jac(consts, a32)
    dap, dap_m = np.zeros((n, vf.NP)), np.zeros((n, vf.NP))
    with np.errstate(all="ignore"):
        for i in range(n):
            dap[i], dap_m[i] = vf.complete_bwd_ref(jv[i], jm[i], dl[i], dlm[i])
    return torch.from_numpy(dap), torch.from_numpy(vf.tol_c("cbwd") * ef.EPS32 * dap_m + ef.TINY)


def evopf_actor_chain(consts, actor, critic, state, x0a, h1a, raw, noise, eps_t, actions, x0c, h1c, nu, g_act=None):
    """RPODDPG's policy step on EVOPF-v0 (the generic chain; the kernels add the Lagrangian's d/d action inside
    rpo_evopf_complete_bwd) from the launches' raw actor outputs [n,14], noise and completed actions [n,43]: evopf_f64.lagrangian
    -> Mlp64.backward of the (concatenating) critic -> evopf_f64.complete_bwd_ref at the float64 Jacobian of the stored action,
    row by row -> heads_f64.tanh_box with heads_f64.evopf_box -> Mlp64.backward of the actor.  Returns ddpg_actor_chain's dict."""
    import evopf_f64 as vf
    B = state.shape[0]
    s32, a32 = np.asarray(t64(state).numpy(), np.float32), np.asarray(t64(actions).numpy(), np.float32)
    nu = np.asarray(nu, np.float32).reshape(-1)
    lag = _evopf_lagrangian(consts, s32, a32, nu, g_act)
    gv, g_b = lag["g"]
    q, q_abs, Lq = critic.head(h1c)
    dq = torch.full((B,), -1.0 / B, dtype=F64)
    da, da_b, _ = _critic_da([(critic, x0c, h1c)], state, actions, [(dq, U * dq.abs())], False, B)
    dl = da.numpy() + gv
    # (the running bound complete_bwd_ref takes is in units of tol_c * eps32: the incoming bounds in those units + the add's rounding)
    dlm = (da_b.numpy() + g_b) / (vf.tol_c("cbwd") * ef.EPS32) + np.abs(dl)
    dap, dap_b = _evopf_complete_bwd(consts, a32, dl, dlm)
    lo, hi, scale, base, scale_mag, base_mag = hf.evopf_box(s32)
    o = t64(raw).view(B, vf.NP)
    nz = t64(noise).view(B, vf.NP)
    bw = hf.tanh_box(o, nz, eps_t, scale, base, lo, hi, dap=dap)
    inside = (bw["pre"] >= lo) & (bw["pre"] <= hi)
    width = hf.EPS32 * (scale_mag + base_mag) * 8                # (the kernel computes the box itself: tests/test_heads_gpu.py)
    seam = ((bw["pre"] - lo).abs() <= width) | ((bw["pre"] - hi).abs() <= width)
    y = torch.tanh(o)
    do = bw["g"]
    do_b = (hf.MARGIN * hf.C_REF_BOX_BWD * hf.EPS32 * hf.tanh_box_mags(o, scale, dap, scale_mag=scale_mag)
            + scale.abs() * (1 - y * y) * dap_b) * inside + mf.TINY
    res = actor.backward(state, None, x0a, h1a, do)
    res_b = actor.backward(state, None, x0a, h1a, do_b)
    grads = {k: param_allowed(res, res_b, k, B) for k in mf.FIELDS if k in res}
    qb = mf.bound(q_abs, Lq).view(-1)
    loss = lag["loss"][0] - float(q.mean())
    loss_b = lag["loss"][1] + float(qb.mean()) + float(mf.bound(q.abs().mean(), B + 16))
    return dict(grads=grads, gnu=lag["gnu"], loss=(loss, loss_b), lag=lag, do=(do, do_b), dap=(dap, dap_b), seam=seam.any(dim=1),
                clipped=~inside, q=(q.view(-1), qb))


def evopf_gauss(state, raw, noise, dap=None, dlogp=0.0):
    """The 14-wide squashed-Gaussian head in EVOPF-v0's state-dependent box (heads_f64.gauss_head / gauss_mags at
    heads_f64.evopf_box(state)) from the launch's raw heads [n,28] -- rpo_evopf_gauss_head's layout: the 14 means, then the 14
    log-stds -- and the draw [n,14]: dict(fw, mags, box, ap (value, bound) [n,14], logp (value, bound) [n], args).  log pi is the
    sum over the 14 components; its bound is every component's own plus the rounding of the float32 sum (a 16-lane butterfly:
    four more additions), the form of tests/test_heads_gpu.py::test_evopf_gauss_head."""
    n = state.shape[0]
    s32 = np.asarray(t64(state).numpy(), np.float32)
    lo, hi, scale, base, scale_mag, base_mag = hf.evopf_box(s32)
    raw, e = t64(raw).view(n, -1), t64(noise).view(n, -1)
    P = e.shape[1]
    assert raw.shape[1] == 2 * P
    args = (raw[:, :P], raw[:, P:], e, scale, base, lo, hi)
    fw = hf.gauss_head(*args, dap=dap, dlogp=dlogp)
    mags = hf.gauss_mags(*args[:5], dap=dap, dlogp=dlogp, scale_mag=scale_mag, base_mag=base_mag)
    logp = fw["logp"].sum(1)
    logp_b = hf.MARGIN * hf.C_REF_LOGP * hf.EPS32 * (mags["logp"].sum(1) + 4 * fw["logp"].abs().sum(1)) + mf.TINY
    ap_b = hf.MARGIN * hf.C_REF_AP * hf.EPS32 * mags["ap"] + mf.TINY
    return dict(fw=fw, mags=mags, box=(lo, hi, scale, base, scale_mag, base_mag), ap=(fw["ap"], ap_b), logp=(logp, logp_b), args=args)


def evopf_sac_actor_chain(consts, actor, critics, state, x0a, h1a, raw, noise, actions, saved, w1, nu, alpha, g_act=None):
    """RPOSAC's policy step on EVOPF-v0 (the generic chain; rpo_evopf_complete_bwd adds the second critic's and the Lagrangian's
    d/d action itself) from the launches' raw heads [n,28], the policy step's own draw [n,14] and the completed actions [n,43]:

        heads_f64.gauss_head in heads_f64.evopf_box(state)              ap [n,14], log pi [n] (summed over the 14 components)
        evopf_f64.lagrangian at the stored actions                      the loss term, g = d/d action, d/d nu (_evopf_lagrangian)
        Mlp64.head of both (concatenating) critics at those actions     min(Q1, Q2); its split w1 is the launch's (from its dq1)
        Mlp64.backward of both with dq_k = w_k (-1 / B)                 da1, da2 (_critic_da)
        (da1 + da2) + g                                                 the association include/rpo_hip.h states for
                                                                        rpo_evopf_complete_bwd, one rounding per add
        evopf_f64.complete_bwd_ref at the float64 Jacobian, row by row  d/d ap [n,14]
        heads_f64.gauss_head backward with alpha / B on log pi          d/d (14 means, 14 log-stds) -> Mlp64.backward of the actor

    critics: [critic1, critic2] (Mlp64); saved: [(x0, h1)] of both at the policy's actions.  Returns sac_actor_chain's dict."""
    import evopf_f64 as vf
    B = state.shape[0]
    s32, a32 = np.asarray(t64(state).numpy(), np.float32), np.asarray(t64(actions).numpy(), np.float32)
    nu = np.asarray(nu, np.float32).reshape(-1)
    a_32 = hf.f32(alpha)
    dlogp = hf.f32(a_32 / B)
    # ---- the Gaussian head
    head = evopf_gauss(state, raw, noise)
    fw, (lo, hi, scale, base, scale_mag, base_mag) = head["fw"], head["box"]
    logp, logp_b = head["logp"]
    # ---- the Lagrangian and min(Q1, Q2)
    lag = _evopf_lagrangian(consts, s32, a32, nu, g_act)
    gv, g_b = lag["g"]
    w1 = t64(w1).view(-1)
    qs = [c.head(h1) for c, (x0, h1) in zip(critics, saved)]
    qv = [q[0].view(-1) for q in qs]
    qb = [mf.bound(q[1], q[2]).view(-1) for q in qs]
    tie = (qv[0] - qv[1]).abs() <= qb[0] + qb[1]                 # min(Q1, Q2): either critic may have been the smaller one
    # ---- the three-way add
    dqs = [(w * (-1.0 / B), U * (w * (-1.0 / B)).abs()) for w in (w1, 1.0 - w1)]
    das = [_critic_da([(c, x0, h1)], state, actions, [dq], False, B)[:2] for c, (x0, h1), dq in zip(critics, saved, dqs)]
    d12 = (das[0][0] + das[1][0]).numpy()
    dl = d12 + gv
    # (complete_bwd_ref's running bound is in units of tol_c * eps32: the three incoming bounds in those units + the rounding of
    #  each of the two adds)
    dlm = (das[0][1].numpy() + das[1][1].numpy() + g_b) / (vf.tol_c("cbwd") * ef.EPS32) + np.abs(d12) + np.abs(dl)
    # ---- backward through the completion and the head
    dap, dap_b = _evopf_complete_bwd(consts, a32, dl, dlm)
    back = evopf_gauss(state, raw, noise, dap=dap, dlogp=dlogp)
    bw, bmag = back["fw"], back["mags"]
    lin = hf.gauss_head(*head["args"], dap=dap_b, dlogp=0.0)     # |map| on the incoming bound
    draw = torch.cat([bw["g_mean"], bw["g_ls"]], dim=1)
    draw_b = torch.cat([hf.MARGIN * hf.C_REF_G_MEAN * hf.EPS32 * bmag["g_mean"] + lin["g_mean"].abs(),
                        hf.MARGIN * hf.C_REF_G_LS * hf.EPS32 * bmag["g_ls"] + lin["g_ls"].abs()], dim=1) + mf.TINY
    res = actor.backward(state, None, x0a, h1a, draw)
    res_b = actor.backward(state, None, x0a, h1a, draw_b)
    grads = {k: param_allowed(res, res_b, k, B) for k in mf.FIELDS if k in res}
    # ---- loss and seams
    qmin = torch.minimum(qv[0], qv[1])
    term = a_32 * logp - qmin
    term_b = abs(a_32) * logp_b + torch.maximum(qb[0], qb[1]) + 2 * U * (abs(a_32) * logp.abs() + qmin.abs())
    loss = lag["loss"][0] + float(term.mean())
    loss_b = lag["loss"][1] + float(term_b.mean()) + float(mf.bound(term.abs().mean(), B + 16))
    mean, rls, e = head["args"][:3]
    ls = rls - 3.0
    pre = scale * torch.tanh(mean + e * torch.clamp(ls, hf.LS_MIN, hf.LS_MAX).exp()) + base
    width = hf.EPS32 * (scale_mag + base_mag) * 8                # (the kernel computes the box itself: tests/test_heads_gpu.py)
    a_seam = hf.near_seam(pre, lo, hi) | ((pre - lo).abs() <= width) | ((pre - hi).abs() <= width)
    ls_seam = ((ls - hf.LS_MIN).abs() <= 8 * hf.EPS32 * 23) | ((ls - hf.LS_MAX).abs() <= 8 * hf.EPS32 * 3)
    return dict(grads=grads, gnu=lag["gnu"], loss=(loss, loss_b), lag=lag, logp=(logp, logp_b), draw=(draw, draw_b),
                dap=(dap, dap_b), seam=(a_seam | ls_seam).any(dim=1), tie=tie, q=list(zip(qv, qb)), ap=head["ap"])


def noise_t(noise):
    return t64(noise).view(-1)


def alpha_grad(logp, logp_b, target_entropy):
    """log_alpha.grad = -(mean log pi + H_target) (rpo_sac.py:210) -> (ref, bound)."""
    n = logp.numel()
    ref = -(float(logp.mean()) + float(target_entropy))
    return ref, float(logp_b.mean()) + float(mf.bound(logp.abs().mean(), n + 4)) + 2 * U * (abs(ref) + abs(float(target_entropy)))


# ================================================================================================ the harness on a trainer
def _sync(tr):
    if tr.device.type == "cuda":
        torch.cuda.synchronize()


def _cpu(t):
    return t.detach().to("cpu").clone()


def scratch(tr, *names, **kw):
    """The first of the named ``fused.buf(...)`` buffers that exists with batch_size rows (``rows=``: that many elements in one
    of its dimensions -- the flat [B * P] buffers of a P-wide head), as a CPU copy."""
    B = kw.get("rows", tr.batch_size)
    for name in names:
        hit = [v for k, v in tr.fused._scratch.items() if k[0] == name and B in k[1:]]
        if hit:
            assert len(hit) == 1, (name, [tuple(v.shape) for v in hit])
            return _cpu(hit[0])
    raise KeyError("none of the buffers %s exists" % (names,))


def split_head(part, bias):
    """Head output of every row from the 8 column-group partials the split stages leave ([8, B, 2], output 0), in the consumers'
    own float32 order (nsplit_dev.h ns_head: bias first, then the groups in order) -- the value the next stage computed."""
    v = bias.reshape(()).to(torch.float32).expand(part.shape[1]).clone()
    for g in range(part.shape[0]):
        v = v + part[g, :, 0]
    return v.view(-1, 1)


def read_params(tr):
    """{network: {field: CPU copy}} of every network descriptor of the trainer."""
    return {name: {k: _cpu(v) for k, v in d.tensors.items() if v is not None} for name, d in tr.fused.descs.items()}


def net64(tr, params, name):
    d = tr.fused.descs[name]
    return mf.Mlp64(params[name], d.S, d.A, d.E, d.H, n_out=d.n_out, cat=bool(d.cat), head_dim=getattr(d, "head_dim", 1))


def critic_names(tr):
    return [("critic1", "critic_target1"), ("critic2", "critic_target2")] if tr.sac else [("critic", "critic_target")]


def run_update(tr, critic_only=False):
    """One eager update of the trainer with a policy step, cut open between the backward launches and the optimiser steps
    (trainer.train's body): flat.grad.zero_(), _critic_update | read | _critic_step(True) | _actor_update | read.  Returns the
    snapshot (CPU copies) that ``check_update`` judges; the optimiser step of the policy is left to the caller
    (``tr._actor_step(snap["actor_out"])``).  ``critic_only``: stop behind the first read."""
    ag, fl = tr.agent, tr.agent.flat
    snap = dict(rec={})
    rec = snap["rec"]
    project = tr._project_batch

    def _project(state, ap):                                     # (the critic update projects once: the next actions)
        out = project(state, ap)
        rec["next_actions"] = _cpu(out)
        return out
    tr._project_batch = _project
    tr._uclock_ok = False
    tr._sync_uclock(rollout_pending=False)
    bump, tr._bump = tr._bump, False
    try:
        cols = tr._sample()
        snap["params0"] = read_params(tr)
        snap["t"] = int(tr._uctrl[0])
        fl.grad.zero_()
        tr._iter_actor_step = True                               # (as _critic_half does: the split stages' hand-overs)
        tr._critic_update(cols)
        _sync(tr)
        c = tr.buffer.split(tr._batch)                           # (the pipelines gather the batch themselves, into `_batch`)
        snap["cols"] = [_cpu(c[k]) for k in ("state", "action", "next_state", "reward", "done")]
        snap["grad_c"] = _cpu(fl.grad)
        snap["loss_c"] = float(tr.last_losses["critic"])
        snap["parts_c"] = _cpu(tr.last_losses["critic"].parts)
        snap["gradmax_c"] = float(ag.critic_optim.gradmax.max()) if tr._gradmax_ready else None
        names = critic_names(tr)
        sfx = ["1", "2"] if tr.sac else [""]
        split_c = bool(tr._pipelines and tr._split_state() is not None)
        split_a = bool(tr._actor_pipeline and tr._split_state() is not None)
        snap["path"] = (("split" if split_c else "row-tile" if tr._pipelines else "generic"),
                        ("split" if split_a else "row-tile" if tr._actor_pipeline else "generic"))
        snap["critic"] = []
        for k, ((c, t), s) in enumerate(zip(names, sfx)):
            one = dict(x0=scratch(tr, c + ".x0"), h1=scratch(tr, c + ".h1"), dq=scratch(tr, "dq" + s))
            if split_c:                                          # (no q / qn buffers: the consumers sum the head partials)
                one["q"] = split_head(scratch(tr, "split.part_q%d" % (k + 1)), snap["params0"][c]["b1"])
                one["qn"] = split_head(scratch(tr, "split.part_qn%d" % (k + 1)), snap["params0"][t]["b1"])
            else:
                one["q"], one["qn"] = scratch(tr, "q" + s), scratch(tr, "qn" + s)
            snap["critic"].append(one)
        if split_c and int(tr._split_state().st.env) == 1:
            # (SpringPendulum: the batch projection hands the next actions to fwd_b through this buffer; CartSafe's fwd_b
            #  completes and projects per row in its own prologue and exports nothing)
            rec["next_actions"] = scratch(tr, "split.next_actions")
        if tr.sac:
            rec["logp_next"] = scratch(tr, "crit.logp")
            # the critic update's draw, reproduced from the trainer's own Philox stream at the same clock (the pipelines draw
            # inside their launches); the generic launches keep theirs, and the heads log pi was taken from
            from rpo_amd.algo.trainer import _SALT_CRITIC
            rec["eps_next"] = _cpu(tr._draw_batch(_SALT_CRITIC, buf=torch.zeros_like(tr._noise_b))).view(-1)
            _sync(tr)
            if not tr._pipelines:
                rec["raw_next"] = scratch(tr, "crit.raw")
                rec["ap_next"] = scratch(tr, "crit.ap", rows=tr.batch_size * tr.kernels.partial_dim).view(tr.batch_size, -1)
                assert torch.equal(rec["eps_next"], _cpu(tr._noise_b).view(-1)), "the reproduced draw is not the update's"
        tr._iter_actor_step = None
        if critic_only:
            return snap
        tr._critic_step(True)
        snap["params1"] = read_params(tr)
        snap["nu"] = _cpu(ag.nju.weight).view(-1)
        snap["nu_off"] = (fl.offset[id(ag.nju.weight)], fl.offset[id(ag.nju.weight)] + ag.nju.weight.numel())
        out = tr._actor_update(cols)
        _sync(tr)
        snap["actor_out"] = out
        snap["grad_a"] = _cpu(fl.grad)
        snap["loss_a"] = float(tr.last_losses["actor"])
        snap["gradmax_a"] = float(ag.actor_optim.gradmax.max()) if tr._actor_gradmax_ready else None
        a = dict(x0=scratch(tr, "actor.x0", "pi.x0"), h1=scratch(tr, "actor.h1", "pi.h1"), actions=scratch(tr, "act_pi"),
                 g_act=scratch(tr, "g_act"))
        a["critic"] = [dict(x0=scratch(tr, c + ".x0"), h1=scratch(tr, c + ".h1")) for c, _ in names]
        if tr.sac:
            a["raw"] = scratch(tr, "pi.raw")                      # [B, 2 P]: the P means, then the P log-stds (P = kernels.partial_dim)
            a["logp"] = scratch(tr, "pi.logp")
            if not tr._actor_pipeline:
                a["ap"] = scratch(tr, "pi.ap", rows=tr.batch_size * tr.kernels.partial_dim).view(tr.batch_size, -1)
            a["noise"] = _actor_noise(tr, ("act.noise" if split_a else "pi.noise",), tr._noise_pi)
            if split_a:                                          # (the split of min(Q1, Q2) from the head partials, as pol_c reads them)
                q1, q2 = (split_head(scratch(tr, "split.part_q%d" % k), snap["params1"]["critic%d" % k]["b1"]) for k in (1, 2))
                w1 = (q1 < q2).float() + 0.5 * (q1 == q2).float()
            else:
                w1 = scratch(tr, "dq1_pi" if tr._actor_pipeline else "dq1") / torch.tensor(-1.0 / tr.batch_size, dtype=torch.float32)
            a["w1"] = w1.view(-1)
        else:                                                    # (EVOPF-v0: "pi.out" holds the raw outputs, the env kernels apply the box)
            a["ap_det"] = scratch(tr, "act.ap_det" if tr._actor_pipeline else "pi.out")
            a["noise"] = _actor_noise(tr, ("act.noise",), tr._noise_b)
        snap["actor"] = a
        snap["log_alpha_grad"] = float(ag.log_alpha.grad) if getattr(ag, "log_alpha", None) is not None else None
    finally:
        tr._bump = bump
        tr._uclock_ok = False
        tr._iter_actor_step = None
        del tr._project_batch
    return snap


def _actor_noise(tr, names, fallback):
    """The policy step's draw: the pipelines' own noise buffer, or the generic launches' draw buffer."""
    if tr._actor_pipeline:
        return scratch(tr, *names).view(-1)
    return _cpu(fallback).view(-1)


def _slices(tr, name, got_flat):
    """{field: the launch's gradient of that parameter tensor}, read through FlatParams.offset."""
    fl, d = tr.agent.flat, tr.fused.descs[name]
    out = {}
    for k, p in d.tensors.items():
        if p is not None and id(p) in fl.offset:
            off = fl.offset[id(p)]
            out[k] = (off, got_flat[off:off + p.numel()].view(p.shape))
    return out


def _judge(tag, got, ref, allowed, worst, key):
    got = got.to(F64).reshape(ref.shape)
    assert bool(torch.isfinite(got).all()), "%s: non-finite" % tag
    r = float(((got - ref).abs() / allowed).max())
    worst[key] = max(worst.get(key, 0.0), r)
    return r


def _cap(tag, rows, worst, key):
    """At most AMBIG_CAP of the rows of a comparison may be ambiguous."""
    share = float(torch.as_tensor(rows).double().mean())
    worst["ambiguous " + key] = max(worst.get("ambiguous " + key, 0.0), share)
    assert share <= AMBIG_CAP, "%s: %.3g of the rows are ambiguous (cap %.3g)" % (tag, share, AMBIG_CAP)


def check_update(tr, snap, strict=True, target_chain=False):
    """Judge a snapshot of ``run_update``: every element of the critic, shared and actor slices of flat.grad and of the
    multipliers' gradient within its bound, padding and the other optimiser's private slice exactly 0, the losses within theirs,
    gradmax exact, the launches' intermediates layer-locally within float64.  Returns {what: worst |err| / bound}; with
    ``strict`` a ratio above 1 fails where it is found, otherwise it is only recorded (the planted-error tests).
    ``target_chain`` (CartSafe): judge qn against the recomputed target chain (cart_target_chain) and run the TD chain from it even
    where the launches exported their next actions -- the form every launch that keeps them to itself is judged in."""
    ag, fl, B = tr.agent, tr.agent.flat, tr.batch_size
    worst, fails = {}, []
    evopf = tr.kernels.name.startswith("EVOPF")
    env = None if evopf else EnvRef.of(tr.kernels)
    state, action, next_state, reward, done = snap["cols"]
    rec = snap["rec"]
    names = critic_names(tr)
    p0, p1 = snap["params0"], snap["params1"]
    shared = fl.sizes[1] > 0
    box = None if evopf else (hf.f32(tr._box_affine[0]), hf.f32(tr._box_affine[1]), hf.f32(tr._box_lo), hf.f32(tr._box_hi))
    alpha = float(getattr(ag, "alpha", 0.0)) if tr.sac else 0.0

    def judge(tag, got, ref, allowed, key):
        r = _judge(tag, got, ref, allowed, worst, key)
        if r > 1.0:
            fails.append("%s: |got - ref| is %.4g x the bound" % (tag, r))
            assert not strict, fails[-1]

    # ---------------------------------------------------------------------------------------------------------- critic half
    nxt = rec.get("next_actions")
    # (CartSafe's pipelines and split stages alone keep the next actions inside their launch)
    assert nxt is not None or (env is not None and env.kind == "cart" and snap["path"][0] != "generic"), "next actions not captured"
    qn64, qn_err = [], []
    chain = None
    if nxt is None or target_chain:
        # CartSafe's pipelines and split stages do not export the next actions: the target chain is recomputed in float64 from the
        # batch, and qn judged against it (cart_target_chain).  A row whose projection may have branched otherwise in the launch
        # keeps the launch's own qn (its decision), at most AMBIG_CAP of the batch.
        chain = cart_target_chain(tr, snap, env, box)
        amb = chain["ambiguous"]
        _cap("the target chain's projection", amb, worst, "proj(s')")
        for (cname, tname), c, (ref, b) in zip(names, snap["critic"], chain["qn"]):
            got = c["qn"].view(-1).to(F64)
            judge(tname + " qn", got[~amb], ref[~amb], b[~amb], "qn target chain")
            qn64.append(torch.where(amb, got, ref))
            qn_err.append(torch.where(amb, torch.zeros_like(b), b))
    for (cname, tname), c in zip(names, snap["critic"]):
        if nxt is not None:
            out, absval, L = net64(tr, p0, tname).forward_bound(next_state, nxt)
            if chain is None:
                qn64.append(out.view(-1))
                qn_err.append(mf.bound(absval, L).view(-1))
            judge(tname + " qn", c["qn"].view(-1), out.view(-1), mf.bound(absval, L).view(-1), "qn")
    # What the TD chain starts from: the float64 target values with their bound (mlp_f64.td, qn_err).  Where the launch keeps its
    # next actions that bound carries the proposal's interval and is some tens of times wider than a forward bound, so there the
    # chain is ALSO run from the launch's own qn with no target bound -- what the TD prologue read, judged above -- under the plain
    # keys, as before the target chain existed; the run from qn64 goes under "... from qn64".
    sources = [("", qn64, torch.maximum(qn_err[0], qn_err[-1]))]
    if nxt is None:
        sources = [("", [c["qn"].view(-1).to(F64) for c in snap["critic"]], None), (" from qn64",) + sources[0][1:]]
    got_c, covered = snap["grad_c"], torch.zeros(fl.total, dtype=torch.bool)
    loss_ref, loss_b = {sfx: 0.0 for sfx, _, _ in sources}, {sfx: 0.0 for sfx, _, _ in sources}
    parts = snap["parts_c"].view(len(names), -1)
    for i, ((cname, tname), c) in enumerate(zip(names, snap["critic"])):
        net = net64(tr, p0, cname)
        forward_checks(net, state, action, c["x0"], c["h1"], c["q"], worst, cname)
        logp = rec.get("logp_next")
        if tr.sac and i == 0 and evopf:
            # EVOPF-v0 (generic launches): the 28 heads at s', then log pi(a'|s') and the sampled ap' from those heads at the box of
            # s' and the critic update's draw.  (The basic components of the next actions are the projected proposal: the
            # completion and the projection are held by tests/test_evopf_f64_gpu.py.)
            out, absval, L = net64(tr, p0, "actor").forward_bound(next_state)
            judge("actor raw(s')", rec["raw_next"], out, mf.bound(absval, L), "raw")
            hd = evopf_gauss(next_state, rec["raw_next"], rec["eps_next"])
            judge("log pi(a'|s')", logp.view(-1), hd["logp"][0], hd["logp"][1], "logp")
            judge("ap(s')", rec["ap_next"], hd["ap"][0], hd["ap"][1], "ap")
        elif tr.sac and i == 0 and "raw_next" in rec:           # log pi(a'|s'): the generic launches keep the heads it was taken from
            out, absval, L = net64(tr, p0, "actor").forward_bound(next_state)
            judge("actor raw(s')", rec["raw_next"], out, mf.bound(absval, L), "raw")
            rn = rec["raw_next"].to(F64)
            fw = hf.gauss_head(rn[:, 0], rn[:, 1], rec["eps_next"], *box)
            mg = hf.gauss_mags(rn[:, 0], rn[:, 1], rec["eps_next"], box[0], box[1])
            judge("log pi(a'|s')", logp.view(-1), fw["logp"], hf.MARGIN * hf.C_REF_LOGP * hf.EPS32 * mg["logp"] + mf.TINY, "logp")
        elif tr.sac and i == 0:
            # the pipelines keep the heads inside their launch: log pi(a'|s') from the float64 actor at s' and the reproduced draw,
            # the head stage's own bound plus |d log pi / d heads| (autograd of heads_f64.gauss_head) on the forward bound of the heads
            out, absval, L = net64(tr, p0, "actor").forward_bound(next_state)
            rb = mf.bound(absval, L)
            fw = hf.gauss_head(out[:, 0], out[:, 1], rec["eps_next"], *box, dap=torch.zeros(B, dtype=F64), dlogp=1.0)
            mg = hf.gauss_mags(out[:, 0], out[:, 1], rec["eps_next"], box[0], box[1])
            allowed = hf.MARGIN * hf.C_REF_LOGP * hf.EPS32 * mg["logp"] + fw["g_mean"].abs() * rb[:, 0] + fw["g_ls"].abs() * rb[:, 1] + mf.TINY
            judge("log pi(a'|s')", logp.view(-1), fw["logp"], allowed, "logp(s')")
        for sfx, src, err in sources:
            grads, (lo_, lo_b), (dq, dq_b) = critic_chain(net, state, action, c["x0"], c["h1"], c["q"], src[0], err, reward, done,
                                                            ag.gamma, src[1] if tr.sac else None, logp, alpha)
            judge(cname + " dq" + sfx, c["dq"].view(-1), dq, dq_b, "dq" + sfx)
            got_loss = float(parts[i].double().sum())
            r = abs(got_loss - lo_) / lo_b
            worst["loss parts" + sfx] = max(worst.get("loss parts" + sfx, 0.0), r)
            loss_ref[sfx], loss_b[sfx] = loss_ref[sfx] + lo_, loss_b[sfx] + lo_b
            for k, (off, got) in _slices(tr, cname, got_c).items():
                ref, allowed = grads[k]
                judge("%s d%s%s" % (cname, k, sfx), got, ref, allowed, "critic " + k + sfx)
                covered[off:off + got.numel()] = True
    lo, hi = fl.critic_range
    assert int(torch.count_nonzero(got_c[lo:hi][~covered[lo:hi]])) == 0, "critic update: padding floats of its slice written"
    assert int(torch.count_nonzero(got_c[hi:])) == 0, "critic update: the actor's private slice or the multipliers written"
    for sfx, _, _ in sources:
        allowed = loss_b[sfx] + float(mf.bound(parts.double().abs().sum(), parts.numel()))
        r = abs(snap["loss_c"] - loss_ref[sfx]) / allowed
        worst["critic loss" + sfx] = r
        if r > 1.0:
            fails.append("critic loss%s %.9g vs %.9g: %.4g x the bound" % (sfx, snap["loss_c"], loss_ref[sfx], r))
            assert not strict, fails[-1]
    if snap["gradmax_c"] is not None:
        assert snap["gradmax_c"] == float(got_c[lo:hi].abs().max()), ("critic gradmax", snap["gradmax_c"], float(got_c[lo:hi].abs().max()))

    # ----------------------------------------------------------------------------------------------------------- policy half
    a = snap["actor"]
    actor = net64(tr, p1, "actor")
    forward_checks(actor, state, None, a["x0"], a["h1"], None, worst, "actor")
    crit64 = [net64(tr, p1, c) for c, _ in names]
    for net, (cname, _), sv in zip(crit64, names, a["critic"]):
        forward_checks(net, state, a["actions"], sv["x0"], sv["h1"], None, worst, cname + "@pi")
    nu = snap["nu"].numpy()
    eps_t = hf.eps_schedule(tr.eps_start, tr.eps, tr.decay_value, snap["t"])
    if tr.sac and evopf:
        import evopf_f64 as vf
        w1 = a["w1"].to(F64)
        ch = evopf_sac_actor_chain(tr.kernels.consts, actor, crit64, state, a["x0"], a["h1"], a["raw"], a["noise"], a["actions"],
                                   [(sv["x0"], sv["h1"]) for sv in a["critic"]], w1, nu, alpha, g_act=a["g_act"])
        r, ab, L = actor.head(a["h1"])
        mf.check("actor raw", a["raw"], r, ab, L, worst)
        judge("log pi", a["logp"].view(-1), ch["logp"][0], ch["logp"][1], "logp")
        judge("ap", a["ap"], ch["ap"][0], ch["ap"][1], "ap")
        # (the basic components of the stored action are the head's sample -- _gauss emits finished actions, hence no noise and
        #  no clip here; its Newton completion is held by tests/test_evopf_f64_gpu.py)
        worst["actions"] = vf.check_proposal(tr.kernels.consts, state.numpy(), a["ap"].numpy(), None, vf.NOISE_NONE, False, 0.0, 0,
                                             np.arange(B), snap["t"], a["actions"].numpy()[:, vf.PARTA])["act"]
    elif tr.sac:
        w1 = a["w1"].to(F64)
        ch = sac_actor_chain(env, actor, crit64, state, a["x0"], a["h1"], a["raw"], a["noise"], box, a["actions"],
                             [(sv["x0"], sv["h1"]) for sv in a["critic"]], w1, nu, alpha, shared, g_act=a["g_act"])
        r, ab, L = actor.head(a["h1"])
        mf.check("actor raw", a["raw"], r, ab, L, worst)
        judge("log pi", a["logp"].view(-1), ch["logp"][0], ch["logp"][1], "logp")
        judge("ap", a["actions"][:, env.p], ch["ap"][0], ch["ap"][1], "ap")     # (the basic component: the Gaussian head's sample)
        worst["actions"] = env.check_actions(a["actions"].numpy(), a["actions"].numpy()[:, env.p], None, 0.0, box[2], box[3], state.numpy())
    if tr.sac:
        _cap("min(Q1, Q2)", ch["tie"], worst, "min")
        decided = ~ch["tie"]
        want = (ch["q"][0][0] < ch["q"][1][0]).to(F64)
        assert bool((w1[decided] == want[decided]).all()), "d min(Q1, Q2): a row outside the ambiguity band took the other critic"
        assert bool(((w1 == 0) | (w1 == 1) | (w1 == 0.5)).all())
    elif evopf:
        import evopf_f64 as vf
        r, ab, L = actor.head(a["h1"])
        mf.check("actor raw", a["ap_det"], r, ab, L, worst)
        ch = evopf_actor_chain(tr.kernels.consts, actor, crit64[0], state, a["x0"], a["h1"], a["ap_det"], a["noise"], eps_t, a["actions"],
                               a["critic"][0]["x0"], a["critic"][0]["h1"], nu, g_act=a["g_act"])
        # (the basic components of the stored action are the proposal; its Newton completion is held by tests/test_evopf_f64_gpu.py)
        worst["actions"] = vf.check_proposal(tr.kernels.consts, state.numpy(), a["ap_det"].view(B, -1).numpy(), a["noise"].view(B, -1).numpy(),
                                             vf.NOISE_EXPLICIT, True, eps_t, 0, np.arange(B), snap["t"],
                                             a["actions"].numpy()[:, vf.PARTA])["act"]
    else:
        ch = ddpg_actor_chain(env, actor, crit64[0], state, a["x0"], a["h1"], a["noise"], eps_t, box, a["actions"],
                              a["critic"][0]["x0"], a["critic"][0]["h1"], nu, shared, g_act=a["g_act"])
        judge("ap_det", a["ap_det"].view(-1), ch["ap_det"][0], ch["ap_det"][1], "ap_det")
        worst["actions"] = env.check_actions(a["actions"].numpy(), a["ap_det"].view(-1).numpy(), a["noise"].numpy(), eps_t, box[2], box[3],
                                             state.numpy())
    assert worst["actions"] <= 1.0, "completed actions: %.4g x the tolerance" % worst["actions"]
    _cap("clip / clamp seams", ch["seam"], worst, "seam")
    _cap("relu(g)", ch["lag"]["ambiguous"], worst, "relu(g)")
    worst["g_act"] = float(ch["lag"]["ratio"].max()) / (1.0 if evopf else ef.tol_c(env.kind + "_lag"))
    if worst["g_act"] > 1.0:
        fails.append("g_act: %.4g x the tolerance" % worst["g_act"])
        assert not strict, fails[-1]
    got_a, covered = snap["grad_a"], torch.zeros(fl.total, dtype=torch.bool)
    for k, (off, got) in _slices(tr, "actor", got_a).items():
        ref, allowed = ch["grads"][k]
        judge("actor d%s" % k, got, ref, allowed, ("shared " if shared and k in ("Ws", "bs") else "actor ") + k)
        covered[off:off + got.numel()] = True
    lo, hi = fl.actor_range
    assert int(torch.count_nonzero(got_a[lo:hi][~covered[lo:hi]])) == 0, "policy step: padding floats of its slice written"
    assert int(torch.count_nonzero(got_a[:lo])) == 0, "policy step: the critic's private slice written"
    off = fl.offset[id(ag.nju.weight)]
    J = ag.nju.weight.numel()
    gnu, gnu_b = ch["gnu"]
    judge("d nu", got_a[off:off + J], torch.from_numpy(gnu), torch.from_numpy(gnu_b), "nu")
    other = torch.ones(fl.total, dtype=torch.bool)
    other[:hi] = False
    other[off:off + J] = False
    if snap["log_alpha_grad"] is not None:
        oa = fl.offset[id(ag.log_alpha)]
        if tr.automatic_entropy_tuning:
            other[oa] = False
            ref, b = alpha_grad(ch["logp"][0], ch["logp"][1], ag.target_entropy)
            r = abs(snap["log_alpha_grad"] - ref) / b
            worst["log_alpha"] = r
            if r > 1.0:
                fails.append("log_alpha.grad %.9g vs %.9g: %.4g x the bound" % (snap["log_alpha_grad"], ref, r))
                assert not strict, fails[-1]
        # (a log_alpha that is not tuned stays in `other`: its gradient word must be exactly 0)
    assert int(torch.count_nonzero(got_a[other])) == 0, "policy step: floats behind the actor's slice written (lambda, padding)"
    r = abs(snap["loss_a"] - ch["loss"][0]) / ch["loss"][1]
    worst["actor loss"] = r
    if r > 1.0:
        fails.append("actor loss %.9g vs %.9g: %.4g x the bound" % (snap["loss_a"], ch["loss"][0], r))
        assert not strict, fails[-1]
    if snap["gradmax_a"] is not None:
        assert snap["gradmax_a"] == float(got_a[lo:hi].abs().max()), ("actor gradmax", snap["gradmax_a"], float(got_a[lo:hi].abs().max()))
    info = dict(violating=ch["lag"]["violating"], gnu=gnu, fails=fails, g_act=float(a["g_act"].abs().max()))
    return worst, info


def report(tag, worst):
    print("%s: worst |err| / bound %s" % (tag, ", ".join("%s %.3g" % (k, v) for k, v in sorted(worst.items()))))
