"""RPO-DDPG on MI355X (reference: rpo/algo/rpo_ddpg.py).  Same constructor, attributes and methods as the reference's
``RPODDPG``; the loop is vectorised over ``num_envs`` lanes (extra keyword / ``RPO_NUM_ENVS``, default 1)."""
import torch

from .. import ops as hip_ops
from .agent import PDDDPG_PA
from .model import BoxConstraint
from .agent.flat import FusedAdam
from .lazy import LazyLoss, LazySum
from .trainer import _SALT_ACTOR, RPOTrainerBase, _LagrangianFn, _TDHuberFn, hyperparameters


class RPODDPG(RPOTrainerBase):

    def __init__(self, env, work_dir, name, logger, max_steps=10, embed_dim=256, hidden_dim=256, hidden_layer=1,
                 shared_param=True, value_type="add", ex_action_dim=0, lr_actor=1e-4, lr_critic=3e-4, lr_dual=1e-4,
                 reg=0, eps=0.1, eps_start=1.0, eps_epoch=10000, tau=0.005, gamma=0.95, capacity=10000, warmup=1000,
                 corr_lr=1e-5, eval_lr=1e-5, corr_mode=0, corr_eps=1e-5, corr_momentum=0.5, batch_size=256,
                 policy_fre=2, eval_fre=500, max_epochs=100000, grad_eps=1e-3, eval_steps=None, init_lamb=0.0,
                 init_nju=0.0, fixed=False, clip_thres="inf", partial=False, partial_idx=None,
                 device=torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu"),
                 num_envs=None, seed=None, backend=None, use_graph=None, updates_per_step=None, schedule=None,
                 eval_episodes=None, keep_best=None, scenarios=None, deal="uniform"):
        base = getattr(env, "unwrapped", env)
        agent = PDDDPG_PA(
            base.state_dim, base.action_dim, base.eq_num, base.ineq_num, embed_dim=embed_dim, hidden_dim=hidden_dim,
            hidden_layer=hidden_layer, shared_param=shared_param, value_type=value_type, ex_action_dim=ex_action_dim,
            box_constraint=BoxConstraint(*base.box_constraint_partial, device=device, volatile=base.volatile,
                                         update=base.update),
            lr_actor=lr_actor, lr_critic=lr_critic, lr_dual=lr_dual, reg=reg, eps=eps_start, tau=tau, gamma=gamma,
            capacity=capacity, init_lamb=init_lamb, init_nju=init_nju, partial=partial,
            partial_idx=base.partial_actions if partial_idx is None else partial_idx, device=device, backend=backend,
            clip_thres=clip_thres)
        self._setup(env, work_dir, name, logger, agent, hyperparameters(locals()), device, num_envs, seed, backend, use_graph,
                    updates_per_step, schedule=schedule, scenarios=scenarios, deal=deal)

    # ---- rollout policy (rpo_ddpg.py:98-106, agent/ddpg_pa.py:101-112) ----------------------------------------
    def _actor_out(self, name, obs, save=False, tag=None):
        """Deterministic basic action [n] of `actor` / `actor_target` through the fused MLP kernel.  `tag`: the output buffer's
        name when it must not be the rollout's (the policy step's prefix runs on a second stream BESIDE other launches: with
        num_envs == batch_size the shape-keyed "actor.out" would be one buffer for both)."""
        f = self.fused
        P = self.kernels.partial_dim
        # P > 1 (EVOPF): raw outputs; the env kernels apply the state-dependent tanh box (ap_is_raw)
        return f.forward(name, obs, None, f.buf((tag or name) + ".out", obs.shape[0], P), save=save,
                         tanh_box=self._box_affine).view(-1)

    def _policy_partial(self, obs, warm):
        if warm:
            return None, hip_ops.NOISE_UNIFORM                      # BoxConstraint.sample, inside the kernel
        if self.fused is not None:
            return self._actor_out("actor", obs), hip_ops.NOISE_PHILOX
        return self.agent.actor(obs).reshape(-1), hip_ops.NOISE_PHILOX   # + eps_t * N(0,1), clip: inside the kernel

    def _eval_partial(self, obs):
        if self.fused is not None:
            return self._actor_out("actor", obs)
        return self.agent.actor(obs).reshape(-1)

    # ---- fused pipelines (one launch per stage group; CartSafe kernels provide them) -----------------------------
    @property
    def _pipelines(self):
        return self._critic_pipeline_ok("ddpg_critic", "actor_target", "critic")

    @property
    def _actor_pipeline(self):
        return self._actor_pipeline_ok("ddpg_actor_forward", "critic")

    def _critic_update_pipeline(self, cols):
        f, B, buf = self.fused, self.batch_size, self.buffer
        d = f.descs["critic"]
        scale, base = self._box_affine
        parts = f.buf("loss_parts", (B + 15) // 16)
        idx_in = self._idx_inject() if self._idx_inject is not None else None
        if not hasattr(self.kernels, "ddpg_critic_forward"):
            # SpringPendulum: the chain is cut at the batch-coupled projection (front | project | back)
            ap = f.buf("crit.ap", B)
            self.kernels.ddpg_critic_front(f.descs["actor_target"], scale, base, buf.rows, buf.capacity, buf.n_envs,
                                           self._batch, None, idx_in, buf.seed, 0, self._uctrl, ap)
            next_actions = self._project_batch(cols[2], ap)
            q, qn = f.buf("q", B, 1), f.buf("qn", B, 1)
            self.kernels.ddpg_critic_back(f.descs["critic_target"], d, self._batch, next_actions, q, qn,
                                          f.buf("critic.x0", B, d.ein), f.buf("critic.h1", B, d.H))
            return self._critic_backward_td(cols, q, qn, parts)
        q, qn = f.buf("q", B, 1), f.buf("qn", B, 1)
        self.kernels.ddpg_critic_forward(
            f.descs["actor_target"], f.descs["critic_target"], d, scale, base, buf.rows, buf.capacity, buf.n_envs,
            self._batch, None, idx_in, buf.seed, 0, self._uctrl, self.max_steps, self.corr_lr, self.corr_eps,
            self.corr_momentum, self._box_lo, self._box_hi, q, qn, f.buf("critic.x0", B, d.ein), f.buf("critic.h1", B, d.H))
        self._critic_backward_td(cols, q, qn, parts)

    def _critic_backward_td(self, cols, q, qn, parts):
        """Backward of the critic with the TD target / Huber loss as its prologue (rpo_td): the forward pipeline's target
        chain and critic ran in separate workgroups and meet here."""
        f, B = self.fused, self.batch_size
        td = self.backend.Td(q.view(-1), qn.view(-1), None, None, cols[3], cols[4], 0.0, self.agent.gamma,
                             f.buf("dq", B, 1).view(-1), parts)
        self._zero_grads()
        gm = self._critic_gradmax()
        f.backward("critic", cols[0], cols[1], None, gradmax=gm, td=td)
        self._gradmax_ready = gm is not None
        self.last_losses["critic"] = LazySum(parts)

    # ---- the update through the generic MLP launches (same arithmetic as critic_loss / actor_loss below) ---------
    def _critic_update_generic(self, cols):
        f, B = self.fused, self.batch_size
        state, action, next_state = cols[:3]
        next_actions = self._project_batch(next_state, self._actor_out("actor_target", next_state))
        qn, q = f.forward_multi([("critic_target", next_state, next_actions, f.buf("qn", B, 1), False),
                                 ("critic", state, action, f.buf("q", B, 1), True)])
        # TD target / Huber loss: the prologue of the backward pass (rpo_td)
        self._critic_backward_td(cols, q, qn, f.buf("loss_parts", (B + 15) // 16))

    def _actor_update_pipeline(self, cols):
        """The policy step in two launches + the actor's weights pass (fused.hip)."""
        f, ag, B, k = self.fused, self.agent, self.batch_size, self.kernels
        da_, dc = f.descs["actor"], f.descs["critic"]
        scale, base = self._box_affine
        b = f.buf
        parts = b("actor.parts", (B + 15) // 16, 8)
        ap_det, noise, actions = b("act.ap_det", B), b("act.noise", B), b("act_pi", B, k.action_dim)
        q, dq, g_act = b("q_pi", B, 1), b("dq_pi", B, 1), b("g_act", B, k.action_dim)
        # (tests replay the reference's draw)
        noise_in = self._draw_batch(_SALT_ACTOR).view(-1) if self._idx_inject is not None else None
        self.backend.ddpg_actor_forward(k, da_, dc, scale, base, self._box_lo, self._box_hi, self.eps_start, self.eps, self.decay_value,
                             self._batch, noise_in, self.seed, self.dist.rank * B, _SALT_ACTOR, self._uctrl,
                             ag.nju.weight.view(-1), ap_det, noise, actions, q, dq, g_act, parts, b("actor.x0", B, da_.ein),
                             b("actor.h1", B, da_.H), b("critic.x0", B, dc.ein), b("critic.h1", B, dc.H))
        self._zero_grads()
        shared = ag.flat.sizes[1] > 0
        gm = self._fused_gradmax(ag.actor_optim)
        lag = b("actor.lag", 2)
        self.backend.ddpg_actor_backward(k, da_, dc, shared, self._batch, actions, g_act, ap_det, noise, dq, self.eps_start, self.eps,
                              self.decay_value, self._box_lo, self._box_hi, scale, base, self._uctrl,
                              b("actor.x0", B, da_.ein), b("actor.h1", B, da_.H), b("critic.x0", B, dc.ein),
                              b("critic.h1", B, dc.H), b("actor.dh", B, da_.H), b("actor.dx0", B, da_.ein),
                              b("critic.dh", B, dc.H), b("critic.dx0", B, dc.ein), b("da", B, k.action_dim), b("do", B),
                              parts, lag, ag.nju.weight.grad.view(-1), gm)
        self._actor_gradmax_ready = gm is not None
        return self._pipeline_actor_out(lag, parts, None)

    def _pipeline_actor_out(self, lag, parts, logp):
        """What `_actor_update` returns from the words the policy pipelines (row-tile or column-split) leave on the device:
        mean Lagrangian term - mean Q."""
        loss = self.last_losses["actor"] = LazyLoss(lambda lag: lag[0] - lag[1], lag)
        return loss

    def _actor_update_generic(self, cols, pre):
        f, ag, B, k = self.fused, self.agent, self.batch_size, self.kernels
        state = cols[0]
        ap_det, noise, actions, lag, g_act, fa = pre
        # (its own buffer: the lazily reduced actor loss below keeps a reference to it, and the next critic-only update writes
        #  Q(s, a_replay) into "q" -- ADVICE r03)
        q = f.forward("critic", state, actions, f.buf("q_pi", B, 1), save=True)
        dq = self._const_dq(B)                                 # d mean(-Q) / dQ: a constant, filled once
        da = f.buf("da", B, k.action_dim)
        shared = ag.flat.sizes[1] > 0      # shared embedding: the critic path contributes to its gradient
        f.backward("critic", state, actions, dq, da=da, param_grads=shared, first_layer_state_only=True)
        P = k.partial_dim
        dap, do = f.buf("dap", B * P), f.buf("do", B, P)
        if fa:
            k.complete_bwd(state, da, dap, action=actions, grad_action2=g_act)
        else:
            da.add_(g_act)
            k.complete_bwd(state, da, dap, action=actions)
        if self._box_affine is None:       # state-dependent box: the env's kernel knows it
            k.tanh_box_bwd(state, ap_det, noise, self.eps_start, self.eps, self.decay_value, self._uctrl, dap, do.view(-1))
        else:
            scale, base = self._box_affine
            self.backend.tanh_box_bwd(dap, ap_det, noise, self.eps_start, self.eps, self.decay_value, self._uctrl,
                                      self._box_lo, self._box_hi, scale, base, do.view(-1))
        # (no shared embedding: every gradient of the actor's slice is written by this backward -- it leaves the inf-norm for
        #  clip_grad_norm_, no rpo_absmax launch)
        gm = self._fused_gradmax(ag.actor_optim, alone=not shared)
        f.backward("actor", state, None, do, gradmax=gm)
        self._actor_gradmax_ready = gm is not None
        # mean Lagrangian term (one device word) - mean Q (a [B, 1] buffer), reduced only when somebody looks
        loss = self.last_losses["actor"] = LazyLoss(lambda lag, q: lag[0] - q.mean(), lag, q)
        return loss

    def _actor_prefix(self, cols):
        """What the policy step computes from the ACTOR alone (generic launches): pi(s) with saved activations, the exploration
        draw, Complete, and the Lagrangian term of the completed actions (its d/d action and d/d nu).  None of it reads what
        the critic update writes, so the graph windows of EVOPF-v0 run it on the second captured branch BESIDE the critic
        update of a policy iteration (trainer._overlapped_window; round 5: ~50 us off a 364 us chain) -- same launches, same
        arguments, same bits as inside `_actor_update`."""
        state = cols[0]
        ap_det = self._actor_out("actor", state, save=True, tag="pi")
        noise = self._draw_batch(_SALT_ACTOR).view(-1)
        actions = self._complete_only(state, ap_det, noise)
        return (ap_det, noise, actions) + self._lagrangian_term(state, actions)

    def _const_dq(self, B):
        key = ("dq_pi_const", B)
        if key not in self.fused._scratch:
            self.fused._scratch[key] = torch.full((B, 1), -1.0 / B, device=self.device)
        return self.fused._scratch[key]

    # ---- losses ---------------------------------------------------------------------------------------------
    def critic_loss(self, state, action, next_state, done, reward, ineq_viol=None, eq_viol=None):
        """Huber(Q(s,a), r + gamma (1-d) Q_targ(s', Proj(Complete(pi_targ(s'))))) (rpo_ddpg.py:327-337)."""
        ag = self.agent
        with torch.no_grad():
            next_partial = ag.take_action(next_state, deterministic=True, target=True)
            next_actions = self.process_action(next_state, next_partial)
            next_q = ag.critic_target(next_state, next_actions)
        q = ag.critic(state, action)
        return _TDHuberFn.apply(self.backend, ag.gamma, 0.0, reward, done, next_q, None, None, q, None)

    def actor_loss(self, state):
        """mean(-Q(s, Complete(pi(s) + noise)) + nu . relu(g)) (rpo_ddpg.py:307-324); the exploration noise of
        take_action comes from the Philox stream instead of torch's global generator."""
        ag = self.agent
        ap = ag.actor(state)
        noise = self._draw_batch(_SALT_ACTOR)
        ap = ag.actor.box_constraint.clip(ap + self._eps_now() * noise, state)
        actions = self.base_env.complete_partial(state, ap)
        loss = (-ag.critic(state, actions)).mean()
        return loss + _LagrangianFn.apply(self.kernels, actions, ag.nju.weight, state)

    # ---- optimiser steps (rpo_ddpg.py:178-205) --------------------------------------------------------------
    # The Polyak updates of a policy step (rpo_ddpg.py:205) ride in the Adam launches that produce the parameters they
    # average -- same arithmetic, two launches fewer.  With a shared state embedding the critic's target must see the
    # embedding AFTER the actor's step, so its update stays a separate launch at the end.
    def _critic_step(self, actor_step):
        ag = self.agent
        fuse = actor_step and ag.flat.sizes[1] == 0
        ag.critic_optim.step(target=ag.critic_target_flat if fuse else None, tau=ag.tau,
                             gradmax_ready=self._take("_gradmax_ready"), clock=self._clock(not actor_step),
                             prepared=self._take("_critic_prepared"))

    def _actor_step(self, actor_out):
        # actor Adam (+ Polyak of the actor target) | multiplier DualAdam | Polyak of the critic target: one launch.
        # With a shared state embedding the actor's step moves the critic's copy of it too, so the shared part of the
        # critic target follows inside the actor's slice (target2) and only the critic-only part is a slice of its own.
        ag, fl = self.agent, self.agent.flat
        c = fl.actor_range[0]                                  # [critic-only | shared | actor-only], padded offsets
        sh = fl.critic_range[1] - c if fl.sizes[1] > 0 else 0
        segs = [ag.actor_optim.segment(target=ag.actor_target_flat, tau=ag.tau,
                                       gradmax_ready=self._take("_actor_gradmax_ready"),
                                       target2=ag.critic_target_flat[c:c + sh] if sh > 0 else None, n2=sh)]
        if not self.fixed:
            segs.append(ag.nju_optim.segment())                    # lambda is never stepped (rpo_ddpg.py:202)
        if sh > 0 and c > 0:
            segs.append(dict(polyak_only=True, param=fl.param((0, c)), target=ag.critic_target_flat[:c], tau=ag.tau))
        FusedAdam.step_many(self.backend, segs, clock=self._clock(True), prepared=self._take("_actor_prepared"))
