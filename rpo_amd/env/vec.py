"""Device-resident state of N vectorised env instances (the rollout side of the hot path).

One ``VecEnv`` per (rank, purpose): the training rollout owns ``n_envs`` lanes plus the replay ring it scatters into;
evaluation uses a second, small one.  All tensors live in HBM; nothing here synchronises with the host.
"""
import torch

from .. import ops as hip_ops


class VecEnv(object):

    def __init__(self, kernels, n_envs, device, seed=0, env_id_base=0, max_episode_steps=None, viol_thresh=1e-3,
                 stats_cap=4096, ctrl=None, scenario=None, bank=None):
        self.k = kernels
        self.n = int(n_envs)
        self.device = device
        self.seed = int(seed)
        self.env_id_base = int(env_id_base)
        # no TimeLimit wrapper -> effectively unbounded (int32 max) episode length
        self.max_episode_steps = int(max_episode_steps) if max_episode_steps else 2 ** 31 - 1
        self.viol_thresh = float(viol_thresh)
        self.internal = torch.zeros(self.n, kernels.internal_dim, device=device)
        # CartSafe observes its internal state directly; SpringPendulum has a separate observation
        self.obs = self.internal if kernels.obs_dim == kernels.internal_dim else \
            torch.zeros(self.n, kernels.obs_dim, device=device)
        self.action = torch.zeros(self.n, kernels.action_dim, device=device)
        self.ep_len = torch.zeros(self.n, dtype=torch.int32, device=device)
        self.ep_ret = torch.zeros(self.n, device=device)
        self.ep_count = torch.zeros(self.n, dtype=torch.int32, device=device)
        self.stats = hip_ops.new_stats(stats_cap, device)
        self.ctrl = ctrl if ctrl is not None else torch.zeros(hip_ops.CTRL_LEN, dtype=torch.int64, device=device)
        self.steps_host = 0
        # (table [days, SCEN_DAY] float32, day [n] int32) on the device: the lanes play the caller's days, not the Philox draws
        # (EVOPF-v0 only: ops.evopf_reset_scenario / evopf_step_scenario; an evaluation seam -- no auto-reset)
        self.scenario = scenario
        if scenario is not None and not isinstance(kernels, hip_ops.EvopfKernels):
            raise NotImplementedError("scenarios are built for the HIP kernels of EVOPF-v0 only (its step kernel reads the "
                                      "table), not %s" % type(kernels).__name__)

        # (table [days, SCEN_DAY] float32 on the device, deal "uniform" | "cycle", stride = the run's total lane count): a scenario
        # BANK -- lane env_id_base + i is dealt one of the caller's days anew for every episode, a function of (seed, env id,
        # ep_count[i]) alone (ops.evopf_reset_bank / evopf_step_bank; auto-resets like the Philox days: the training seam)
        self.bank = None if bank is None else tuple(bank)
        if bank is not None and scenario is not None:
            raise ValueError("VecEnv takes scenario= (one fixed day per lane, evaluation) or bank= (a day per episode, training), "
                             "not both")
        if bank is not None and not isinstance(kernels, hip_ops.EvopfKernels):
            raise NotImplementedError("a scenario bank is built for the HIP kernels of EVOPF-v0 only (its step kernel reads the "
                                      "table), not %s" % type(kernels).__name__)
        if bank is not None and len(self.bank) != 3:
            raise ValueError("bank must be (table, deal, stride)")

    def reset(self):
        if self.bank is not None:
            hip_ops.evopf_reset_bank(self.k, self.internal, self.ep_len, self.ep_ret, self.ep_count, self.seed, self.env_id_base,
                                     *self.bank)
            return self.obs
        if self.scenario is not None:
            hip_ops.evopf_reset_scenario(self.k, self.internal, self.ep_len, self.ep_ret, *self.scenario)
            return self.obs
        self.k.reset(self.internal, self.obs, self.ep_len, self.ep_ret, self.ep_count, self.seed, self.env_id_base)
        return self.obs

    def set_internal(self, internal):
        """Inject explicit initial states (parity tests; SURVEY 8c 'parity tests inject initial states')."""
        self.internal.copy_(torch.as_tensor(internal, dtype=torch.float32, device=self.device))
        self.ep_len.zero_()
        self.ep_ret.zero_()
        if self.obs is not self.internal:
            th = self.internal[:, 0]
            self.obs.copy_(torch.stack([torch.cos(th), torch.sin(th), self.internal[:, 1], self.internal[:, 2],
                                        self.internal[:, 3]], dim=1))

    def step(self, action, rows=None, cap_steps=1, auto_reset=True):
        """One fused vector step; scatters the transitions into ``rows`` (the replay ring) when given."""
        if self.bank is not None:
            hip_ops.evopf_step_bank(self.k, self.internal, action, self.ep_len, self.ep_ret, self.ep_count, rows, cap_steps,
                                    self.stats, self.ctrl, self.max_episode_steps, auto_reset, self.viol_thresh, self.seed,
                                    self.env_id_base, *self.bank)
            self.steps_host += 1
            return self.obs
        if self.scenario is not None:
            if auto_reset:
                raise ValueError("a VecEnv with a scenario never auto-resets: step(auto_reset=False)")
            hip_ops.evopf_step_scenario(self.k, self.internal, action, self.ep_len, self.ep_ret, self.ep_count, rows, cap_steps,
                                        self.stats, self.ctrl, self.max_episode_steps, self.viol_thresh, *self.scenario)
            self.steps_host += 1
            return self.obs
        self.k.step(self.internal, self.obs, action, self.ep_len, self.ep_ret, self.ep_count, rows, cap_steps,
                    self.stats, self.ctrl, self.max_episode_steps, auto_reset, self.viol_thresh, self.seed,
                    self.env_id_base)
        self.steps_host += 1
        return self.obs
