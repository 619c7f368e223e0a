"""EVOPF-v0: AC optimal power flow on the IEEE 14-bus network with a battery at every generator bus (reference:
rpo/env/electrical_grid/evopf.py).  One episode = 24 hourly steps of a random load / price day.

Observation [57] = per-unit active / reactive demand of the 14 buses, state of charge of the 5 batteries, 24-hour price
look-ahead.  Action [43] = (pg[5], qg[5], vm[14], va[14], pe[5]).  The actor sets the 14 basic actions (pg at the 4 PV
generators, vm at the 5 generator buses, pe); ``complete_partial`` solves the 28 power-balance equations for the rest
by Newton's method, ``ineq_partial_grad`` is the reduced gradient used by the GRG projection.  All of it runs in the
HIP kernels of rpo_amd/csrc/evopf.hip (one wavefront per env lane); this class holds the tables and the Python surface.

Differences to the reference, all stated in DESIGN.md: the loaders' random day (np.random.dirichlet / rand / randn,
data/demand.py:53-62, data/price.py:41-43) comes from the build's Philox streams keyed by (seed, lane, episode);
``render`` (igraph) is not part of the hot path.

The optimal power flow: ``opf(state, pe)`` solves every row's single-step AC-OPF -- the cheapest (pg, qg, vm, va) that meets the
power balance and the bounds, for the row's demand and a GIVEN battery power -- on the device (rpo_amd/csrc/evopf_opf.hip: a
primal-dual interior point method, one wavefront per state) and returns an ``OpfResult`` of device tensors.  ``opt_solve(X)`` is
the reference's method of that name (there: pypower's interior-point OPF, one state at a time on the CPU) on top of it, and
``EvalTrajectory.opf_gap(env)`` (rpo_amd/algo/evaluation.py) the optimality gap of a recorded evaluation.  ``opf(state,
pe="free")`` dispatches the batteries too: it minimises ``obj_fn + pe_cost . pe`` over all 43 components with the battery box of
the row's state of charge, by default at the price that makes the optimum the best one-step reward (``reward_fn``); it is the
controller of ``trainer.evaluate_opf`` and the reference of ``opf_gap(pe="free")``.  ``nearest_feasible(obs, action)`` is the safety
filter: the dispatch nearest to a policy's action, in its 14 controlled components, that meets the same equations and bounds (a
third instance of that kernel; ``NearestResult``; ``trainer.evaluate_filtered`` plays whole episodes through it).  There is no CPU
path: on the oracle backend or a CPU device all of these raise NotImplementedError with that reason.
"""
import numpy as np
import torch

from ... import ops as hip_ops
from ..base import HardConstraintEnv, gym
from . import case14

spaces = gym.spaces


class EVOPFEnv(HardConstraintEnv):
    metadata = {"render.modes": ["human", "rgb_array"], "video.frames_per_second": 50}
    volatile = True                                                      # evopf.py:346

    def __init__(self, backend=None, device=None):
        super().__init__(backend, device)
        bus, gen = case14.BUS, case14.GEN
        self.nbus, self.ng = bus.shape[0], gen.shape[0]
        self.ne = self.ng
        self.nahead = case14.NAHEAD
        self.baseMVA = case14.BASE_MVA
        self.genbase = gen[:, case14.GEN_MBASE]
        # bus classes and index sets, evopf.py:225-239,278-311
        self.slack = np.where(bus[:, case14.BUS_TYPE] == 3)[0]
        self.pv = np.where(bus[:, case14.BUS_TYPE] == 2)[0]
        self.spv = np.sort(np.concatenate([self.slack, self.pv]))
        self.pq = np.setdiff1d(np.arange(self.nbus), self.spv)
        self.slack_ = np.array([np.where(x == self.spv)[0][0] for x in self.slack])
        self.pv_ = np.array([np.where(x == self.spv)[0][0] for x in self.pv])
        self.spv_ = np.arange(self.ng)
        self.nslack, self.npv = len(self.slack), len(self.pv)
        if list(self.spv) != [0, 1, 2, 5, 7]:
            raise ValueError("the EVOPF kernels are compiled for the IEEE-14 bus classification")
        self.pg_start_yidx, self.qg_start_yidx = 0, self.ng
        self.vm_start_yidx, self.va_start_yidx = 2 * self.ng, 2 * self.ng + self.nbus
        self.pe_start_yidx = 2 * self.ng + 2 * self.nbus
        self._xdim, self._ydim = 2 * self.nbus, 2 * self.ng + 2 * self.nbus + self.ne
        self._partial_vars = np.concatenate([self.pg_start_yidx + self.pv_, self.vm_start_yidx + self.spv,
                                             self.va_start_yidx + self.slack, self.pe_start_yidx + self.spv_])
        self._other_vars = np.setdiff1d(np.arange(self._ydim), self._partial_vars)
        self._partial_actions = np.concatenate([self.pg_start_yidx + self.pv_, self.vm_start_yidx + self.spv,
                                                self.pe_start_yidx + self.spv_])
        self._other_actions = self._other_vars.copy()
        self.we, self.wg = 5.0, 1.0                                                       # evopf.py:244-245
        self.pmax, self.pmin = gen[:, case14.GEN_PMAX] / self.genbase, gen[:, case14.GEN_PMIN] / self.genbase
        self.qmax, self.qmin = gen[:, case14.GEN_QMAX] / self.genbase, gen[:, case14.GEN_QMIN] / self.genbase
        self.vmax, self.vmin = bus[:, case14.VMAX].copy(), bus[:, case14.VMIN].copy()
        # Battery(p_data, num=ne, genbase=baseMVA, init_strategy="empty"), evopf.py:243 with the defaults of :25-26
        self.evs_low, self.evs_high, self.evs_p_min, self.evs_p_max = 0.1, 0.8, -0.2, 0.2
        self.eta_in = self.eta_out = 0.9
        pd_max = qd_max = 10.0                                                            # evopf.py:319-331
        high = np.array([pd_max] * self.nbus + [qd_max] * self.nbus + [self.evs_high] * self.ne + [240.0] * self.nahead)
        low = np.array([-pd_max] * self.nbus + [-qd_max] * self.nbus + [self.evs_low] * self.ne + [0.0] * self.nahead)
        a_high = np.concatenate([self.pmax, self.qmax, self.vmax, [np.pi] * self.nbus, [self.evs_p_max] * self.ne])
        a_low = np.concatenate([self.pmin, self.qmin, self.vmin, [-np.pi] * self.nbus, [self.evs_p_min] * self.ne])
        self.action_space = spaces.Box(low=a_low.astype(np.float32), high=a_high.astype(np.float32), dtype=np.float32)
        self.observation_space = spaces.Box(low=low.astype(np.float32), high=high.astype(np.float32), dtype=np.float32)
        self.state_dim, self.action_dim = self.observation_space.shape[0], self.action_space.shape[0]
        self.eq_num, self.ineq_num = 28, 58                                               # evopf.py:336-337
        # the blocks of ineq_resid (evopf.py:548-563) / eq_resid in their order: generator limits, voltage bands, battery
        # charge rates (pg - pmax, pmin - pg, ...); active and reactive power balance per bus
        blocks = (("pgmax", self.ng), ("pgmin", self.ng), ("qgmax", self.ng), ("qgmin", self.ng), ("vmax", self.nbus),
                  ("vmin", self.nbus), ("pemax", self.ne), ("pemin", self.ne))
        self.ineq_names = tuple("%s[%d]" % (b, j) for b, m in blocks for j in range(m))
        self.eq_names = tuple("%s[%d]" % (b, j) for b in ("pbal", "qbal") for j in range(self.nbus))
        self._table = case14.kernel_constants(hip_ops.CONST, hip_ops.CONST["RPO_EVOPF_CONSTS_LEN"])
        self._box_cache = {}
        self.seed()
        self.state = None
        self._episodes = 0

    # ------------------------------------------------------------------------------------------ properties
    partial_actions = property(lambda self: self._partial_actions)
    other_actions = property(lambda self: self._other_actions)
    partial_vars = property(lambda self: self._partial_vars)
    other_vars = property(lambda self: self._other_vars)
    xdim = property(lambda self: self._xdim)
    ydim = property(lambda self: self._ydim)
    neq = property(lambda self: 2 * self.nbus)
    nineq = property(lambda self: 4 * self.ng + 2 * self.nbus)

    @property
    def box_constraint(self):
        return self.action_space.low, self.action_space.high

    @property
    def box_constraint_partial(self):
        return self.action_space.low[self.partial_actions], self.action_space.high[self.partial_actions]

    def _make_kernels(self):
        return self._backend.EvopfKernels(self._table)

    # ------------------------------------------------------------------------------------------ state-dependent box
    def battery_bounds(self, soc):
        """Battery.update_bound (evopf.py:127-143): charge-rate limits shrunk by the state of charge; torch or numpy."""
        if isinstance(soc, torch.Tensor):
            p_max = torch.clamp(self.evs_high - soc, max=self.evs_p_max) / self.eta_in
            p_min = self.eta_out * torch.clamp(self.evs_low - soc, min=self.evs_p_min)
        else:
            p_max = np.minimum(self.evs_p_max, self.evs_high - soc) / self.eta_in
            p_min = self.eta_out * np.maximum(self.evs_p_min, self.evs_low - soc)
        return p_max, p_min

    def update(self, state, full=False):
        """(low, high) of the action box for every row of ``state`` (evopf.py:769-783).  Tensors in, tensors out (on
        the state's device, no host round trip -- the reference goes through numpy); arrays in, arrays out."""
        low, high = self.box_constraint if full else self.box_constraint_partial
        if isinstance(state, torch.Tensor):
            if state.dim() == 1:
                state = state.view(1, -1)
            key = (state.device, bool(full))
            if key not in self._box_cache:
                self._box_cache[key] = (torch.as_tensor(low, device=state.device), torch.as_tensor(high, device=state.device))
            lo, hi = self._box_cache[key]
            n = state.shape[0]
            soc = state[:, -self.ne - self.nahead:-self.nahead]
            p_max, p_min = self.battery_bounds(soc)
            return (torch.cat([lo[:-self.ne].expand(n, -1), p_min], dim=1),
                    torch.cat([hi[:-self.ne].expand(n, -1), p_max], dim=1))
        state = np.asarray(state)
        if state.ndim == 1:
            state = state[None]
        n = state.shape[0]
        p_max, p_min = self.battery_bounds(state[:, -self.ne - self.nahead:-self.nahead])
        low, high = low[None].repeat(n, axis=0), high[None].repeat(n, axis=0)
        low[:, -self.ne:], high[:, -self.ne:] = p_min, p_max
        return low, high

    # ------------------------------------------------------------------------------------------ gym API (1 env)
    def reset(self):
        """evopf.py:369-380: hour 0 of a fresh random day (episode counter of this env instance)."""
        vec = self._single()
        vec.ep_count.fill_(self._episodes)
        self._episodes += 1
        vec.reset()
        self.state = vec.obs[0].cpu().numpy().astype(np.float64)
        return self.state.copy()

    def step(self, action):
        """evopf.py:348-366 through the vectorised kernel (n = 1, no auto-reset): (obs, reward, done, info)."""
        vec = self._single()
        a = self._t(np.asarray(action, dtype=np.float32).reshape(1, -1))
        vec.ctrl.zero_()
        self.kernels.step(vec.internal, vec.obs, a, vec.ep_len, vec.ep_ret, vec.ep_count, self._row, 1, None, vec.ctrl,
                          2 ** 31 - 1, False, vec.viol_thresh, vec.seed, 0)
        row = self._row[0].cpu().numpy()
        c = self.kernels.cols
        self.state = vec.obs[0].cpu().numpy().astype(np.float64)
        info = {"ineq_viol": row[c["ineq_viol"][0]:c["ineq_viol"][1]][None].copy(),
                "eq_viol": row[c["eq_viol"][0]:c["eq_viol"][1]][None].copy()}
        return self.state.copy(), float(row[c["reward"][0]]), bool(row[c["done"][0]] > 0.5), info

    def decompose(self, state):
        return state[:2 * self.nbus], state[2 * self.nbus:]

    def get_action_vars(self, action):
        ng, nb = self.ng, self.nbus
        return (action[:, :ng], action[:, ng:2 * ng], action[:, 2 * ng:2 * ng + nb], action[:, -self.ne - nb:-self.ne],
                action[:, -self.ne:])

    def obj_fn(self, action):
        """Generation cost / mean(genbase)^2 (evopf.py:509-518)."""
        action = self._t(action)
        if action.dim() == 1:
            action = action.view(1, -1)
        pg_mw = action[:, :self.ng] * self._t(self.genbase)
        quad, lin = self._t(case14.GENCOST[:, 4]), self._t(case14.GENCOST[:, 5])
        cost = (quad * pg_mw ** 2).sum(dim=1) + (lin * pg_mw).sum(dim=1) + float(case14.GENCOST[:, 6].sum())
        return cost / float(self.genbase.mean() ** 2)

    # ------------------------------------------------------------------------------------------ constraint API
    def complete_partial(self, state, action_partial):
        state, ap = self._t(state), self._t(action_partial)
        if ap.dim() == 1:
            ap = ap.view(1, -1)
        return super().complete_partial(state if state.dim() == 2 else state.view(1, -1), ap)

    def _resid_backward(self, obs, action, grad_eq, grad_ineq):
        """d/d action of the residuals: inequality rows are constant +-identity blocks (evopf.py:663-707); the equality
        rows go through rpo_evopf_eq_vjp (torch autograd through eq_resid, used by the Lagrangian baselines)."""
        ng, nb = self.ng, self.nbus
        g = torch.zeros_like(action)
        if grad_eq is not None:                                 # J_eq^T grad_eq, what autograd derives from eq_resid
            self.kernels.eq_vjp(action.contiguous(), grad_eq.contiguous(), g, autograd_sign=True)
        if grad_ineq is not None:
            g[:, :ng] += grad_ineq[:, :ng] - grad_ineq[:, ng:2 * ng]
            g[:, ng:2 * ng] += grad_ineq[:, 2 * ng:3 * ng] - grad_ineq[:, 3 * ng:4 * ng]
            g[:, 2 * ng:2 * ng + nb] += grad_ineq[:, 4 * ng:4 * ng + nb] - grad_ineq[:, 4 * ng + nb:4 * ng + 2 * nb]
            g[:, -self.ne:] += grad_ineq[:, -2 * self.ne:-self.ne] - grad_ineq[:, -self.ne:]
        return g

    # -- the reference's remaining constraint functions (evopf.py:564-594,614-707), thin host methods over the kernels:
    # Jacobian entries come from rpo_evopf_eq_vjp with unit cotangents (autograd_sign = 0: eq_jac's own battery sign, DESIGN E1)
    def eq_jac(self, action):
        """d eq_resid / d action as eq_jac builds it (evopf.py:614-661) -> [n, 28, 43]."""
        a = self._t(action)
        a = (a if a.dim() == 2 else a.view(1, -1)).contiguous()
        n, m, y = a.shape[0], self.eq_num, self._ydim
        rows = a.repeat_interleave(m, dim=0).contiguous()                    # row (b, r) = action b with cotangent e_r
        cot = torch.eye(m, device=a.device, dtype=a.dtype).repeat(n, 1).contiguous()
        out = torch.empty(n * m, y, device=a.device, dtype=a.dtype)
        self.kernels.eq_vjp(rows, cot, out, autograd_sign=False)
        return out.view(n, m, y)

    def ineq_jac(self, state, action):
        """Constant +-identity blocks (evopf.py:663-707), expanded over the batch -> [n, 58, 43]."""
        n = self._t(action).reshape(-1, self._ydim).shape[0]
        key = ("ineq_jac", self.device)
        if key not in self._box_cache:
            ng, nb, ne, y = self.ng, self.nbus, self.ne, self._ydim
            j = torch.zeros(self.ineq_num, y)
            r = 0
            for start, size in ((self.pg_start_yidx, ng), (self.qg_start_yidx, ng), (self.vm_start_yidx, nb),
                                (self.pe_start_yidx, ne)):
                j[r:r + size, start:start + size] = torch.eye(size)
                j[r + size:r + 2 * size, start:start + size] = -torch.eye(size)
                r += 2 * size
            self._box_cache[key] = j.to(self.device)
        return self._box_cache[key].unsqueeze(0).expand(n, -1, -1)

    def eq_grad(self, state, action):
        """2 J_eq^T eq_resid (evopf.py:574-577) -> [n, 43]."""
        state, a = self._t(state), self._t(action)
        a = (a if a.dim() == 2 else a.view(1, -1)).contiguous()
        resid = self.eq_resid(state if state.dim() == 2 else state.view(1, -1), a).detach().contiguous()
        out = torch.empty_like(a)
        self.kernels.eq_vjp(a, resid, out, autograd_sign=False)
        return 2 * out

    def _ineq_jac_t(self, weights):
        """ineq_jac^T weights for [n, 58] weights: every inequality bounds one action component from above or below."""
        ng, nb, ne = self.ng, self.nbus, self.ne
        g = torch.zeros(weights.shape[0], self._ydim, device=weights.device, dtype=weights.dtype)
        g[:, :ng] = weights[:, :ng] - weights[:, ng:2 * ng]
        g[:, ng:2 * ng] = weights[:, 2 * ng:3 * ng] - weights[:, 3 * ng:4 * ng]
        g[:, 2 * ng:2 * ng + nb] = weights[:, 4 * ng:4 * ng + nb] - weights[:, 4 * ng + nb:4 * ng + 2 * nb]
        g[:, -ne:] = weights[:, -2 * ne:-ne] - weights[:, -ne:]
        return g

    def _dist2(self, state, action):
        state, a = self._t(state), self._t(action)
        return self.ineq_dist(state if state.dim() == 2 else state.view(1, -1), a if a.dim() == 2 else a.view(1, -1)).detach()

    def ineq_grad(self, state, action, eps=0.0):
        """2 J_ineq^T (dist + eps 1[dist > 0]) (evopf.py:579-583)."""
        d = self._dist2(state, action)
        return 2 * self._ineq_jac_t(d + (d > 0) * eps)

    def ineq_grad_new(self, state, action, eps=0.0):
        """J_ineq^T 1[dist > 0]: +-1 per violated bound (evopf.py:585-589); `eps` is unused there too."""
        return self._ineq_jac_t((self._dist2(state, action) > 0).to(torch.float32))

    def ineq_dist_np(self, state, action):
        """evopf.py:564-567: one (state, action) pair in, [1, 58] array out."""
        a = torch.as_tensor(np.asarray(action), dtype=torch.float32, device=self.device).view(1, -1)
        s = torch.as_tensor(np.asarray(state), dtype=torch.float32, device=self.device).view(1, -1)
        return self.ineq_dist(s, a).detach().cpu().numpy()

    def eq_resid_np(self, state, action):
        """evopf.py:569-572."""
        a = torch.as_tensor(np.asarray(action), dtype=torch.float32, device=self.device).view(1, -1)
        s = torch.as_tensor(np.asarray(state), dtype=torch.float32, device=self.device).view(1, -1)
        return self.eq_resid(s, a).detach().cpu().numpy()

    # ------------------------------------------------------------------------------------------ optimal power flow
    def _opf_kernel(self):
        """The backend's single-step OPF kernel, or NotImplementedError with the reason there is none."""
        fn = getattr(self._backend, "evopf_opf", None)
        if fn is None:
            raise NotImplementedError("this backend has no evopf_opf kernel: the AC-OPF solver exists as the HIP kernel "
                                      "rpo_evopf_opf only (the CPU oracle backend has none; pypower is not a dependency)")
        if self.device.type != "cuda":
            raise NotImplementedError("the AC-OPF solver is the HIP kernel rpo_evopf_opf and needs a GPU device, got %s: "
                                      "there is no CPU path" % self.device)
        return fn

    def _opf_free_kernel(self):
        """The backend's free-pe OPF kernel, or NotImplementedError with the reason there is none."""
        self._opf_kernel()
        fn = getattr(self._backend, "evopf_opf_free", None)
        if fn is None:
            raise NotImplementedError("this backend has no evopf_opf_free kernel: the free-pe AC-OPF solver exists as the HIP "
                                      "kernel rpo_evopf_opf_free only")
        return fn

    def _nearest_kernel(self):
        """The backend's nearest-feasible kernel (the safety filter), or NotImplementedError with the reason there is none."""
        self._opf_kernel()
        fn = getattr(self._backend, "evopf_nearest", None)
        if fn is None:
            raise NotImplementedError("this backend has no evopf_nearest kernel: the safety filter exists as the HIP kernel "
                                      "rpo_evopf_nearest only")
        return fn

    # ------------------------------------------------------------------------------------------ scenarios
    def scenarios(self, n, seed=0, env_id_base=0, episode=0):
        """The ``Scenarios`` (scenarios.py) that lanes ``env_id_base .. env_id_base + n - 1`` are dealt under ``seed`` in episode
        ``episode``: the Philox days, written by the device function the reset and step kernels draw with
        (rpo_evopf_scenario_table), so playing them back gives those kernels' bits.  There is no CPU path."""
        fn = getattr(self._backend, "evopf_scenario_table", None)
        if fn is None:
            raise NotImplementedError("this backend has no evopf_scenario_table kernel: the days the Philox streams deal are "
                                      "written by the HIP kernel rpo_evopf_scenario_table only (the CPU oracle backend has none)")
        if self.device.type != "cuda":
            raise NotImplementedError("the scenario table is written by the HIP kernel rpo_evopf_scenario_table and needs a GPU "
                                      "device, got %s: there is no CPU path" % self.device)
        for name, x in (("n", n), ("env_id_base", env_id_base), ("episode", episode)):
            if isinstance(x, bool) or int(x) != x or x < (1 if name == "n" else 0):
                raise ValueError("scenarios: %s must be an integer >= %d, got %r" % (name, 1 if name == "n" else 0, x))
        from .scenarios import Scenarios
        table = torch.empty(int(n), hip_ops.CONST["RPO_EVOPF_SCEN_DAY"], device=self.device)
        ep = torch.full((int(n),), int(episode), dtype=torch.int32, device=self.device) if episode else None
        fn(self.kernels, table, ep, int(seed), int(env_id_base))
        return Scenarios.from_table(table.cpu().numpy())

    def default_pe_cost(self, state):
        """The price of a unit of battery power in units of ``obj_fn`` under the env's reward, per row of observations [n, 57]
        -> [n, 5]: (we / wg) * the row's current price in every component (what rpo_evopf_opf_free uses for a NULL pe_cost)."""
        price = state[:, 2 * self.nbus + self.ne:2 * self.nbus + self.ne + 1]
        return ((self.we / self.wg) * price).expand(-1, self.ne).contiguous()

    def reward_fn(self, state, action):
        """The env step's reward formula (evopf.py:348-366) for rows of observations [n, 57] and actions [n, 43] -> [n]:
        wg * (-obj_fn(action)) - we * price * sum(pe), price the row's current price.  Torch tensors in, a tensor out; arrays in,
        a float64 array out."""
        col = 2 * self.nbus + self.ne
        if isinstance(state, torch.Tensor) or isinstance(action, torch.Tensor):
            state, action = self._t(state), self._t(action)
            state = state.view(1, -1) if state.dim() == 1 else state
            action = action.view(1, -1) if action.dim() == 1 else action
            return self.wg * (-self.obj_fn(action)) - self.we * state[:, col] * action[:, -self.ne:].sum(dim=1)
        state, action = np.atleast_2d(np.asarray(state, dtype=np.float64)), np.atleast_2d(np.asarray(action, dtype=np.float64))
        pg_mw = action[:, :self.ng] * self.genbase
        cost = ((case14.GENCOST[:, 4] * pg_mw ** 2).sum(axis=1) + (case14.GENCOST[:, 5] * pg_mw).sum(axis=1)
                + float(case14.GENCOST[:, 6].sum())) / float(self.genbase.mean() ** 2)
        return self.wg * (-cost) - self.we * state[:, col] * action[:, -self.ne:].sum(axis=1)

    def _opf_free(self, fn, state, pe_cost, tol, iters, out):
        """``opf(pe="free")`` behind the checks the two forms share."""
        if state.shape[1] != self.state_dim:
            raise ValueError("opf: pe='free' needs [n, %d] observations -- demands alone carry neither the state of charge (the "
                             "battery box) nor the price (the default pe_cost), got %s" % (self.state_dim, tuple(state.shape)))
        n = state.shape[0]
        if pe_cost is not None:
            pe_cost = self._t(pe_cost)
            if pe_cost.dim() == 0 or (pe_cost.dim() == 1 and pe_cost.shape[0] == self.ne):
                pe_cost = pe_cost.expand(n, self.ne)
            if tuple(pe_cost.shape) != (n, self.ne):
                raise ValueError("opf: pe_cost must be None, a number, [%d] or [%d, %d], got %s"
                                 % (self.ne, n, self.ne, tuple(pe_cost.shape)))
            pe_cost = pe_cost.to(torch.float32).contiguous()
        fn(self.kernels, state, pe_cost, out.action, out.info, tol, iters)
        out.pe_cost = self.default_pe_cost(state) if pe_cost is None else pe_cost
        return out

    def opf(self, state, pe=None, tol=1e-4, max_iters=40, out=None, state_in=None, state_out=None, pe_cost=None):
        """The cheapest dispatch of every row's single-step AC-OPF, on the device (rpo_evopf_opf, csrc/evopf_opf.hip).

        ``state`` [n, 57] observations or [n, 28] demands (pd, qd); ``pe`` [n, 5] battery power, a PARAMETER of the problem
        (None: zero, the reference's ``opt_solve``; a policy's own pe for optimality gaps).  Minimises ``obj_fn`` over (pg, qg,
        vm, va) subject to ``eq_resid = 0`` and the bounds on pg, qg, vm by a primal-dual interior point method from the flat
        start; stops when the primal infeasibility, |L_x|_inf and z^T mu are all below ``tol``, or after ``max_iters``
        iterations (``converged`` False: infeasible single-step problems exist, and end this way).  Returns an ``OpfResult`` of
        device tensors; nothing synchronises with the host.  ``out``: an earlier result of the same n, whose buffers are
        reused.  ``state_in`` / ``state_out``: contiguous float32 device tensors [n, 168] (action[43] | lambda[28] | z_u[24] |
        z_l[24] | mu_u[24] | mu_l[24] | gamma, bounded variables in the order pg, qg, vm) -- the interior-point state to start
        from in place of the flat start (it carries pe: ``pe`` must then be None; ``iters`` counts from it) and the state at
        exit, written in place.

        ``pe="free"``: the battery power is a variable too (rpo_evopf_opf_free) -- minimise ``obj_fn + sum_j pe_cost[j] pe[j]`` over
        (pg, qg, vm, va, pe) with the 10 battery bounds ``battery_bounds(soc)`` of the row's observation added (58 inequalities).
        ``state`` must then be [n, 57] observations; ``pe_cost`` None ((we / wg) * the row's current price: the optimum maximises
        the env's one-step reward), a number, [5] or [n, 5]; ``state_in`` / ``state_out`` are refused.  The result's ``action``
        carries the optimal pe, ``cost`` stays ``obj_fn`` of the point, ``pe_cost`` / ``objective`` what was minimised."""
        free = isinstance(pe, str)
        if free and pe != "free":
            raise ValueError("opf: pe must be None, [n, %d] or the string 'free', got %r" % (self.ne, pe))
        if free and (state_in is not None or state_out is not None):
            raise ValueError("opf: pe='free' has no state seam: state_in / state_out must be None")
        if pe_cost is not None and not free:
            raise ValueError("opf: pe_cost is the linear cost of the free battery power: pass pe='free' with it")
        fn = self._opf_free_kernel() if free else self._opf_kernel()
        tol, iters = float(tol), int(max_iters)
        if not tol > 0.0 or iters != max_iters or iters < 0:
            raise ValueError("opf: tol must be > 0 and max_iters an integer >= 0, got %r and %r" % (tol, max_iters))
        state = self._t(state)
        if state.dim() == 1:
            state = state.view(1, -1)
        if state.dim() != 2 or state.shape[0] < 1 or state.shape[1] not in (self.state_dim, 2 * self.nbus):
            raise ValueError("opf: state must be [n, %d] observations or [n, %d] demands, got %s"
                             % (self.state_dim, 2 * self.nbus, tuple(state.shape)))
        if state.stride(1) != 1:
            state = state.contiguous()
        n = state.shape[0]
        if pe is not None and not free:
            pe = self._t(pe)
            pe = (pe.view(1, -1) if pe.dim() == 1 else pe).contiguous()
            if tuple(pe.shape) != (n, self.ne):
                raise ValueError("opf: pe must be [%d, %d], got %s" % (n, self.ne, tuple(pe.shape)))
        if out is None:
            out = OpfResult(torch.empty(n, self._ydim, device=state.device), torch.empty(n, 4, device=state.device))
        elif not isinstance(out, OpfResult) or tuple(out.action.shape) != (n, self._ydim) or tuple(out.info.shape) != (n, 4) \
                or out.action.device != state.device or out.info.device != state.device \
                or not (out.action.is_contiguous() and out.info.is_contiguous()) \
                or out.action.dtype != torch.float32 or out.info.dtype != torch.float32:
            raise ValueError("opf: out must be an OpfResult of %d rows on %s" % (n, state.device))
        for name, st in (("state_in", state_in), ("state_out", state_out)):
            if st is not None and (not isinstance(st, torch.Tensor) or tuple(st.shape) != (n, 168) or st.dtype != torch.float32
                                   or st.device != state.device or not st.is_contiguous()):
                raise ValueError("opf: %s must be a contiguous float32 tensor [%d, 168] on %s" % (name, n, state.device))
        if state_in is not None and pe is not None:
            raise ValueError("opf: state_in carries pe (columns 38..42): pe must be None with it")
        if free:
            return self._opf_free(fn, state, pe_cost, tol, iters, out)
        out.pe_cost = None
        if state_in is None and state_out is None:
            fn(self.kernels, state, pe, out.action, out.info, tol, iters)
        else:
            fn(self.kernels, state, pe, out.action, out.info, tol, iters, state_in=state_in, state_out=state_out)
        return out

    def opt_solve(self, X, solver_type="hip", tol=1e-4):
        """The reference's ``opt_solve`` (evopf.py:729-759) on the device: demands X [n, 28] -> (Y [n, 38] numpy = (pg, qg, vm,
        va) of the optimal dispatch with pe = 0, total time, time per state) in seconds of wall clock, kernel and copy-back.
        Rows whose problem did not converge (``opf``) are NaN.  ``solver_type``: "hip"; the reference's "pypower" is refused."""
        if solver_type != "hip":
            raise NotImplementedError("opt_solve(solver_type=%r): pypower is not a dependency of this build; the solver is "
                                      "the HIP kernel behind solver_type='hip' (EVOPFEnv.opf)" % (solver_type,))
        self._opf_kernel()
        import time
        X = X.detach() if isinstance(X, torch.Tensor) else np.asarray(X, dtype=np.float32)
        if X.ndim != 2 or X.shape[1] != 2 * self.nbus:
            raise ValueError("opt_solve: X must be [n, %d] demands, got %s" % (2 * self.nbus, tuple(X.shape)))
        start = time.perf_counter()
        res = self.opf(X, tol=tol).numpy()
        total = time.perf_counter() - start
        Y = res["action"][:, :self.pe_start_yidx].astype(np.float64)
        Y[~res["converged"]] = np.nan
        return Y, total, total / X.shape[0]

    # ------------------------------------------------------------------------------------------ safety filter
    def _check_weight(self, weight, n, what):
        """``weight`` of the safety filter -> None or a contiguous float32 device tensor [14] / [n, 14].  Values given on the
        host are checked here (finite and > 0: ValueError); a device tensor's are not read -- the kernel ends a row whose
        weights are not finite numbers > 0 as not converged."""
        if weight is None:
            return None
        P = len(self._partial_actions)
        on_device = isinstance(weight, torch.Tensor) and weight.device.type != "cpu"
        if not on_device:
            host = np.asarray(weight.detach().numpy() if isinstance(weight, torch.Tensor) else weight, dtype=np.float64)
            if not (np.all(np.isfinite(host)) and np.all(host > 0)):
                raise ValueError("%s: weight must hold finite numbers > 0" % what)
        weight = self._t(weight).to(torch.float32)
        if tuple(weight.shape) not in ((P,), (n, P)):
            raise ValueError("%s: weight must be None, [%d] or [%d, %d], got %s" % (what, P, n, P, tuple(weight.shape)))
        return weight.contiguous()

    def nearest_feasible(self, obs, action, weight=None, tol=1e-4, max_iters=40, out=None):
        """The safety filter: for every row the dispatch nearest to ``action`` that meets the power-flow equations and all 58
        bounds, on the device (rpo_evopf_nearest, a third instance of the interior-point kernel of ``opf``).

        ``obs`` [n, 57] observations; ``action`` [n, 43] actions, [n, 14] in ``partial_actions`` order, or an ``ActResult`` (its
        ``action``).  Minimises ``0.5 * sum_k w_k (y_k - t_k)^2`` over the 14 components the actor controls (pg at the four
        non-slack generators, vm at the five generator buses, pe) subject to ``eq_resid = 0`` and the bounds of ``ineq_resid``;
        the equations fix every other component.  ``weight`` None: ``w_k = 1 / s_k^2`` with s_k the half-width of the variable's
        box (per row for pe: ``battery_bounds``), the distance in box units that ``pretrain`` uses; else [14] or [n, 14], finite
        and > 0.  Same method, flat start (not the target), ``tol`` and ``max_iters`` as ``opf``; an infeasible single-step problem
        ends with ``converged`` False.  Returns a ``NearestResult`` of device tensors; nothing synchronises with the host.
        ``out``: an earlier result of the same n, whose buffers are reused."""
        fn = self._nearest_kernel()
        tol, iters = float(tol), int(max_iters)
        if not tol > 0.0 or iters != max_iters or iters < 0:
            raise ValueError("nearest_feasible: tol must be > 0 and max_iters an integer >= 0, got %r and %r" % (tol, max_iters))
        obs = self._t(obs)
        if obs.dim() == 1:
            obs = obs.view(1, -1)
        if obs.dim() != 2 or obs.shape[0] < 1 or obs.shape[1] != self.state_dim:
            raise ValueError("nearest_feasible: obs must be [n, %d] observations, got %s" % (self.state_dim, tuple(obs.shape)))
        if obs.stride(1) != 1:
            obs = obs.contiguous()
        n, P = obs.shape[0], len(self._partial_actions)
        if not isinstance(action, (torch.Tensor, np.ndarray, list, tuple)) and hasattr(action, "action"):
            action = action.action                              # an ActResult
        action = self._t(action)
        if action.dim() == 1:
            action = action.view(1, -1)
        if action.dim() != 2 or action.shape[0] != n or action.shape[1] not in (self._ydim, P):
            raise ValueError("nearest_feasible: action must be [%d, %d], [%d, %d] (partial_actions order) or an ActResult of %d "
                             "rows, got %s" % (n, self._ydim, n, P, n, tuple(action.shape)))
        weight = self._check_weight(weight, n, "nearest_feasible")
        if out is None:
            out = NearestResult(torch.empty(n, self._ydim, device=obs.device), torch.empty(n, 4, device=obs.device),
                                torch.empty(n, P, device=obs.device), torch.empty(n, P, device=obs.device))
        elif not isinstance(out, NearestResult) or tuple(out.action.shape) != (n, self._ydim) or tuple(out.info.shape) != (n, 4) \
                or any(tuple(t.shape) != (n, P) for t in (out.target, out.moved)) \
                or any(t.device != obs.device or t.dtype != torch.float32 or not t.is_contiguous()
                       for t in (out.action, out.info, out.target, out.moved)):
            raise ValueError("nearest_feasible: out must be a NearestResult of %d rows on %s" % (n, obs.device))
        idx = self._partial_index(obs.device)
        action = action.to(torch.float32)
        if action.shape[1] == P:
            out.target.copy_(action)
            full = torch.zeros(n, self._ydim, device=obs.device)
            full.index_copy_(1, idx, out.target)
        else:
            full = action if action.stride(1) == 1 else action.contiguous()
            torch.index_select(full, 1, idx, out=out.target)
        fn(self.kernels, obs, full, weight, out.action, out.info, tol, iters)
        lo, hi = self.update(obs)                                # the box of the 14 controlled components, per row
        torch.div((out.action.index_select(1, idx) - out.target).abs_(), 0.5 * (hi - lo), out=out.moved)
        return out

    def _partial_index(self, device):
        key = ("partial_index", device)
        if key not in self._box_cache:
            self._box_cache[key] = torch.as_tensor(np.asarray(self._partial_actions), dtype=torch.int64, device=device)
        return self._box_cache[key]


class OpfResult(object):
    """What ``EVOPFEnv.opf`` returns: device tensors, row i for state i.  ``action`` [n, 43]: the full action vector (va at the
    slack bus = slack_va, pe as given), so ``eq_resid`` / ``ineq_resid`` / ``obj_fn`` apply to it; ``cost`` [n] = its ``obj_fn``;
    ``residual`` [n]: the largest of the three stop quantities at exit (NaN if one of them was); ``iters`` [n] int32;
    ``converged`` [n] bool.  The last four are views of / elementwise ops on ``info`` [n, 4], the kernel's own output.
    ``pe_cost``: the [n, 5] linear cost of pe that ``opf(pe="free")`` minimised with, None for a fixed-pe result; ``objective`` [n]
    = ``cost + (pe_cost * pe).sum(1)``, what was minimised (``cost`` itself when ``pe_cost`` is None)."""

    def __init__(self, action, info, pe_cost=None):
        self.action, self.info, self.pe_cost = action, info, pe_cost

    cost = property(lambda self: self.info[:, 0])
    residual = property(lambda self: self.info[:, 1])
    iters = property(lambda self: self.info[:, 2].to(torch.int32))
    converged = property(lambda self: self.info[:, 3] > 0.5)

    @property
    def objective(self):
        if self.pe_cost is None:
            return self.cost
        return self.cost + (self.pe_cost * self.action[:, -self.pe_cost.shape[1]:]).sum(dim=1)

    def numpy(self):
        """dict of numpy arrays (one device-to-host copy per buffer; this synchronises); a free-pe result adds ``pe_cost`` and
        ``objective``."""
        info = self.info.detach().cpu().numpy()
        host = dict(action=self.action.detach().cpu().numpy(), cost=info[:, 0].copy(), residual=info[:, 1].copy(),
                    iters=info[:, 2].astype(np.int32), converged=info[:, 3] > 0.5)
        if self.pe_cost is not None:                             # a free-pe result carries what it minimised as well
            host.update(pe_cost=self.pe_cost.detach().cpu().numpy(), objective=self.objective.detach().cpu().numpy())
        return host

    def converged_rate(self):
        return float((self.info[:, 3] > 0.5).float().mean())

    def __repr__(self):
        return "OpfResult(n=%d)" % self.action.shape[0]


class NearestResult(object):
    """What ``EVOPFEnv.nearest_feasible`` returns: device tensors, row i for observation i.  ``action`` [n, 43]: the feasible
    dispatch nearest to the target (the solver's last iterate where ``converged`` is False); ``target`` [n, 14]: what was asked
    for, in ``partial_actions`` order; ``moved`` [n, 14] = |action - target| / half-width of the variable's box, in box units;
    ``distance`` [n] = ``0.5 * sum w (y - t)^2``, what was minimised; ``residual`` [n]: the largest of the three stop quantities
    at exit (NaN if one of them was); ``iters`` [n] int32; ``converged`` [n] bool.  The last four are views of / elementwise ops
    on ``info`` [n, 4], the kernel's own output."""

    def __init__(self, action, info, target, moved):
        self.action, self.info, self.target, self.moved = action, info, target, moved

    distance = property(lambda self: self.info[:, 0])
    residual = property(lambda self: self.info[:, 1])
    iters = property(lambda self: self.info[:, 2].to(torch.int32))
    converged = property(lambda self: self.info[:, 3] > 0.5)

    def numpy(self):
        """dict of numpy arrays (one device-to-host copy per buffer; this synchronises)."""
        info = self.info.detach().cpu().numpy()
        return dict(action=self.action.detach().cpu().numpy(), distance=info[:, 0].copy(), residual=info[:, 1].copy(),
                    iters=info[:, 2].astype(np.int32), converged=info[:, 3] > 0.5, target=self.target.detach().cpu().numpy(),
                    moved=self.moved.detach().cpu().numpy())

    def converged_rate(self):
        return float((self.info[:, 3] > 0.5).float().mean())

    def __repr__(self):
        return "NearestResult(n=%d)" % self.action.shape[0]
