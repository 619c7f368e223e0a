"""Scenarios of EVOPF-v0: the caller's days in the place of the Philox-drawn ones.

A day is what the loaders of the reference deal per episode (data/demand.py, data/price.py): the per-unit active / reactive
demand of the 14 buses for each of the 24 hours, and the price of 48 hours in the observation's units -- the day's own 24 and the
look-ahead past midnight, which the observation's 24-hour price window reads from hour 1 on.  ``Scenarios`` holds D such days on
the host; ``table()`` lays them out as the step kernel reads them (include/rpo_hip.h, RPO_EVOPF_SCEN_DAY) and
``trainer.evaluate(scenarios=S)`` / ``rpo_amd.algo.evaluate_opf(trainer, scenarios=S)`` play them: episode e plays day e % len(S).
``RPODDPG(..., scenarios=S, deal=)`` / ``RPOSAC`` TRAIN on them: S is a bank, and every episode of a training lane is dealt one of
its days (rpo_evopf_step_bank); ``split`` parts a bank into the days to train on and the days to hold out.

Where days come from: ``Scenarios(demand, price)`` (any source), ``Scenarios.from_system_days(env, load, price)`` (system-level
load curves and prices, split over the buses the way the reference's ``DemandLoader.process`` does -- the reference's
``regularized=False`` branch, which cannot execute there), ``env.scenarios(n, seed)`` (the days the Philox streams deal, written
by the device function the step kernel draws with).
"""
import numpy as np
import torch

from ... import ops as hip_ops
from . import case14

T, NAHEAD, NBUS = case14.T, case14.NAHEAD, case14.BUS.shape[0]
HOUR = 2 * NBUS                      # floats of an hour's demand: pd[14], qd[14]
DAY = hip_ops.CONST["RPO_EVOPF_SCEN_DAY"]
MIN_PF, MAX_PF = 0.9, 1.0            # DemandLoader(min_pf=0.9, max_pf=1.0), demand.py:9 (kMinPf / kMaxPf of evopf_dev.h)

assert DAY == T + NAHEAD + T * HOUR


def _real_array(x, what, dtype=np.float32):
    """``x`` as a float32 (``dtype``) array; TypeError for what holds no real numbers, ValueError for a non-finite entry (also one that
    float32 cannot hold)."""
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    a = np.asarray(x)
    if a.dtype == np.bool_ or a.dtype.kind not in "fiu":
        raise TypeError("Scenarios: %s must hold real numbers, got dtype %s" % (what, a.dtype))
    with np.errstate(over="ignore"):
        a = a.astype(dtype)                                      # (a copy: the source stays the caller's)
    if not np.all(np.isfinite(a)):
        raise ValueError("Scenarios: %s must be finite (in %s)" % (what, np.dtype(dtype).name))
    return a


def _factor(f, days, hours, what):
    """A scale factor -> float32 broadcastable to [days, hours * k]: a number, [days] (per day) or [24] (per hour of the day)."""
    f = _real_array(f, what)
    if f.ndim == 0:
        return f.reshape(1, 1)
    if f.ndim == 1 and days == T and f.shape[0] == T:
        raise ValueError("Scenarios: %s of length 24 is ambiguous with 24 days; pass [24, 1] (per day) or [1, 24] (per hour)" % what)
    if f.ndim == 1 and f.shape[0] == days:
        return f.reshape(days, 1)
    if f.ndim == 1 and f.shape[0] == T:
        return np.tile(f, hours // T).reshape(1, hours)
    if f.shape == (days, 1):
        return f
    if f.shape == (1, T):
        return np.tile(f, (1, hours // T))
    raise ValueError("Scenarios: %s must be a number, [%d] (per day) or [%d] (per hour), got shape %s" % (what, days, T, f.shape))


class Scenarios(object):
    """D days of EVOPF-v0 on the host: ``demand`` float32 [D, 24, 28] = (pd[14], qd[14]) per hour, per unit as the observation
    carries them; ``price`` float32 [D, 48] in the observation's units, hours 24..47 the look-ahead past midnight ([D, 24] is
    padded with zeros, what the Philox days carry there).  Both are copies and read-only: every operation returns a new object."""

    def __init__(self, demand, price):
        demand, price = _real_array(demand, "demand"), _real_array(price, "price")
        if demand.ndim != 3 or demand.shape[0] < 1 or demand.shape[1:] != (T, HOUR):
            raise ValueError("Scenarios: demand must be [D >= 1, %d, %d], got %s" % (T, HOUR, demand.shape))
        D = demand.shape[0]
        if price.ndim != 2 or price.shape[0] != D or price.shape[1] not in (T, T + NAHEAD):
            raise ValueError("Scenarios: price must be [%d, %d] or [%d, %d], got %s" % (D, T + NAHEAD, D, T, price.shape))
        if price.shape[1] == T:
            price = np.concatenate([price, np.zeros((D, NAHEAD), dtype=np.float32)], axis=1)
        self.demand, self.price = np.ascontiguousarray(demand), np.ascontiguousarray(price)
        self.demand.setflags(write=False)
        self.price.setflags(write=False)
        self._dev = {}

    def __len__(self):
        return self.demand.shape[0]

    def __getitem__(self, key):
        """A day (index), or days (slice, index array) -> Scenarios."""
        if isinstance(key, (int, np.integer)):
            key = [int(key)]
        elif not isinstance(key, slice):
            key = np.asarray(key)
            if key.dtype == np.bool_ or key.dtype.kind not in "iu" or key.ndim != 1:
                raise TypeError("Scenarios: index with an integer, a slice or a 1-d integer array")
        demand = self.demand[key]
        if demand.shape[0] < 1:
            raise IndexError("Scenarios: the selection holds no day")
        return Scenarios(demand, self.price[key])

    @staticmethod
    def concat(parts):
        """The days of several Scenarios, in order."""
        parts = list(parts)
        if not parts or not all(isinstance(p, Scenarios) for p in parts):
            raise TypeError("Scenarios.concat: a non-empty sequence of Scenarios")
        return Scenarios(np.concatenate([p.demand for p in parts]), np.concatenate([p.price for p in parts]))

    def split(self, frac, seed=0):
        """A disjoint random split -> (train, test): round(frac * D) days drawn by ``numpy.random.default_rng(seed)`` go to the
        first part, the others to the second, each in the order they have here.  ValueError when a part would hold no day: train
        on the one (``RPODDPG(..., scenarios=train)``), hold the other out (``evaluate(scenarios=test)``)."""
        if isinstance(frac, bool) or not isinstance(frac, (int, float, np.integer, np.floating)) or not 0.0 < float(frac) < 1.0:
            raise ValueError("Scenarios.split: frac must be a number in (0, 1), got %r" % (frac,))
        D = len(self)
        k = int(round(float(frac) * D))
        if k < 1 or k > D - 1:
            raise ValueError("Scenarios.split: frac=%r of %d day(s) leaves a part empty (%d / %d)" % (frac, D, k, D - k))
        perm = np.random.default_rng(seed).permutation(D)
        return self[np.sort(perm[:k])], self[np.sort(perm[k:])]

    def digest(self):
        """sha1 of the float32 table bytes: what a checkpoint records of the bank a trainer was trained on."""
        import hashlib
        return hashlib.sha1(np.ascontiguousarray(self.table(), dtype=np.float32).tobytes()).hexdigest()

    def scale_demand(self, f):
        """Demand (pd and qd) times ``f``: a number, [D] per day or [24] per hour.  A new object."""
        f = _factor(f, len(self), T, "scale_demand's factor")
        return Scenarios(self.demand * f[:, :, None], self.price)

    def scale_price(self, f):
        """Price times ``f``: a number, [D] per day or [24] per hour of the day (the look-ahead's hour h + 24 takes hour h's)."""
        return Scenarios(self.demand, self.price * _factor(f, len(self), T + NAHEAD, "scale_price's factor"))

    def save(self, path):
        with open(path, "wb") as fh:                             # (a file object: numpy appends no suffix)
            np.savez(fh, demand=self.demand, price=self.price)

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            return cls(z["demand"], z["price"])

    def table(self, device=None):
        """The days in the step kernel's layout, float32 [D, 720]: floats [0, 48) of a row the price, [48 + 28 t, 48 + 28 t + 28)
        hour t's demand.  ``device`` None: a fresh numpy array; a torch device: the copy there, made once."""
        if device is None:
            return np.concatenate([self.price, self.demand.reshape(len(self), T * HOUR)], axis=1)
        device = torch.device(device)
        if device not in self._dev:
            self._dev[device] = torch.from_numpy(self.table()).to(device)
        return self._dev[device]

    @classmethod
    def from_table(cls, table):
        """The inverse of ``table()``: float32 [D, 720] -> Scenarios."""
        table = _real_array(table, "table")
        if table.ndim != 2 or table.shape[1] != DAY:
            raise ValueError("Scenarios: a table is [D, %d], got %s" % (DAY, table.shape))
        return cls(table[:, T + NAHEAD:].reshape(-1, T, HOUR), table[:, :T + NAHEAD])

    @classmethod
    def from_system_days(cls, env, load, price, seed=0):
        """Days from system-level data: ``load`` [D, 24], a system load curve per day in any unit (>= 0, not all zero);
        ``price`` [D, 24 | 48] in the unit of the price data.  The reference's ``DemandLoader.process`` (demand.py:47-67) on the
        host: the curve normalised to the case's daily energy, split over the load buses by (1 - rho) * nominal share + rho *
        Dirichlet(1), power factors uniform in [min_pf, max_pf] with the sign of the case's Qd, all divided by baseMVA; the
        price divided by baseMVA, the base of the observation's price.  The draws come from ``numpy.random.default_rng(seed)``:
        host randomness, not tied to the Philox streams."""
        load = _real_array(load, "load", np.float64)
        if load.ndim != 2 or load.shape[0] < 1 or load.shape[1] != T:
            raise ValueError("Scenarios.from_system_days: load must be [D >= 1, %d], got %s" % (T, load.shape))
        if np.any(load < 0) or np.any(load.sum(axis=1) <= 0):
            raise ValueError("Scenarios.from_system_days: a load curve must be >= 0 with a positive sum")
        D = load.shape[0]
        rng = np.random.default_rng(seed)
        bus_pd, bus_qd = case14.BUS[:, case14.PD], case14.BUS[:, case14.QD]
        idx = np.nonzero(bus_pd)[0]
        ps = load / load.sum(axis=1, keepdims=True) * (bus_pd.sum() * T)                 # demand.py:51-52
        ratio = np.broadcast_to(bus_pd / bus_pd.sum() * (1.0 - case14.RHO), (D, T, NBUS)).copy()
        ratio[:, :, idx] += case14.RHO * rng.dirichlet(np.ones(len(idx)), size=(D, T))     # :54-58
        pd = ratio * ps[:, :, None]
        pf = rng.random((D, T, NBUS)) * (MAX_PF - MIN_PF) + MIN_PF                        # :63
        qd = pd * np.tan(np.arccos(pf)) * np.sign(bus_qd)                                 # :64
        demand = np.concatenate([pd, qd], axis=2) / env.baseMVA                           # :43
        return cls(demand, _real_array(price, "price", np.float64) / env.baseMVA)

    def __repr__(self):
        return "Scenarios(days=%d)" % len(self)
