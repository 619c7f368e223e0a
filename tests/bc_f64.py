"""Float64 restatement of the behaviour-cloning head (include/rpo_hip.h: rpo_bc_head, rpo_evopf_bc_head; csrc/bc.hip), its edge
inputs and the yardstick that turns "close to float64" into a number.  Not collected; used by test_pretrain.py (CPU) and
test_pretrain_gpu.py.

For a batch row i and a basic action component j < P, with (lo, hi) the actor's box of that row and component:

    scale = (hi - lo) / 2,  base = lo + scale
    u  = clamp((a* - base) / scale, -clip, +clip)
    y  = tanh(raw)
    L  = 1 / (B P) sum_ij w_j (y - u)^2
    dL / draw_ij = 2 w_j / (B P) (y - u) (1 - y^2)

and a term whose scale <= 1e-6 contributes 0 to both (the denominator stays B P).  heads = 2 (RPOSAC): raw is [B, 2 P], the
mean half is read and the log-std half receives gradient exactly 0.  ``bc_loss`` is written from these lines in torch, the
gradient by autograd; ``bc_grad_formula`` is the hand-written last line (test_pretrain.py holds the two together).

Magnitude sums, by the method of tests/heads_f64.py (every term with its absolute value, every intermediate with its own sum
times the derivative of what follows), in units of eps32:
    num = a* - base:      nm  = |a*| + base_mag + |num|
    q = num / scale:      qm  = nm / |scale| + |num| scale_mag / scale^2 + |q|        (the clamp is 1-Lipschitz: u keeps qm)
    y:                    ym  = (1 - y^2) |raw| + |y|
    d = y - u:            dm  = ym + qm + |d|
    1 - y^2:              omm = 2 |y| ym + 1 + y^2
    term = w d^2:         tm  = w (2 |d| dm + 2 d^2)
    grad = c d (1 - y^2): gm  = |c| (dm om + |d| omm + 4 |d| om),   c = 2 w / (B P), om = 1 - y^2 without the cancellation
    a sum of K terms / (B P): (sum tm + (depth) sum |term|) / (B P) + 2 |sum|,  depth = the additions a term passes through
scale_mag / base_mag are the box's own sums: |scale| and |scale| + |base| for a box handed over as float32 numbers
(``const_box``), heads_f64.evopf_box's for the box the kernel computes from the state of charge.  A float32 evaluation of the
formula is expected within a small multiple c of eps32 * magnitude sum everywhere; c is measured, per output, as ``C_REF_*``.
"""
import numpy as np
import torch

import heads_f64 as hf
import mlp_f64
from oracle import evopf as oe

EPS32, TINY, MARGIN = hf.EPS32, hf.TINY, hf.MARGIN
MIN_SCALE = 1e-6                                     # boxes with scale <= this are empty
GROUP = 16                                           # rows per loss partial

# The yardstick: max over the edge rows and 257 random rows, heads 1 and 2, weights None and with a zero, every box below, of
# |float32 - float64| / (EPS32 * magnitude sum), the float32 side being THIS file's functions run by torch on the CPU in float32
# (never a kernel).  Measured by tests/test_pretrain.py::test_yardstick, which recomputes them and fails on a drift beyond 2x.
C_REF_BC_LOSS = 0.04     # measured 0.0382: a loss partial (16 rows) and the whole loss (small: the bound counts every addition a
#                          term passes through, 4 + 16 and one per partial, at its worst)
C_REF_BC_GRAD = 0.15     # measured 0.1414: d L / d raw per element
# The chain actor forward -> head -> actor backward against float64 autograd through float64 copies of the weights (one step's
# parameter gradients, test_pretrain_gpu.py::test_gradient_against_float64): worst |float32 CPU torch autograd - float64| /
# (EPS32 * ``chain_mags``) over the parameter tensors of the evopf256 RPODDPG / RPOSAC and cart RPODDPG actors at their initial
# weights, a batch of 16 ``random_rows``.  Far below 1 because chain_mags composes worst-case chains of a few hundred roundings;
# measured by tests/test_pretrain.py::test_chain_yardstick.
C_REF_BC_CHAIN = 0.0035  # measured 0.0031 (evopf256 RPODDPG; cart 0.0020, evopf256 RPOSAC 0.0005)


# ================================================================================================== boxes
def const_box(lo, hi, n):
    """A constant box given as P float32 numbers: float64 (lo, hi, scale, base, scale_mag, base_mag), each [n, P]."""
    lo = torch.tensor(np.asarray(lo, dtype=np.float32).astype(np.float64)).reshape(1, -1).expand(n, -1)
    hi = torch.tensor(np.asarray(hi, dtype=np.float32).astype(np.float64)).reshape(1, -1).expand(n, -1)
    scale = (hi - lo) * 0.5
    scale_mag = scale.abs()
    return lo, hi, scale, lo + scale, scale_mag, scale_mag + (lo + scale).abs()


def evopf_box(state):
    """The state-dependent box of the 14 basic actions from oracle/evopf.py, as tests/heads_f64.py takes it."""
    return hf.evopf_box(state)


def evopf_box32(state):
    """The same box evaluated in float32, as the kernel's basic_box does: table entries rounded once, the battery limits
    min(0.2, 0.8 - soc) / 0.9 and 0.9 max(-0.2, 0.1 - soc) in float32 -> float32 (lo, hi) [n, 14]."""
    f = np.float32
    s = np.asarray(state, dtype=np.float32)
    g = oe.GRID
    lo = np.tile(g.action_low[g.partial_actions].astype(f), (s.shape[0], 1))
    hi = np.tile(g.action_high[g.partial_actions].astype(f), (s.shape[0], 1))
    soc = s[:, -g.ne - oe.NAHEAD:-oe.NAHEAD]
    hi[:, -g.ne:] = np.minimum(f(oe.B_PMAX), f(oe.B_HIGH) - soc) / f(oe.ETA_IN)
    lo[:, -g.ne:] = f(oe.ETA_OUT) * np.maximum(f(oe.B_PMIN), f(oe.B_LOW) - soc)
    return torch.from_numpy(lo), torch.from_numpy(hi)


# ================================================================================================== the loss
def _w(weights, P, dtype):
    return torch.ones(P, dtype=dtype) if weights is None else torch.as_tensor(np.asarray(weights, dtype=np.float32)).to(dtype)


def bc_loss(raw, target, lo, hi, weights=None, clip=0.98, heads=1, dtype=torch.float64, grad=True):
    """The loss of the module docstring for raw [n, heads * P], target / lo / hi [n, P] -> dict(loss, terms [n, P] (already
    divided by n P), parts [(n + 15) // 16], draw [n, heads * P] by autograd, live [n, P])."""
    raw = torch.as_tensor(raw).to(dtype).clone().requires_grad_(grad)
    target, lo, hi = (torch.as_tensor(v).to(dtype) for v in (target, lo, hi))
    n, P = target.shape
    w = _w(weights, P, dtype)
    scale = (hi - lo) * 0.5
    base = lo + scale
    live = scale > MIN_SCALE
    safe = torch.where(live, scale, torch.ones_like(scale))
    c = float(np.float32(clip))
    u = torch.clamp((target - base) / safe, min=-c, max=c)
    y = torch.tanh(raw[:, :P])
    terms = torch.where(live, w * (y - u) ** 2, torch.zeros_like(y)) / (n * P)
    # a row's terms, then the 16 rows of a group one after the other, then the partials one after the other (cumsum adds in
    # index order): the association the entry point's contract describes, so that the float32 evaluation rounds like it
    pad = torch.zeros((-n) % GROUP, P, dtype=dtype)
    rows = torch.cat([terms, pad]).sum(dim=1).view(-1, GROUP)
    parts = torch.cumsum(rows, dim=1)[:, -1]
    loss = torch.cumsum(parts, dim=0)[-1]
    out = dict(loss=loss.detach(), terms=terms.detach(), live=live, parts=parts.detach())
    if grad:
        out["draw"], = torch.autograd.grad(loss, (raw,))
    return out


def bc_grad_formula(raw, target, lo, hi, weights=None, clip=0.98, heads=1, dtype=torch.float64):
    """d L / d raw written out: 2 w / (B P) (y - u) (1 - y^2), 0 where the box is empty and in the log-std half."""
    raw = torch.as_tensor(raw).to(dtype)
    target, lo, hi = (torch.as_tensor(v).to(dtype) for v in (target, lo, hi))
    n, P = target.shape
    w = _w(weights, P, dtype)
    scale = (hi - lo) * 0.5
    base = lo + scale
    live = scale > MIN_SCALE
    safe = torch.where(live, scale, torch.ones_like(scale))
    c = float(np.float32(clip))
    u = torch.clamp((target - base) / safe, min=-c, max=c)
    y = torch.tanh(raw[:, :P])
    g = torch.where(live, 2.0 * w / (n * P) * (y - u) * (1.0 - y * y), torch.zeros_like(y))
    return torch.cat([g, torch.zeros(n, (heads - 1) * P, dtype=dtype)], dim=1)


def bc_mags(raw, target, box, weights=None, clip=0.98):
    """The magnitude sums of bc_loss's outputs (module docstring), float64: dict(draw [n, P], parts [G], loss).  ``box``: the six
    tensors of ``const_box`` / ``evopf_box``."""
    d = torch.float64
    lo, hi, scale, base, scale_mag, base_mag = (torch.as_tensor(v).to(d) for v in box)
    raw, target = torch.as_tensor(raw).to(d), torch.as_tensor(target).to(d)
    n, P = target.shape
    raw = raw[:, :P]
    w = _w(weights, P, d)
    live = scale > MIN_SCALE
    safe = torch.where(live, scale, torch.ones_like(scale))
    c = float(np.float32(clip))
    num = target - base
    q = num / safe
    nm = target.abs() + base_mag + num.abs()
    qm = nm / safe.abs() + num.abs() * scale_mag / safe ** 2 + q.abs()
    u = q.clamp(-c, c)
    y = torch.tanh(raw)
    om = 4.0 / (torch.exp(raw) + torch.exp(-raw)) ** 2
    ym = om * raw.abs() + y.abs()
    dd = y - u
    dm = ym + qm + dd.abs()
    omm = 2 * y.abs() * ym + 1 + y * y
    inv = 1.0 / (n * P)
    z = torch.zeros_like(y)
    term = torch.where(live, w * dd * dd, z)
    tm = torch.where(live, w * (2 * dd.abs() * dm + 2 * dd * dd), z)
    gm = torch.where(live, 2 * w * inv * (dm * om + dd.abs() * omm + 4 * dd.abs() * om), z)
    pad = torch.zeros((-n) % GROUP, P, dtype=d)
    grp = lambda t: torch.cat([t, pad]).view(-1, GROUP * P).sum(dim=1)           # noqa: E731
    depth = 4 + GROUP                                          # the butterfly over a row's 16 lanes, then the 16 rows in turn
    parts = inv * (grp(tm) + depth * grp(term)) + 2 * inv * grp(term)
    G = parts.numel()
    loss = inv * (tm.sum() + (depth + G) * term.sum()) + 2 * inv * term.sum()
    return dict(draw=gm, parts=parts, loss=loss)


def worst(got, ref, mag):
    return hf.worst(got, ref, mag)


# ================================================================================================== inputs
RAWS = (0.0, 1e-4, -1e-4, 3.0, -3.0, 9.0, -9.0, 20.0, -20.0)                   # tanhf is exactly 1 from about 9.01 on
KINDS = ("lo", "hi", "below", "above", "seam+", "seam-", "inside")
SOCS = (0.1, 0.8, oe.B_INIT, 1.0, -0.3)              # the last two are out of band: hi < lo, the battery box is empty
CLIP = 0.98


def _targets(kind, lo, hi, clip, rng):
    """float32 targets [n, P] of one kind for float64 boxes lo / hi [n, P] (an empty box takes whatever comes out)."""
    scale = (hi - lo) * 0.5
    base = lo + scale
    c = float(np.float32(clip))
    t = {"lo": lo, "hi": hi, "below": lo - 0.3 * np.abs(scale) - 0.01, "above": hi + 0.3 * np.abs(scale) + 0.01,
         "seam+": base + c * scale, "seam-": base - c * scale,
         "inside": base + scale * rng.uniform(-0.9, 0.9, size=lo.shape)}[kind]
    return t.astype(np.float32)


def states(socs, seed=0):
    """EVOPF-v0 observations [n, 57] whose five states of charge are ``socs`` [n] or [n, 5]; the rest plausible noise (the box
    reads the state of charge alone)."""
    socs = np.asarray(socs, dtype=np.float64)
    n = socs.shape[0]
    rng = np.random.RandomState(seed + 11)
    s = rng.uniform(0.0, 1.0, size=(n, oe.GRID.state_dim))
    s[:, -oe.GRID.ne - oe.NAHEAD:-oe.NAHEAD] = socs.reshape(n, -1)
    return s.astype(np.float32)


def edge_rows(P, heads, box_of, seed=0):
    """RAWS x KINDS x SOCS rows: float32 (raw [n, heads * P], target [n, P], state [n, 57]); ``box_of(state)`` -> float64 numpy
    (lo, hi) [n, P] (a constant box ignores the state).  Row r: every component has raw RAWS[.] (alternating sign pattern along
    j so that both tails meet both ends of the box) and a target of kind KINDS[.]; the log-std half is noise."""
    rng = np.random.RandomState(seed + 5)
    combos = [(r, k, s) for r in RAWS for k in KINDS for s in SOCS]
    n = len(combos)
    st = states(np.array([c[2] for c in combos]), seed)
    lo, hi = box_of(st)
    raw = np.zeros((n, heads * P), dtype=np.float32)
    tgt = np.zeros((n, P), dtype=np.float32)
    sign = np.where(np.arange(P) % 2 == 0, 1.0, -1.0)
    for i, (r, k, _) in enumerate(combos):
        raw[i, :P] = r * sign
        tgt[i] = _targets(k, lo[i:i + 1], hi[i:i + 1], CLIP, rng)[0]
    if heads == 2:
        raw[:, P:] = rng.randn(n, P).astype(np.float32)
    return raw, tgt, st


def random_rows(n, P, heads, box_of, seed=0):
    """n random rows: raw N(0, 1.5) with a tail into saturation, targets inside and (a fifth) outside the box, states of charge
    across the band and (one row in eight) out of it."""
    rng = np.random.RandomState(seed + 9)
    soc = rng.uniform(0.05, 0.85, size=(n, oe.GRID.ne))
    out = rng.rand(n) < 0.125
    soc[out] = rng.choice([1.0, 1.1, -0.3], size=(int(out.sum()), 1))
    st = states(soc, seed + 1)
    lo, hi = box_of(st)
    raw = np.where(rng.rand(n, heads * P) < 0.8, 1.5 * rng.randn(n, heads * P), rng.uniform(-12, 12, (n, heads * P)))
    scale = (hi - lo) * 0.5
    tgt = lo + scale + scale * rng.uniform(-1.25, 1.25, size=lo.shape)
    return raw.astype(np.float32), tgt.astype(np.float32), st


def evopf_lohi(state):
    lo, hi = oe.partial_box(np.asarray(state, dtype=np.float64))
    return lo, hi


def const_lohi(lo, hi):
    lo, hi = (np.asarray(v, dtype=np.float32).astype(np.float64).reshape(1, -1) for v in (lo, hi))
    return lambda state: (np.repeat(lo, state.shape[0], 0), np.repeat(hi, state.shape[0], 0))


#: the constant boxes of the tests: P = 1 (CartSafe / SpringPendulum shapes) and a three-component one
CONST_BOXES = {"unit": ([-1.0], [1.0]), "offset": ([4.9], [5.1]), "three": ([-1.0, 4.9, -10.0], [1.0, 5.1, 10.0])}
WEIGHT_SETS = {1: (None, [2.5]), 3: (None, [1.0, 0.0, 0.5]),
               14: (None, [1.0, 1.0, 0.0, 1.0, 0.5, 0.5, 0.5, 0.5, 0.5, 2.0, 2.0, 0.0, 2.0, 2.0])}


def all_rows(P, heads, box_of, seed=0):
    """The edge rows followed by 257 random rows."""
    a, b = edge_rows(P, heads, box_of, seed), random_rows(257, P, heads, box_of, seed)
    return tuple(np.concatenate([x, y]) for x, y in zip(a, b))


def away_from_empty_seam(scale):
    """Rows / components whose float64 scale is not within float32 rounding of MIN_SCALE (there the two sides may disagree on
    whether the box is empty, and a comparison says nothing).  No row of this file is."""
    return (torch.as_tensor(scale) - MIN_SCALE).abs() > 1e-9


# ================================================================================================== the chain through the actor
def actor_chain(params, S, E, H, n_out, hd, obs, target, lo, hi, weights=None, clip=0.98, dtype=torch.float64):
    """One cloning step's loss and parameter gradients by autograd through explicit matmuls in ``dtype``: params maps Ws, bs, W0,
    b0, W1, b1 (, W1b, b1b) to tensors in nn.Linear layout; obs [n, S]; lo / hi [n, P] in ``dtype``'s own evaluation.
    Returns (loss, {name: grad}, (x0, h1, raw))."""
    p = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in params.items() if v is not None}
    s = torch.as_tensor(obs).to(dtype)
    x0 = s @ p["Ws"].t() + p["bs"]
    h1 = torch.relu(x0) @ p["W0"].t() + p["b0"]
    r1 = torch.relu(h1)
    outs = [r1 @ p["W1"].view(hd, H).t() + p["b1"].view(hd)]
    if n_out > 1:
        outs.append(r1 @ p["W1b"].view(hd, H).t() + p["b1b"].view(hd))
    raw = torch.cat(outs, dim=1)
    target, lo, hi = (torch.as_tensor(v).to(dtype) for v in (target, lo, hi))
    n, P = target.shape
    w = _w(weights, P, dtype)
    scale = (hi - lo) * 0.5
    base = lo + scale
    live = scale > MIN_SCALE
    safe = torch.where(live, scale, torch.ones_like(scale))
    c = float(np.float32(clip))
    u = torch.clamp((target - base) / safe, min=-c, max=c)
    y = torch.tanh(raw[:, :P])
    loss = (torch.where(live, w * (y - u) ** 2, torch.zeros_like(y)) / (n * P)).sum()
    names = sorted(p)
    grads = torch.autograd.grad(loss, [p[k] for k in names], allow_unused=True)
    return loss.detach(), {k: (torch.zeros_like(p[k]) if g is None else g) for k, g in zip(names, grads)}, \
        (x0.detach(), h1.detach(), raw.detach())


def chain_mags(params, S, E, H, n_out, hd, obs, target, box, x0, h1, raw, draw, weights=None, clip=0.98):
    """Magnitudes of the parameter gradients of ``actor_chain``, in units of eps32, at the float64 values x0, h1, raw, draw.  With
    B(v) the |.|-expression of mlp_f64.Mlp64.backward for a head gradient of magnitude v, L its chain length and n the rows:
        (L + n) B(|draw|)                     the backward's own roundings: one row's chain plus the batch sum
      + B(gm + |d draw / d raw| raw_mag)      the head's roundings (``bc_mags``) and the forward's error in raw (forward_bound's
                                              |.|-expression times its length), carried through the head's derivative
                                              c om (om + 2 |y| |d|) and then through the backward like a gradient
      + |draw|^T a1 (L0 + L1)  (W1, W1b)      the forward's error in the activations the outer products read
      + |dh|^T a0 L0           (W0)
    ReLU masks are taken as equal on both sides (a pre-activation within an ulp of zero is not among these inputs)."""
    d = torch.float64
    net = mlp_f64.Mlp64(params, S, 0, E, H, n_out=n_out, cat=False, head_dim=hd)
    obs, x0, h1, raw, draw = (torch.as_tensor(v).to(d) for v in (obs, x0, h1, raw, draw))
    n, P = target.shape
    _, a0, L0 = net.first_layer(obs)
    _, _, L1 = net.hidden(x0)
    a1 = a0 @ net.p["W0"].abs().t() + net.p["b0"].abs()
    _, a2, Lf = net.forward_bound(obs)
    lo, hi, scale = (torch.as_tensor(v).to(d) for v in box[:3])
    live = scale > MIN_SCALE
    safe = torch.where(live, scale, torch.ones_like(scale))
    base = lo + scale
    c = float(np.float32(clip))
    u = torch.clamp((torch.as_tensor(target).to(d) - base) / safe, min=-c, max=c)
    r = raw[:, :P]
    y = torch.tanh(r)
    om = 4.0 / (torch.exp(r) + torch.exp(-r)) ** 2
    w = _w(weights, P, d)
    sens = torch.where(live, 2 * w / (n * P) * om * (om + 2 * y.abs() * (y - u).abs()), torch.zeros_like(y))
    dmag = bc_mags(raw, target, box, weights, clip)["draw"] + sens * (a2[:, :P] * Lf)
    dmag = torch.cat([dmag, torch.zeros(n, (n_out - 1) * P, dtype=d)], dim=1)
    own = net.backward(obs, None, x0, h1, draw)
    car = net.backward(obs, None, x0, h1, dmag)
    out = {k: own[k][1] * (own[k][2] + n) + car[k][1] for k in own if k not in ("dx0", "da")}
    ws, _ = net._heads()
    douts = [draw[:, k * hd:(k + 1) * hd].abs() for k in range(n_out)]
    for k, name in enumerate(("W1", "W1b")[:n_out]):
        out[name] = out[name] + (douts[k].t() @ (a1 * (L0 + L1))).view(out[name].shape)
    dh_abs = sum(dk @ wk.abs() for dk, wk in zip(douts, ws)) * (h1 > 0).to(d)
    out["W0"] = out["W0"] + dh_abs.t() @ (a0 * L0)
    return out
