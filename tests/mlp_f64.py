"""Float64 restatement of the MLP kernels (include/rpo_hip.h: rpo_mlp_forward, rpo_mlp_backward, rpo_td) with a running-error
bound beside every value.  Explicit torch matmuls, so the same code runs on the CPU and on the GPU.

Layer-local: every layer starts from the KERNEL's float32 input to that layer (its saved x0 / h1; ReLU masks from those
values), so a pre-activation within an ulp of zero cannot flip a mask between the two sides.  Alongside each reference value
the same expression is evaluated on absolute values (|A| |B|): a float32 result that is a sum of K products, in ANY order
and with or without fused multiply-adds, differs from the exact value by at most gamma_L |A| |B| with L = K + 1 (K - 1 adds
in the deepest chain, plus the product's own rounding and the bias add), gamma_L = L u / (1 - L u) and u = 2^-24.  Chains
compose: a value computed from a float32 intermediate that is itself within gamma_L1 of its own |.| expression carries
L1 + L2 (first order; ``bound`` adds the (1 - L u) denominator back).  Every function returns (ref, abs, L).
"""
import torch

U = 2.0 ** -24
TINY = 1e-30          # absolute slack: float32 underflow of products far below every value compared here

FIELDS = ("Ws", "bs", "Wa", "ba", "W0", "b0", "W1", "b1", "W1b", "b1b")


def bound(absval, L):
    """|float32 result - float64 reference| <= gamma_L * absval + TINY."""
    return (L * U / (1.0 - L * U)) * absval + TINY


def ratio(got, ref, absval, L):
    """Worst |got - ref| / bound over the elements (<= 1 passes)."""
    err = (got.to(torch.float64) - ref).abs()
    return float((err / bound(absval, L)).max())


class Mlp64(object):
    """The float64 parameters of one network in the layout of ``rpo_mlp``: ``tensors`` maps Ws, bs, Wa, ba, W0, b0, W1, b1,
    W1b, b1b to tensors (absent / None where the network has none), nn.Linear layout [out][in]."""

    def __init__(self, tensors, S, A, E, H, n_out=1, cat=False, head_dim=1, device=None):
        self.p = {k: (None if tensors.get(k) is None else tensors[k].detach().to(device=device, dtype=torch.float64))
                  for k in FIELDS}
        self.S, self.A, self.E, self.H, self.n_out, self.cat = int(S), int(A), int(E), int(H), int(n_out), bool(cat)
        self.hd = max(1, int(head_dim))
        self.ein = self.E * (2 if self.cat else 1)

    @staticmethod
    def _f64(t):
        return t.to(torch.float64)

    def _heads(self):
        """[W_k, b_k] of the n_out heads, each [hd, H] / [hd]."""
        ws = [self.p["W1"].view(self.hd, self.H)] + ([self.p["W1b"].view(self.hd, self.H)] if self.n_out > 1 else [])
        bs = [self.p["b1"].view(self.hd)] + ([self.p["b1b"].view(self.hd)] if self.n_out > 1 else [])
        return ws, bs

    # ------------------------------------------------------------------------------------------------------ forward
    def first_layer(self, s, a=None):
        """x0 = s Ws^T + bs (+ a Wa^T + ba; cat: side by side).  L: S (+ A) products and one or two bias adds."""
        s = self._f64(s)
        xs = s @ self.p["Ws"].t() + self.p["bs"]
        xs_abs = s.abs() @ self.p["Ws"].abs().t() + self.p["bs"].abs()
        if self.A == 0:
            return xs, xs_abs, self.S + 1
        a = self._f64(a)
        xa = a @ self.p["Wa"].t() + self.p["ba"]
        xa_abs = a.abs() @ self.p["Wa"].abs().t() + self.p["ba"].abs()
        if self.cat:
            return torch.cat([xs, xa], 1), torch.cat([xs_abs, xa_abs], 1), max(self.S, self.A) + 1
        return xs + xa, xs_abs + xa_abs, self.S + self.A + 3

    def hidden(self, x0):
        """h1 = relu(x0) W0^T + b0 from the kernel's x0.  L = Ein + 1."""
        r = self._f64(x0).clamp_min(0.0)
        return r @ self.p["W0"].t() + self.p["b0"], r @ self.p["W0"].abs().t() + self.p["b0"].abs(), self.ein + 1

    def head(self, h1):
        """out = relu(h1) W1_k^T + b1_k (head-major when hd > 1) from the kernel's h1.  L = H + 1."""
        r = self._f64(h1).clamp_min(0.0)
        ws, bs = self._heads()
        out = torch.cat([r @ w.t() + b for w, b in zip(ws, bs)], 1)
        out_abs = torch.cat([r @ w.abs().t() + b.abs() for w, b in zip(ws, bs)], 1)
        return out, out_abs, self.H + 1

    def forward(self, s, a=None):
        """The whole network in float64 (not layer-local: for the check against autograd)."""
        x0 = self.first_layer(s, a)[0]
        h1 = self.hidden(x0)[0]
        return self.head(h1)[0], x0, h1

    def forward_bound(self, s, a=None):
        """The whole network in float64 with a bound on a float32 forward of the same inputs: (out, abs, L) with
        |out32 - out| <= gamma_L abs.  ReLU is 1-Lipschitz and |relu(x)| <= |x|, so an error of gamma_L0 A0 in x0 reaches h1 as
        at most gamma_L0 (|W0| A0) <= gamma_L0 A1 with A1 = |W0| A0 + |b0| (A0 the first layer's |.| expression, no mask), and
        h1's own rounding adds gamma_L1 A1; gamma_a + gamma_b + gamma_a gamma_b <= gamma_(a+b).  Likewise for the heads."""
        x0, a0, L0 = self.first_layer(s, a)
        h1, _, L1 = self.hidden(x0)
        a1 = a0 @ self.p["W0"].abs().t() + self.p["b0"].abs()
        out, _, L2 = self.head(h1)
        ws, bs = self._heads()
        a2 = torch.cat([a1 @ w.abs().t() + b.abs() for w, b in zip(ws, bs)], 1)
        return out, a2, L0 + L1 + L2

    def forward_running(self, s, a=None, a_err=None):
        """The whole network in float64 with the running bound of a float32 forward of the same inputs carried layer by layer:
        (out, err) with |out32 - out| <= err.  forward_bound pushes the first layer's |.| expression through |W0| and |W1| and
        multiplies by gamma of the whole chain; here every layer adds gamma_L of ITS OWN |.| expression at the float64
        activations (widened by the error they carry) to |W| applied to the error it was handed (relu is 1-Lipschitz):
            e0 = gamma_L0 A0 (+ |Wa| a_err),   e1 = e0 |W0| + gamma_L1 ((relu(x0) + e0) |W0| + |b0|),   e2 likewise.
        The same inequalities, a factor of some tens tighter at 256 -> 256.  ``a_err`` [n, A]: a bound on what the launch read in
        place of ``a``, every weight in absolute value (valid through the relu; a first-order gradient is not)."""
        g = lambda L: L * U / (1.0 - L * U)                                       # noqa: E731
        x0, a0, L0 = self.first_layer(s, a)
        e0 = g(L0) * a0
        if a_err is not None:
            ea = self._f64(a_err) @ self.p["Wa"].abs().t()
            e0 = e0 + (torch.cat([torch.zeros_like(ea), ea], 1) if self.cat else ea) * (1.0 + g(L0))
        h1, _, L1 = self.hidden(x0)
        w0 = self.p["W0"].abs().t()
        e1 = e0 @ w0 + g(L1) * ((x0.clamp_min(0.0) + e0) @ w0 + self.p["b0"].abs())
        out, _, L2 = self.head(h1)
        ws, bs = self._heads()
        r1 = h1.clamp_min(0.0) + e1
        e2 = torch.cat([e1 @ w.abs().t() + g(L2) * (r1 @ w.abs().t() + b.abs()) for w, b in zip(ws, bs)], 1)
        return out, e2 + TINY

    # ----------------------------------------------------------------------------------------------------- backward
    def backward(self, s, a, x0, h1, dout, param_grads=True, first_layer_state_only=False):
        """What rpo_mlp_backward computes from the kernel's saved x0 / h1 and a float32 dout [n, n_out * hd]:
        {name: (ref, abs, L_inner)} for every parameter gradient it writes (Ws .. b1b) and for 'dx0' and 'da'.

        L_inner counts the chain INSIDE one row (dh, dx0, da) plus one for the product that meets the batch sum; the caller
        adds the batch reduction's chain (rows per slice + Z + ..., or n) for parameter gradients -- da / dx0 are per row."""
        s, x0, h1, dout = self._f64(s), self._f64(x0), self._f64(h1), self._f64(dout)
        a = None if a is None else self._f64(a)
        H, E, hd = self.H, self.E, self.hd
        m1 = (h1 > 0).to(torch.float64)
        r1 = h1.clamp_min(0.0)
        r0 = x0.clamp_min(0.0)
        m0 = (x0 > 0).to(torch.float64)
        ws, _ = self._heads()
        douts = [dout[:, k * hd:(k + 1) * hd] for k in range(self.n_out)]
        res = {}
        # dh = mask (.) sum_k dout_k W1_k: n_out * hd products per element
        dh = sum(d @ w for d, w in zip(douts, ws)) * m1
        dh_abs = sum(d.abs() @ w.abs() for d, w in zip(douts, ws)) * m1
        L_dh = self.n_out * hd + 1
        # dx0 = (dh W0) (.) 1[x0 > 0]: H more products (the streaming rows kernel multiplies by dout after this k-sum: the
        # same |.| expression)
        dx0 = (dh @ self.p["W0"]) * m0
        dx0_abs = (dh_abs @ self.p["W0"].abs()) * m0
        L_dx0 = L_dh + H + 1
        res["dx0"] = (dx0, dx0_abs, L_dx0)
        dxs, dxs_abs = (dx0[:, :E], dx0_abs[:, :E]) if self.cat else (dx0, dx0_abs)
        dxa, dxa_abs = (dx0[:, E:], dx0_abs[:, E:]) if self.cat else (dx0, dx0_abs)
        if self.A > 0:
            # da = dx0_a Wa: E more products
            res["da"] = (dxa @ self.p["Wa"], dxa_abs @ self.p["Wa"].abs(), L_dx0 + E + 1)
        if not param_grads:
            return res
        res["Ws"] = (dxs.t() @ s, dxs_abs.t() @ s.abs(), L_dx0 + 1)
        res["bs"] = (dxs.sum(0), dxs_abs.sum(0), L_dx0 + 1)
        if first_layer_state_only:
            return res
        if self.A > 0:
            res["Wa"] = (dxa.t() @ a, dxa_abs.t() @ a.abs(), L_dx0 + 1)
            res["ba"] = (dxa.sum(0), dxa_abs.sum(0), L_dx0 + 1)
        res["W0"] = (dh.t() @ r0, dh_abs.t() @ r0, L_dh + 1)
        res["b0"] = (dh.sum(0), dh_abs.sum(0), L_dh + 1)
        for k, (wn, bn) in enumerate((("W1", "b1"), ("W1b", "b1b"))[:self.n_out]):
            d = douts[k]
            res[wn] = ((d.t() @ r1).view(self.p[wn].shape), (d.abs().t() @ r1).view(self.p[wn].shape), 1)
            res[bn] = (d.sum(0).view(self.p[bn].shape), d.abs().sum(0).view(self.p[bn].shape), 1)
        return res


def td(q, qn1, reward, done, gamma, qn2=None, logp=None, alpha=0.0, qn_err=None):
    """rpo_td in float64 from the kernel's float32 inputs (rpo_ddpg.py:331-335 / rpo_sac.py:346-353):
        y = reward + gamma (1 - done) (min(qn1, qn2) - alpha logp),  d = q - y,
        dq = clamp(d, -1, 1) / n,  loss = mean smooth_l1(d).
    Returns (dq, dq_bound, loss, loss_bound, d).  clamp and smooth_l1 are continuous with a continuous first derivative at
    the kink, so a float32 d within delta of the float64 d moves dq by <= delta / n and a row's Huber term by <=
    (min(|d|, 1) + delta) delta / n whichever side of the kink either lands on.
    delta: y is five float32 operations on its inputs and d one more: delta <= gamma_8 (|q| + |r| + |gamma (1 - done)| (|qn| +
    |alpha logp|)).  dq then gains the rounding of 1 / n and of the product (2 u |dq|); a Huber term its own three roundings
    (0.5 d d / n, or |d| - 0.5 and / n); the kernel adds 16 rows per tile share (gamma_16 of the tile's |terms|) and the test
    adds the shares in float64.
    qn_err: when qn1 / qn2 are float64 references of the values the kernel read (not those values themselves), a bound on
    |qn_kernel - qn| per row; min() is 1-Lipschitz in each argument, so it reaches d as |gamma (1 - done)| qn_err."""
    f = lambda t: None if t is None else t.to(torch.float64).reshape(-1)      # noqa: E731
    q, qn1, reward, done, qn2, logp = f(q), f(qn1), f(reward), f(done), f(qn2), f(logp)
    n = q.numel()
    g32 = float(torch.tensor(gamma, dtype=torch.float32))
    a32 = float(torch.tensor(alpha, dtype=torch.float32))
    qn = qn1 if qn2 is None else torch.minimum(qn1, qn2)
    qn_abs = qn.abs()
    if logp is not None:
        qn = qn - a32 * logp
        qn_abs = qn_abs + abs(a32) * logp.abs()
    y = reward + g32 * (1.0 - done) * qn
    d = q - y
    d_abs = q.abs() + reward.abs() + abs(g32) * (1.0 - done).abs() * qn_abs
    delta = bound(d_abs, 8)
    if qn_err is not None:
        delta = delta + abs(g32) * (1.0 - done).abs() * f(qn_err) * (1.0 + 8 * U)
    dq = d.clamp(-1.0, 1.0) / n
    dq_bound = delta / n + 2 * U * dq.abs() + TINY
    ad = d.abs()
    hub = torch.where(ad < 1.0, 0.5 * d * d, ad - 0.5) / n
    row_bound = (ad.clamp(max=1.0) + delta) * delta / n + bound(hub.abs(), 3)
    loss = float(hub.sum())
    loss_bound = float(row_bound.sum() + bound(hub.abs(), 16).sum())
    return dq, dq_bound, loss, loss_bound, d


def _td_rows(q, qn1, reward, done, gamma, qn2=None, logp=None, alpha=0.0):
    """Per-row float64 TD error d, the bound delta on a float32 d, the Huber term / n and its bound (see ``td``)."""
    f = lambda t: None if t is None else t.to(torch.float64).reshape(-1)      # noqa: E731
    q, qn1, reward, done, qn2, logp = f(q), f(qn1), f(reward), f(done), f(qn2), f(logp)
    n = q.numel()
    g32 = float(torch.tensor(gamma, dtype=torch.float32))
    a32 = float(torch.tensor(alpha, dtype=torch.float32))
    qn = qn1 if qn2 is None else torch.minimum(qn1, qn2)
    qn_abs = qn.abs()
    if logp is not None:
        qn = qn - a32 * logp
        qn_abs = qn_abs + abs(a32) * logp.abs()
    d = q - (reward + g32 * (1.0 - done) * qn)
    delta = bound(q.abs() + reward.abs() + abs(g32) * (1.0 - done).abs() * qn_abs, 8)
    ad = d.abs()
    hub = torch.where(ad < 1.0, 0.5 * d * d, ad - 0.5) / n
    row_bound = (ad.clamp(max=1.0) + delta) * delta / n + bound(hub.abs(), 3)
    return d, delta, hub, row_bound


def td_partials(q, qn1, reward, done, gamma, qn2=None, logp=None, alpha=0.0):
    """loss_partial of rpo_td tile by tile: (ref [ceil(n / 16)], bound) -- the float64 sum of the Huber terms / n of rows
    [16 t, 16 t + 16) (the last tile holds n - 16 t rows, each STILL divided by n), the rows' own bounds (``td``) and gamma_16 of
    the tile's |terms| for the 16-term sum of the kernel."""
    d, delta, hub, row_bound = _td_rows(q, qn1, reward, done, gamma, qn2, logp, alpha)
    n = d.numel()
    pad = (-n) % 16
    z = torch.zeros(pad, dtype=torch.float64, device=d.device)
    tiles = lambda t: torch.cat([t, z]).view(-1, 16).sum(1)                   # noqa: E731
    return tiles(hub), tiles(row_bound) + bound(tiles(hub.abs()), 16)


# ------------------------------------------------------------------------------- out_mode 1: the tanh box on output 0
def box_out(o, scale, base):
    """out_mode = 1 of rpo_mlp_forward from the kernel's own float32 o: (ref, allowed) with ref = scale tanh(o) + base in
    float64 and allowed = MARGIN * C_REF_BOX_FWD * eps32 * magnitude sum -- the convention of tests/heads_f64.py for the same
    map (tanh_box_fwd_mags there: |scale| ((1 - y^2) |o| + |y|) + |scale y| + |base|; C_REF_BOX_FWD the float32-CPU constant)."""
    import heads_f64
    o = o.to(torch.float64)
    s32, b32 = heads_f64.f32(scale), heads_f64.f32(base)
    ref = s32 * torch.tanh(o) + b32
    return ref, heads_f64.MARGIN * heads_f64.C_REF_BOX_FWD * heads_f64.EPS32 * heads_f64.tanh_box_fwd_mags(o, s32, b32) + TINY


# ------------------------------------------------------------------------------------------------- the += form
def accumulate(entry, g0):
    """A parameter gradient ADDED onto a buffer that held g0 (float32): ref g0 + grad, |.| expression |g0| + abs, one more
    rounding."""
    ref, absval, L = entry
    g0 = g0.to(torch.float64).reshape(ref.shape)
    return ref + g0, absval + g0.abs(), L + 1


# ----------------------------------------------------------------------- networks, inputs and the checker of the small-n tests
# (name, kind, S, A, E, n_out, head_dim): the smallest set that reaches every instantiation and first-layer form of the row-tile,
# multi-output and layer-by-layer kernels (tests/test_mlp_small_f64_gpu.py; the float32 CPU stand-in of tests/test_mlp_f64.py)
NETWORKS = [
    ("add_6_2", "add", 6, 2, 128, 1, 1), ("add_5_2", "add", 5, 2, 128, 1, 1),            # cart / pendulum critics (MFMA layer 1)
    ("actor_6", "actor", 6, 0, 128, 1, 1), ("actor_1", "actor", 1, 0, 128, 1, 1),        # lower edge of the k slots
    ("gauss_5", "gauss", 5, 0, 128, 2, 1),                                               # second scalar head
    ("add_3_1", "add", 3, 1, 128, 1, 1), ("add_6_4", "add", 6, 4, 128, 1, 1),            # edges of the MFMA first layer
    ("add_7_2", "add", 7, 2, 128, 1, 1), ("add_6_5", "add", 6, 5, 128, 1, 1),            # vector first layer just beyond them
    ("add_64_48", "add", 64, 48, 128, 1, 1),                                             # the full LDS input strides
    ("add256_6_2", "add", 6, 2, 256, 1, 1), ("gauss256_5", "gauss", 5, 0, 256, 2, 1),    # Ein 256 (layer by layer; 2 head problems)
    ("cat_57_43", "cat", 57, 43, 256, 1, 1),                                             # EVOPF critic (Ein 512)
    ("actor14", "actor", 57, 0, 256, 1, 14), ("gauss14", "gauss", 57, 0, 256, 2, 14),    # EVOPF actors
    ("wide14", "actor", 6, 0, 128, 1, 14), ("wide2", "actor", 6, 0, 128, 1, 2), ("wide16", "actor", 6, 0, 128, 1, 16),
]
NET_BY_NAME = {t[0]: t for t in NETWORKS}
H = 256
ZERO_COL = 5            # the planted dead column of the first layer (make_params)


def make_params(spec, seed, device=None, zero_col=True):
    """Float32 parameters of one network of NETWORKS, nn.Linear layout and its default U(-1/sqrt(fan_in), 1/sqrt(fan_in))
    ranges.  zero_col: row ZERO_COL of Ws (and Wa, unless concatenated) and its biases are exactly 0 -- x0[:, ZERO_COL] is
    exactly 0 for every input and contributes exactly nothing to h1."""
    _, kind, S, A, E, n_out, hd = spec
    g = torch.Generator().manual_seed(seed)
    u = lambda shape, fan: ((torch.rand(*shape, generator=g) * 2 - 1) / fan ** 0.5)      # noqa: E731
    ein = 2 * E if kind == "cat" else E
    p = dict(Ws=u((E, S), S), bs=u((E,), S), W0=u((H, ein), ein), b0=u((H,), ein), W1=u((hd, H), H), b1=u((hd,), H))
    if A:
        p.update(Wa=u((E, A), A), ba=u((E,), A))
    if n_out > 1:
        p.update(W1b=u((hd, H), H), b1b=u((hd,), H))
    if zero_col:
        for k in ("Ws", "bs") + (("Wa", "ba") if A and kind != "cat" else ()):
            p[k][ZERO_COL] = 0.0
    return {k: v.to(device) for k, v in p.items()}


def mlp64_of(spec, params, device=None):
    _, kind, S, A, E, n_out, hd = spec
    return Mlp64(params, S, A, E, H, n_out=n_out, cat=kind == "cat", head_dim=hd, device=device)


HUGE, SMALL = 1e30, 1e-38


def make_inputs(spec, n, seed, device=None, guard=4, planted=True):
    """s / a [n, S] / [n, A] as strided column views of ONE wider matrix with `guard` rows of NaN before and after (a padded lane
    that reads past row n - 1 AND lets it contribute shows as NaN).  planted (n >= 4): row 1 holds +-1e30 and row 2 +-1e-38
    (float32 denormals) in every input -- a float32 forward stays finite: |x0| <= (S + A) 1e30, |h1| <= 512 (S + A) 1e30 / 16,
    |out| below 1e36 -- and row 3 exact zeros."""
    _, kind, S, A, E, n_out, hd = spec
    g = torch.Generator().manual_seed(seed)
    wide = torch.randn(n + 2 * guard, S + A + 3, generator=g)
    wide[:guard] = float("nan")
    wide[guard + n:] = float("nan")
    if planted and n >= 4:
        sign = torch.where(torch.rand(S + A + 3, generator=g) < 0.5, -1.0, 1.0)
        wide[guard + 1] = HUGE * sign
        wide[guard + 2] = SMALL * sign
        wide[guard + 3] = 0.0
    wide = wide.to(device)
    body = wide[guard:guard + n]
    return body[:, 1:1 + S], (body[:, 1 + S:1 + S + A] if A else None), wide


def plant_activations(x0, h1, seed):
    """Edge values written INTO saved pre-activations (the backward reads them): per row >= 2 one entry each of +0, -0, the
    smallest positive and negative denormal at seeded columns of x0 and of h1; row 0 of x0 all +0 and row 1 of h1 all -0 (n
    permitting).  The mask is `> 0`: the gradient through +-0 and the negative denormal is exactly 0, through the positive
    denormal it passes."""
    g = torch.Generator().manual_seed(seed)
    den = float(torch.tensor(1, dtype=torch.int32).view(torch.float32))      # 2^-149
    vals = torch.tensor([0.0, -0.0, den, -den], dtype=torch.float32)
    for t in (x0, h1):
        n, w = t.shape
        cols = torch.rand(n, w, generator=g).topk(4, dim=1).indices.to(t.device)     # four distinct columns per row
        t.scatter_(1, cols, vals.to(t.device).expand(n, 4).contiguous())
    x0[0] = 0.0
    if x0.shape[0] > 1:
        h1[1] = -0.0
    return x0, h1


def check(what, got, ref, absval, L, worst, allowed=None):
    """Every element of got within gamma_L absval (or `allowed`) of ref; the worst ratio is recorded under the last word of
    `what` ("probe" / "+=" prefixed when `what` says so)."""
    got = got.to(torch.float64).reshape(ref.shape)
    assert bool(torch.isfinite(got).all()), "%s: non-finite (never written?)" % what
    if allowed is None:
        r = ratio(got, ref, absval, L)
    else:
        r = float(((got - ref).abs() / allowed).max())
    key = ("probe " if " probe " in what else "+= " if " += " in what else "") + what.split()[-1]
    worst[key] = max(worst.get(key, 0.0), r)
    assert r <= 1.0, "%s: |got - ref| is %.3g x the bound%s" % (what, r, "" if allowed is not None else " gamma_%d |A||B|" % L)


def report(tag, worst):
    print("%s: worst |err| / bound %s" % (tag, ", ".join("%s %.3g" % (k, v) for k, v in sorted(worst.items()))))


def check_forward(net, s, a, out, x0, h1, worst, tag):
    """out / x0 / h1 of one forward, layer by layer from the given (the kernel's own float32) input to each layer."""
    r, ab, L = net.first_layer(s, a)
    check(tag + " x0", x0, r, ab, L, worst)
    r, ab, L = net.hidden(x0)
    check(tag + " h1", h1, r, ab, L, worst)
    r, ab, L = net.head(h1)
    check(tag + " out", out, r, ab, L, worst)


def batch_chain(rows):
    """Additions a parameter-gradient element meets over `rows` rows in ANY of the small-n paths.  Every path gives an element
    one owner and a fixed order over a partition of the batch: the one-owner pass 4 wave (or 16 / 8 slice) partials of
    contiguous row ranges added in order, then one add onto the gradient (mlp_bwd_weights_body, mlp_bwd_first_layer_impl: 16
    phases); the MFMA first-layer role of the 256-wide networks (mlp_bwd_first_layer_mfma) and the dW0 tiles k-steps of 4 rows
    per wave, ((t0 + t1) + t2) + t3 and the add onto the gradient; the multi-output head role 16 slices of each 256-row pass.
    The deepest chain of any such order has at most rows - 1 + (partials <= 16) additions; + 1 for the add onto the gradient and
    + 3 of slack: rows + 20, the one-owner figure of tests/test_large_batch_f64_gpu.py (batch_chain(n, 0)).  The rows launches of
    the layer-by-layer path (gemm_backward_rows: dh, dx0, da) are per-row chains over H / Ein / E products in k order, or -- with
    the k range split over four waves -- in another order: the bound gamma_L |A||B| holds for any order, no batch term.
    rows = 1 (a one-hot probe): every other row adds exact zeros (0 x finite, x + 0), so the row's product meets ONE addition."""
    return 1 if rows == 1 else rows + 20


def check_backward(net, s, a, x0, h1, dout, got, pre, worst, tag, param_grads=True, state_only=False, rows=None, want_da=True):
    """One backward call against float64 from the x0 / h1 / dout it read.  got: dict(dx0=, da=, <parameter>=gradient buffer
    after the call); pre: {parameter: what the buffer held before}.  Parameter gradients are judged as pre + gradient (+= form);
    every parameter a reduced mode must not write is compared BITWISE with `pre`.  rows: the number of rows with a non-zero
    dout (one-hot probes: 1 -- every other row adds exact zeros); default the batch."""
    res = net.backward(s, a, x0, h1, dout, param_grads=param_grads, first_layer_state_only=state_only)
    chain = batch_chain(dout.shape[0] if rows is None else rows)
    r, ab, L = res["dx0"]
    check(tag + " dx0", got["dx0"], r, ab, L, worst)
    if net.A > 0 and want_da:
        r, ab, L = res["da"]
        check(tag + " da", got["da"], r, ab, L, worst)
    written = []
    for name in FIELDS:
        if net.p[name] is None:
            continue
        if name in res:
            r, ab, L = accumulate(res[name], pre[name])
            check("%s %s" % (tag, name), got[name], r, ab, L + chain, worst)
            written.append(got[name])
        else:
            same = torch.equal(got[name].reshape(-1).view(torch.int32), pre[name].reshape(-1).view(torch.int32))
            assert same, "%s %s: written by a mode that must not touch it" % (tag, name)
    return written


def gradmax_of(written):
    """max |element| over the gradient tensors a call wrote: what its gradmax slots must hold, exactly."""
    return max([float(t.abs().max()) for t in written] + [0.0])


def plant_td_kink(q, qn1, reward, done, gamma, qn2=None, logp=None):
    """Rows with |q - y| EXACTLY 1 and within a few float32 ulps either side, written into q / qn1 / reward / done (/ qn2 / logp)
    in place (n permitting): rows 0 / 1 (of the first five) d = +1 / -1, then 1 + 2 ulp, 1 - 2 ulp, -(1 + 2 ulp).  With reward,
    qn1, qn2, logp and done all 0 the target is y = 0 exactly whatever gamma and alpha, and d = q.  Returns the planted rows."""
    up = float(torch.nextafter(torch.nextafter(torch.tensor(1.0), torch.tensor(2.0)), torch.tensor(2.0)))
    dn = float(torch.nextafter(torch.nextafter(torch.tensor(1.0), torch.tensor(0.0)), torch.tensor(0.0)))
    rows = []
    for i, d in enumerate((1.0, -1.0, up, dn, -up)):
        if i >= q.numel():
            break
        qn1[i], done[i], reward[i] = 0.0, 0.0, 0.0
        for extra in (qn2, logp):
            if extra is not None:
                extra[i] = 0.0
        q[i] = d
        rows.append(i)
    return rows
