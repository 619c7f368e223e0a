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
