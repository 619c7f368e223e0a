"""The float64 yardstick of the large-batch kernel tests (tests/mlp_f64.py) against torch.autograd on float64 copies of the
model modules (rpo_amd/algo/model): forward outputs, every parameter gradient, the action-input gradient, the TD / Huber
prologue.  CPU only."""
import copy

import pytest
import torch
import torch.nn.functional as F

import mlp_f64
from rpo_amd.algo.model import ActionEmbedding, GaussianSharedPolicy, SharedPolicy, SharedValueAdd, SharedValueCat, StateEmbedding


def _net(kind, S, A, E, H, heads):
    torch.manual_seed(S * 31 + A + E)
    se = StateEmbedding(S, E, H)
    if kind == "actor":
        return SharedPolicy(S, heads, se, E, H, 1, None)
    if kind == "gauss":
        return GaussianSharedPolicy(S, heads, se, E, H, 1, None)
    return (SharedValueCat if kind == "cat" else SharedValueAdd)(S, A, se, ActionEmbedding(A, E, H), E, H)


def _tensors(kind, net):
    t = dict(Ws=net.state_embed.embeds[0].weight, bs=net.state_embed.embeds[0].bias, W0=net.affines[0].weight,
             b0=net.affines[0].bias)
    if kind == "gauss":
        t.update(W1=net.affine_mean.weight, b1=net.affine_mean.bias, W1b=net.affine_log_std.weight, b1b=net.affine_log_std.bias)
    else:
        t.update(W1=net.affines[1].weight, b1=net.affines[1].bias)
    if kind in ("add", "cat"):
        t.update(Wa=net.action_embed.embeds[0].weight, ba=net.action_embed.embeds[0].bias)
    return t


def _module_out(kind, net, s, a):
    if kind == "actor":
        return net(s)
    if kind == "gauss":                                          # the raw heads rpo_mlp_forward returns: [mean | log-std head]
        x = F.relu(net.affines[0](F.relu(net.state_embed(s))))
        return torch.cat([net.affine_mean(x), net.affine_log_std(x)], 1)
    return net(s, a)


@pytest.mark.parametrize("kind,S,A,E,H,heads", [("add", 6, 2, 128, 256, 1), ("cat", 57, 43, 256, 256, 1), ("actor", 6, 0, 128, 256, 1),
                                                ("actor", 57, 0, 256, 256, 14), ("gauss", 5, 0, 128, 256, 1),
                                                ("gauss", 57, 0, 256, 256, 14)])
def test_float64_reference_matches_autograd(kind, S, A, E, H, heads):
    n = 37
    net = copy.deepcopy(_net(kind, S, A, E, H, heads)).double()
    ref = mlp_f64.Mlp64(_tensors(kind, net), S, A, E, H, n_out=2 if kind == "gauss" else 1, cat=kind == "cat",
                        head_dim=heads)
    g = torch.Generator().manual_seed(7)
    s = torch.randn(n, S, generator=g, dtype=torch.float64)
    a = torch.randn(n, A, generator=g, dtype=torch.float64).requires_grad_() if A else None
    out = _module_out(kind, net, s, a)
    got, x0, h1 = ref.forward(s, a)
    torch.testing.assert_close(got, out.detach(), rtol=1e-12, atol=1e-12)
    # layer-local pieces from the module's own intermediate values
    lin = net.state_embed.embeds[0](s)
    if A:
        la = net.action_embed.embeds[0](a)
        lin = torch.cat([lin, la], 1) if kind == "cat" else lin + la
    torch.testing.assert_close(x0, lin.detach(), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(h1, net.affines[0](F.relu(lin)).detach(), rtol=1e-12, atol=1e-12)
    for val, absval, _ in (ref.first_layer(s, a), ref.hidden(x0), ref.head(h1)):
        assert bool((val.abs() <= absval * (1 + 1e-12) + 1e-300).all())       # |sum| <= sum |.|
    dout = torch.randn(n, out.shape[1], generator=g, dtype=torch.float64)
    out.backward(dout)
    res = ref.backward(s, a, x0, h1, dout)
    names = {k for k in mlp_f64.FIELDS if _tensors(kind, net).get(k) is not None}
    assert names <= set(res), names - set(res)
    for k, t in _tensors(kind, net).items():
        torch.testing.assert_close(res[k][0], t.grad, rtol=1e-10, atol=1e-13, msg=k)
        assert bool((res[k][0].abs() <= res[k][1] * (1 + 1e-12) + 1e-300).all()), k
    if A:
        torch.testing.assert_close(res["da"][0], a.grad, rtol=1e-10, atol=1e-13)
    # param_grads = 0: only dx0 / da; first_layer_state_only: of the parameters only Ws / bs
    assert set(ref.backward(s, a, x0, h1, dout, param_grads=False)) == ({"dx0", "da"} if A else {"dx0"})
    fl = ref.backward(s, a, x0, h1, dout, first_layer_state_only=True)
    assert set(fl) - {"dx0", "da"} == {"Ws", "bs"}
    torch.testing.assert_close(fl["Ws"][0], res["Ws"][0], rtol=0, atol=0)


@pytest.mark.parametrize("sac", [False, True])
def test_float64_td_prologue_matches_autograd(sac):
    """dq and the loss of mlp_f64.td are d/dq of smooth_l1(q, y) (mean) and that loss (rpo_ddpg.py:331-335, rpo_sac.py:346-353)."""
    n = 200
    g = torch.Generator().manual_seed(3)
    q = (2 * torch.randn(n, generator=g, dtype=torch.float64)).requires_grad_()
    qn1, qn2, logp = (torch.randn(n, generator=g, dtype=torch.float64) for _ in range(3))
    reward = torch.randn(n, generator=g, dtype=torch.float64)
    done = (torch.rand(n, generator=g, dtype=torch.float64) > 0.7).double()
    gamma, alpha = 0.95, (0.2 if sac else 0.0)
    g32, a32 = (float(torch.tensor(v, dtype=torch.float32)) for v in (gamma, alpha))     # (the kernel's float32 constants)
    y = reward + g32 * (1 - done) * (torch.minimum(qn1, qn2) - a32 * logp if sac else qn1)
    loss = F.smooth_l1_loss(q, y)
    loss.backward()
    dq, dq_b, lo, lo_b, d = mlp_f64.td(q.detach(), qn1, reward, done, gamma, qn2 if sac else None, logp if sac else None, alpha)
    torch.testing.assert_close(dq, q.grad, rtol=1e-12, atol=1e-15)
    assert abs(lo - float(loss.detach())) < 1e-12
    torch.testing.assert_close(d, q.detach() - y, rtol=0, atol=0)
    assert bool((dq_b > 0).all()) and lo_b > 0 and bool((d.abs() > 1).any()) and bool((d.abs() < 1).any())   # both sides of the kink


# ============================================================================================ the small-n checker is not vacuous
# A plain torch float32 CPU forward / backward of every network of mlp_f64.NETWORKS stands in for the kernels: it must pass the
# checker the GPU tests use (tests/test_mlp_small_f64_gpu.py) with ratio <= 1 -- the derived bounds hold for an honest float32
# evaluation in torch's own summation order -- and each seeded mutation of it must FAIL.
class StandIn(object):
    """What the four entry points compute, in float32 torch on the CPU.  `bug` names one seeded mistake."""

    def __init__(self, spec, params, bug=None):
        self.spec, self.p, self.bug = spec, params, bug
        _, self.kind, self.S, self.A, self.E, self.n_out, self.hd = spec

    def heads(self):
        ks = [("W1", "b1")] + ([("W1b", "b1b")] if self.n_out > 1 else [])
        if self.bug == "heads_swapped":
            ks = ks[::-1]
        return ks

    def forward(self, s, a):
        p = self.p
        x0 = s @ p["Ws"].t() + p["bs"] * (2.0 if self.bug == "bias_twice" else 1.0)
        if self.A:
            xa = a @ p["Wa"].t() + p["ba"]
            x0 = torch.cat([x0, xa], 1) if self.kind == "cat" else x0 + xa
        h1 = x0.clamp_min(0) @ p["W0"].t() + p["b0"]
        r = h1.clamp_min(0)
        out = torch.cat([r @ p[w].t() + p[b] for w, b in self.heads()], 1)
        if self.bug == "row_major_head":                         # [n, hd, n_out] instead of head-major [n, n_out, hd]
            out = out.view(-1, self.n_out, self.hd).transpose(1, 2).reshape(out.shape)
        return out, x0, h1

    def backward(self, s, a, x0, h1, dout, grads, param_grads=True, state_only=False):
        """Returns dict(dx0, da, gradmax) and adds the parameter gradients onto `grads` in place."""
        p, hd, E, n = self.p, self.hd, self.E, s.shape[0]
        gt = (lambda t: t >= 0) if self.bug == "mask_ge" else (lambda t: t > 0)
        douts = [dout[:, k * hd:(k + 1) * hd] for k in range(self.n_out)]
        ws = [p["W1"]] + ([p["W1b"]] if self.n_out > 1 else [])
        dh = sum(d @ w for d, w in zip(douts, ws)) * gt(h1)
        dx0 = (dh @ p["W0"]) * gt(x0)
        out = dict(dx0=dx0, da=None)
        dxs, dxa = (dx0[:, :E], dx0[:, E:]) if self.kind == "cat" else (dx0, dx0)
        if self.A:
            out["da"] = dxa @ p["Wa"]
        rows = slice(0, n)                                       # the rows the batch sums see
        if self.bug == "last_row_dropped":
            rows = slice(0, n - 1)
        idx = torch.arange(n)[rows]
        if self.bug == "last_row_twice":
            idx = torch.cat([idx, idx[-1:]])
        new = {}
        if param_grads:
            new["Ws"], new["bs"] = dxs[idx].t() @ s[idx], dxs[idx].sum(0)
            if self.A and (not state_only or self.bug == "state_only_writes_wa"):
                new["Wa"], new["ba"] = dxa[idx].t() @ a[idx], dxa[idx].sum(0)
            if not state_only:
                new["W0"], new["b0"] = dh[idx].t() @ x0[idx].clamp_min(0), dh[idx].sum(0)
                for k, (wn, bn) in enumerate((("W1", "b1"), ("W1b", "b1b"))[:self.n_out]):
                    new[wn], new[bn] = douts[k][idx].t() @ h1[idx].clamp_min(0), douts[k][idx].sum(0)
        for k, v in new.items():
            v = v.reshape(grads[k].shape)
            grads[k].copy_(v if self.bug == "assign" else grads[k] + v)
        seen = list(new)
        if self.bug == "gradmax_misses_one" and seen:
            seen.remove(max(seen, key=lambda k: float(grads[k].abs().max())))
        out["gradmax"] = max([float(grads[k].abs().max()) for k in seen] + [0.0])
        return out


def td_standin(q, qn1, reward, done, gamma, bug=None):
    """rpo_td in float32 torch: (dq [n], loss_partial [ceil(n / 16)])."""
    n = q.numel()
    g = torch.tensor(gamma, dtype=torch.float32)
    d = q - (reward + g * (1.0 - done) * qn1)
    if bug == "strict_clamp":                                    # d where |d| < 1, the sign where |d| > 1: nothing AT 1
        dq = (d * (d.abs() < 1) + torch.sign(d) * (d.abs() > 1)) / n
    else:
        dq = d.clamp(-1.0, 1.0) / n
    hub = torch.where(d.abs() < 1, 0.5 * d * d, d.abs() - 0.5)
    parts = []
    for t0 in range(0, n, 16):
        rows = hub[t0:t0 + 16]
        parts.append(rows.sum() / (rows.numel() if bug == "tile_mean" else n))
    return dq, torch.stack(parts)


def _standin_case(name, n, bug=None, form="full"):
    """One forward + backward of the stand-in through the checker of the GPU tests (pre-filled gradients, planted
    activations, gradmax); raises AssertionError where the checker objects."""
    spec = mlp_f64.NET_BY_NAME[name]
    _, kind, S, A, E, n_out, hd = spec
    params = mlp_f64.make_params(spec, seed=len(name) + n)
    net = mlp_f64.mlp64_of(spec, params)
    st = StandIn(spec, params, bug)
    s, a, _ = mlp_f64.make_inputs(spec, n, seed=n)
    out, x0, h1 = st.forward(s, a)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(h1).all())     # (the 1e30 row stays finite in float32)
    worst = {}
    mlp_f64.check_forward(net, s, a, out, x0, h1, worst, "%s n=%d" % (name, n))
    # backward on unplanted inputs (a 1e30 row would drown every batch sum's bound) with planted +-0 / denormal activations
    s, a, _ = mlp_f64.make_inputs(spec, n, seed=n + 1, planted=False)
    _, x0, h1 = StandIn(spec, params).forward(s, a)
    x0, h1 = mlp_f64.plant_activations(x0.clone(), h1.clone(), seed=n)
    g = torch.Generator().manual_seed(n)
    dout = torch.randn(n, n_out * hd, generator=g) / n
    pre = {k: torch.randn(v.shape, generator=g) * 0.01 for k, v in params.items()}
    grads = {k: v.clone() for k, v in pre.items()}
    state_only = form == "state_only"
    got = st.backward(s, a, x0, h1, dout, grads, state_only=state_only)
    got.update(grads)
    tag = "%s n=%d %s +=" % (name, n, form)
    written = mlp_f64.check_backward(net, s, a, x0, h1, dout, got, pre, worst, tag, state_only=state_only)
    assert got["gradmax"] == mlp_f64.gradmax_of(written), (tag, "gradmax")
    return worst


@pytest.mark.parametrize("n", [17, 257])
@pytest.mark.parametrize("name", [t[0] for t in mlp_f64.NETWORKS])
def test_float32_cpu_standin_passes_the_small_n_checker(name, n):
    worst = _standin_case(name, n)
    mlp_f64.report("stand-in %s n=%d" % (name, n), worst)
    assert 0.0 < max(worst.values()) <= 1.0


MUTATIONS = [("mask_ge", "add_6_2", "full"), ("last_row_dropped", "add_6_2", "full"), ("last_row_twice", "add_6_2", "full"),
             ("bias_twice", "add_6_2", "full"), ("heads_swapped", "gauss_5", "full"), ("row_major_head", "gauss14", "full"),
             ("assign", "add_6_2", "full"), ("state_only_writes_wa", "add_6_2", "state_only"),
             ("gradmax_misses_one", "add_6_2", "full")]


@pytest.mark.parametrize("bug,name,form", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_seeded_mutations_fail_the_small_n_checker(bug, name, form):
    _standin_case(name, 17, form=form)                           # (the same case passes without the mutation)
    with pytest.raises(AssertionError):
        _standin_case(name, 17, bug=bug, form=form)


def _td_case(n, bug=None):
    """TD prologue of the stand-in through the bounds of mlp_f64.td / td_partials, with rows planted at |q - y| exactly 1 and
    a few ulps either side."""
    g = torch.Generator().manual_seed(n)
    q, qn1, reward = (torch.randn(n, generator=g) for _ in range(3))
    done = (torch.rand(n, generator=g) > 0.7).float()
    gamma = 0.5                                                  # (exact in float32: y = reward + 0.5 qn1 can be hit exactly)
    rows = mlp_f64.plant_td_kink(q, qn1, reward, done, gamma)
    dq, parts = td_standin(q, qn1, reward, done, gamma, bug)
    dq_r, dq_b, _, _, d = mlp_f64.td(q, qn1, reward, done, gamma)
    assert bool((d[rows[:2]].abs() == 1.0).all())                # the planted rows sit exactly on the kink
    assert float(((dq.double() - dq_r).abs() / dq_b).max()) <= 1.0
    p_r, p_b = mlp_f64.td_partials(q, qn1, reward, done, gamma)
    assert parts.numel() == p_r.numel() and float(((parts.double() - p_r).abs() / p_b).max()) <= 1.0


@pytest.mark.parametrize("n", [1, 17, 256])
def test_td_standin_passes(n):
    _td_case(n)


@pytest.mark.parametrize("bug", ["strict_clamp", "tile_mean"])
def test_td_mutations_fail(bug):
    with pytest.raises(AssertionError):
        _td_case(17, bug)


def test_box_forward_yardstick():
    """C_REF_BOX_FWD of tests/heads_f64.py, recomputed: a float32 CPU evaluation of scale tanh(o) + base against float64 in units
    of eps32 * magnitude sum over the yardstick rows and the three boxes (fails on a drift beyond 2x either way)."""
    import heads_f64
    o = heads_f64.box_fwd_rows()
    worst = 0.0
    for b in heads_f64.BOXES.values():
        ref = b.scale * torch.tanh(o.double()) + b.base
        got = torch.tensor(b.scale) * torch.tanh(o) + torch.tensor(b.base)
        mag = heads_f64.tanh_box_fwd_mags(o, b.scale, b.base)
        worst = max(worst, float(((got.double() - ref).abs() / (heads_f64.EPS32 * mag + heads_f64.TINY)).max()))
        _, allowed = mlp_f64.box_out(o, b.scale, b.base)
        assert bool(((got.double() - ref).abs() <= allowed).all())
    print("box forward yardstick: %.3f (C_REF_BOX_FWD %.2f)" % (worst, heads_f64.C_REF_BOX_FWD))
    assert heads_f64.C_REF_BOX_FWD / 2 <= worst <= heads_f64.C_REF_BOX_FWD
