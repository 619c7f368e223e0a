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
