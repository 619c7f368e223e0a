"""The float64 yardstick of the policy-head kernel tests (tests/heads_f64.py): its gradients against finite differences of its
own forward, its agreement with the float32 torch modules (rpo_amd/algo/model), and the measurement of C_REF_* -- how far a
float32 evaluation of the same formulas lands from float64, in units of eps32 * magnitude sum.  CPU only."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import heads_f64 as hf
from rpo_amd.algo.model import BoxConstraint, GaussianSharedPolicy, SharedPolicy

DLOGP = 0.01
N_RANDOM = 4099 - hf.N_EDGE


def _inputs(seed=0):
    m, r, e, edge = hf.rows(4099, seed)
    return m, r, e, edge, hf.gradient_weights(4099, seed)


@pytest.mark.parametrize("box", list(hf.BOXES.values()), ids=str)
def test_reference_gradients_match_finite_differences(box):
    """Central differences of the float64 forward on the random rows, away from the masks (the clamp of the log-std head and the
    clip of ap are kinks: rows within the step of one are left out) and out of deep saturation (where the quotient of two
    differences of the size of 1e-16 says nothing)."""
    m, r, e, edge, dap = _inputs()
    m, r, e, dap = (torch.from_numpy(v[~edge]).double() for v in (m, r, e, dap))
    args = (box.scale, box.base, box.lo, box.hi)
    ref = hf.gauss_head(m, r, e, *args, dap=dap, dlogp=DLOGP)
    h = 1e-6

    def f(mm, rr):
        o = hf.gauss_head(mm, rr, e, *args)
        return dap * o["ap"] + DLOGP * o["logp"]
    fd_mean = (f(m + h, r) - f(m - h, r)) / (2 * h)
    fd_ls = (f(m, r + h) - f(m, r - h)) / (2 * h)
    ls = r - 3
    x = m + e * ls.clamp(hf.LS_MIN, hf.LS_MAX).exp()
    a = box.scale * torch.tanh(x) + box.base
    keep = ((ls - hf.LS_MIN).abs() > 1e-3) & ((ls - hf.LS_MAX).abs() > 1e-3) & (x.abs() < 6) \
        & ((a - box.lo).abs() > 1e-4 * box.scale) & ((a - box.hi).abs() > 1e-4 * box.scale)
    assert int(keep.sum()) > 0.7 * N_RANDOM
    scale = 1 + ref["g_mean"].abs() + ref["g_ls"].abs()
    assert float(((fd_mean - ref["g_mean"]).abs() / scale)[keep].max()) < 1e-6
    assert float(((fd_ls - ref["g_ls"]).abs() / scale)[keep].max()) < 1e-6
    assert bool((ref["g_ls"][(ls > hf.LS_MAX) | (ls < hf.LS_MIN)] == 0).all()) and bool((ls > hf.LS_MAX).any())
    # the deterministic head with noise and clip
    o, noise = (torch.from_numpy(v).double() for v in hf.box_rows(box, 2000))
    dap = torch.from_numpy(hf.gradient_weights(2000, 1)).double()
    eps_t = 0.5 * box.scale
    t = hf.tanh_box(o, noise, eps_t, *args, dap=dap)
    fd = (dap * (hf.tanh_box(o + h, noise, eps_t, *args)["ap"] - hf.tanh_box(o - h, noise, eps_t, *args)["ap"])) / (2 * h)
    keep = ~hf.near_seam(t["pre"], box.lo, box.hi, 1e-4)
    clipped = (t["pre"] < box.lo) | (t["pre"] > box.hi)
    assert 0.05 < float(clipped.double().mean()) < 0.95
    assert float((fd - t["g"]).abs()[keep].max()) < 1e-6 and bool((t["g"][clipped] == 0).all())


def _gauss_module(box):
    """GaussianSharedPolicy whose two heads return given raw values: the input row is (mean+, mean-, ls+, ls-) >= 0 (the ReLU in
    front of the heads is the identity there) and the heads subtract the halves -- exact, one half is zero."""
    bc = BoxConstraint(np.array([box.lo], np.float32), np.array([box.hi], np.float32), "cpu")
    bc.scale_torch, bc.base_torch = torch.tensor([box.scale]), torch.tensor([box.base])      # (the offset box's own scale / base)
    net = GaussianSharedPolicy(4, 1, nn.Identity(), 4, hidden_dim=4, hidden_layer=1, box_constraint=bc)
    net.affines = nn.ModuleList()
    with torch.no_grad():
        net.affine_mean.weight.copy_(torch.tensor([[1.0, -1.0, 0.0, 0.0]]))
        net.affine_log_std.weight.copy_(torch.tensor([[0.0, 0.0, 1.0, -1.0]]))
        net.affine_mean.bias.zero_()
        net.affine_log_std.bias.zero_()
    kept = {}
    for name in ("affine_mean", "affine_log_std"):
        getattr(net, name).register_forward_hook(lambda mod, inp, out, name=name: (out.retain_grad(), kept.__setitem__(name, out))[0])
    return net, bc, kept


@pytest.mark.parametrize("box", list(hf.BOXES.values()), ids=str)
def test_reference_matches_the_float32_modules(box):
    """GaussianSharedPolicy (+ the clip of take_action) and SharedPolicy's tanh + BoxConstraint (+ noise + clip) in float32, same
    draw, on the rows with raw_ls - 3 >= -10.  Tolerance: MARGIN * C_REF_* * eps32 * magnitude sum as for the kernels, plus --
    the modules write log_prob as Normal.log_prob does -- MARGIN * eps32 * hf.module_cancel for the cancellation of x - mean."""
    m, r, e, edge, dap = _inputs()
    yard = hf.yard_mask(r)
    m, r, e, dap = (torch.from_numpy(v[yard]) for v in (m, r, e, dap))
    args = (box.scale, box.base, box.lo, box.hi)
    net, bc, kept = _gauss_module(box)
    s = torch.stack([m.clamp_min(0), (-m).clamp_min(0), r.clamp_min(0), (-r).clamp_min(0)], 1)
    x, logp, _ = net(s, eps=e[:, None])
    ap = bc.clip(x)
    (dap[:, None] * ap + DLOGP * logp).sum().backward()
    ref = hf.gauss_head(m, r, e, *args, dap=dap, dlogp=DLOGP)
    mag = hf.gauss_mags(m, r, e, box.scale, box.base, dap=dap, dlogp=DLOGP)
    extra = hf.module_cancel(m, r, e, DLOGP)
    got = dict(ap=ap.detach()[:, 0], logp=logp.detach()[:, 0], g_mean=kept["affine_mean"].grad[:, 0],
               g_ls=kept["affine_log_std"].grad[:, 0])
    cref = dict(ap=hf.C_REF_AP, logp=hf.C_REF_LOGP, g_mean=hf.C_REF_G_MEAN, g_ls=hf.C_REF_G_LS)
    for k in ("ap", "logp", "g_mean", "g_ls"):
        bound = cref[k] * mag[k] + extra.get(k, 0.0)
        assert hf.worst(got[k], ref[k], bound) <= hf.MARGIN, k
    # deterministic actor head: SharedPolicy ends in box(tanh(.)); its MLP is replaced by the identity the same way
    pol = SharedPolicy(2, 1, nn.Identity(), 2, hidden_dim=2, hidden_layer=1, box_constraint=bc)
    pol.affines = nn.ModuleList([nn.Linear(2, 1)])
    with torch.no_grad():
        pol.affines[0].weight.copy_(torch.tensor([[1.0, -1.0]]))
        pol.affines[0].bias.zero_()
    o, noise = (torch.from_numpy(v) for v in hf.box_rows(box, 2000))
    dap = torch.from_numpy(hf.gradient_weights(2000, 1))
    eps_t = hf.f32(0.5 * box.scale)
    raw = torch.zeros(0)

    def keep_raw(mod, inp, out):
        out.retain_grad()
        nonlocal raw
        raw = out
    h = pol.affines[0].register_forward_hook(keep_raw)
    pre = pol(torch.stack([o.clamp_min(0), (-o).clamp_min(0)], 1))
    h.remove()
    act = bc.clip(pre + eps_t * noise[:, None])                   # PDDDPG_PA.take_action, agent/ddpg_pa.py:108-110
    (dap[:, None] * act).sum().backward()
    t = hf.tanh_box(o, noise, eps_t, *args, dap=dap)
    keep = ~hf.near_seam(t["pre"], box.lo, box.hi)
    assert float(keep.double().mean()) > 0.99
    assert hf.worst(raw.grad[:, 0][keep], t["g"][keep], hf.C_REF_BOX_BWD * hf.tanh_box_mags(o, box.scale, dap)[keep]) <= hf.MARGIN


def measure_c_ref():
    """C_REF_* as heads_f64.py defines them: float32 torch-CPU evaluation of the helper's formulas against float64 over the three
    boxes; returns (dict, share of the random rows measured, number of edge rows measured)."""
    m, r, e, edge, dap = _inputs()
    yard = hf.yard_mask(r)
    c = dict(ap=0.0, logp=0.0, g_mean=0.0, g_ls=0.0, box_bwd=0.0)
    mt, rt, et, dt = (torch.from_numpy(v[yard]) for v in (m, r, e, dap))
    for box in hf.BOXES.values():
        args = (box.scale, box.base, box.lo, box.hi)
        for dlogp in (DLOGP, 0.0):
            for det in ((False, True) if dlogp == 0.0 else (False,)):
                ref = hf.gauss_head(mt, rt, et, *args, dap=dt, dlogp=dlogp, deterministic=det)
                got = hf.gauss_head(mt, rt, et, *args, dap=dt, dlogp=dlogp, deterministic=det, dtype=torch.float32)
                mag = hf.gauss_mags(mt, rt, et, box.scale, box.base, dap=dt, dlogp=dlogp, deterministic=det)
                for k in ("ap", "logp", "g_mean", "g_ls"):
                    c[k] = max(c[k], hf.worst(got[k], ref[k], mag[k]))
        o, noise = (torch.from_numpy(v) for v in hf.box_rows(box, 2000))
        db = torch.from_numpy(hf.gradient_weights(2000, 1))
        for nz in (None, noise):
            eps_t = hf.f32(0.5 * box.scale)
            ref = hf.tanh_box(o, nz, eps_t, *args, dap=db)
            got = hf.tanh_box(o, nz, eps_t, *args, dap=db, dtype=torch.float32)
            keep = ~hf.near_seam(ref["pre"], box.lo, box.hi)
            c["box_bwd"] = max(c["box_bwd"], hf.worst(got["g"][keep], ref["g"][keep], hf.tanh_box_mags(o, box.scale, db)[keep]))
    return c, float(yard[~edge].mean()), int(yard[edge].sum())


def test_yardstick():
    c, random_share, n_edge = measure_c_ref()
    print("measured C_REF:", c)
    raw, ls = hf.ls_edges()
    assert all(np.isfinite(v) and v > 0 for v in c.values()), c
    assert random_share >= 0.99
    assert n_edge == len(hf.MEANS) * int((ls >= hf.YARD_LS).sum()) * len(hf.DRAWS)      # every edge row with raw_ls - 3 >= -10
    const = dict(ap=hf.C_REF_AP, logp=hf.C_REF_LOGP, g_mean=hf.C_REF_G_MEAN, g_ls=hf.C_REF_G_LS, box_bwd=hf.C_REF_BOX_BWD)
    for k, v in c.items():
        assert const[k] / 2 <= v <= const[k] * 2, (k, v, const[k])


def test_edge_inputs_are_what_they_claim():
    raw, ls = hf.ls_edges()
    assert list(ls[[1, 6]]) == [-23.0, -2.0] and ls[2] < -23.0 < ls[3] and ls[7] < -2.0 < ls[8]
    assert np.float32(np.tanh(9.5)) == 1.0 and np.float32(np.tanh(3.0)) < 1.0      # correctly rounded, y is 1 at 9.5
    for box in hf.BOXES.values():
        for eps_t in (0.5, 0.125):
            ap_det, noise, target, inside = hf.clip_mask_rows(box, eps_t)
            assert list(inside) == [True, True, False, True, True, False]
    m, r, e, edge = hf.rows(4099)
    assert int(edge.sum()) == hf.N_EDGE == len(set(zip(m[edge].tolist(), r[edge].tolist(), e[edge].tolist())))
    for n in (1, 255, 256, 257):
        assert all(len(v) == n for v in hf.rows(n))
    # the TD restatement against torch's own smooth_l1_loss + autograd
    g = torch.Generator().manual_seed(3)
    q1, q2, qn1, qn2, logp, rew = (2 * torch.randn(300, generator=g) for _ in range(6))
    done = (torch.rand(300, generator=g) > 0.7).float()
    t = hf.td_huber(q1, qn1, rew, done, 0.95, q2=q2, qn2=qn2, logp=logp, alpha=0.2)
    a, b = q1.double().requires_grad_(), q2.double().requires_grad_()
    y = rew.double() + hf.f32(0.95) * (1 - done.double()) * (torch.minimum(qn1, qn2).double() - hf.f32(0.2) * logp.double())
    loss = torch.nn.functional.smooth_l1_loss(a, y) + torch.nn.functional.smooth_l1_loss(b, y)
    loss.backward()
    assert abs(t["loss"] - float(loss.detach())) < 1e-12
    torch.testing.assert_close(t["g1"], a.grad, rtol=1e-12, atol=1e-15)
    torch.testing.assert_close(t["g2"], b.grad, rtol=1e-12, atol=1e-15)
