"""The opt-in 3 x bf16 split-precision form of the streaming forward (csrc/mlp_stream_bf16x3.h; ops.tuning(fwd_bf16x3=1)).

The split form is f32-accurate but deliberately NOT bit-equal to the exact-f32 form, so it is held to the float64 yardstick of
tests/mlp_f64.py with the derived bound gamma_L |A||B| per layer (test_large_batch_f64_gpu._check_forward, from the kernel's own
input to each layer), to the exact kernel's own measured error (<= 2 x: the criterion of VERDICT r06 "next round" 1), and to
bit-equality where it must not differ: the first layer (x0), and every launch the switch does not cover.
Outputs are NaN-filled before every call: an element the kernel never writes fails.
"""
import math

import pytest
import torch

import mlp_f64
import test_large_batch_f64_gpu as lb                            # (the module, not its names: its tests are not collected twice)
from rpo_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
SIZES = [12288, 12301, 65589]    # the smallest streaming size (all tiles full) / a ragged last tile / more tiles than waves on the chip
NETS = {"critic_add": ("add", 6, 2), "actor_gauss": ("gauss", 6, 0), "critic_pendulum": ("add", 3, 1)}
_NETS = {}


def _net(name, seed=20):
    if (name, seed) not in _NETS:
        _NETS[(name, seed)] = lb.Net(*NETS[name], seed)
    return _NETS[(name, seed)]


def _bufs(net, n, save="both"):
    """NaN-filled (out, x0, h1); a buffer that is not saved is None."""
    out, x0, h1 = (lb._aligned(n * w).view(n, w).fill_(NAN) for w in (net.n_out, net.desc.ein, net.H))
    return out, (x0 if save == "both" else None), (h1 if save in ("both", "h1") else None)


def _forward(net, s, a, n, save="both", split=1, **tune):
    out, x0, h1 = _bufs(net, n, save)
    with ops.tuning(fwd_bf16x3=split, **tune):
        ops.mlp_forward(net.desc, s, a, out, x0, h1)
    torch.cuda.synchronize()
    return out, x0, h1


# ------------------------------------------------------------------------------------------------- 1. float64, derived bound
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", list(NETS))
def test_split_forward_matches_float64(name, n):
    """Every row of out, x0, h1 under the switch within gamma_L |A||B| of float64; the three save modes (both saved: the
    compile-time tiles; none; only h1: the run-time tile) compute the same bits, so the modes that do not return x0 / h1 are
    checked through the ones of the mode that does."""
    net = _net(name)
    s, a = lb._inputs(n, net.S, net.A, 100)
    worst = {}
    out, x0, h1 = _forward(net, s, a, n, "both")
    lb._check_forward(net, s, a, out, x0, h1, worst, "both")
    out_n, _, _ = _forward(net, s, a, n, "none")
    lb._check_forward(net, s, a, out_n, x0, h1, worst, "none")
    assert torch.equal(out_n, out)
    out_h, _, h1_h = _forward(net, s, a, n, "h1")
    lb._check_forward(net, s, a, out_h, x0, h1_h, worst, "h1only")
    assert torch.equal(out_h, out) and torch.equal(h1_h, h1)
    lb._report("bf16x3 forward %s n=%d" % (name, n), worst)


@pytest.mark.parametrize("n", SIZES[1:])
@pytest.mark.parametrize("count", [2, 4])
def test_split_forward_multi_matches_float64(count, n):
    """mlp_forward_multi (gridDim.y = network) with 2 and 4 networks on their own inputs."""
    nets = [_net("critic_add", 20 + k) for k in range(count)]
    calls = []
    for k, net in enumerate(nets):
        s, a = lb._inputs(n, net.S, net.A, 100 + k)
        calls.append((net, s, a) + _bufs(net, n))
    with ops.tuning(fwd_bf16x3=1):
        ops.mlp_forward_multi([(c[0].desc,) + c[1:] for c in calls])
    torch.cuda.synchronize()
    worst = {}
    for k, (net, s, a, out, x0, h1) in enumerate(calls):
        lb._check_forward(net, s, a, out, x0, h1, worst, "net%d" % k)
    lb._report("bf16x3 forward multi%d n=%d" % (count, n), worst)


def test_split_forward_ignores_fwd_stream_waves():
    """The split kernel is instantiated for 12 waves only (16 spill): both values of fwd_stream_waves launch it -- same bits,
    within the bound."""
    n = SIZES[1]
    net = _net("critic_add")
    s, a = lb._inputs(n, net.S, net.A, 100)
    got = {w: _forward(net, s, a, n, fwd_stream_waves=w) for w in (12, 16)}
    worst = {}
    lb._check_forward(net, s, a, *got[16], worst, "waves16")
    assert all(torch.equal(x, y) for x, y in zip(got[12], got[16]))


# ------------------------------------------------------------------------- 2. the new kernel ran, and only where it should
def test_split_kernel_runs_where_the_switch_covers_and_nowhere_else():
    n = SIZES[1]
    net = _net("critic_add")
    s, a = lb._inputs(n, net.S, net.A, 100)
    before = _forward(net, s, a, n, split=0)
    got = _forward(net, s, a, n, split=1)
    after = _forward(net, s, a, n, split=0)
    assert all(torch.equal(x, y) for x, y in zip(before, after))            # switch back at 0: the exact form's bits
    assert torch.equal(got[1], before[1])                                    # x0: the first layer is the exact form's
    assert not torch.equal(got[2], before[2])                                # h1: another arithmetic
    assert bool(torch.isfinite(got[2]).all())
    # a misaligned x0 buffer keeps the row-tile kernels, n = 12 287 is below the streaming size: the switch changes nothing
    res = {}
    for split in (0, 1):
        out, _, h1 = _bufs(net, n)
        x0 = lb._aligned(n * 128 + 4)[1:1 + n * 128].view(n, 128).fill_(NAN)
        assert x0.data_ptr() % 16 == 4
        with ops.tuning(fwd_bf16x3=split):
            ops.mlp_forward(net.desc, s, a, out, x0, h1)
        torch.cuda.synchronize()
        res[split] = (out, x0, h1)
    assert all(torch.equal(x, y) for x, y in zip(res[0], res[1])) and bool(torch.isfinite(res[1][2]).all())
    m = 12287
    small = {split: _forward(net, s[:m], a[:m], m, split=split) for split in (0, 1)}
    assert all(torch.equal(x, y) for x, y in zip(small[0], small[1])) and bool(torch.isfinite(small[1][2]).all())


# --------------------------------------------------------------------------------- 3. accuracy against the exact form
def _h1_error(net, x0, h1):
    ref, absval, _ = net.ref.hidden(x0)
    err = (h1.to(torch.float64) - ref).abs()
    return math.sqrt(float((err * err).mean())), float((err / absval).max())


def test_split_error_is_within_twice_the_exact_kernels():
    """VERDICT r06 item 1's kill criterion on the add critic at 65 589 rows: RMS error of h1 and max |err| / (|A||B|), both
    against Mlp64.hidden(x0) of the form's own (bit-equal) x0: split <= 2 x exact.  The baseline is the exact kernel.

    Measured on an MI355X at this size: exact RMS 5.553e-8, max 3.404e-7; split RMS 3.225e-8, max 1.594e-7."""
    n = SIZES[2]
    net = _net("critic_add")
    s, a = lb._inputs(n, net.S, net.A, 100)
    fig = {}
    for split in (0, 1):
        _, x0, h1 = _forward(net, s, a, n, split=split)
        assert bool(torch.isfinite(h1).all())
        fig[split] = _h1_error(net, x0, h1)
    print("h1 error vs float64, n=%d: exact rms %.4g max/|A||B| %.4g; bf16x3 rms %.4g max/|A||B| %.4g (u = %.3g)"
          % (n, fig[0][0], fig[0][1], fig[1][0], fig[1][1], mlp_f64.U))
    assert fig[1][0] <= 2.0 * fig[0][0], ("rms", fig)
    assert fig[1][1] <= 2.0 * fig[0][1], ("max", fig)


# ------------------------------------------------------------------------------ 4. values that break a careless split
def _edited_net(seed, edit):
    """A fresh add critic whose parameters `edit(tensors)` changed in place, with a float64 twin of the changed values."""
    net = lb.Net("add", 6, 2, seed)
    with torch.no_grad():
        edit(net.desc.tensors)
    net.ref = mlp_f64.Mlp64(net.desc.tensors, net.S, net.A, net.E, net.H, net.n_out, False, device=DEV)
    return net


@pytest.mark.parametrize("power", [40, -40])
def test_split_survives_scaled_operands(power):
    """Both operands of the hidden layer scaled by 2^40 / 2^-40 (x0 through the inputs and the first-layer biases, exactly; W0,
    and b0 by the product's 2^80 so that the products still matter): within the bound."""
    n, k = SIZES[1], 2.0 ** power

    def edit(t):
        for name in ("bs", "ba", "W0"):
            t[name].mul_(k)
        t["b0"].mul_(k * k)
    net = _edited_net(31, edit)
    s, a = lb._inputs(n, net.S, net.A, 100)
    s, a = s * k, a * k
    worst = {}
    lb._check_forward(net, s, a, *_forward(net, s, a, n), worst, "scaled 2^%d" % power)
    lb._report("bf16x3 scaled 2^%d" % power, worst)


def test_split_keeps_3e38_times_1e_38_finite():
    """x0[row 7][e = 5] = 3e38 exactly (one-hot first-layer row, zero biases) against W0[:, 5] = 1e-38: a hi plane rounded up
    would be infinite; truncation keeps h1 finite and within the bound."""
    n, e, r = SIZES[1], 5, 7

    def edit(t):
        t["Ws"][:, 0] = 0.0
        t["Ws"][e, :] = 0.0
        t["Ws"][e, 0] = 1.0
        t["Wa"][e, :] = 0.0
        t["bs"][e] = 0.0
        t["ba"][e] = 0.0
        t["W0"][:, e] = 1e-38
    net = _edited_net(32, edit)
    s, a = lb._inputs(n, net.S, net.A, 100)
    s = s.clone()
    s[r, 0] = 3e38
    out, x0, h1 = _forward(net, s, a, n)
    assert float(x0[r, e]) == float(torch.tensor(3e38, dtype=torch.float32))
    assert bool(torch.isfinite(h1).all()) and bool(torch.isfinite(out).all())
    worst = {}
    lb._check_forward(net, s, a, out, x0, h1, worst, "3e38")
    lb._report("bf16x3 3e38 x 1e-38", worst)


def test_split_propagates_nan_and_inf_like_the_exact_form():
    """A NaN in one W0 entry: exactly that hidden column of h1 is non-finite, in every row.  An input of +Inf: that row of h1
    and its output are non-finite, no other row is."""
    n, j, r = SIZES[1], 77, 12300

    def edit(t):
        t["W0"][j, 33] = NAN
    net = _edited_net(33, edit)
    s, a = lb._inputs(n, net.S, net.A, 100)
    _, _, h1 = _forward(net, s, a, n)
    bad = ~torch.isfinite(h1)
    assert bool(bad[:, j].all()) and int(bad.sum()) == n
    net = _net("critic_add")
    s = s.clone()
    s[r, 0] = float("inf")
    _, _, h1 = _forward(net, s, a, n)
    bad = ~torch.isfinite(h1)
    assert bool(bad[r].all()) and int(bad.sum()) == net.H


# ------------------------------------------------------------------------------------------------------ 5. whole update
@pytest.mark.parametrize("algo,lanes,batch", [("ddpg", 4096, 2 ** 20), ("sac", 256, 65536)], ids=["ddpg_2e20", "sac_65536"])
def test_large_batch_critic_update_matches_float64_under_the_switch(algo, lanes, batch):
    """The existing whole-update check, unchanged, with every streaming forward of the trainer in the split form: its bounds
    come from the kernel's own saved activations and already allow an f32 forward error on the targets."""
    with ops.tuning(fwd_bf16x3=1):
        lb.test_large_batch_critic_update_matches_float64(algo, lanes, batch)


def test_large_batch_trainer_runs_in_graph_windows_under_the_switch(monkeypatch):
    """bench.py's large_batch configuration (RPODDPG, CartSafe-v0, 4096 lanes, one 2^20-row batch per step) for 32 iterations
    through hipGraph windows captured under the switch: finite parameters, no failure flag."""
    import bench
    from rpo_amd import _lib
    monkeypatch.setenv("RPO_VERBOSE", "0")
    monkeypatch.setenv("RPO_GRAPH_CYCLE", "4")
    with ops.tuning(fwd_bf16x3=1):
        tr = bench.make_trainer(4096, torch.device("cuda:0"), 10 ** 9, capacity=64, workload="cart_ddpg", batch_size=256 * 4096)
        tr.vec.reset()
        tr.run_steps(32)
        tr._harvest(final=True)
        torch.cuda.synchronize()
    assert tr._large_batch and any(e["graph"] is not None for e in tr._graphs.entries.values()) and not tr._graphs.capture_failed
    assert int(tr.vec.ctrl[_lib.CONST["RPO_CTRL_NONFINITE"]]) == 0
    assert bool(torch.isfinite(tr.agent.flat.data).all()) and bool(torch.isfinite(tr.agent.critic_target_flat).all())
