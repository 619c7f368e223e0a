"""The large-batch MLP kernels against a float64 restatement of the same mathematics (tests/mlp_f64.py).

The kernels are exact-f32 fmaf / MFMA chains and bitwise reproducible, so a fixed-seed comparison with a DERIVED bound cannot
flake: |got - ref| <= gamma_L |A| |B| (mlp_f64.bound), where |A| |B| is the reference expression evaluated on absolute values
and L the longest chain of float32 roundings an element passes through:
  * forward layers: K products + the bias (mlp_f64: first layer S + A + 3, hidden Ein + 1, heads H + 1), from the kernel's own
    float32 input to the layer;
  * parameter gradients: the chain inside a row (dh: the heads' products; dx0: + H; one more for the product that meets the
    batch sum; mlp_f64.Mlp64.backward) plus the batch reduction of the path, from the kernel's plan (``batch_chain``);
  * da / dx0: per row, no batch chain.
Outputs are NaN and scratch is NaN before every call: an element a kernel never writes fails.  One-hot probes (dout = e_r)
isolate a row, which catches what a float64 bound cannot resolve at 2^20 rows: a tile dropped or counted twice, a slice
boundary off by one, a padded row that reads the clamped row n - 1 and contributes.
"""
import numpy as np
import pytest
import torch

import mlp_f64
from rpo_amd.algo.model import ActionEmbedding, GaussianSharedPolicy, SharedValueAdd, SharedValueCat, StateEmbedding

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
SPLITK_FROM = 16384
BIG = 2 ** 20 + 13


# ------------------------------------------------------------------------------------------------------------------ plumbing
def _aligned(numel):
    buf = torch.zeros(numel + 8, device=DEV)
    off = (-buf.data_ptr() // 4) % 4
    return buf[off:off + numel]


class Net(object):
    """One network on the GPU: parameters 16-byte aligned, every gradient inside ONE flat buffer (like agent/flat.py, each
    tensor at a multiple of 4 floats), its ``MlpDesc`` and its float64 twin."""

    def __init__(self, kind, S, A, seed):
        from rpo_amd import ops
        torch.manual_seed(seed)
        E = 256 if kind == "cat" else 128
        H = 256
        se = StateEmbedding(S, E, H)
        if kind == "gauss":
            m = GaussianSharedPolicy(S, 1, se, E, H, 1, None)
            t = dict(W1=m.affine_mean.weight, b1=m.affine_mean.bias, W1b=m.affine_log_std.weight, b1b=m.affine_log_std.bias)
        else:
            m = (SharedValueCat if kind == "cat" else SharedValueAdd)(S, A, se, ActionEmbedding(A, E, H), E, H)
            t = dict(Wa=m.action_embed.embeds[0].weight, ba=m.action_embed.embeds[0].bias, W1=m.affines[1].weight,
                     b1=m.affines[1].bias)
        t.update(Ws=se.embeds[0].weight, bs=se.embeds[0].bias, W0=m.affines[0].weight, b0=m.affines[0].bias)
        for p in m.parameters():
            v = _aligned(p.numel()).view(p.shape)
            v.copy_(p.data)
            p.data = v
        self.total = sum((p.numel() + 3) // 4 * 4 for p in m.parameters())
        self.flat = _aligned(self.total)
        off, self.used = 0, torch.zeros(self.total, dtype=torch.bool, device=DEV)
        for p in m.parameters():
            p.grad = self.flat[off:off + p.numel()].view(p.shape)
            self.used[off:off + p.numel()] = True
            off += (p.numel() + 3) // 4 * 4
        self.module, self.kind, self.S, self.A, self.E, self.H = m, kind, S, A, E, H
        self.n_out = 2 if kind == "gauss" else 1
        self.desc = ops.MlpDesc(t, S, A, E, H, self.n_out, kind == "cat")
        self.ref = mlp_f64.Mlp64(t, S, A, E, H, self.n_out, kind == "cat", device=DEV)
        self.tensors = {k: v for k, v in self.desc.tensors.items() if v is not None}
        # the span splitk_plan addresses: first to last gradient element, its slice stride rounded up to 4 floats
        lo = min(v.grad.data_ptr() for v in self.tensors.values())
        hi = max(v.grad.data_ptr() + 4 * v.numel() for v in self.tensors.values())
        self.span = (hi - lo) // 4
        self.stride = (self.span + 3) // 4 * 4

    def grad(self, k):
        return self.tensors[k].grad


def plan_z(n, net, scratch_floats):
    """splitk_plan (csrc/mlp_bwd.h): Z = min(256, n / 512), cut to what the scratch holds; < 2 (or no scratch, or n <
    RPO_SPLITK_FROM): no split, the one-owner pass."""
    if scratch_floats is None or n < SPLITK_FROM:
        return 0
    z = min(256, n // 512)
    if z * net.stride > scratch_floats:
        z = scratch_floats // net.stride
    return z if z >= 2 else 0


def batch_chain(n, z):
    """Longest chain of additions a parameter-gradient element sees over the batch.
    One-owner pass (z = 0): n rows + 16 (the 16 row phases of the first-layer sums, mlp_bwd.h) + 4.
    Split-K: a slice holds <= 16 ceil(ceil(n / 16) / z) rows (the streaming / one-pass kernels split 16-row tiles as t_lo =
    tiles z / Z; the split-K weights pass rows n z / Z rounded down to 4: never more, + 4), + 16 row phases inside a slice,
    + z for splitk_reduce (four quarters of ceil(z / 4) slices in order, then three adds), + 4 (the += onto the gradient)."""
    if z < 2:
        return n + 20
    tiles = (n + 15) // 16
    return 16 * (-(-tiles // z)) + 4 + 16 + z + 4


def _slice_edges(n, z):
    """Rows at the slice boundaries of both split forms (tile-based t_lo = tiles z / Z, row-based (n z / Z) & ~3)."""
    if z < 2:
        return []
    tiles = (n + 15) // 16
    rows = []
    for lo_of in (lambda q: 16 * (tiles * q // z), lambda q: (n * q // z) & ~3):
        rows += [lo_of(1) - 1, lo_of(1), lo_of(z - 1)]
    return rows


def probe_rows(n, z):
    return sorted({r for r in [0, 15, 16, n - 16, n - 1] + _slice_edges(n, z) if 0 <= r < n})


def _check(what, got, ref, absval, L, worst):
    got = got.to(torch.float64).reshape(ref.shape)
    assert bool(torch.isfinite(got).all()), "%s: non-finite (never written?)" % what
    r = mlp_f64.ratio(got, ref, absval, L)
    key = ("probe " if " probe " in what else "+= " if " += " in what else "") + what.split()[-1]
    worst[key] = max(worst.get(key, 0.0), r)
    assert r <= 1.0, "%s: |got - ref| is %.3g x the bound gamma_%d |A||B|" % (what, r, L)


def _report(tag, worst):
    print("%s: worst |err| / bound %s" % (tag, ", ".join("%s %.3g" % (k, v) for k, v in sorted(worst.items()))))


def _inputs(n, S, A, seed):
    """s / a as strided column views of one wider batch matrix (the trainer's gathered rows)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    wide = torch.randn(n, S + A + 3, device=DEV, generator=g)
    return wide[:, 1:1 + S], (wide[:, 1 + S:1 + S + A] if A else None)


# ------------------------------------------------------------------------------------------------------------------- forward
FWD_SIZES = [12287, 12288, 20011, 131071, BIG]
FWD_PATHS = {"tile64": dict(fwd_stream=0), "stream16": dict(fwd_stream=1, fwd_stream_waves=16),
             "stream12": dict(fwd_stream=1, fwd_stream_waves=12), "multi2": dict(), "multi4": dict(), "gemm_cat": dict()}


def _check_forward(net, s, a, out, x0, h1, worst, tag):
    x0r, x0a, L0 = net.ref.first_layer(s, a)
    _check(tag + " x0", x0, x0r, x0a, L0, worst)
    h1r, h1a, L1 = net.ref.hidden(x0)
    _check(tag + " h1", h1, h1r, h1a, L1, worst)
    outr, outa, L2 = net.ref.head(h1)
    _check(tag + " out", out, outr, outa, L2, worst)


@pytest.mark.parametrize("n", FWD_SIZES)
@pytest.mark.parametrize("path", list(FWD_PATHS))
def test_forward_matches_float64(path, n):
    """Every row of out, x0 and h1 of the large-n forward paths against float64, layer by layer from the kernel's own input to
    each layer: the 64-row tiles, the streaming kernel with 16 and 12 waves, forward_multi with 2 and 4 networks, the
    layer-by-layer path of the 256-wide networks."""
    from rpo_amd import ops
    worst = {}
    if path == "gemm_cat":
        nets = [Net("cat", 57, 43, 11)]
    else:
        nets = [Net("add", 6, 2, 20 + k) for k in range(4 if path == "multi4" else 2 if path == "multi2" else 1)]
    calls = []
    for k, net in enumerate(nets):
        s, a = _inputs(n, net.S, net.A, 100 + k)
        bufs = [_aligned(n * w).view(n, w).fill_(NAN) for w in (net.n_out, net.desc.ein, net.H)]
        calls.append((net, s, a, *bufs))
    with ops.tuning(**FWD_PATHS[path]):
        if path.startswith("multi"):
            ops.mlp_forward_multi([(c[0].desc,) + c[1:] for c in calls])
        else:
            net, s, a, out, x0, h1 = calls[0]
            ops.mlp_forward(net.desc, s, a, out, x0, h1)
    torch.cuda.synchronize()
    for k, (net, s, a, out, x0, h1) in enumerate(calls):
        _check_forward(net, s, a, out, x0, h1, worst, "net%d" % k)
    _report("forward %s n=%d" % (path, n), worst)


def test_float64_reference_spot_checks_on_the_host():
    """The GPU float64 reference does not rest on a GPU BLAS alone: a few of its elements recomputed with numpy on the host."""
    n = 16385
    net = Net("add", 6, 2, 5)
    s, a = _inputs(n, 6, 2, 6)
    x0r = net.ref.first_layer(s, a)[0]
    h1r = net.ref.hidden(x0r)[0]
    dout = torch.randn(n, 1, device=DEV, dtype=torch.float64) / n
    res = net.ref.backward(s, a, x0r, h1r, dout)
    P = {k: v.cpu().numpy() for k, v in net.ref.p.items() if v is not None}
    sh, ah, dh_ = s.double().cpu().numpy(), a.double().cpu().numpy(), dout.cpu().numpy()
    x0h = sh @ P["Ws"].T + P["bs"] + ah @ P["Wa"].T + P["ba"]
    h1h = np.maximum(x0h, 0) @ P["W0"].T + P["b0"]
    dh = (dh_ @ P["W1"]) * (h1h > 0)
    dx0 = (dh @ P["W0"]) * (x0h > 0)
    for r in (0, 7777, n - 1):
        np.testing.assert_allclose(h1r[r].cpu().numpy(), h1h[r], rtol=1e-11, atol=1e-13)
    for j, e in ((0, 0), (100, 57), (255, 127)):
        np.testing.assert_allclose(res["W0"][0][j, e].item(), dh[:, j] @ np.maximum(x0h[:, e], 0), rtol=1e-9, atol=1e-15)
    for e, i in ((0, 0), (77, 5)):
        np.testing.assert_allclose(res["Ws"][0][e, i].item(), dx0[:, e] @ sh[:, i], rtol=1e-9, atol=1e-15)
    np.testing.assert_allclose(res["da"][0][n - 1].cpu().numpy(), dx0[n - 1] @ P["Wa"], rtol=1e-10, atol=1e-15)


# ------------------------------------------------------------------------------------------------------------------ backward
BWD_PATHS = {"stream": dict(bwd_stream=1), "onepass": dict(bwd_stream=0, bwd_onepass=1),
             "splitk": dict(bwd_stream=0, bwd_onepass=0), "plain": dict(), "pair_own": dict(), "pair_shared": dict()}
FORMS = ("params", "td_ddpg", "td_sac", "da", "da_fl", "gauss")
_CACHE = {}


def _setup(n, form, pair):
    """Networks, inputs and the KERNEL's forward (its x0 / h1 are the backward's inputs), cached per size."""
    kind = "gauss" if form == "gauss" else "add"
    key = (n, kind)
    if key not in _CACHE:
        from rpo_amd import ops
        if any(k[0] != n for k in _CACHE):                       # (one size at a time on the device)
            _CACHE.clear()
            torch.cuda.empty_cache()
        S, A = (6, 0) if kind == "gauss" else (6, 2)
        nets = [Net(kind, S, A, 40 + k) for k in range(2)]
        s, a = _inputs(n, S, A, 7)
        fw = []
        for net in nets:
            out, x0, h1 = (_aligned(n * w).view(n, w) for w in (net.n_out, net.E, net.H))
            ops.mlp_forward(net.desc, s, a, out, x0, h1)
            fw.append((out, x0, h1))
        g = torch.Generator(device=DEV).manual_seed(n)
        dout = [torch.randn(n, net.n_out, device=DEV, generator=g) / n for net in nets]
        wide = torch.randn(n, 4, device=DEV, generator=g)
        td_in = dict(qn1=torch.randn(n, device=DEV, generator=g), qn2=torch.randn(n, device=DEV, generator=g),
                     logp=torch.randn(n, device=DEV, generator=g), reward=wide[:, 1:2], done=(wide[:, 2:3] > 0.8).float())
        _CACHE[key] = (nets, s, a, fw, dout, td_in)
    nets, s, a, fw, dout, td_in = _CACHE[key]
    return (nets if pair else nets[:1]), s, a, fw, dout, td_in


class Call(object):
    """One rpo_mlp_backward / _pair call of a form: fresh NaN outputs and scratch, zeroed gradients."""

    def __init__(self, nets, s, a, fw, form, path, n, td_in, scratch_floats=None):
        self.nets, self.s, self.a, self.fw, self.form, self.path, self.n = nets, s, a, fw, form, path, n
        self.td_in = td_in
        self.pair = len(nets) == 2
        self.param_grads = form != "da"
        self.fl = form == "da_fl"
        self.want_da = form in ("da", "da_fl")
        self.td = form.startswith("td")
        full = max(2, min(256, n // 512)) * nets[0].stride
        floats = scratch_floats if scratch_floats is not None else full
        if path == "plain":
            for net in nets:
                net.desc.splitk = None
        elif path == "pair_shared":
            shared = _aligned(floats)
            for net in nets:
                net.desc.splitk = shared
        else:
            for net in nets:
                net.desc.splitk = _aligned(floats)
        # the plan the kernels take: a scratch shared by both networks of a pair keeps the one-owner weights pass (csrc/mlp.hip)
        self.z = 0 if path in ("plain", "pair_shared") or not self.param_grads else \
            plan_z(n, nets[0], None if nets[0].desc.splitk is None else nets[0].desc.splitk.numel())
        self.tuning = BWD_PATHS.get(path, {})

    def run(self, douts, zero=True, gm=None):
        from rpo_amd import ops
        n, H = self.n, self.nets[0].H
        args = []
        self.da, self.dq, self.parts = [], [], []
        for k, net in enumerate(self.nets):
            if net.desc.splitk is not None:
                net.desc.splitk.fill_(NAN)                          # (garbage: the launch zeroes what it uses)
            if zero:
                net.flat.zero_()
            out, x0, h1 = self.fw[k]
            dh = torch.full((n, H), NAN, device=DEV)
            dx0 = torch.full((n, net.desc.ein), NAN, device=DEV)
            da = torch.full((n, net.A), NAN, device=DEV) if self.want_da else None
            td = None
            if self.td:
                ti = self.td_in
                dq = torch.full((n,), NAN, device=DEV)
                parts = torch.full(((n + 15) // 16,), NAN, device=DEV)
                sac = self.form == "td_sac"
                td = ops.Td(out.view(-1), ti["qn1"], ti["qn2"] if sac else None, ti["logp"] if sac else None, ti["reward"],
                            ti["done"], 0.2 if sac else 0.0, 0.99, dq, parts)
                self.dq.append(dq)
                self.parts.append(parts)
            self.da.append(da)
            args.append((x0, h1, None if self.td else douts[k], dh, dx0, da, td))
        with ops.tuning(**self.tuning):
            if self.pair:
                (x1, h1_, d1, dh1, dx1, da1, t1), (x2, h2, d2, dh2, dx2, da2, t2) = args
                ops.mlp_backward_pair(self.nets[0].desc, self.nets[1].desc, self.s, self.a, x1, h1_, d1, dh1, dx1, da1,
                                      x2, h2, d2, dh2, dx2, da2, param_grads=self.param_grads,
                                      first_layer_state_only=self.fl, gradmax=gm, td1=t1, td2=t2)
            else:
                x0, h1, d, dh, dx0, da, td = args[0]
                ops.mlp_backward(self.nets[0].desc, self.s, self.a, x0, h1, d, dh, dx0, da, param_grads=self.param_grads,
                                 first_layer_state_only=self.fl, gradmax=gm, td=td)
        torch.cuda.synchronize()

    def check_grads(self, k, res, rows, worst, tag, scale=1.0, extra=0):
        """Every parameter gradient of network k against `res` (mlp_f64 backward) times `scale`; the ones this form does not
        write, and the padding floats between tensors, exactly zero."""
        net = self.nets[k]
        # one row (probe): every other row adds exact zeros; + 1 for the add onto the zeroed gradient
        chain = 1 if rows == 1 else batch_chain(self.n, self.z)
        for name in net.tensors:
            got = net.grad(name)
            if self.param_grads and name in res:
                ref, absval, L = res[name]
                _check("%s net%d %s" % (tag, k, name), got, scale * ref, scale * absval, L + chain + extra, worst)
            else:
                assert float(got.abs().max()) == 0.0, "%s net%d %s written by a form that does not ask for it" % (tag, k, name)
        assert int(torch.count_nonzero(net.flat[~net.used])) == 0, "%s net%d: padding floats of the flat gradient written" % (tag, k)


def _ref(net, s, a, fw, dout, call, rows=None):
    out, x0, h1 = fw
    if rows is not None:
        s, x0, h1, dout = s[rows], x0[rows], h1[rows], dout[rows]
        a = None if a is None else a[rows]
    return net.ref.backward(s, a, x0, h1, dout, param_grads=call.param_grads, first_layer_state_only=call.fl)


def _backward_case(path, form, n, scratch_floats=None, full_matrix=True):
    nets, s, a, fw, dout, td_in = _setup(n, form, path.startswith("pair"))
    call = Call(nets, s, a, fw, form, path, n, td_in, scratch_floats=scratch_floats)
    worst = {}
    tag = "%s/%s/n=%d/Z=%d" % (path, form, n, call.z)
    gm = torch.zeros(512, device=DEV) if call.param_grads else None
    refs = []
    if full_matrix:
        call.run(dout, gm=gm)
        for k, net in enumerate(nets):
            d_eff = dout[k]
            if call.td:
                # TD / Huber prologue: dq and the summed loss shares against float64; the backward then from the kernel's dq
                dq_r, dq_b, loss_r, loss_b, _ = mlp_f64.td(fw[k][0], td_in["qn1"], td_in["reward"], td_in["done"], 0.99,
                                                           td_in["qn2"] if form == "td_sac" else None,
                                                           td_in["logp"] if form == "td_sac" else None,
                                                           0.2 if form == "td_sac" else 0.0)
                dq = call.dq[k].double()
                assert bool(torch.isfinite(dq).all()) and bool(torch.isfinite(call.parts[k]).all()), tag
                r = float(((dq - dq_r).abs() / dq_b).max())
                worst["dq"] = max(worst.get("dq", 0.0), r)
                assert r <= 1.0, (tag, "dq", r)
                loss = float(call.parts[k].double().sum())
                assert abs(loss - loss_r) <= loss_b, (tag, "loss", loss, loss_r, loss_b)
                worst["loss"] = max(worst.get("loss", 0.0), abs(loss - loss_r) / loss_b)
                d_eff = call.dq[k].view(n, 1)
            res = _ref(net, s, a, fw[k], d_eff, call)
            refs.append((res, d_eff))
            if call.want_da:
                ref, absval, L = res["da"]
                _check("%s net%d da" % (tag, k), call.da[k], ref, absval, L, worst)
            if not (path == "plain" and n > 2 * SPLITK_FROM and call.param_grads):
                # (the one-owner pass at 2^20 rows: a chain of n -- the bound says little there; the probes below pin it)
                call.check_grads(k, res, n, worst, tag)
        if call.param_grads:
            written = max(float(net.flat.abs().max()) for net in nets)
            assert float(gm.max()) == written, (tag, "gradmax", float(gm.max()), written)
            # += onto the existing gradients: twice the reference, one more rounding
            call.run(dout, zero=False)
            for k, net in enumerate(nets):
                if not (path == "plain" and n > 2 * SPLITK_FROM):
                    call.check_grads(k, refs[k][0], n, worst, tag + " +=", scale=2.0, extra=1)
    if not call.td:
        # one-hot probes: dout = e_r * dout[r].  Every other row contributes exact zeros (0 x finite, x + 0), so each gradient is
        # row r's own float32 chain: the in-row L of mlp_f64 (a few roundings for dW0 / db0 / dW1 / db1, + H for the
        # first-layer gradients and da through dx0[r]) and one add onto the zeroed gradient instead of a batch chain
        for r in probe_rows(n, call.z if call.z else plan_z(n, nets[0], 256 * nets[0].stride)):
            one = []
            for k in range(len(nets)):
                d = torch.zeros_like(dout[k])
                d[r] = dout[k][r]
                one.append(d)
            call.run(one)
            for k, net in enumerate(nets):
                res = _ref(net, s, a, fw[k], dout[k], call, rows=slice(r, r + 1))
                call.check_grads(k, res, 1, worst, "%s probe r=%d" % (tag, r))
                if call.want_da:
                    ref, absval, L = res["da"]
                    _check("%s probe r=%d net%d da" % (tag, r, k), call.da[k][r:r + 1], ref, absval, L, worst)
                    other = call.da[k].clone()
                    other[r] = 0.0
                    assert int(torch.count_nonzero(other)) == 0, "%s: da written on rows other than the probe %d" % (tag, r)
    _report(tag, worst)


PATH_FORM = [(p, f) for p in BWD_PATHS for f in FORMS]


@pytest.mark.parametrize("path,form", PATH_FORM, ids=["%s-%s" % pf for pf in PATH_FORM])
@pytest.mark.parametrize("n", [16385, BIG])
def test_backward_paths_and_forms_match_float64(path, form, n):
    """Every backward path (streaming, one-pass, rows + split-K, the one-owner pass, the twin-critic pair with its own and with
    one shared scratch) in every form (all parameter gradients, TD prologue DDPG / SAC, da alone, da with the state part of
    the first layer, the Gaussian two-head actor) at the RPO_SPLITK_FROM edge and at 2^20 + 13 rows."""
    _backward_case(path, form, n)


@pytest.mark.parametrize("n", [16383, 16384, 16385, 40007, 131071, 131072, 2 ** 20, BIG])
def test_default_backward_sizes_match_float64(n):
    """The default path of the critic update across the sizes where the plan changes: below / at / above RPO_SPLITK_FROM,
    Z = 78, the 256-slice cap (n >= 131 072), the bench's 2^20 rows and a ragged last tile."""
    _backward_case("default", "params", n)


@pytest.mark.parametrize("scratch", ["fewer", "two", "one"])
@pytest.mark.parametrize("n", [131072, BIG])
def test_default_backward_scratch_sizes_match_float64(scratch, n):
    """Scratch buffers that hold fewer slices than planned, exactly 2 slices, and 1 slice (no split: the one-owner pass)."""
    nets = _setup(n, "params", False)[0]
    stride = nets[0].stride
    floats = {"fewer": 100 * stride + 3, "two": 2 * stride + 3, "one": stride + 3}[scratch]
    _backward_case("default", "params", n, scratch_floats=floats, full_matrix=not (scratch == "one" and n > 2 * SPLITK_FROM))


def test_misaligned_splitk_scratch_is_refused():
    """A split-K scratch that is not 16-byte aligned is refused (RPO_ERR_ARG), not zeroed with a memset."""
    from rpo_amd import _lib, ops
    n = 16385
    nets, s, a, fw, dout, _ = _setup(n, "params", False)
    net = nets[0]
    buf = _aligned(plan_z(n, net, 10 ** 9) * net.stride + 4)
    net.desc.splitk = buf[1:]
    out, x0, h1 = fw[0]
    with pytest.raises(_lib.RpoHipError):
        ops.mlp_backward(net.desc, s, a, x0, h1, dout[0], torch.empty(n, 256, device=DEV), torch.empty(n, 128, device=DEV))
    net.desc.splitk = None


# ------------------------------------------------------------------------------------------------ one trainer critic update
def _critic_tensors(m, k=""):
    se, ae, aff = getattr(m, "state_embed" + k), getattr(m, "action_embed" + k), getattr(m, "affines" + k)
    assert len(se.embeds) == 1 and len(ae.embeds) == 1 and len(aff) == 2
    return dict(Ws=se.embeds[0].weight, bs=se.embeds[0].bias, Wa=ae.embeds[0].weight, ba=ae.embeds[0].bias,
                W0=aff[0].weight, b0=aff[0].bias, W1=aff[1].weight, b1=aff[1].bias)


def _desc_z(desc, n):
    """Z of splitk_plan for a trainer descriptor and its enable_splitk scratch."""
    grads = [t.grad for t in desc.tensors.values() if t is not None]
    lo = min(g.data_ptr() for g in grads)
    hi = max(g.data_ptr() + 4 * g.numel() for g in grads)
    stride = ((hi - lo) // 4 + 3) // 4 * 4
    if desc.splitk is None or n < SPLITK_FROM:
        return 0
    z = min(256, n // 512)
    if z * stride > desc.splitk.numel():
        z = desc.splitk.numel() // stride
    return z if z >= 2 else 0


@pytest.mark.parametrize("algo,lanes,batch", [("ddpg", 4096, 2 ** 20), ("sac", 256, 65536)], ids=["ddpg_2e20", "sac_65536"])
def test_large_batch_critic_update_matches_float64(algo, lanes, batch):
    """One eager large-batch critic update of the trainer (its own _sample and _critic_update, after a few iterations fill the
    ring) against a float64 restatement of the TD / Huber critic loss on the batch it sampled: the critic's slice of
    agent.flat.grad (read through FlatParams' offsets) and last_losses["critic"].  bench.py's `large_batch` configuration
    (RPODDPG, CartSafe, 4096 lanes, 2^20 rows) and RPOSAC on CartSafe at 65 536 rows (twin critics through
    rpo_mlp_backward_pair).  This pins the plumbing the kernel tests above do not see: the column split of the batch, gamma,
    the 1 / B scaling, which saved activations feed the backward, the flat-gradient offsets with enable_splitk's scratch.

    Reference: the target values from float64 critic-target networks at the trainer's own next actions (and, for SAC, the
    kernel's log pi), with the float32 forward's error bound (Mlp64.forward_bound) carried into the TD error (mlp_f64.td
    qn_err); the critic's own q and the activations its backward reads from a separate forward launch of the trainer's
    critic descriptor (the kernel's values: layer-local, no mask can flip).  Gradient bound: gamma_(L + batch chain of the
    trainer's split-K plan) |A||B| with the float64 dq, plus |A||B| evaluated with the dq bound as dout (the gradients are
    linear in dq)."""
    from rpo_amd import ops
    from test_train_step_golden import build_trainer
    dev = torch.device("cuda")
    torch.manual_seed(5)
    tr = build_trainer(algo, "cart", ops, dev, fused=True, num_envs=lanes, use_graph=False, batch_size=batch, capacity=32)
    tr.vec.reset()
    tr.run_steps(6)                                              # (fills the ring; every step also updates)
    torch.cuda.synchronize()
    ag, f, fl = tr.agent, tr.fused, tr.agent.flat
    assert tr._large_batch and not tr._pipelines
    rec = {}
    project = tr._project_batch

    def _project(state, ap):                                     # (the critic update projects once: the next actions)
        rec["next_actions"] = project(state, ap).clone()
        return rec["next_actions"]
    tr._project_batch = _project
    if algo == "sac":
        gauss = tr._gauss

        def _gauss(obs, eps, tag, **kw):
            out = gauss(obs, eps, tag, **kw)
            if tag == "crit":
                rec["logp"] = out[1].clone()
            return out
        tr._gauss = _gauss
    cols = tr._sample()
    state, action, next_state, reward, done = (c.clone() for c in cols[:5])
    fl.grad.zero_()
    tr._critic_update(cols)
    torch.cuda.synchronize()
    del tr._project_batch
    if algo == "sac":
        del tr._gauss
    nxt = rec["next_actions"]
    assert nxt.shape[0] == batch
    gamma = ag.gamma
    names = [("critic", "critic_target", "")] if algo == "ddpg" else [("critic1", "critic_target1", "1"),
                                                                        ("critic2", "critic_target2", "2")]
    # float64 targets at the trainer's next actions, each with its float32 forward bound
    qn, qn_err = [], []
    for _, tname, k in names:
        tdesc = f.descs[tname]
        t64 = mlp_f64.Mlp64(_critic_tensors(ag.critic_target, k), tdesc.S, tdesc.A, tdesc.E, tdesc.H, device=dev)
        out, absval, L = t64.forward_bound(next_state, nxt)
        qn.append(out.view(-1))
        qn_err.append(mlp_f64.bound(absval, L).view(-1))
    err_min = torch.maximum(qn_err[0], qn_err[-1])                  # (min(qn1, qn2): 1-Lipschitz in each)
    worst, loss_ref, loss_b = {}, 0.0, 0.0
    parts = tr.last_losses["critic"].parts
    parts = parts.view(len(names), -1)
    for i, (cname, _, k) in enumerate(names):
        d = f.descs[cname]
        assert d.A == action.shape[1]
        q = torch.full((batch, 1), NAN, device=DEV)
        x0 = torch.full((batch, d.ein), NAN, device=DEV)
        h1 = torch.full((batch, d.H), NAN, device=DEV)
        ops.mlp_forward(d, state, action, q, x0, h1)              # the critic's forward: bitwise the trainer's (one kernel)
        sac = algo == "sac"
        dq, dq_b, lo, lo_b, _ = mlp_f64.td(q, qn[0], reward, done, gamma, qn[1] if sac else None, rec["logp"] if sac else None,
                                           float(ag.alpha) if sac else 0.0, qn_err=err_min)
        loss_ref += lo
        loss_b += lo_b
        got_loss = float(parts[i].double().sum())
        assert abs(got_loss - lo) <= lo_b, (cname, got_loss, lo, lo_b)
        worst["loss"] = max(worst.get("loss", 0.0), abs(got_loss - lo) / lo_b)
        c64 = mlp_f64.Mlp64(_critic_tensors(ag.critic, k), d.S, d.A, d.E, d.H, device=dev)
        res = c64.backward(state, action, x0, h1, dq.view(-1, 1))
        res_b = c64.backward(state, action, x0, h1, dq_b.view(-1, 1))
        chain = batch_chain(batch, _desc_z(d, batch))
        for name, p in _critic_tensors(ag.critic, k).items():
            off = fl.offset[id(p)]
            got = fl.grad[off:off + p.numel()].view(p.shape).double()
            ref, absval, L = res[name]
            allowed = mlp_f64.bound(absval, L + chain) + res_b[name][1] * (1.0 + (L + chain) * mlp_f64.U * 2)
            assert bool(torch.isfinite(got).all()), (cname, name)
            r = float(((got - ref).abs() / allowed).max())
            worst[name] = max(worst.get(name, 0.0), r)
            assert r <= 1.0, "%s %s: |got - ref| is %.3g x the bound" % (cname, name, r)
    # last_losses["critic"] sums the float32 shares with torch: gamma_(number of shares) of their |.| on top
    m = parts.numel()
    got = float(tr.last_losses["critic"])
    allowed = loss_b + float(mlp_f64.bound(parts.double().abs().sum(), m))
    assert abs(got - loss_ref) <= allowed, (got, loss_ref, allowed)
    worst["last_losses"] = abs(got - loss_ref) / allowed
    _report("critic update %s B=%d" % (algo, batch), worst)
