"""The small-batch MLP kernels -- what rpo_mlp_forward, rpo_mlp_forward_multi, rpo_mlp_backward and rpo_mlp_backward_pair run
below the large-batch thresholds -- against the float64 restatement of tests/mlp_f64.py, row by row and at their edges:
the 16-row tile forward (mlp_tile.h), the multi-output forward (mlp_forward_wide_kernel), the layer-by-layer path of the
256-wide networks (mlp_gemm.h), mlp_forward_multi_kernel, the two-pass backward with one owner per element
(mlp_bwd_rows_kernel(2), mlp_bwd_weights_kernel(2), gemm_backward_rows) and the TD prologue.

Every element of out, x0, h1, dx0, da and of every parameter gradient is judged with mlp_f64.ratio <= 1 against the derived
bound gamma_L |A||B| (no measured constant), layer-local from the kernel's own float32 input to each layer:
  * forward chains: first layer S (+ A) + 1 .. 3, hidden Ein + 1, heads H + 1 (mlp_f64.Mlp64);
  * parameter gradients: the chain inside a row (Mlp64.backward) + the batch chain of the path + 1 for the += onto the
    pre-filled gradient.  Batch chain (mlp_f64.batch_chain): every small-n path gives an element ONE owner that adds the rows
    of a partition of the batch in a fixed order and then the partials in a fixed order -- mlp_bwd_weights_body: 4 wave
    partials of k-steps of 4 rows (dW0), of contiguous quarters (db0 / dW1 / db1), 16 or 4 slices (first layer, scalar role),
    4 wave partials of k-steps (first layer of the 256-wide networks on the matrix cores), 16 slices per 256-row pass (multi-
    output heads), 8 slices (their db1) -- so at most n - 1 + 16 additions whatever the order: n + 20 covers all of them, the
    one-owner figure of tests/test_large_batch_f64_gpu.py;
  * the rows launches of the layer-by-layer path (gemm_backward_rows) and its k-split are per-row k chains in another order:
    the bound holds for any order, no new chain;
  * out_mode 1: 4 c_ref eps32 (magnitude sum) with c_ref the float32-CPU constant of tests/heads_f64.py (C_REF_BOX_FWD).
Outputs are NaN before each call; every input and output is a view into a larger allocation -- guard rows of inputs hold NaN
(a padded lane that reads past row n - 1 and lets it contribute shows), guard rows of outputs a sentinel bit pattern that must
survive; inputs are strided column views of a wider matrix; gradient buffers are pre-filled with random values and the padding
between them must survive.  One-hot probes (dout zero except row r) hold every parameter gradient to ONE row's bound.

NaN contract (include/rpo_hip.h, rpo_mlp_forward): a NaN pre-activation of either sign stays NaN through the relu and reaches
the row's output, in every forward form; every other row keeps its bits.  inf * 0 in a dead first-layer column is NaN.
"""
import pytest
import torch

import heads_f64
import mlp_f64 as M

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
G = 4                       # guard rows (16-byte multiples for every width: the aligned paths stay the ones taken)
PAD = 8                     # guard floats around the flat gradient buffer
SENT = 0x4B5AA5A5           # sentinel bit pattern of output guards and gradient padding (a finite float)
SIZES = [1, 15, 16, 17, 255, 256, 257]
GEMM_SIZES = [63, 64, 65]   # kGemmCols = 64
ONCE = 1000                 # once per kernel family
GEMM_LIMIT = 16384          # gemm_path_ok: n <= 16384
NAMES = [t[0] for t in M.NETWORKS]


def _ops():
    from rpo_amd import ops
    return ops


def _sync():
    if DEV == "cuda":
        torch.cuda.synchronize()


def _bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and bool(torch.equal(_bits(a), _bits(b)))


def same_bits_or_nan(a, b):
    """Bitwise equal where neither is NaN, NaN in the same places (a NaN's payload is not part of any contract)."""
    na, nb = torch.isnan(a), torch.isnan(b)
    return bool(torch.equal(na, nb)) and bool(torch.equal(_bits(torch.where(na, 0.0, a)), _bits(torch.where(nb, 0.0, b))))


class Out(object):
    """An [n, w] output inside a larger allocation: NaN body, G sentinel guard rows before and after."""

    def __init__(self, n, w):
        self.n = n
        self.full = torch.empty(n + 2 * G, w, device=DEV)
        self.full.view(torch.int32).fill_(SENT)
        self.t = self.full[G:G + n]
        self.t.fill_(NAN)

    def intact(self):
        i = self.full.view(torch.int32)
        return bool((i[:G] == SENT).all()) and bool((i[G + self.n:] == SENT).all())


def guarded_input(t):
    """A contiguous copy of t [n, w] with G rows of NaN before and after."""
    full = torch.full((t.shape[0] + 2 * G,) + tuple(t.shape[1:]), NAN, device=DEV)
    full[G:G + t.shape[0]] = t
    return full[G:G + t.shape[0]]


class Net(object):
    """One network of mlp_f64.NETWORKS on the device: parameters 16-byte aligned in one flat buffer, every gradient inside ONE
    flat buffer (each tensor at a multiple of 4 floats, sentinel padding between and around them), its MlpDesc, its float64
    twin."""

    def __init__(self, name, seed):
        self.spec = spec = M.NET_BY_NAME[name]
        self.name, self.kind, self.S, self.A, self.E, self.n_out, self.hd = spec
        self.ein = self.E * (2 if self.kind == "cat" else 1)
        self.outs = self.n_out * self.hd
        host = M.make_params(spec, seed)
        size = {k: (v.numel() + 3) // 4 * 4 for k, v in host.items()}
        total = sum(size.values())
        self.pbuf = torch.zeros(total, device=DEV)
        self.gfull = torch.empty(total + 2 * PAD, device=DEV)
        self.gbuf = self.gfull[PAD:PAD + total]
        self.used = torch.zeros(total + 2 * PAD, dtype=torch.bool, device=DEV)
        self.t, off = {}, 0
        for k, v in host.items():
            p = self.pbuf[off:off + v.numel()].view(v.shape)
            p.copy_(v)
            p.grad = self.gbuf[off:off + v.numel()].view(v.shape)
            self.used[PAD + off:PAD + off + v.numel()] = True
            self.t[k] = p
            off += size[k]
        self.desc = _ops().MlpDesc(self.t, self.S, self.A, self.E, M.H, self.n_out, self.kind == "cat", head_dim=self.hd)
        self.ref = M.mlp64_of(spec, self.t, device=DEV)
        self.gemm = self.E == 256                                 # the layer-by-layer path applies (x0 / h1 given, n <= 16384)
        self.l1_mfma = self.E == 128 and self.kind != "cat" and self.S <= 6 and self.A <= 4

    def prefill(self, seed, zero=False):
        """Random values (or zeros) into every gradient, the sentinel into the padding; returns {name: copy}."""
        self.gfull.view(torch.int32).fill_(SENT)
        g = torch.Generator().manual_seed(seed)
        for p in self.t.values():
            p.grad.copy_(torch.zeros(p.shape) if zero else 0.01 * torch.randn(p.shape, generator=g))
        return {k: p.grad.clone() for k, p in self.t.items()}

    def grads(self):
        return {k: p.grad for k, p in self.t.items()}

    def padding_intact(self):
        return bool((self.gfull.view(torch.int32)[~self.used] == SENT).all())


def forward(net, s, a, n, save=True, tune=None, **mode):
    """One rpo_mlp_forward into fresh NaN outputs with guards: (out, x0, h1) tensors (x0 / h1 None when not saved)."""
    ops = _ops()
    out, x0, h1 = Out(n, net.outs), Out(n, net.ein), Out(n, M.H)
    with ops.tuning(**(tune or {})):
        ops.mlp_forward(net.desc, s, a, out.t, x0.t if save else None, h1.t if save else None, **mode)
    _sync()
    assert out.intact() and x0.intact() and h1.intact(), "%s n=%d: an output guard row was written" % (net.name, n)
    if not save:
        assert bool(torch.isnan(x0.t).all()) and bool(torch.isnan(h1.t).all())
    return out.t, (x0.t if save else None), (h1.t if save else None)


def forward_sizes(net):
    sizes = list(SIZES) + (GEMM_SIZES if net.gemm else [])
    if net.name in ("add_6_2", "wide14", "cat_57_43", "actor14"):
        sizes.append(ONCE)
    if net.name == "cat_57_43":
        sizes += [GEMM_LIMIT, GEMM_LIMIT + 1]
    return sizes


# ------------------------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("name", NAMES)
def test_forward_matches_float64(name):
    """Every row of out, x0 and h1 at every row count, on planted inputs (a 1e30 row, a 1e-38 row, a zero row, a dead
    first-layer column): the row-tile / multi-output kernel, with the first layer on the vector ALU where the matrix-core
    form applies (bitwise equal), unsaved (bitwise equal outputs), and for the 256-wide networks the layer-by-layer path with
    and without the k split beside the row tile."""
    net = Net(name, 11)
    worst = {}
    for n in forward_sizes(net):
        s, a, _ = M.make_inputs(net.spec, n, seed=n, device=DEV)
        tag = "%s n=%d" % (name, n)
        tile = forward(net, s, a, n, tune=dict(mlp_gemm=0))
        M.check_forward(net.ref, s, a, *tile, worst, tag + " tile")
        assert float(tile[1][:, M.ZERO_COL].abs().max()) == 0.0, tag + ": the dead column of x0 is not exactly 0"
        if n >= 4:
            assert float(tile[0][1].abs().max()) > 1e20 and float(tile[1][3].abs().max()) <= 2.0    # (the planted rows arrived)
        unsaved = forward(net, s, a, n, save=False)
        assert same_bits(unsaved[0], tile[0]), tag + ": saved and unsaved outputs differ"
        if net.l1_mfma:
            vec = forward(net, s, a, n, tune=dict(l1_mfma=0))
            assert all(same_bits(x, y) for x, y in zip(vec, tile)), tag + ": l1_mfma 0 / 1 differ"
        if net.gemm and n <= GEMM_LIMIT:
            for ks in (1, 0):
                got = forward(net, s, a, n, tune=dict(gemm_ksplit=ks))
                M.check_forward(net.ref, s, a, *got, worst, tag + " gemm%d" % ks)
        elif net.gemm:
            got = forward(net, s, a, n)                           # above the limit the default IS the row tile
            assert all(same_bits(x, y) for x, y in zip(got, tile)), tag
    M.report("forward %s" % name, worst)


@pytest.mark.parametrize("box", ["wide", "unit", "offset"])
@pytest.mark.parametrize("name", ["actor_6", "actor_1", "gauss_5", "add256_6_2"])
def test_forward_tanh_box_matches_float64(name, box):
    """out_mode 1 against the float64 map scale tanh(o) + base from the kernel's own o (recomputed with out_mode 0; x0 / h1
    bitwise the same in both launches), symmetric and offset boxes; a second head is not mapped."""
    net = Net(name, 12)
    net.t["W1"].mul_(16.0)                                        # (|o| up to a few units: both tails of tanh)
    b = heads_f64.BOXES[box]
    worst = {}
    for n in (1, 17, 257):
        s, a, _ = M.make_inputs(net.spec, n, seed=n, device=DEV, planted=False)
        raw = forward(net, s, a, n, tune=dict(mlp_gemm=0))
        got = forward(net, s, a, n, out_mode=1, scale=b.scale, base=b.base)
        assert same_bits(got[1], raw[1]) and same_bits(got[2], raw[2])
        ref, allowed = M.box_out(raw[0][:, 0], b.scale, b.base)
        M.check("%s %s n=%d ap" % (name, box, n), got[0][:, 0], ref, None, 0, worst, allowed=allowed)
        if net.n_out > 1:
            assert same_bits(got[0][:, 1], raw[0][:, 1])
        unsaved = forward(net, s, a, n, save=False, out_mode=1, scale=b.scale, base=b.base)
        assert same_bits(unsaved[0], got[0])
    M.report("tanh box %s %s" % (name, box), worst)


@pytest.mark.parametrize("count", [1, 2, 3, 4])
@pytest.mark.parametrize("name", ["add_6_2", "gauss_5", "cat_57_43", "gauss256_5"])
def test_forward_multi_matches_float64_and_single_launches(name, count):
    """rpo_mlp_forward_multi with 1..4 networks, each on its own inputs: all saved (the 256-wide shapes then run layer by
    layer: 4 concatenating critics / 4 two-head policies are exactly kGemmProblems problems) and with x0_save / h1_save partly NULL (row tile);
    every network against float64 and bitwise equal to its single launch."""
    ops = _ops()
    nets = [Net(name, 20 + k) for k in range(count)]
    worst = {}
    for n in [1, 17, 256, 257] + ([ONCE] if name == "add_6_2" and count == 4 else []):
        ins = [M.make_inputs(net.spec, n, seed=100 * k + n, device=DEV) for k, net in enumerate(nets)]
        for partly in (False, True):
            saves = [not partly or k % 2 == 1 for k in range(count)]
            tile = partly or not nets[0].gemm                     # (one NULL keeps every network on the row tile)
            bufs = [(Out(n, net.outs), Out(n, net.ein), Out(n, M.H)) for net in nets]
            ops.mlp_forward_multi([(net.desc, ins[k][0], ins[k][1], bufs[k][0].t, bufs[k][1].t if saves[k] else None,
                                    bufs[k][2].t if saves[k] else None) for k, net in enumerate(nets)])
            _sync()
            for k, net in enumerate(nets):
                tag = "%s x%d n=%d net%d%s" % (name, count, n, k, " partly" if partly else "")
                assert all(o.intact() for o in bufs[k]), tag + ": guard rows"
                one = forward(net, ins[k][0], ins[k][1], n, tune=dict(mlp_gemm=0) if tile else None)
                M.check_forward(net.ref, ins[k][0], ins[k][1], *one, worst, tag)
                assert same_bits(bufs[k][0].t, one[0]), tag + ": out differs from the single launch"
                if saves[k]:
                    assert same_bits(bufs[k][1].t, one[1]) and same_bits(bufs[k][2].t, one[2]), tag + ": x0 / h1"
                else:
                    assert bool(torch.isnan(bufs[k][1].t).all()) and bool(torch.isnan(bufs[k][2].t).all()), tag
    M.report("forward_multi %s x%d" % (name, count), worst)


# ------------------------------------------------------------------------------------------------------------------ backward
class Bwd(object):
    """The inputs of one backward problem: unplanted s / a, the KERNEL's x0 / h1 with +-0 / denormal entries planted into
    them, a random dout / n -- all as views with NaN guard rows."""

    def __init__(self, net, n, seed, plant=True, tune=None):
        self.net, self.n = net, n
        self.s, self.a, _ = M.make_inputs(net.spec, n, seed=seed, device=DEV, planted=False)
        _, x0, h1 = forward(net, self.s, self.a, n, tune=tune)
        x0, h1 = x0.clone(), h1.clone()
        if plant:
            x0c, h1c = M.plant_activations(x0.cpu(), h1.cpu(), seed)
            x0, h1 = x0c.to(DEV), h1c.to(DEV)
        self.x0, self.h1 = guarded_input(x0), guarded_input(h1)
        g = torch.Generator().manual_seed(seed + 1)
        self.dout = guarded_input((torch.randn(n, net.outs, generator=g) / n).to(DEV))

    def one_hot(self, r):
        d = torch.zeros_like(self.dout)
        d[r] = self.dout[r]
        return guarded_input(d)


GM_SENT = 7.0


def new_gradmax():
    gm = torch.full((512,), GM_SENT, device=DEV)
    gm[::32] = 0.0
    return gm


def check_gradmax(gm, written, tag):
    """Slots [32 j] hold, together, exactly max |element written|; nothing else of the buffer is touched."""
    other = gm.clone()
    other[::32] = GM_SENT
    assert bool((other == GM_SENT).all()), tag + ": gradmax written outside the slots [32 j]"
    want = M.gradmax_of(written)
    assert float(gm[::32].max()) == want, "%s: gradmax %r, the written gradients' maximum %r" % (tag, float(gm[::32].max()), want)


def backward(net, p, dout, pre_seed, worst, tag, tune=None, param_grads=True, state_only=False, want_da=True, rows=None,
             zero=False, gm=None, td=None, check=True):
    """One rpo_mlp_backward on pre-filled gradients, judged by mlp_f64.check_backward.  Returns (got, pre, written)."""
    ops = _ops()
    n = p.n
    pre = net.prefill(pre_seed, zero=zero)
    dh, dx0 = Out(n, M.H), Out(n, net.ein)
    da = Out(n, net.A) if (net.A and want_da) else None
    own_gm = gm is None and param_grads
    if own_gm:
        gm = new_gradmax()
    with ops.tuning(**(tune or {})):
        ops.mlp_backward(net.desc, p.s, p.a, p.x0, p.h1, dout, dh.t, dx0.t, None if da is None else da.t,
                         param_grads=param_grads, first_layer_state_only=state_only, gradmax=gm, td=td)
    _sync()
    assert dh.intact() and dx0.intact() and (da is None or da.intact()), tag + ": an output guard row was written"
    assert net.padding_intact(), tag + ": padding of the flat gradient written"
    got = dict(net.grads(), dx0=dx0.t, da=None if da is None else da.t, dh=dh.t)
    if not check:
        return got, pre, None
    d_eff = dout if td is None else td.dq_out.view(n, 1)
    written = M.check_backward(net.ref, p.s, p.a, p.x0, p.h1, d_eff, got, pre, worst, tag, param_grads=param_grads,
                               state_only=state_only, rows=rows, want_da=da is not None)
    if own_gm:
        check_gradmax(gm, written, tag)
    return got, pre, written


def backward_sizes(net):
    sizes = list(SIZES) + (GEMM_SIZES if net.gemm else [])
    if net.name in ("add_6_2", "cat_57_43", "actor14"):          # scalar roles | layer by layer + MFMA first layer | multi-output role
        sizes.append(ONCE)
    if net.name == "cat_57_43":
        sizes += [GEMM_LIMIT, GEMM_LIMIT + 1]
    return sizes


@pytest.mark.parametrize("name", NAMES)
def test_backward_matches_float64(name):
    """rpo_mlp_backward at every row count: the full form += onto random gradients with gradmax; at 17 and 257 rows also
    param_grads = 0, first_layer_state_only = 1, da NULL (tensors a reduced mode must not write compared bitwise), the 256-wide
    networks without the k split and on the row-tile rows kernel, a pre-set larger gradmax slot, and the one-hot probes."""
    net = Net(name, 13)
    worst = {}
    for n in backward_sizes(net):
        p = Bwd(net, n, seed=n)
        tag = "%s n=%d" % (name, n)
        backward(net, p, p.dout, n, worst, tag + " full +=")
        if n not in (17, 257):
            continue
        backward(net, p, p.dout, n, worst, tag + " dx0-only", param_grads=False)
        backward(net, p, p.dout, n, worst, tag + " state-only +=", state_only=True)
        if net.A:
            backward(net, p, p.dout, n, worst, tag + " no-da +=", want_da=False)
            backward(net, p, p.dout, n, worst, tag + " dx0-only-no-da", param_grads=False, want_da=False)
        if net.gemm:
            backward(net, p, p.dout, n, worst, tag + " gemm0 +=", tune=dict(gemm_ksplit=0))
            backward(net, p, p.dout, n, worst, tag + " rows-kernel +=", tune=dict(mlp_gemm=0))
        # a slot that already holds more survives; no other slot exceeds this call's maximum
        gm = new_gradmax()
        gm[96] = 1e9
        _, _, written = backward(net, p, p.dout, n, worst, tag + " preset +=", gm=gm)
        assert float(gm[96]) == 1e9 and float(gm[::32].sort().values[-2]) <= M.gradmax_of(written), tag + ": pre-set gradmax slot"
        for r in sorted({r for r in (0, 15, 16, n - 16, n - 1) if 0 <= r < n}):
            backward(net, p, p.one_hot(r), n, worst, "%s probe r=%d" % (tag, r), rows=1, zero=True)
    M.report("backward %s" % name, worst)


def _td(p, n, seed, sac):
    """A Td on planted rows (|q - y| exactly 1, a few ulps either side), done in {0, 1}, strided reward / done columns."""
    ops = _ops()
    g = torch.Generator().manual_seed(seed)
    q, qn1, qn2, logp = (torch.randn(n, generator=g) for _ in range(4))
    wide = torch.randn(n + 2 * G, 5, generator=g)
    wide[:, 3] = (wide[:, 3] > 0.3).float()
    reward, done = wide[G:G + n, 1], wide[G:G + n, 3]
    M.plant_td_kink(q, qn1, reward, done, 0.99, qn2=qn2, logp=logp)
    wide[:G] = NAN
    wide[G + n:] = NAN
    wide = wide.to(DEV)
    cols = dict(reward=wide[G:G + n, 1:2], done=wide[G:G + n, 3:4])
    vec = {k: guarded_input(v.view(n, 1).to(DEV)).view(-1) for k, v in dict(q=q, qn1=qn1, qn2=qn2, logp=logp).items()}
    dq, parts = Out(n, 1), Out((n + 15) // 16, 1)
    td = ops.Td(vec["q"], vec["qn1"], vec["qn2"] if sac else None, vec["logp"] if sac else None, cols["reward"], cols["done"],
                0.2 if sac else 0.0, 0.99, dq.t.view(-1), parts.t.view(-1))
    return td, dq, parts


def check_td(td, dq, parts, sac, worst, tag):
    args = (td.q, td.qn1, td.reward, td.done, 0.99, td.qn2 if sac else None, td.logp if sac else None, 0.2 if sac else 0.0)
    assert dq.intact() and parts.intact(), tag + ": guard rows of dq_out / loss_partial"
    dq_r, dq_b, _, _, d = M.td(*args)
    assert bool((d[:min(2, d.numel())].abs() == 1.0).all())       # (the planted rows sit exactly on the kink)
    M.check(tag + " dq", dq.t.view(-1), dq_r, None, 0, worst, allowed=dq_b)
    p_r, p_b = M.td_partials(*args)
    M.check(tag + " loss_partial", parts.t.view(-1), p_r, None, 0, worst, allowed=p_b)


@pytest.mark.parametrize("sac", [False, True], ids=["ddpg", "sac"])
@pytest.mark.parametrize("name", ["add_6_2", "cat_57_43"])
def test_td_prologue_matches_float64(name, sac):
    """The TD / Huber prologue of the rows pass (row tile and layer by layer) at n = 1, 17, 256: dq_out and EVERY
    loss_partial, the partial last tile included, within mlp_f64.td's bounds; the gradients then from the kernel's dq."""
    net = Net(name, 14)
    worst = {}
    for n in (1, 17, 256):
        p = Bwd(net, n, seed=n)
        td, dq, parts = _td(p, n, n, sac)
        tag = "%s td n=%d" % (name, n)
        backward(net, p, None, n, worst, tag + " +=", td=td)
        check_td(td, dq, parts, sac, worst, tag)
    M.report("td %s %s" % (name, "sac" if sac else "ddpg"), worst)


PAIRS = [("add_6_2", False), ("add_6_2", True), ("cat_57_43", False), ("cat_57_43", True), ("gauss_5", False)]   # (rpo_td: n_out 1)


@pytest.mark.parametrize("name,with_td", PAIRS, ids=["%s-%s" % (p[0], "td" if p[1] else "dout") for p in PAIRS])
def test_backward_pair_is_two_single_calls(name, with_td):
    """rpo_mlp_backward_pair of two different networks on the same inputs, with and without td1 / td2: bitwise equal to two
    single calls (which are judged against float64 here), guards and padding intact."""
    ops = _ops()
    nets = [Net(name, 15), Net(name, 16)]
    worst = {}
    for n in (17, 256):
        ps = [Bwd(nets[0], n, seed=n)]
        q = Bwd(nets[1], n, seed=n)                               # (same seed: the same s / a values; the pair reads ps[0]'s)
        assert same_bits(q.s, ps[0].s)
        ps.append(q)
        tds = [_td(ps[k], n, n + k, sac=True) if with_td else (None, None, None) for k in range(2)]
        singles = []
        for k in range(2):
            tag = "%s pair n=%d net%d" % (name, n, k)
            got, pre, _ = backward(nets[k], ps[k], None if with_td else ps[k].dout, n + k, worst, tag + " single +=", td=tds[k][0])
            if with_td:
                check_td(tds[k][0], tds[k][1], tds[k][2], True, worst, tag)
            singles.append({key: (None if v is None else v.clone()) for key, v in got.items()})
            if with_td:
                singles[k].update(dq=tds[k][1].t.clone(), parts=tds[k][2].t.clone())
        for k in range(2):
            nets[k].prefill(n + k)
        tds2 = [_td(ps[k], n, n + k, sac=True) if with_td else (None, None, None) for k in range(2)]
        outs = [(Out(n, M.H), Out(n, nets[0].ein), Out(n, nets[0].A) if nets[0].A else None) for _ in range(2)]
        gm = new_gradmax()
        s, a = ps[0].s, ps[0].a
        da = [None if o[2] is None else o[2].t for o in outs]
        ops.mlp_backward_pair(nets[0].desc, nets[1].desc, s, a, ps[0].x0, ps[0].h1, None if with_td else ps[0].dout, outs[0][0].t,
                              outs[0][1].t, da[0], ps[1].x0, ps[1].h1, None if with_td else ps[1].dout, outs[1][0].t, outs[1][1].t,
                              da[1], gradmax=gm, td1=tds2[0][0], td2=tds2[1][0])
        _sync()
        for k in range(2):
            tag = "%s pair n=%d net%d" % (name, n, k)
            assert all(o is None or o.intact() for o in outs[k]) and nets[k].padding_intact(), tag + ": guards"
            assert same_bits(outs[k][0].t, singles[k]["dh"]) and same_bits(outs[k][1].t, singles[k]["dx0"]), tag + ": dh / dx0"
            if nets[k].A:
                assert same_bits(outs[k][2].t, singles[k]["da"]), tag + ": da"
            for key, g in nets[k].grads().items():
                assert same_bits(g, singles[k][key]), "%s: gradient %s differs from the single call" % (tag, key)
            if with_td:
                assert tds2[k][1].intact() and tds2[k][2].intact()
                assert same_bits(tds2[k][1].t, singles[k]["dq"]) and same_bits(tds2[k][2].t, singles[k]["parts"]), tag + ": td"
        check_gradmax(gm, [g for net in nets for g in net.grads().values()], "%s pair n=%d" % (name, n))
    M.report("backward_pair %s%s" % (name, " td" if with_td else ""), worst)


# --------------------------------------------------------------------------------------------------------------- NaN and inf
def _f32_bits(pattern):
    return torch.tensor([pattern - (1 << 32) if pattern >= (1 << 31) else pattern], dtype=torch.int32).view(torch.float32)[0]


PLANTS = {"nan+": 0x7FC00000, "nan-": 0xFFC00000, "inf+": 0x7F800000}


def _forward_forms(net, s, a, n):
    """{form: (out, x0, h1)} of every forward form of the network; forms of one list entry are claimed bit-identical."""
    ops = _ops()
    groups = []
    tile = {"tile": forward(net, s, a, n, tune=dict(mlp_gemm=0)), "unsaved": forward(net, s, a, n, save=False)}
    if net.l1_mfma:
        tile["l1_vec"] = forward(net, s, a, n, tune=dict(l1_mfma=0))
    if net.hd == 1:
        bufs = [(Out(n, net.outs), Out(n, net.ein), Out(n, M.H)) for _ in range(2)]
        with ops.tuning(mlp_gemm=0):
            ops.mlp_forward_multi([(net.desc, s, a, b[0].t, b[1].t, b[2].t) for b in bufs])
        _sync()
        tile["multi"] = tuple(o.t for o in bufs[1])
        if ops.mlp_split_supported(net.desc):
            part = torch.full((8, n, 2), NAN, device=DEV)
            out, x0, h1 = Out(n, net.outs), Out(n, net.ein), Out(n, M.H)
            ops.mlp_forward_split([(net.desc, s, a, part, x0.t, h1.t)])
            ops.mlp_split_head(net.desc, part, out.t)
            _sync()
            assert out.intact() and x0.intact() and h1.intact()
            tile["split"] = (out.t, x0.t, h1.t)
    groups.append(tile)
    if net.gemm:
        groups.append({"gemm1": forward(net, s, a, n, tune=dict(gemm_ksplit=1))})
        groups.append({"gemm0": forward(net, s, a, n, tune=dict(gemm_ksplit=0))})
    return groups


@pytest.mark.parametrize("plant", list(PLANTS))
@pytest.mark.parametrize("name", ["add_6_2", "gauss_5", "add_7_2", "cat_57_43", "actor14", "wide14"])
def test_nan_and_inf_reach_the_row_output_in_every_forward_form(name, plant):
    """One NaN (either sign bit) or +inf in row r of s.  Contract (include/rpo_hip.h): the NaN pre-activations of row r stay
    NaN through both relus -- x0[r] (its state part), h1[r] and out[r] are NaN in EVERY form: row tile, first layer on the
    vector ALU, unsaved, forward_multi, column split + split_head, layer by layer with and without the k split -- and every
    other row keeps the bits it has without the plant.  +inf: inf * 0 in the dead column of the first layer is NaN, not 0,
    so the same holds."""
    net = Net(name, 17)
    n = 33
    for r in (0, 16, n - 1):
        s, a, wide = M.make_inputs(net.spec, n, seed=5, device=DEV, planted=False)
        base = _forward_forms(net, s, a, n)
        wide[G + r, 1 + (r % net.S)] = _f32_bits(PLANTS[plant]).to(DEV)
        assert not bool(torch.isfinite(s[r]).all())
        planted = _forward_forms(net, s, a, n)
        rest = [i for i in range(n) if i != r]
        for gb, gp in zip(base, planted):
            first = next(iter(gp))
            for form, (out, x0, h1) in gp.items():
                tag = "%s %s r=%d %s" % (name, plant, r, form)
                assert bool(torch.isnan(out[r]).all()), tag + ": the NaN did not reach out[r]"
                assert same_bits(out[rest], gb[form][0][rest]), tag + ": another row of out changed"
                assert same_bits_or_nan(out, gp[first][0]), tag + ": out differs from " + first
                if x0 is None:
                    continue
                state = x0[r, :net.E]
                if plant.startswith("nan"):
                    assert bool(torch.isnan(state).all()), tag + ": x0[r] is not NaN"
                else:
                    assert bool(torch.isnan(state[M.ZERO_COL])) and not bool(torch.isfinite(state).any()), tag + ": inf * 0"
                assert bool(torch.isnan(h1[r]).all()), tag + ": h1[r] is not NaN"
                assert same_bits(x0[rest], gb[form][1][rest]) and same_bits(h1[rest], gb[form][2][rest]), tag + ": other rows"
                assert same_bits_or_nan(x0, gp[first][1]) and same_bits_or_nan(h1, gp[first][2]), tag + ": differs from " + first


@pytest.mark.parametrize("sign", ["nan+", "nan-"])
@pytest.mark.parametrize("name", ["add_6_2", "cat_57_43", "gauss14"])
def test_nan_in_dout_reaches_every_gradient_its_row_touches(name, sign):
    """A NaN in dout[r]: dh[r, j] is NaN where h1[r, j] > 0 and 0 elsewhere; so are db0[j] and row j of dW0, and every other
    element of them keeps its bits; dW1 / db1 of the head that read the NaN are NaN throughout (NaN * relu = NaN, also at 0);
    dx0[r, e] is NaN where x0[r, e] > 0, with it row e of the first-layer gradients, and da[r]; no other row of dh / dx0 / da
    changes.  gradmax skips NaN: it is the maximum over the finite elements written (as rpo_absmax / rpo_adam_step pin)."""
    net = Net(name, 18)
    n, r = 33, 16
    p = Bwd(net, n, seed=3, plant=False)
    base, _, _ = backward(net, p, p.dout, 0, {}, "base", zero=True, check=False)
    base = {k: (None if v is None else v.clone()) for k, v in base.items()}
    d = p.dout.clone()
    d[r, 0] = _f32_bits(PLANTS[sign]).to(DEV)
    gm = new_gradmax()
    got, _, _ = backward(net, p, guarded_input(d), 0, {}, "nan", zero=True, check=False, gm=gm)
    hpos, xpos = p.h1[r] > 0, p.x0[r] > 0
    assert bool(hpos.any()) and bool((~hpos).any()) and bool(xpos.any()) and bool((~xpos).any())
    rest = [i for i in range(n) if i != r]

    def rows_nan(what, mask):
        """Rows of gradient `what` selected by mask all NaN, the others bitwise the baseline."""
        t2, b2 = got[what].reshape(mask.numel(), -1), base[what].reshape(mask.numel(), -1)
        assert bool(torch.isnan(t2[mask]).all()), "%s %s: a row the NaN touches is not NaN" % (name, what)
        assert same_bits(t2[~mask], b2[~mask]), "%s %s: a row the NaN does not touch changed" % (name, what)

    for key, mask in (("dh", hpos), ("dx0", xpos)):
        assert bool(torch.isnan(got[key][r][mask]).all()) and float(got[key][r][~mask].abs().max()) == 0.0, key
        assert same_bits(got[key][rest], base[key][rest]), key
    for key in ("W0", "b0"):
        rows_nan(key, hpos)
    first = torch.arange(net.hd, device=DEV) == 0                # (only output 0 of head 0 read the NaN)
    rows_nan("W1", first)
    rows_nan("b1", first)
    if net.n_out > 1:
        assert same_bits(got["W1b"], base["W1b"]) and same_bits(got["b1b"], base["b1b"])
    E = net.E
    for key in ("Ws", "bs"):
        rows_nan(key, xpos[:E])
    if net.A:
        for key in ("Wa", "ba"):
            rows_nan(key, xpos[E:] if net.kind == "cat" else xpos)
        assert bool(torch.isnan(got["da"][r]).all()) and same_bits(got["da"][rest], base["da"][rest])
    finite = [torch.where(torch.isnan(g), 0.0, g) for g in net.grads().values()]
    check_gradmax(gm, finite, "%s nan dout" % name)
