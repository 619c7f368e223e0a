"""The policy-head launches (rpo_gauss_head, rpo_gauss_head_bwd, rpo_tanh_box_bwd and their EVOPF forms) and rpo_td_huber, called
directly, against the float64 restatement of tests/heads_f64.py at the edges where such kernels go wrong: both clamps of the
log-std head and their float32 neighbours, saturated tanh, samples exactly on the clip seam, an offset box, NaN, ragged row
counts and the second pass of the grid-stride loops.  Needs an MI355X.

Tolerance, everywhere: MARGIN (4) * C_REF_* * eps32 * magnitude sum (heads_f64.py).  C_REF_* is the reference's own float32
error, measured on the CPU (test_heads_f64.py::test_yardstick); the factor 4 is for device expf / tanhf / logf of a few ulp and
for the fused vs unfused association.  Every test prints its worst ratio to that tolerance.  Every output buffer is 64 elements
too long and pre-filled; the tail must come back untouched.
"""
import functools

import numpy as np
import pytest
import torch

import heads_f64 as hf
from test_evopf_gpu import states

pytestmark = pytest.mark.gpu

DEV = "cuda"
PAD, SENTINEL = 64, -12345.0
DLOGP = 0.01
ROW_COUNTS = (1, 255, 256, 257, 4099)
BIG = 2048 * 256 + 5                                 # one row into the second pass of a 2048-workgroup grid-stride loop
C = dict(ap=hf.C_REF_AP, logp=hf.C_REF_LOGP, g_mean=hf.C_REF_G_MEAN, g_ls=hf.C_REF_G_LS, box_bwd=hf.C_REF_BOX_BWD)


@pytest.fixture(scope="module")
def ops():
    from rpo_amd import ops as _ops
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return _ops


@pytest.fixture(scope="module")
def evopf(ops):
    from rpo_amd.env import EVOPFEnv
    return EVOPFEnv(device=DEV).kernels


def dev(x, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).to(DEV)


class Out(object):
    """An output buffer of n floats with PAD sentinel elements behind it; ``view`` is what the launch gets."""

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((n + PAD,), SENTINEL, device=DEV)
        self.view = self.buf[:n]

    def get(self):
        assert bool((self.buf[self.n:] == SENTINEL).all()), "the launch wrote past the end of its output"
        return self.view.cpu()


def within(name, got, ref, mag, c, keep=None):
    """Assert |got - ref| <= MARGIN * c * eps32 * mag on every (kept) element; prints and returns the worst ratio to that."""
    got, ref, mag = (torch.as_tensor(v).reshape(-1) for v in (got, ref, mag))
    if keep is not None:
        keep = torch.as_tensor(keep).reshape(-1)
        got, ref, mag = got[keep], ref[keep], mag[keep]
    r = hf.worst(got, ref, c * mag) / hf.MARGIN
    print("%-40s worst |err| = %.3f of the tolerance" % (name, r))
    assert r <= 1.0, "%s: %.3f times the tolerance" % (name, r)
    return r


@functools.lru_cache(maxsize=None)
def gauss_case(boxname, n, seed=0):
    """Inputs (float32 numpy) and the float64 forward of one (box, row count): shared, read-only."""
    box = hf.BOXES[boxname]
    if n == BIG:
        m, r, e = hf.random_rows(n, seed)
    else:
        m, r, e, _ = hf.rows(n, seed)
    args = (box.scale, box.base, box.lo, box.hi)
    ref = hf.gauss_head(m, r, e, *args)
    det = hf.gauss_head(m, r, e, *args, deterministic=True)
    mag = hf.gauss_mags(m, r, e, box.scale, box.base)
    mag_det = hf.gauss_mags(m, r, e, box.scale, box.base, deterministic=True)
    return dict(box=box, args=args, m=m, r=r, e=e, raw=np.stack([m, r], 1), ref=ref, det=det, mag=mag, mag_det=mag_det,
                dap=hf.gradient_weights(n, seed))


def run_gauss_head(ops, raw, e, args, deterministic, with_logp=True):
    n = raw.shape[0]
    ap, logp = Out(n), Out(n)
    ops.gauss_head(raw, e, *args, deterministic, ap.view, logp.view if with_logp else None)
    lp = logp.get()
    if not with_logp:
        assert bool((lp == SENTINEL).all())
    return ap.get(), lp


# ========================================================================================================== rpo_gauss_head
@pytest.mark.parametrize("n", ROW_COUNTS)
@pytest.mark.parametrize("boxname", list(hf.BOXES))
def test_gauss_head(ops, boxname, n):
    c = gauss_case(boxname, n)
    box, raw, e = c["box"], dev(c["raw"]), dev(c["e"])
    ap, logp = run_gauss_head(ops, raw, e, c["args"], False)
    within("ap[%s, %d]" % (boxname, n), ap, c["ref"]["ap"], c["mag"]["ap"], C["ap"])
    within("logp[%s, %d]" % (boxname, n), logp, c["ref"]["logp"], c["mag"]["logp"], C["logp"])
    assert bool(((ap >= box.lo) & (ap <= box.hi)).all())
    # logp_out = NULL: same ap
    ap2, _ = run_gauss_head(ops, raw, e, c["args"], False, with_logp=False)
    assert torch.equal(ap, ap2)
    # deterministic: a function of the mean column alone
    det, _ = run_gauss_head(ops, raw, e, c["args"], True)
    within("ap_det[%s, %d]" % (boxname, n), det, c["det"]["ap"], c["mag_det"]["ap"], C["ap"])
    raw2 = raw.clone()
    raw2[:, 1] = torch.flip(raw[:, 1], [0]) + 1.0
    det2, _ = run_gauss_head(ops, raw2, 3.0 - 2.0 * e, c["args"], True)
    assert torch.equal(det, det2)
    assert bool(((det >= box.lo) & (det <= box.hi)).all())


def test_gauss_head_second_grid_pass(ops):
    c = gauss_case("wide", BIG)
    raw, e = dev(c["raw"]), dev(c["e"])
    ap, logp = run_gauss_head(ops, raw, e, c["args"], False)
    within("ap[big]", ap, c["ref"]["ap"], c["mag"]["ap"], C["ap"])
    within("logp[big]", logp, c["ref"]["logp"], c["mag"]["logp"], C["logp"])
    back = hf.gauss_head(c["m"], c["r"], c["e"], *c["args"], dap=c["dap"], dlogp=DLOGP)
    mag = hf.gauss_mags(c["m"], c["r"], c["e"], c["box"].scale, c["box"].base, dap=c["dap"], dlogp=DLOGP)
    draw = Out(2 * BIG)
    ops.gauss_head_bwd(raw, e, dev(c["dap"]), DLOGP, *c["args"], draw.view)
    g = draw.get().view(BIG, 2)
    within("g_mean[big]", g[:, 0], back["g_mean"], mag["g_mean"], C["g_mean"])
    within("g_ls[big]", g[:, 1], back["g_ls"], mag["g_ls"], C["g_ls"])


def test_gauss_head_propagates_nan(ops):
    """A NaN mean head must come out as NaN (NonFiniteError depends on it), not clamped to lo or hi; its neighbours stay."""
    c = gauss_case("wide", 257)
    raw = dev(c["raw"])
    bad = [0, 63, 64, 256]
    raw[bad, 0] = float("nan")
    for deterministic in (False, True):
        ap, logp = run_gauss_head(ops, raw, dev(c["e"]), c["args"], deterministic)
        good = torch.ones(257, dtype=torch.bool)
        good[bad] = False
        assert bool(torch.isnan(ap[bad]).all()) and bool(torch.isfinite(ap[good]).all())
        want = (c["det"] if deterministic else c["ref"])["ap"]
        within("ap beside NaN rows", ap, want, (c["mag_det"] if deterministic else c["mag"])["ap"], C["ap"], keep=good)


# ====================================================================================================== rpo_gauss_head_bwd
def run_gauss_bwd(ops, c, dap, dlogp, args=None):
    n = c["raw"].shape[0]
    draw = Out(2 * n)
    ops.gauss_head_bwd(dev(c["raw"]), dev(c["e"]), dev(dap), dlogp, *(args or c["args"]), draw.view)
    return draw.get().view(n, 2)


@pytest.mark.parametrize("n", ROW_COUNTS)
@pytest.mark.parametrize("boxname", list(hf.BOXES))
def test_gauss_head_bwd(ops, boxname, n):
    c = gauss_case(boxname, n)
    box = c["box"]
    ls = c["r"].astype(np.float64) - 3.0
    outside = torch.from_numpy((ls < hf.LS_MIN) | (ls > hf.LS_MAX))
    on_clamp = torch.from_numpy((ls == hf.LS_MIN) | (ls == hf.LS_MAX))
    zeros = np.zeros(n, np.float32)
    for tag, dap, dlogp in (("both", c["dap"], DLOGP), ("dlogp=0", c["dap"], 0.0), ("dap=0", zeros, DLOGP)):
        ref = hf.gauss_head(c["m"], c["r"], c["e"], *c["args"], dap=dap, dlogp=dlogp)
        mag = hf.gauss_mags(c["m"], c["r"], c["e"], box.scale, box.base, dap=dap, dlogp=dlogp)
        g = run_gauss_bwd(ops, c, dap, dlogp)
        assert bool(torch.isfinite(g).all())
        within("g_mean[%s, %d, %s]" % (boxname, n, tag), g[:, 0], ref["g_mean"], mag["g_mean"], C["g_mean"])
        within("g_ls[%s, %d, %s]" % (boxname, n, tag), g[:, 1], ref["g_ls"], mag["g_ls"], C["g_ls"])
        # the clamp of the log-std head: exactly zero outside [-23, -2], the gradient itself AT -23 and AT -2 (torch.clamp)
        assert bool((g[:, 1][outside] == 0.0).all()) and bool((ref["g_ls"][outside] == 0.0).all())
        if dlogp != 0.0:
            assert bool((g[:, 1][on_clamp] != 0.0).all()) and bool((ref["g_ls"][on_clamp] != 0.0).all())
    if n == 4099:
        assert int(outside.sum()) > 300 and int(on_clamp.sum()) == 2 * len(hf.MEANS) * len(hf.DRAWS)


@pytest.mark.parametrize("boxname", list(hf.BOXES))
def test_gauss_head_bwd_clip_mask_is_inclusive(ops, boxname):
    """mean = 0, e = 0: y = tanhf(0) = 0 and a = base exactly.  With hi (or lo) = base the sample sits ON the clip bound and the
    gradient passes -- exactly dap * scale -- as torch.clip's does; one float32 step inside the bound it is exactly zero."""
    box = hf.BOXES[boxname]
    n = 257
    c = dict(raw=np.zeros((n, 2), np.float32), e=np.zeros(n, np.float32))
    dap = hf.gradient_weights(n, 5)
    base = np.float32(box.base)
    below, above = (float(v) for v in hf._neighbours(base))
    full = torch.from_numpy(dap * np.float32(box.scale))
    for lo, hi, passes in ((box.lo, box.base, True), (box.base, box.hi, True), (box.lo, below, False), (above, box.hi, False),
                           (box.lo, box.hi, True)):
        g = run_gauss_bwd(ops, c, dap, 0.0, (box.scale, box.base, lo, hi))
        ref = hf.gauss_head(c["raw"][:, 0], c["raw"][:, 1], c["e"], box.scale, box.base, lo, hi, dap=dap, dlogp=0.0)
        assert torch.equal(g[:, 0], full if passes else torch.zeros(n)), (lo, hi)
        assert torch.equal(ref["g_mean"].float(), g[:, 0]), (lo, hi)
        assert bool((g[:, 1] == 0.0).all())                      # e = 0 and dlogp = 0: nothing reaches the log-std head


# ======================================================================================================== rpo_tanh_box_bwd
def box_case(box, n, noise_on, eps_t, seed=0):
    """o -> ap_det = the float32 nearest to scale tanh(o) + base (what the actor launch hands over, at its best), float64 gradient
    with respect to o and its magnitude sum; ``keep`` leaves out rows within a few roundings of the clip seam."""
    o, noise = hf.box_rows(box, n, seed)
    dap = hf.gradient_weights(n, seed)
    ref = hf.tanh_box(o, noise if noise_on else None, eps_t, box.scale, box.base, box.lo, box.hi, dap=dap)
    keep = ~hf.near_seam(ref["pre"], box.lo, box.hi) if noise_on else torch.ones(n, dtype=torch.bool)
    return dict(o=o, noise=noise, dap=dap, ap_det=ref["ap_det"].float().numpy(), ref=ref, keep=keep,
                mag=hf.tanh_box_mags(o, box.scale, dap))


def run_box_bwd(ops, box, ap_det, noise, dap, eps=(0.0, 0.0, 0.0), ctrl=None):
    out = Out(len(ap_det))
    ops.tanh_box_bwd(dev(dap), dev(ap_det), None if noise is None else dev(noise), eps[0], eps[1], eps[2], ctrl, box.lo, box.hi,
                     box.scale, box.base, out.view)
    return out.get()


def offset_box_loss():
    """rpo_tanh_box_bwd recovers tanh(o) as (ap_det - base) / scale from the rounded ap_det.  With the offset box (4.9, 5.1), scale
    0.1 and base 5, ap_det rounds at the size of 5 and y = (ap_det - 5) / 0.1 carries |base| / scale = 50 roundings instead of
    one; 1 - y^2 near saturation loses them.  Measured (the row function is float32 +, -, *, / only, so the float32 CPU evaluation
    of it gives the device's bits): worst error 9.4 (257 rows) / 10.0 (4099 rows) eps32 * magnitude sum = 7.8 / 8.3 times the
    tolerance, against 0.29 / 0.32 = 0.24 / 0.27 of the tolerance for the symmetric boxes.  Recorded in DESIGN.md (parity); the
    cure is to hand the launch the raw head output, as rpo_evopf_tanh_box_bwd gets it, which changes the C ABI."""
    return pytest.mark.xfail(strict=True, reason="offset box: (ap_det - base) / scale loses |base| / scale roundings, measured "
                                                 "8.3x the tolerance, 10 eps32 * magnitude sum (DESIGN.md, parity section)")


@pytest.mark.parametrize("noise_on", [False, True], ids=["no_noise", "noise"])
@pytest.mark.parametrize("boxname", ["wide", "unit", pytest.param("offset", marks=offset_box_loss())])
def test_tanh_box_bwd(ops, boxname, noise_on):
    box = hf.BOXES[boxname]
    eps_t = hf.f32(0.5 * box.scale)
    for n in (257, 4099):
        c = box_case(box, n, noise_on, eps_t)
        g = run_box_bwd(ops, box, c["ap_det"], c["noise"] if noise_on else None, c["dap"], (eps_t, eps_t, 0.0))
        assert float(c["keep"].double().mean()) > 0.99
        if noise_on:
            clipped = ((c["ref"]["pre"] < box.lo) | (c["ref"]["pre"] > box.hi)) & c["keep"]
            assert bool((g[clipped] == 0.0).all()) and 0.05 < float(clipped.double().mean()) < 0.95
        within("tanh_box_bwd[%s, %d, %s]" % (boxname, n, "noise" if noise_on else "no noise"), g, c["ref"]["g"], c["mag"],
               C["box_bwd"], keep=c["keep"])


@pytest.mark.parametrize("boxname", list(hf.BOXES))
def test_tanh_box_bwd_clip_mask_is_inclusive(ops, boxname):
    """ap_det = base and noise that puts ap_det + eps_t * noise exactly on lo, on hi and on their float32 neighbours (every product
    exact): dap * scale * (1 - 0) on lo, on hi and inside, exactly 0.0 one float32 step outside."""
    box = hf.BOXES[boxname]
    eps_t = 0.5 if box.scale >= 1.0 else 0.125
    ap_det, noise, target, inside = hf.clip_mask_rows(box, eps_t)
    dap = np.array([1.5, -0.75, 2.0, 1.25, -1.0, 0.5], np.float32)
    g = run_box_bwd(ops, box, ap_det, noise, dap, (eps_t, eps_t, 0.0))
    want = np.where(inside, dap * np.float32(box.scale) * np.float32(1.0), np.float32(0.0)).astype(np.float32)
    assert np.array_equal(g.numpy(), want), (g, want, target)
    assert list(inside) == [True, True, False, True, True, False]


def test_tanh_box_bwd_eps_schedule(ops):
    """eps_t = max(eps_end, eps_start - eps_decay * ctrl[RPO_CTRL_T]) with 1, 1/4, 1/64: 17/64 at t = 47, 1/4 at t = 48 (where the
    schedule reaches eps_end) and at t = 49 (past it); ctrl = NULL means t = 0.  The first five rows (ap_det = 0, noise 9, 11, 36,
    39, 41 against hi = 10) pass or not depending on which eps_t was used."""
    box = hf.BOXES["wide"]
    start, end, decay = 1.0, 0.25, 2.0 ** -6
    n = 517
    o, noise = hf.box_rows(box, n, 9)
    o[:5], noise[:5] = 0.0, [9.0, 11.0, 36.0, 39.0, 41.0]
    noise[5:] *= 8.0
    dap = hf.gradient_weights(n, 9)
    seen = {}
    for t, pattern in ((None, [1, 0, 0, 0, 0]), (47, [1, 1, 1, 0, 0]), (48, [1, 1, 1, 1, 0]), (49, [1, 1, 1, 1, 0])):
        eps_t = hf.eps_schedule(start, end, decay, 0 if t is None else t)
        ref = hf.tanh_box(o, noise, eps_t, box.scale, box.base, box.lo, box.hi, dap=dap)
        ctrl = None
        if t is not None:
            ctrl = torch.zeros(ops.CTRL_LEN, dtype=torch.int64, device=DEV)
            ctrl[ops.CONST["RPO_CTRL_T"]] = t
        g = run_box_bwd(ops, box, ref["ap_det"].float().numpy(), noise, dap, (start, end, decay), ctrl)
        keep = ~hf.near_seam(ref["pre"], box.lo, box.hi)
        within("tanh_box_bwd[t = %s]" % t, g, ref["g"], hf.tanh_box_mags(o, box.scale, dap), C["box_bwd"], keep=keep)
        assert [int(v != 0.0) for v in g[:5]] == pattern, (t, g[:5])
        seen[t] = g
    assert torch.equal(seen[48], seen[49]) and not torch.equal(seen[47], seen[48]) and not torch.equal(seen[None], seen[47])


# ============================================================================================================= EVOPF heads
EVOPF_ROWS = (1, 15, 16, 17, 4099)                   # ragged against the 16 rows per workgroup of rpo_evopf_gauss_head
NP = 14


@functools.lru_cache(maxsize=None)
def evopf_states():
    """states() of test_evopf_gpu.py, the first four rows with the batteries' state of charge at and just inside both limits."""
    s, _ = states(4099)
    lo, hi = np.float32(0.1), np.float32(0.8)
    soc = slice(28, 33)
    s[0, soc], s[1, soc], s[2, soc], s[3, soc] = lo, np.nextafter(lo, np.float32(1)), hi, np.nextafter(hi, np.float32(0))
    return s


@functools.lru_cache(maxsize=None)
def evopf_case(n):
    s = evopf_states()[:n]
    m, r, e, _ = hf.rows(n * NP, 11)
    m, r, e = (v.reshape(n, NP) for v in (m, r, e))
    lo, hi, scale, base, scale_mag, base_mag = hf.evopf_box(s)
    assert bool((scale > 0).all())
    return dict(s=s, m=m, r=r, e=e, raw=np.concatenate([m, r], 1), lo=lo, hi=hi, scale=scale, base=base, scale_mag=scale_mag,
                base_mag=base_mag, args=(scale, base, lo, hi), dap=hf.gradient_weights(n * NP, 11).reshape(n, NP))


def strided(s):
    wide = torch.zeros(s.shape[0], 80, device=DEV)
    wide[:, 11:68] = dev(s)
    return wide[:, 11:68]


@pytest.mark.parametrize("n", EVOPF_ROWS)
def test_evopf_gauss_head(evopf, n):
    c = evopf_case(n)
    ref = hf.gauss_head(c["m"], c["r"], c["e"], *c["args"])
    mag = hf.gauss_mags(c["m"], c["r"], c["e"], c["scale"], c["base"], scale_mag=c["scale_mag"], base_mag=c["base_mag"])
    raw, e = dev(c["raw"]), dev(c["e"])
    results = []
    for s in (dev(c["s"]), strided(c["s"])):
        ap, logp = Out(n * NP), Out(n)
        evopf.gauss_head(s, raw, e, False, ap.view, logp.view)
        results.append((ap.get().view(n, NP), logp.get()))
    ap, logp = results[0]
    assert torch.equal(ap, results[1][0]) and torch.equal(logp, results[1][1])
    within("evopf ap[%d]" % n, ap, ref["ap"], mag["ap"], C["ap"])
    # logp: the sum over the 14 dimensions (a 16-lane butterfly: four more additions on top of each term's own bound)
    within("evopf logp[%d]" % n, logp, ref["logp"].sum(1), mag["logp"].sum(1) + 4 * ref["logp"].abs().sum(1), C["logp"])
    assert bool(((ap.double() >= c["lo"] - 1e-6) & (ap.double() <= c["hi"] + 1e-6)).all())
    det = hf.gauss_head(c["m"], c["r"], c["e"], *c["args"], deterministic=True)
    mag_det = hf.gauss_mags(c["m"], c["r"], c["e"], c["scale"], c["base"], deterministic=True, scale_mag=c["scale_mag"],
                            base_mag=c["base_mag"])
    ap_d = Out(n * NP)
    evopf.gauss_head(dev(c["s"]), raw, e, True, ap_d.view, None)
    within("evopf ap_det[%d]" % n, ap_d.get().view(n, NP), det["ap"], mag_det["ap"], C["ap"])


@pytest.mark.parametrize("n", EVOPF_ROWS)
def test_evopf_gauss_head_bwd(evopf, n):
    c = evopf_case(n)
    ls = torch.from_numpy(c["r"].astype(np.float64) - 3.0)
    outside = (ls < hf.LS_MIN) | (ls > hf.LS_MAX)
    on_clamp = (ls == hf.LS_MIN) | (ls == hf.LS_MAX)
    raw, e = dev(c["raw"]), dev(c["e"])
    for tag, dap, dlogp in (("both", c["dap"], DLOGP), ("dlogp=0", c["dap"], 0.0), ("dap=0", np.zeros_like(c["dap"]), DLOGP)):
        ref = hf.gauss_head(c["m"], c["r"], c["e"], *c["args"], dap=dap, dlogp=dlogp)
        mag = hf.gauss_mags(c["m"], c["r"], c["e"], c["scale"], c["base"], dap=dap, dlogp=dlogp, scale_mag=c["scale_mag"],
                            base_mag=c["base_mag"])
        results = []
        for s in (dev(c["s"]), strided(c["s"])):
            draw = Out(2 * n * NP)
            evopf.gauss_head_bwd(s, raw, e, dev(dap), dlogp, draw.view)
            results.append(draw.get().view(n, 2 * NP))
        g = results[0]
        assert torch.equal(g, results[1]) and bool(torch.isfinite(g).all())
        within("evopf g_mean[%d, %s]" % (n, tag), g[:, :NP], ref["g_mean"], mag["g_mean"], C["g_mean"])
        within("evopf g_ls[%d, %s]" % (n, tag), g[:, NP:], ref["g_ls"], mag["g_ls"], C["g_ls"])
        assert bool((g[:, NP:][outside] == 0.0).all())
        if dlogp != 0.0:
            assert bool((g[:, NP:][on_clamp] != 0.0).all())


@pytest.mark.parametrize("n", EVOPF_ROWS)
def test_evopf_tanh_box_bwd(evopf, ops, n):
    c = evopf_case(n)
    o, dap = c["m"], c["dap"]
    noise = (hf.random_rows(n * NP, 13)[2] * 1.5).reshape(n, NP)
    mag = hf.tanh_box_mags(o, c["scale"], dap, scale_mag=c["scale_mag"])
    start, end, decay, t = 1.0, 0.25, 2.0 ** -6, 40
    ctrl = torch.zeros(ops.CTRL_LEN, dtype=torch.int64, device=DEV)
    ctrl[ops.CONST["RPO_CTRL_T"]] = t
    for tag, nz, eps_t in (("no noise", None, 0.0), ("noise", noise * np.float32(0.25), hf.eps_schedule(start, end, decay, t))):
        ref = hf.tanh_box(o, nz, eps_t, *c["args"], dap=dap)
        results = []
        for s in (dev(c["s"]), strided(c["s"])):
            out = Out(n * NP)
            evopf.tanh_box_bwd(s, dev(o), None if nz is None else dev(nz), start, end, decay, ctrl, dev(dap), out.view)
            results.append(out.get().view(n, NP))
        g = results[0]
        assert torch.equal(g, results[1])
        # (the kernel computes the box itself: the seam is as wide as the box's own float32 error)
        seam = hf.EPS32 * (c["scale_mag"] + c["base_mag"]) * 8
        keep = torch.ones(n, NP, dtype=torch.bool) if nz is None else \
            ((ref["pre"] - c["lo"]).abs() > seam) & ((ref["pre"] - c["hi"]).abs() > seam)
        assert n < 100 or float(keep.double().mean()) > 0.99
        if nz is not None and n == 4099:
            clipped = ((ref["pre"] < c["lo"]) | (ref["pre"] > c["hi"])) & keep
            assert 0.05 < float(clipped.double().mean()) < 0.95 and bool((g[clipped] == 0.0).all())
        within("evopf tanh_box_bwd[%d, %s]" % (n, tag), g, ref["g"], mag, C["box_bwd"], keep=keep)


# ============================================================================================================ rpo_td_huber
@pytest.mark.parametrize("sac", [False, True], ids=["ddpg", "sac"])
def test_td_huber_seam_second_pass_and_accumulation(ops, sac):
    """q - y exactly +-1 (the seam of smooth-L1 and of the gradient clamp) and +-(1 +- one float32 step), done in {0, 1}, one row
    into the second pass of the grid-stride loop, a second call that adds onto loss_out, and the SAC form without grad_q2."""
    n = BIG
    rng = np.random.RandomState(17)
    q1, q2, qn1, qn2 = [(3 * rng.randn(n)).astype(np.float32) for _ in range(4)]
    logp, reward = rng.randn(n).astype(np.float32), rng.randn(n).astype(np.float32)
    done = (rng.rand(n) < 0.2).astype(np.float32)
    one = np.float32(1.0)
    seam = np.array([one, -one] + [s * v for v in hf._neighbours(one) for s in (one, -one)], np.float32)
    at = np.concatenate([np.arange(6), n - 6 + np.arange(6)])           # first rows, and the rows of the second grid pass
    reward[at], done[at] = 0.0, 1.0                                     # y = 0 + gamma * 0 * qn = 0 exactly: q - y = q
    q1[at], q2[at] = np.tile(seam, 2), np.tile(seam[::-1], 2)
    gamma, alpha = 0.95, 0.1
    ref = hf.td_huber(q1, qn1, reward, done, gamma, q2=q2 if sac else None, qn2=qn2 if sac else None,
                      logp=logp if sac else None, alpha=alpha if sac else 0.0)
    assert np.array_equal(ref["d1"].numpy()[at], np.tile(seam, 2).astype(np.float64))
    loss = torch.zeros(1, device=DEV)
    g1, g2, y = Out(n), Out(n), Out(n)
    d = [dev(v) for v in (q1, q2, qn1, qn2, logp)]
    batch = torch.zeros(n, 3, device=DEV)                               # reward / done as columns of a wider matrix
    batch[:, 0], batch[:, 2] = dev(reward), dev(done)
    rw, dn = batch[:, 0:1], batch[:, 2:3]
    if sac:
        ops.td_huber(d[0], d[1], d[2], d[3], d[4], alpha, rw, dn, gamma, loss, g1.view, g2.view, y.view)
    else:
        ops.td_huber(d[0], None, d[2], None, None, 0.0, rw, dn, gamma, loss, g1.view, None, y.view)
    first = float(loss)
    np.testing.assert_allclose(first, ref["loss"], rtol=1e-5)
    np.testing.assert_allclose(y.get().numpy(), ref["y"].numpy(), rtol=1e-6, atol=1e-6)
    got1 = g1.get().numpy()
    np.testing.assert_allclose(got1, ref["g1"].numpy(), rtol=1e-6, atol=1e-9)
    inv_n = one / np.float32(n)
    want_seam = np.clip(seam, -one, one) * inv_n                         # exact on the seam rows: d is exact, one product
    assert np.array_equal(got1[at], np.tile(want_seam, 2))
    got2 = g2.get().numpy()
    if sac:
        np.testing.assert_allclose(got2, ref["g2"].numpy(), rtol=1e-6, atol=1e-9)
        assert np.array_equal(got2[at], np.tile(want_seam[::-1], 2))
    else:
        assert (got2 == SENTINEL).all()
    # a second call adds onto a non-zero loss_out; SAC form with q2 but without grad_q2: same loss, same grad_q1
    g1b = Out(n)
    if sac:
        ops.td_huber(d[0], d[1], d[2], d[3], d[4], alpha, rw, dn, gamma, loss, g1b.view, None, None)
    else:
        ops.td_huber(d[0], None, d[2], None, None, 0.0, rw, dn, gamma, loss, g1b.view, None, None)
    np.testing.assert_allclose(float(loss), first + ref["loss"], rtol=1e-5)
    assert np.array_equal(g1b.get().numpy(), got1)
