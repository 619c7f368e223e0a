"""The optimiser launches (rpo_absmax, rpo_absmax_slots, rpo_adam_step, rpo_adam_step_multi, rpo_polyak, rpo_min_q_bwd) called
directly, against the float64 restatement of tests/optim_f64.py: exp_avg, exp_avg_sq, the update, the target and the gradient
written back after ONE launch from a state seeded by the host (errors do not compound into the tolerance), at ragged sizes, both
arrival forms (<= 16 workgroups / the two-level tree), the second grid-stride pass, every hyper-parameter the kernel takes, the
clip below / at / above its threshold, overflow, underflow, NaN, a cache that is empty, valid or stale, prepared = 1, and the
bookkeeping words a launch may and may not touch.  Needs an MI355X.

Tolerance, everywhere: MARGIN (4) * C_REF_* * eps32 * magnitude sum (optim_f64.py).  C_REF_* is the float32 emulation's own error
against the reference over these very inputs, measured on the CPU (test_optim_f64.py::test_yardstick); the factor 4 is for device
sqrtf / division of a few ulp and fused against unfused association.  Every test prints its worst ratio to that tolerance.  Every
buffer a launch gets is 64 elements too long and pre-filled; the tail must come back untouched.
"""
import math

import numpy as np
import pytest
import torch

import optim_f64 as of

pytestmark = pytest.mark.gpu

DEV = "cuda"
PAD = 64
SENTINEL = dict([(torch.float32, -12345.0), (torch.int32, 0x5A5A5A5A), (torch.int64, -77)])
NP_OF = dict([(torch.float32, np.float32), (torch.int32, np.int32), (torch.int64, np.int64)])


@pytest.fixture(scope="module")
def ops():
    from rpo_amd import ops as _ops
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    assert _ops.CONST["RPO_ADAM_STATE_LEN"] == of.STATE_LEN and _ops.CONST["RPO_GRADMAX_LEN"] == of.GRADMAX_LEN
    assert _ops.CONST["RPO_GRADMAX_SLOTS"] == of.GRADMAX_SLOTS
    return _ops


class Buf(object):
    """A device buffer holding ``values`` with PAD sentinel elements behind it; ``view`` is what the launch gets."""

    def __init__(self, values, dtype=torch.float32):
        values = np.ascontiguousarray(values, dtype=NP_OF[dtype])
        self.n, self.sentinel = values.size, SENTINEL[dtype]
        host = np.full(self.n + PAD, self.sentinel, dtype=NP_OF[dtype])
        host[:self.n] = values.reshape(-1)
        self.buf = torch.from_numpy(host).to(DEV)
        self.view = self.buf[:self.n]

    def get(self):
        host = self.buf.cpu().numpy()
        assert (host[self.n:] == self.sentinel).all(), "the launch wrote past the end of its buffer"
        return host[:self.n].copy()


def state_words(s0, cache, hp):
    """int32[STATE_LEN] as a launch finds it: the words it may touch 0 (cache: "zero"), every other word a sentinel; ``cache``
    "stale": corrections of another step, wrong doubles; "host": step_dev[0] = s0 + 1 already, the corrections of that step by
    host pow / sqrt from the float32 betas (what adam_prepare in nsplit.hip leaves: the prepared convention)."""
    w = np.full(of.STATE_LEN, SENTINEL[torch.int32], dtype=np.int32)
    w[list(of.STATE_WORDS)] = 0
    w[0], w[1] = s0, s0 + 1
    d = w[4:8].view(np.float64)
    if cache == "stale":
        w[1] = s0 + 7
        d[:] = (0.123, 0.456)
    elif cache == "host":
        w[0] = w[1] = s0 + 1
        d[:] = corrections(hp, s0 + 1)
    else:
        assert cache == "zero", cache
    return w


def corrections(hp, step):
    b1, b2 = of.f32(hp.beta1), of.f32(hp.beta2)
    return 1.0 - math.pow(b1, step), math.sqrt(1.0 - math.pow(b2, step))


def gradmax_words(norm, slot):
    """float32[GRADMAX_LEN]: the norm in ``slot``, smaller non-negative values in the other 15 slots, sentinels between them."""
    g = np.full(of.GRADMAX_LEN, SENTINEL[torch.float32], dtype=np.float32)
    for j in range(of.GRADMAX_SLOTS):
        g[j * of.SLOT_STRIDE] = np.float32(norm) if j == slot else np.float32(norm) * np.float32(j / 32.0)
    return g


def slots_of(g):
    return g[::of.SLOT_STRIDE][:of.GRADMAX_SLOTS]


def between_slots(g):
    return np.delete(g, np.arange(of.GRADMAX_SLOTS) * of.SLOT_STRIDE)


class Launch(object):
    """The device buffers of one optim_f64.Case and the launch on them."""

    def __init__(self, case, cache="zero", words=None, gradmax_on_device=False, ops=None):
        st, hp = case.state, case.hp
        self.case, self.hp = case, hp
        self.param, self.grad, self.m, self.v = Buf(st["param"]), Buf(case.grad), Buf(st["m"]), Buf(st["v"])
        self.target = Buf(st["target"]) if "target" in st else None
        self.target2 = Buf(st["target2"]) if "target2" in st else None
        self.words0 = state_words(case.s0, cache, hp) if words is None else np.array(words, dtype=np.int32)
        self.state = Buf(self.words0, torch.int32)
        self.gradmax = None
        if hp.clip_thres > 0.0:
            if gradmax_on_device:                                 # the inf-norm as the trainers get it: rpo_absmax_slots
                g = np.full(of.GRADMAX_LEN, SENTINEL[torch.float32], dtype=np.float32)
                g[::of.SLOT_STRIDE] = 0.0
                self.gradmax = Buf(g)
                ops.absmax(self.grad.view, self.gradmax.view)
            else:
                self.gradmax = Buf(gradmax_words(case.norm(), case.slot))
            self.gradmax0 = self.gradmax.get()
            assert np.isfinite(slots_of(self.gradmax0)).all() and float(slots_of(self.gradmax0).max()) == case.norm()

    def warm_cache(self, ops):
        """Cache condition "valid": a device launch on throw-away tensors, one step earlier, leaves this step's corrections.
        (For s0 = 0 that launch runs as step 0, where bc1 = 0 and step_size = inf: its throw-away tensors go NaN.  Only the
        bookkeeping it leaves is used, and that is asserted below.)"""
        hp = self.hp
        self.state.view[0] = self.case.s0 - 1
        self.state.view[1] = self.case.s0 - 1                     # stale: the throw-away launch recomputes its own
        t = [Buf(np.full(257, 0.5, np.float32)) for _ in range(4)]
        ops.adam_step(t[0].view, t[1].view, t[2].view, t[3].view, self.state.view, hp.lr, beta1=hp.beta1, beta2=hp.beta2)
        for b in t:
            b.get()
        w = self.state.get()
        assert w[0] == self.case.s0 and w[1] == self.case.s0 + 1 and w[4:8].view(np.float64)[0] != 0.0
        self.words0 = w

    def kwargs(self):
        return dict(self.hp.kwargs(), gradmax=None if self.gradmax is None else self.gradmax.view,
                    target=None if self.target is None else self.target.view)

    def run(self, ops, **extra):
        ops.adam_step(self.param.view, self.grad.view, self.m.view, self.v.view, self.state.view, **dict(self.kwargs(), **extra))
        return self

    def seg(self, **extra):
        """This launch as an entry of ops.adam_step_multi."""
        d = dict(self.kwargs(), param=self.param.view, grad=self.grad.view, exp_avg=self.m.view, exp_avg_sq=self.v.view,
                 step_dev=self.state.view, **extra)
        if self.target2 is not None:
            d.update(target2=self.target2.view, n2=self.case.n2)
        return d

    def results(self):
        r = dict(param=self.param.get(), m=self.m.get(), v=self.v.get(), grad=self.grad.get())
        if self.target is not None:
            r["target"] = self.target.get()
        if self.target2 is not None:
            r["target2"] = self.target2.get()
        return r

    def ratios(self, name, scalars="kernel"):
        """Assert the results within the tolerance of the float64 reference; prints and returns the ratios."""
        c = self.case
        r = of.step_ratios(self.results(), c.state, c.grad, c.hp, n2=c.n2, norm=c.norm(), scalars=scalars)
        print("%-34s %s" % (name, "  ".join("%s %.3f" % kv for kv in sorted(r.items()))))
        assert all(v <= 1.0 for v in r.values()), (name, r)
        return r

    def check_bookkeeping(self, reset_gradmax=True):
        """After an unprepared launch: step advanced, the next step's corrections cached, every counter back at 0, no other word
        of the state buffer touched; the 16 gradmax slots zeroed (or left) and no other word of that buffer touched."""
        s0, w = self.case.s0, self.state.get()
        assert w[0] == s0 + 1 and w[1] == s0 + 2, w[:2]
        assert w[2] == 0 and w[3] == 0, "arrival word"
        assert all(w[32 + 32 * k] == 0 and w[33 + 32 * k] == 0 for k in range(16)), "sub-counters"
        got, want = w[4:8].view(np.float64), np.array(corrections(self.hp, s0 + 2))
        assert (np.abs(got - want) <= 4 * np.spacing(want)).all(), (got, want)
        other = np.ones(of.STATE_LEN, bool)
        other[list(of.STATE_WORDS)] = False
        assert np.array_equal(w[other], self.words0[other]) and (w[other] == SENTINEL[torch.int32]).all()
        if self.gradmax is not None:
            g = self.gradmax.get()
            assert np.array_equal(between_slots(g), between_slots(self.gradmax0))
            if reset_gradmax:
                assert (slots_of(g) == 0.0).all()
            else:
                assert of.bitwise(slots_of(g), slots_of(self.gradmax0))


def same_bits(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert of.bitwise(a[k], b[k]), k


SINGLE = [c for c in of.step_cases() if "target2" not in c.state]
# the inf-norm by rpo_absmax_slots on the device instead of host-written slots: the Launch asserts it equal to the reference's,
# which for nan_under_clip is the norm over the elements that are not NaN
ON_DEVICE = set(c.name for c in SINGLE if c.name.startswith("size") or c.name == "nan_under_clip")


# ======================================================================================================== rpo_adam_step
@pytest.mark.parametrize("case", SINGLE, ids=str)
def test_adam_step(ops, case):
    """One launch from the case's state with the cache (a) empty, (b) left by a device launch, (c) stale: bitwise the same
    results, each within the tolerance of the float64 reference; bookkeeping as the header states it."""
    results = {}
    for cache in ("zero", "valid", "stale"):
        run = Launch(case, "zero" if cache == "valid" else cache, gradmax_on_device=case.name in ON_DEVICE, ops=ops)
        if cache == "valid":
            run.warm_cache(ops)
        run.run(ops)
        results[cache] = run.results()
        run.check_bookkeeping()
        if cache == "zero":
            run.ratios(case.name)
    same_bits(results["zero"], results["valid"])
    same_bits(results["zero"], results["stale"])
    got, st, r = results["zero"], case.state, of.EDGE_ROWS
    if case.name.startswith("edges"):
        for row in (r["zero"], r["stays_zero"], r["g_1e30"]):                    # an update of exactly 0
            assert of.bitwise(got["param"][row], st["param"][row])
        assert np.isinf(got["v"][r["g_1e30"]]) and np.isfinite(got["v"][r["g_1e20"]]) and got["v"][r["g_1e20"]] > 9e36
        bad = r["nan"]
        assert np.isnan(got["m"][bad]) and np.isnan(got["v"][bad])
        if case.hp.clamp_min0:                                                   # fmaxf(NaN, 0) = 0: pinned (rpo_hip.h)
            assert got["param"][bad] == 0.0 and got["param"][r["goes_negative"]] == 0.0 and (got["param"] >= 0.0).all()
        else:
            assert np.isnan(got["param"][bad]) and np.isnan(got["target"][bad])
        keep = np.ones(case.n, bool)
        keep[bad] = False
        assert all(np.isfinite(got[k][keep]).all() for k in ("param", "m", "target")) and int(np.isinf(got["v"]).sum()) == 1
    if case.name == "nan_under_clip":                                            # the device's inf-norm ignored the NaN elements
        bad = np.isnan(case.grad)
        assert case.name in ON_DEVICE and bad.sum() == 2 and np.isfinite(case.norm())
        assert all(np.isnan(got[k][bad]).all() and np.isfinite(got[k][~bad]).all() for k in ("param", "m", "v", "target", "grad"))
    if case.name.startswith("clip[below"):
        assert of.bitwise(got["grad"], case.grad)                                # coefficient exactly 1


def test_adam_step_keeps_gradmax_without_reset(ops):
    for name in ("size[257, s0=999]", "clip[above, slot 7]"):
        run = Launch(of.case(name)).run(ops, reset_gradmax=False)
        run.check_bookkeeping(reset_gradmax=False)
        run.ratios(name + " reset_gradmax=0")


def test_adam_step_clock(ops):
    """``clock`` advances by exactly 1 per unprepared launch, not at all when NULL is passed or the launch is prepared."""
    case = of.case("size[4097, s0=999]")
    clock = Buf([41], torch.int64)
    Launch(case).run(ops, clock=clock.view).check_bookkeeping()
    assert clock.get()[0] == 42
    Launch(case).run(ops, clock=clock.view)
    assert clock.get()[0] == 43
    Launch(case).run(ops)                                                         # NULL
    assert clock.get()[0] == 43
    Launch(case, "host").run(ops, clock=clock.view, prepared=True)
    assert clock.get()[0] == 43


@pytest.mark.parametrize("n", [257, 8449])
def test_adam_step_prepared(ops, n):
    """prepared = 1 is the form the headline runs.  The state an unprepared launch left behind, with step_dev[0] advanced by one
    on a copy, IS the prepared convention for the next step: the prepared launch on the copy and an unprepared launch on the
    original agree bit for bit, and the prepared launch leaves step_dev, gradmax and clock as they were.  Then the cache as
    the host computes it (what adam_prepare of nsplit.hip writes), against the float64 reference."""
    first = of.case("size[%d, s0=999]" % n)
    one = Launch(first).run(ops)
    res, words = one.results(), one.state.get()
    st = dict(param=res["param"], m=res["m"], v=res["v"], target=res["target"], step=first.s0 + 1)
    _, grad = of.make_state(n, 1000, first.hp, seed=21)
    second = of.Case("second step", st, grad, first.hp, slot=5)
    a = Launch(second, words=words).run(ops)
    a.check_bookkeeping()
    a.ratios("unprepared, second step [%d]" % n)
    pwords = words.copy()
    pwords[0] += 1
    clock = Buf([7], torch.int64)
    b = Launch(second, words=pwords).run(ops, prepared=True, clock=clock.view)
    same_bits(a.results(), b.results())
    assert np.array_equal(b.state.get(), pwords) and of.bitwise(b.gradmax.get(), b.gradmax0) and clock.get()[0] == 7
    c = Launch(second, "host").run(ops, prepared=True, clock=clock.view)
    c.ratios("prepared, host cache [%d]" % n)
    assert np.array_equal(c.state.get(), c.words0) and of.bitwise(c.gradmax.get(), c.gradmax0) and clock.get()[0] == 7


def test_adam_step_against_torch_scalars(ops):
    """Section "1 - beta" of DESIGN.md's parity notes: from torch.optim.Adam's own steady state (3000 float32 steps), at step
    100000 where both bias corrections are 1, ONE launch is compared with the reference under torch's scalar convention --
    float32(1 - beta) from the double betas instead of the kernel's float32(1) - float32(beta) -- at the same tolerance.  It
    passes: a single step carries (1 - beta2) * 1.3e-5 * g^2 = 0.11 eps32 * g^2 of the deviation.  The 1.3e-5 (108 eps32) that
    the deviation amounts to in exp_avg_sq builds up over thousands of steps (test_optim_f64.py::test_one_minus_beta_deviation)."""
    st, grad, own = of.torch_steady_state()
    case = of.Case("torch steady state", st, grad, of.HP_SETS["plain"])
    run = Launch(case).run(ops)
    run.check_bookkeeping()
    k = run.ratios("steady state, kernel scalars")
    t = run.ratios("steady state, torch scalars", scalars="torch")
    got = run.results()
    dv = of.worst(got["v"], own["v"], st["v"].astype(np.float64) + grad.astype(np.float64) ** 2)
    print("exp_avg_sq: kernel against torch's own float32 step: %.3f eps32 * (v + g^2)" % dv)
    assert k.keys() == t.keys()                                                  # (ratios() asserted each <= 1)


# ================================================================================================== rpo_adam_step_multi
def polyak_slice(n, tau):
    _, p, t = [c for c in of.polyak_cases() if c[0] == n][0]
    return p, t, Buf(p), Buf(t)


def check_polyak(name, target, p, t, tau):
    mag = np.abs(t.astype(np.float64)) + np.abs(p.astype(np.float64))
    r = of.worst(target.get(), of.polyak(p, t, tau), of.C_REF_TARGET * mag) / of.MARGIN
    print("%-34s target %.3f" % (name, r))
    assert r <= 1.0, (name, r)
    return r


@pytest.mark.parametrize("n2", [0, 1, 768, 8449])
@pytest.mark.parametrize("polyak_at", [0, 3])
def test_adam_step_multi(ops, n2, polyak_at):
    """Four slices of unequal size in one launch (the grid is sized by the largest: the short slices get idle workgroups, which
    still count in), against the float64 reference: actor with a second target over a prefix of n2 | DualAdam of 6 | critic of
    257 | a Polyak-only slice of 4096, in position 3 or in position 0 (then without a clock)."""
    runs = [Launch(of.case("target2[n2=%d]" % n2)), Launch(of.case("hp[dual, 6]")), Launch(of.case("size[257, s0=999]"))]
    tau = 0.005
    p, t, pbuf, tbuf = polyak_slice(4096, tau)
    segs = [r.seg() for r in runs]
    segs.insert(polyak_at, dict(polyak_only=True, param=pbuf.view, target=tbuf.view, tau=tau))
    clock = Buf([10], torch.int64)
    ops.adam_step_multi(segs, clock=clock.view if polyak_at == 3 else None)
    assert clock.get()[0] == (11 if polyak_at == 3 else 10)                      # once, by slice 0 only
    for r in runs:
        r.ratios("multi[n2=%d, polyak at %d] %s" % (n2, polyak_at, r.case.name))
        r.check_bookkeeping()
    check_polyak("multi polyak_only", tbuf, p, t, tau)
    assert of.bitwise(pbuf.get(), p)


def test_adam_step_multi_mixed_prepared(ops):
    """``prepared`` per slice: slice 0 unprepared and slice 2 prepared -- the clock advances once and slice 2's bookkeeping
    words stay; with every stepped slice prepared the clock is untouched.  Either way the results are the single launches'."""
    names = ("target2[n2=768]", "hp[dual, 6]", "size[257, s0=999]")
    single = Launch(of.case(names[1])).run(ops).results()
    for prepared in ((False, False, True), (True, True, True)):
        runs = [Launch(of.case(nm), "host" if pr else "zero") for nm, pr in zip(names, prepared)]
        clock = Buf([3], torch.int64)
        ops.adam_step_multi([r.seg(prepared=pr) for r, pr in zip(runs, prepared)], clock=clock.view)
        assert clock.get()[0] == (3 if all(prepared) else 4)
        for r, pr in zip(runs, prepared):
            r.ratios("multi prepared=%s %s" % (prepared, r.case.name))
            if pr:
                assert np.array_equal(r.state.get(), r.words0)
                assert r.gradmax is None or of.bitwise(r.gradmax.get(), r.gradmax0)
            else:
                r.check_bookkeeping()
        if not prepared[1]:                                                      # (prepared: host pow, not the device's bits)
            same_bits(runs[1].results(), single)


# ======================================================================================= rpo_absmax / rpo_absmax_slots
@pytest.mark.parametrize("n", of.ABSMAX_SIZES)
def test_absmax(ops, n):
    """Exact, wherever the maximum sits -- first, last, in the n % 4 tail, in the second pass of the float4 sweep, negative --
    accumulating on what the word held; the slotted form spreads over the 16 slots and writes no other word.  NaN elements --
    in any lane of a float4 of the sweep, a whole float4, in the n % 4 tail -- are skipped: the result is the maximum over the
    others, and an input of nothing but NaN leaves what was there, in both forms."""
    def slotted(values):
        g = np.full(of.GRADMAX_LEN, SENTINEL[torch.float32], dtype=np.float32)
        g[::of.SLOT_STRIDE] = 0.0
        g[3 * of.SLOT_STRIDE] = 0.25                                              # a previous partial maximum in slot 3
        gb = Buf(g)
        ops.absmax(values.view, gb.view)
        return g, gb.get()

    count = nans = 0
    for where in ("first", "last", "tail", "pass2"):
        for negative in (False, True):
            x, at = of.absmax_input(n, where, negative)
            if x is None:
                continue
            count += 1
            xb = Buf(x)
            for prev, want in ((0.0, 3.0), (1.0, 3.0), (5.0, 5.0)):              # a smaller previous value is replaced, a larger survives
                out = Buf([prev])
                ops.absmax(xb.view, out.view)
                assert out.get()[0] == want == of.absmax(x, prev), (n, where, negative, prev)
            _, got = slotted(xb)
            slots = slots_of(got)
            assert float(slots.max()) == 3.0 and (slots >= 0).all() and slots[3] >= 0.25, (n, where, negative, slots)
            assert (between_slots(got) == SENTINEL[torch.float32]).all()
            blocks = min(of.MAX_GRID, n // 4 // of.BLOCK)                         # workgroups that own at least one full float4 row
            if blocks >= 2:
                assert int((slots > 0.25).sum()) >= min(blocks, of.GRADMAX_SLOTS), slots
            assert of.bitwise(xb.get(), x)
    for where in ("body", "tail", "all"):
        x = of.absmax_nan_input(n, where)
        if x is None:
            continue
        nans += 1
        xb = Buf(x)
        top = 0.0 if where == "all" else 3.0
        for prev in (0.0, 1.0, 5.0):
            out = Buf([prev])
            ops.absmax(xb.view, out.view)
            assert of.bitwise(out.get(), [max(prev, top)]) and of.absmax(x, prev) == max(prev, top), (n, where, prev)
        before, got = slotted(xb)
        if where == "all":
            assert of.bitwise(got, before), (n, slots_of(got))                   # nothing written: no NaN reached the atomic
        else:
            slots = slots_of(got)
            assert np.isfinite(slots).all() and float(slots.max()) == 3.0 and (slots >= 0).all() and slots[3] >= 0.25, (n, where, slots)
            assert (between_slots(got) == SENTINEL[torch.float32]).all()
        assert np.array_equal(np.isnan(xb.get()), np.isnan(x))
    zeros = Buf(np.zeros(n, np.float32))
    for prev in (0.0, 2.0):
        out = Buf([prev])
        ops.absmax(zeros.view, out.view)
        assert out.get()[0] == prev
    print("absmax[%d]: %d placements of the maximum and %d of NaN exact" % (n, count, nans))
    assert count >= 2 and nans >= 1 + (n >= 4) + (n % 4 > 0 and n > 1)


# ============================================================================================================ rpo_polyak
@pytest.mark.parametrize("n", of.SIZES)
def test_polyak(ops, n):
    worst = 0.0
    for tau in of.POLYAK_TAUS:
        p, t, pbuf, tbuf = polyak_slice(n, tau)
        ops.polyak(pbuf.view, tbuf.view, tau)
        worst = max(worst, check_polyak("polyak[%d, tau=%g]" % (n, tau), tbuf, p, t, tau))
        got = tbuf.get()
        if tau == 0.0:
            assert of.bitwise(got, t)
        if tau == 1.0:
            assert of.bitwise(got, p)
        assert of.bitwise(pbuf.get(), p)


# ========================================================================================================= rpo_min_q_bwd
@pytest.mark.parametrize("n", of.MIN_Q_SIZES)
def test_min_q_bwd(ops, n):
    """Exactly the float64 autograd result rounded to float32 (w * scale, w in {0, 0.5, 1}), ties -- +0.0 against -0.0 and inf
    against inf among them -- split evenly.  NaN on either side or both: the kernel's comparisons are false, dq1 = 0 and
    dq2 = scale.  That is NOT torch: torch.minimum's backward hands both inputs the full gradient, dq1 = dq2 = scale
    (test_optim_f64.py::test_inputs_are_what_they_claim asserts it of the reference).  The kernel's behaviour is pinned here with
    its own values and stated as a deviation in rpo_hip.h."""
    scale = -1.0 / 300
    q1, q2 = of.min_q_input(n)
    d1, d2 = Buf(np.zeros(n)), Buf(np.zeros(n))
    ops.min_q_bwd(Buf(q1).view, Buf(q2).view, scale, d1.view, d2.view)
    r1, r2 = of.min_q_bwd(q1, q2, scale)
    assert np.array_equal(d1.get(), r1.astype(np.float32)) and np.array_equal(d2.get(), r2.astype(np.float32))
    assert np.array_equal(r1.astype(np.float32).astype(np.float64), r1)           # (the reference is float32-exact)
    print("min_q_bwd[%d]: exact, %d ties" % (n, int((q1 == q2).sum())))
    if n > 2:
        q1, q2 = q1.copy(), q2.copy()
        q1[0], q2[1], q1[2], q2[2] = np.nan, np.nan, np.nan, np.nan
        ops.min_q_bwd(Buf(q1).view, Buf(q2).view, scale, d1.view, d2.view)
        g1, g2 = d1.get(), d2.get()
        assert (g1[:3] == 0.0).all() and (g2[:3] == np.float32(scale)).all()
        t1, t2 = of.min_q_bwd(q1[:3], q2[:3], scale)                             # (what torch does instead)
        assert (t1 == of.f32(scale)).all() and (t2 == of.f32(scale)).all()
        assert np.array_equal(g1[3:], r1[3:].astype(np.float32)) and np.array_equal(g2[3:], r2[3:].astype(np.float32))
