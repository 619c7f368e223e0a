"""The float64 yardstick of the optimiser kernel tests (tests/optim_f64.py): its agreement with torch.optim.Adam in float64 and with
the float32 oracle, the measurement of C_REF_* -- how far a float32 evaluation of the kernel's formulas lands from float64, in units
of eps32 * magnitude sum -- and the proof that the comparison the GPU tests make (optim_f64.step_ratios, exact absmax) fails for
each of a list of subtly wrong kernels.  Wrong kernels exist only as mutations of the numpy emulation.  CPU only."""
import numpy as np
import pytest
import torch

import optim_f64 as of
from oracle import train_ops as oracle_ops


# ============================================================================================== reference against torch
@pytest.mark.parametrize("mode", ["plain", "maximize", "weight_decay", "betas_eps"])
def test_reference_matches_torch_adam_in_float64(mode):
    """adam(scalars="torch") on float64 state against torch.optim.Adam on float64 parameters, five chained steps."""
    hp = dict(plain=of.HP("plain", 3e-4), maximize=of.HP("maximize", 0.2, maximize=True),
              weight_decay=of.HP("wd", 3e-4, weight_decay=1e-2), betas_eps=of.HP("be", 1e-3, betas=(0.5, 0.9), eps=1e-3))[mode]
    rng = np.random.RandomState(4)
    n = 1000
    p = torch.nn.Parameter(torch.from_numpy(0.1 * rng.randn(n)))
    opt = torch.optim.Adam([p], lr=hp.lr, betas=(hp.beta1, hp.beta2), eps=hp.eps, weight_decay=hp.weight_decay, maximize=hp.maximize)
    st = dict(param=p.detach().numpy().copy(), m=np.zeros(n), v=np.zeros(n), step=0)
    for it in range(5):
        g = rng.randn(n) * (0.05 if it % 2 else 1.0)
        p.grad = torch.from_numpy(g.copy())
        opt.step()
        out = of.adam(st, g, hp, scalars="torch")
        sd = opt.state[p]
        # float64 round-off: a few eps64 of the magnitude sums (|m| + |g| <= 6, v + g^2 <= 30, |w| + |update| <= 1)
        np.testing.assert_allclose(out["m"], sd["exp_avg"].numpy(), rtol=0, atol=6 * 4 * 2.3e-16)
        np.testing.assert_allclose(out["v"], sd["exp_avg_sq"].numpy(), rtol=0, atol=30 * 4 * 2.3e-16)
        np.testing.assert_allclose(out["param"], p.detach().numpy(), rtol=0, atol=4 * 2.3e-16)
        np.testing.assert_allclose(out["update_raw"], p.detach().numpy() - st["param"], rtol=1e-12, atol=4 * 2.3e-16)
        st = dict(param=out["param"], m=out["m"], v=out["v"], step=out["step"])
    assert st["step"] == 5 == int(opt.state[p]["step"])


@pytest.mark.parametrize("convention", ["torch", "kernel"])
def test_reference_matches_the_float32_oracle_and_torch_itself(convention):
    """oracle/train_ops.adam_step (numpy float32) and torch.optim.Adam's own float32 step from a steady state, each within the GPU
    tests' tolerance of the reference.  One step at 100000 cannot tell the two scalar conventions apart (0.11 eps32 of g^2 on
    exp_avg_sq): both pass.  At step 1000 it can, on parameters that are 0 or tiny: sqrt(1 - beta2^t) from the float32 beta2 is
    3.7e-6 (31 eps32) from the double beta2's, so the oracle -- torch's convention -- misses the "kernel" reference's update."""
    for hp in (of.HP_SETS["plain"], of.HP("dual", 0.2, maximize=True, clamp_min0=True), of.HP("wd", 3e-4, weight_decay=1e-2)):
        st, g = of.make_state(4099, 999, hp, seed=8)
        w, m, v = st["param"].copy(), st["m"].copy(), st["v"].copy()
        oracle_ops.adam_step(w, g.copy(), m, v, st["step"], hp.lr, weight_decay=hp.weight_decay, maximize=hp.maximize,
                             clamp_min0=hp.clamp_min0)
        r = of.step_ratios(dict(param=w, m=m, v=v, grad=g), st, g, hp, scalars=convention)
        if convention == "kernel":                               # (the oracle takes its bias corrections from the double betas)
            assert 1.0 < r.pop("update") < 8.0
        assert max(r.values()) <= 1.0, (hp, r)
    st, g, own = of.torch_steady_state()
    r = of.step_ratios(own, st, g, of.HP_SETS["plain"], scalars=convention)
    print("torch's own float32 step against the %r reference: %s" % (convention, r))
    assert max(r.values()) <= 1.0, r


def test_one_minus_beta_deviation():
    """The kernel forms 1 - beta2 as float32(1) - float32(0.999), torch as float32(1 - 0.999): 1.3e-5 apart.  3000 steps of the
    float32 emulation on the same gradients, once with each: exp_avg_sq ends 1.3e-5 apart (about 110 eps32), the denominator half
    of that, the parameters by the accumulated difference of the updates -- harmless for learning, invisible in one step."""
    kernel, torch_ = np.float32(1) - np.float32(0.999), np.float32(1 - 0.999)
    rel = float(torch_) / float(kernel) - 1
    assert 1.2e-5 < rel < 1.4e-5
    hp = of.HP_SETS["plain"]
    rng = np.random.RandomState(12)
    n = 512
    mean = rng.randn(n).astype(np.float32)
    a = dict(param=(0.1 * rng.randn(n)).astype(np.float32), m=np.zeros(n, np.float32), v=np.zeros(n, np.float32), step=0)
    b = dict(a)
    for _ in range(3000):
        g = mean * (1 + 0.1 * rng.randn(n)).astype(np.float32)
        ra, rb = of.emulate_f32(a, g, hp), of.emulate_f32(b, g, hp, one_minus_beta="torch")
        a = dict(param=ra["param"], m=ra["m"], v=ra["v"], step=a["step"] + 1)
        b = dict(param=rb["param"], m=rb["m"], v=rb["v"], step=b["step"] + 1)
    dv = b["v"].astype(np.float64) / a["v"].astype(np.float64) - 1
    print("exp_avg_sq after 3000 steps: torch's 1 - beta2 over the kernel's - 1 = %.3e mean (%.0f eps32), %.3e worst"
          % (dv.mean(), dv.mean() / of.EPS32, np.abs(dv).max()))
    # v is the steady state (1 - beta2) g^2 / (1 - float32(beta2)) times 1 - beta2^3000 = 0.95: the whole 1.3e-5 is in it
    assert 0.8 * rel < dv.mean() < 1.1 * rel and np.abs(dv).max() < 2 * rel
    # the bias correction: sqrt(1 - beta2^t) from float32(0.999) against 0.999, t / 2 * 1.3e-8 * beta2^t / (1 - beta2^t)
    for t, lo, hi in ((1, 6.0e-6, 6.8e-6), (1000, 3.4e-6, 4.0e-6), (100000, 0.0, 1e-12)):
        k, o = of._scalars(hp, t, "kernel", np.float32), of._scalars(hp, t, "torch", np.float64)
        assert lo <= abs(np.sqrt(1 - np.float64(np.float32(0.999)) ** t) / np.sqrt(1 - 0.999 ** t) - 1) <= hi, t
        assert abs(k["bc2s"] / o["bc2s"] - 1) <= hi + of.EPS32
    # one step from the same state: (1 - beta2) g^2 * 1.3e-5 -- a ninth of an eps32 of the magnitude sum
    g = mean
    one = of.emulate_f32(a, g, hp)["v"].astype(np.float64) - of.emulate_f32(a, g, hp, one_minus_beta="torch")["v"].astype(np.float64)
    assert np.abs(one / (of.EPS32 * (a["v"] + g.astype(np.float64) ** 2))).max() < 1.0


# ====================================================================================================== yardstick
def measure_c_ref():
    c = dict(exp_avg=0.0, exp_avg_sq=0.0, update=0.0, target=0.0, grad=0.0)
    exact = 0.0
    term1 = [0.0, 0.0]
    for case in of.step_cases():
        got = of.emulate_f32(case.state, case.grad, case.hp, n2=case.n2)
        term1 = [max(a, b) for a, b in zip(term1, of.update_errors_term1(got, case.state, case.grad, case.hp, n2=case.n2))]
        for k, v in of.step_errors(got, case.state, case.grad, case.hp, n2=case.n2).items():
            if k in c:
                c[k] = max(c[k], v)
            else:
                exact = max(exact, v)
    for n, p, t in of.polyak_cases():
        for tau in of.POLYAK_TAUS:
            ref = of.polyak(p, t, tau)
            c["target"] = max(c["target"], of.worst(of.emulate_polyak(p, t, tau), ref, np.abs(t.astype(np.float64)) + np.abs(p.astype(np.float64))))
    return c, exact, term1


def test_yardstick():
    c, exact, term1 = measure_c_ref()
    print("measured C_REF:", c, "update over |w| + |update| alone: all %.3f, |w| >= %g %.3f" % (term1[0], of.ORDINARY_W, term1[1]))
    assert exact == 0.0                                          # the exact conditions hold for the emulation
    const = dict((k, getattr(of, name)) for k, name in of.C_OF.items())
    for k, v in c.items():
        assert np.isfinite(v) and v > 0, (k, v)
        assert const[k] / 2 <= v <= const[k], (k, v, const[k])
    # the issue's magnitude sum for the update, |w| + |update|: no yardstick where w is 0 or tiny, the same where it is ordinary
    assert of.C_REF_UPDATE_TERM1_ALL / 2 <= term1[0] <= of.C_REF_UPDATE_TERM1_ALL, term1
    assert of.C_REF_UPDATE_TERM1_ORDINARY / 2 <= term1[1] <= of.C_REF_UPDATE_TERM1_ORDINARY, term1


# ====================================================================================================== mutations
def _caught_by(mut):
    """Names of the GPU tests' comparisons that fail for the emulation with mutation ``mut`` (None: the faithful emulation)."""
    caught = []
    for case in of.step_cases():
        if case.n > 10000 and case.s0 != 999:
            continue                                              # (the large size once: a mutation caught here is caught)
        got = of.emulate_f32(case.state, case.grad, case.hp, n2=case.n2, mut=mut)
        r = of.step_ratios(got, case.state, case.grad, case.hp, n2=case.n2)
        caught += ["%s: %s" % (case.name, k) for k, v in r.items() if not v <= 1.0]
    for n in of.ABSMAX_SIZES:                                     # rpo_absmax: exact
        for where in ("first", "last", "tail", "pass2"):
            for negative in (False, True):
                x, at = of.absmax_input(n, where, negative)
                if x is not None and float(of.emulate_absmax(x, mut=mut)) != of.absmax(x):
                    caught.append("absmax[%d, %s]" % (n, where))
        for where in ("body", "tail", "all"):
            x = of.absmax_nan_input(n, where)
            if x is not None and float(of.emulate_absmax(x, prev=0.25, mut=mut)) != of.absmax(x, 0.25):
                caught.append("absmax[%d, nan %s]" % (n, where))
    return caught


def test_the_faithful_emulation_passes_every_comparison():
    assert _caught_by(None) == []


EXPECT = dict(bc_step_minus_1=("size[257, s0=1]: update", "size[257, s0=999]: update"),
              eps_dropped=("edges[edges]: update", "hp[eps, 257]: update"),
              eps_in_sqrt=("hp[eps, 8449]: update", "edges[edges]: update"),
              wd_sign=("hp[weight_decay, 257]: exp_avg", "hp[weight_decay, 8449]: exp_avg_sq"),
              clamp_after_target=("hp[dual_target, 257]: target", "edges[edges_dual]: target"),
              clip_no_1e6=("clip[at, slot 0]: grad", "clip[just_above, slot 15]: grad", "clip[just_above, slot 7]: exp_avg"),
              n2_inclusive=("target2[n2=0]: target2_tail", "target2[n2=1]: target2_tail", "target2[n2=768]: target2_tail"),
              absmax_tail_skipped=("absmax[5, tail]", "absmax[1, first]", "absmax[1025, last]", "absmax[2097159, tail]"),
              maximize_before_writeback=("hp[maximize_clip, 257]: grad", "hp[maximize_clip, 8449]: grad"))


@pytest.mark.parametrize("mut", of.MUTATIONS)
def test_mutation_is_caught(mut):
    caught = _caught_by(mut)
    print("%s: caught by %d comparisons, e.g. %s" % (mut, len(caught), caught[:6]))
    assert caught, mut
    for name in EXPECT[mut]:
        assert name in caught, (mut, name, caught[:20])


def test_every_listed_mutation_has_its_test():
    assert set(EXPECT) == set(of.MUTATIONS) and len(of.MUTATIONS) == 9


# ====================================================================================================== inputs
def test_inputs_are_what_they_claim():
    assert [of.workgroups(n) for n in of.SIZES] == [1, 1, 1, 1, 2, 16, 17, 34, 2048]
    assert of.SIZES[-1] - 2048 * 256 == 517                       # ragged second grid-stride pass of adam_body
    assert len(of.STATE_WORDS) == 40 and max(of.STATE_WORDS) < of.STATE_LEN
    names = [c.name for c in of.step_cases()]
    assert len(names) == len(set(names))
    # the element edges, in the reference
    c = of.case("edges[edges]")
    ref, r = of.adam(c.state, c.grad, c.hp), of.EDGE_ROWS
    assert ref["update"][r["zero"]] == 0.0 and ref["m"][r["zero"]] == 0.0
    assert np.isfinite(ref["v"][r["g_1e20"]]) and ref["v"][r["g_1e20"]] > 9e36 and ref["update"][r["g_1e20"]] != 0.0
    assert np.isinf(ref["v"][r["g_1e30"]]) and ref["update"][r["g_1e30"]] == 0.0
    emu = of.emulate_f32(c.state, c.grad, c.hp)
    assert np.isinf(emu["v"][r["g_1e30"]]) and emu["param"][r["g_1e30"]] == c.state["param"][r["g_1e30"]]
    assert emu["v"][r["g_1e_25"]] == 0.0 and emu["m"][r["g_1e_25"]] != 0.0          # g g underflows, g does not
    bad = r["nan"]
    assert all(np.isnan(ref[k][bad]) for k in ("param", "m", "v", "target"))
    finite = np.ones(of.EDGE_N, bool)
    finite[[bad, r["g_1e30"]]] = False
    assert all(np.isfinite(ref[k][finite]).all() for k in ("param", "m", "v", "target"))
    d = of.case("edges[edges_dual]")
    ref = of.adam(d.state, d.grad, d.hp)
    assert ref["param"][r["stays_zero"]] == 0.0 and ref["update"][r["stays_zero"]] == 0.0
    assert ref["param"][r["goes_negative"]] == 0.0 and d.state["param"][r["goes_negative"]] + ref["update_raw"][r["goes_negative"]] < -0.1
    assert ref["param"][bad] == 0.0 and np.isnan(ref["m"][bad])                       # fmaxf: the kernel convention
    assert np.isnan(of.adam(d.state, d.grad, d.hp, scalars="torch")["param"][bad])
    # the NaN elements under the clip (float4 body and tail of the inf-norm's sweep): the norm is over the others, and they are
    # clipped by it
    c = of.case("nan_under_clip")
    ref = of.adam(c.state, c.grad, c.hp)
    assert c.n % 4 == 1 and list(np.flatnonzero(np.isnan(c.grad))) == [100, c.n - 1]
    assert 0.0 < ref["coef"] < 1.0 and np.array_equal(np.isnan(ref["param"]), np.isnan(c.grad))
    assert ref["coef"] == of.clip_coef(float(np.nanmax(np.abs(c.grad))), of.f32(0.2)) and c.norm() == float(np.nanmax(np.abs(c.grad)))
    # clip cases: coefficient exactly 1 below the threshold, below 1 AT it (the 1e-6)
    assert of.adam(*_sg("clip[below, slot 0]"))["coef"] == 1.0
    assert 0.99999 < of.adam(*_sg("clip[at, slot 0]"))["coef"] < 1.0
    assert of.absmax(of.case("clip[at, slot 15]").grad) == of.f32(0.2)
    # absmax inputs: a second float4 pass exists only at the last size
    assert [n for n in of.ABSMAX_SIZES if of.absmax_input(n, "pass2", False)[0] is not None] == [4 * 2048 * 256 + 7]
    assert [n for n in of.ABSMAX_SIZES if of.absmax_input(n, "tail", False)[0] is None] == [4, 1024]
    x, at = of.absmax_input(1025, "tail", True)
    assert at == 1024 and x[at] == -3.0 and np.abs(np.delete(x, at)).max() < 0.5
    # absmax NaN inputs: every lane of a float4 and a whole float4 in the body; the tail's first element; everything
    x = of.absmax_nan_input(1025, "body")
    bad = np.flatnonzero(np.isnan(x))
    assert set(bad % 4) == {0, 1, 2, 3} and np.isnan(x[4:8]).all() and bad.max() < 1024 and x[1024] == -3.0 and of.absmax(x) == 3.0
    x = of.absmax_nan_input(7, "tail")
    assert list(np.flatnonzero(np.isnan(x))) == [4] and x[6] == -3.0
    x = of.absmax_nan_input(1025, "tail")
    assert list(np.flatnonzero(np.isnan(x))) == [1024] and x[1023] == -3.0
    assert [n for n in of.ABSMAX_SIZES if of.absmax_nan_input(n, "body") is None] == [1, 2, 3]
    assert [n for n in of.ABSMAX_SIZES if of.absmax_nan_input(n, "tail") is None] == [1, 4, 1024]
    assert all(np.isnan(of.absmax_nan_input(n, "all")).all() and of.absmax(of.absmax_nan_input(n, "all"), 0.25) == 0.25
               for n in of.ABSMAX_SIZES)
    # min_q inputs hold every special pair
    q1, q2 = of.min_q_input(257)
    assert np.signbit(q2[0]) and not np.signbit(q1[0]) and q1[0] == q2[0] and np.isinf(q1[6]) and np.isinf(q2[6])
    d1, d2 = of.min_q_bwd(q1, q2, -1.0 / 300)
    s = of.f32(-1.0 / 300)
    assert set(np.unique(d1 / s)) == {0.0, 0.5, 1.0} and np.array_equal(d1 + d2, np.full(257, s))
    assert d1[0] == d2[0] == 0.5 * s and d1[6] == 0.5 * s and d1[2] == 0.0 and d1[3] == s
    # NaN on either side or both: torch.minimum's backward hands BOTH inputs the full gradient (the kernel: dq1 = 0, dq2 = scale,
    # a deviation stated in rpo_hip.h and pinned by test_optim_f64_gpu.py::test_min_q_bwd)
    nan = np.float32(np.nan)
    d1, d2 = of.min_q_bwd(np.array([nan, 1.0, nan], np.float32), np.array([1.0, nan, nan], np.float32), -1.0 / 300)
    assert (d1 == s).all() and (d2 == s).all()


def _sg(name):
    c = of.case(name)
    return c.state, c.grad, c.hp
