"""``keep_best`` on the MI355X: the device-side choice of the best evaluation point of a curve-mode run
(``rpo_eval_keep_best``) and what the trainers build on it (``trainer.best``, ``restore_best()``, ``using_best()``, checkpoints).

The yardstick of the criterion is ``wins_numpy`` below, a restatement of include/rpo_hip.h in numpy that this file carries
itself; the yardstick of the kept parameters is the actor's span of a second trainer with the same seed, copied where the
loop places its evaluations.  Everything is compared bit for bit: the kernels copy and compare, they do not compute.
"""
import numpy as np
import pytest
import torch

from rpo_amd.algo import BestPolicy, curve_seed

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
CURVE_LEN, C_STEP, C_EPISODES, C_RET, C_LENGTH, C_VIOL, C_NONFINITE = 16, 0, 1, 2, 12, 13, 14
NAN, INF = float("nan"), float("inf")


# ------------------------------------------------------------------------------------------------ the criterion in numpy
def rate_numpy(row):
    return INF if row[C_LENGTH] == 0 else row[C_VIOL] / row[C_LENGTH]


def wins_numpy(row, best_row, best_point, max_rate):
    """The candidate ``row`` is taken over the incumbent ``best_row`` (``best_point`` < 0: there is none)."""
    ret = row[C_RET]
    if row[C_NONFINITE] > 0 or np.isnan(ret):
        return False                                             # ineligible: never taken
    if best_point < 0:
        return True
    rate, best_rate, best_ret = rate_numpy(row), rate_numpy(best_row), best_row[C_RET]
    safe, best_safe = rate <= max_rate, best_rate <= max_rate
    if safe and not best_safe:
        return True
    if safe and best_safe:
        return ret > best_ret
    if not safe and not best_safe:
        return rate < best_rate or (rate == best_rate and ret > best_ret)
    return False


def choose_numpy(rows, max_rate):
    """-> (k*, [taken?]) of a sequence of curve rows, -1 while none is held."""
    held, taken = -1, []
    for k, row in enumerate(rows):
        take = wins_numpy(row, rows[held] if held >= 0 else np.zeros(CURVE_LEN), held, max_rate)
        taken.append(take)
        if take:
            held = k
    return held, taken


def make_row(ret, viol, length, nonfinite=0.0, step=0.0, std=1.0):
    row = np.zeros(CURVE_LEN)
    row[C_STEP], row[C_EPISODES], row[C_RET], row[C_RET + 1] = step, 16.0, ret, std
    row[C_LENGTH], row[C_VIOL], row[C_NONFINITE] = length, viol, nonfinite
    return row


#: (max_violation_rate, rows, the takes a reader expects): every branch of the criterion
SEQUENCES = [
    (0.25, [
        make_row(NAN, 0, 200),                # 0  ineligible first point: NaN return
        make_row(5.0, 0, 200, nonfinite=1),   # 1  ineligible: a non-finite episode
        make_row(1.0, 100, 200),              # 2  the first eligible point (unsafe, rate 0.5): taken
        make_row(1.0, 100, 200, std=2.0),     # 3  unsafe, rate and return tie: the incumbent stays
        make_row(2.0, 100, 200),              # 4  unsafe, rate ties, return strictly higher: taken
        make_row(100.0, 120, 200),            # 5  unsafe, higher rate: rejected whatever the return
        make_row(-5.0, 80, 200),              # 6  unsafe, strictly lower rate: taken
        make_row(1000.0, 0, 0),               # 7  LENGTH == 0: rate +inf, rejected
        make_row(-10.0, 50, 200),             # 8  rate exactly at the boundary: safe, beats the unsafe incumbent
        make_row(1e6, 51, 200),               # 9  just above the boundary: unsafe does not beat safe
        make_row(-10.0, 0, 200),              # 10 safe, return ties (the lower rate does not count): the incumbent stays
        make_row(-9.5, 20, 200),              # 11 safe, strictly higher return: taken
        make_row(-9.5, 20, 200, std=3.0),     # 12 safe, tie: stays
        make_row(1e9, 0, 200, nonfinite=3),   # 13 ineligible although safe and high
        make_row(NAN, 0, 200),                # 14 ineligible
        make_row(3.0, 50, 200),               # 15 safe at the boundary, higher: taken
        make_row(2.0, 0, 200),                # 16 safe, lower return: rejected
     ], [0, 0, 1, 0, 1, 0, 1, 0, 1, 0, 0, 1, 0, 0, 0, 1, 0]),
    (0.0, [                                   # keep_best=True
        make_row(1.0, 0, 0),                  # 0  LENGTH == 0 and no incumbent: taken (rate +inf)
        make_row(-7.0, 3, 100),               # 1  unsafe, finite rate < +inf: taken
        make_row(50.0, 3, 100, nonfinite=1),  # 2  ineligible
        make_row(-8.0, 0, 100),               # 3  safe beats unsafe
        make_row(-8.0, 0, 50),                # 4  tie: stays
        make_row(99.0, 1, 100000),            # 5  unsafe does not beat safe
     ], [1, 1, 0, 1, 0, 0]),
]


# ------------------------------------------------------------------------------------------------ 1. kernel vs numpy
def pattern(n, call):
    """Unique per call and position: int32 bit patterns (compared as bits, never as numbers)."""
    return ((np.int32(call + 1) << 17) | np.arange(n, dtype=np.int32)).astype(np.int32)


@pytest.fixture(scope="module")
def hip():
    from rpo_amd import ops
    assert torch.cuda.is_available()
    return ops


GUARD = 8


@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 256, 1027, 65537])
def test_kernel_equals_the_numpy_criterion(hip, n):
    """Every sequence through ``ops.eval_keep_best`` for every pair of offsets (0..3 floats from a 16-byte boundary) of src
    and best: after every call best_point, best_row (bits) and best (bits) are the restatement's, the guard floats around
    best and all of src are untouched."""
    call = 0
    for so in range(4):
        for bo in range(4):
            src_buf = torch.zeros(n + 2 * GUARD + 4, dtype=torch.int32, device=DEV)
            best_buf = torch.full((n + 2 * GUARD + 4,), -7, dtype=torch.int32, device=DEV)
            assert src_buf.data_ptr() % 16 == 0 and best_buf.data_ptr() % 16 == 0
            src = src_buf[GUARD + so:GUARD + so + n].view(torch.float32)
            best = best_buf[GUARD + bo:GUARD + bo + n].view(torch.float32)
            assert src.data_ptr() % 16 == 4 * so and best.data_ptr() % 16 == 4 * bo
            for max_rate, rows, _ in SEQUENCES:
                best_buf.fill_(-7)
                best_row = torch.zeros(CURVE_LEN, dtype=torch.float64, device=DEV)
                best_point = torch.full((1,), -1, dtype=torch.int64, device=DEV)
                want_best = np.full(n + 2 * GUARD + 4, -7, dtype=np.int32)
                want_row, held = np.zeros(CURVE_LEN), -1
                for k, row in enumerate(rows):
                    pat = pattern(n, call)
                    call += 1
                    src_np = np.zeros(n + 2 * GUARD + 4, dtype=np.int32)
                    src_np[GUARD + so:GUARD + so + n] = pat
                    src_buf.copy_(torch.from_numpy(src_np))
                    hip.eval_keep_best(src, best, torch.tensor(row, device=DEV), best_row, best_point, k, max_rate)
                    if wins_numpy(row, want_row, held, max_rate):
                        want_row, held = row.copy(), k
                        want_best[GUARD + bo:GUARD + bo + n] = pat
                    where = (n, so, bo, max_rate, k)
                    assert int(best_point.cpu()[0]) == held, where
                    assert best_row.cpu().numpy().tobytes() == want_row.tobytes(), where
                    assert best_buf.cpu().numpy().tobytes() == want_best.tobytes(), where
                    assert src_buf.cpu().numpy().tobytes() == src_np.tobytes(), where


def test_keep_best_refuses_bad_arguments(hip):
    from rpo_amd import _lib
    lib = _lib.load()
    ARG, NULL = _lib.CONST["RPO_ERR_ARG"], _lib.CONST["RPO_ERR_NULL"]
    assert lib.rpo_eval_keep_best(0, None, None, None, None, None, 0, 0.0, None) == ARG
    assert lib.rpo_eval_keep_best(4, None, None, None, None, None, -1, 0.0, None) == ARG
    assert lib.rpo_eval_keep_best(4, None, None, None, None, None, 0, -0.5, None) == ARG
    assert lib.rpo_eval_keep_best(4, None, None, None, None, None, 0, NAN, None) == ARG
    assert lib.rpo_eval_keep_best(4, None, None, None, None, None, 0, 0.0, None) == NULL
    x, r, p = torch.zeros(8, device=DEV), torch.zeros(16, dtype=torch.float64, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
    with pytest.raises(_lib.RpoHipError):
        hip.eval_keep_best(x, x[:4], r, r.clone(), p, 0, 0.0)    # lengths differ
    with pytest.raises(_lib.RpoHipError):
        hip.eval_keep_best(x, x.clone(), r[:8], r.clone(), p, 0, 0.0)


# ------------------------------------------------------------------------------------------------ whole runs
from test_eval_curve import _fresh  # noqa: E402

#: Chosen from the rows the runs print (seeds 11-13 were looked at), so that the points hold safe and unsafe ones, at least two
#: takes and at least one rejection -- asserted below on the harvested rows.  ``skip``: iterations trained without evaluation
#: in front of the first point (the first points of a fresh CartSafe policy have the longest episodes and no violation: a run
#: evaluated from its start takes point 0 and nothing else).
#: FUSED, as measured: rates 0, .21, .34, .011, 0, 0, 0 and returns 12.6, 11.8, 11.6, 11.6, 11.5, 12.75, 14.75 -> takes 0, 5, 6.
#: STEPWISE: rates 29/96, 32/96, 28/96 -> take (no incumbent), rejected (higher rate), take (safe).
FUSED = dict(algo="ddpg", envname="cart", n_envs=64, episodes=16, eval_fre=10, skip=20, iters=91, rate=0.05, seed=12)
STEPWISE = dict(algo="ddpg", envname="evopf256", n_envs=16, episodes=4, eval_fre=3, skip=0, iters=10, rate=0.3, seed=11)
_RUNS = {}


def _trainer(hip, cfg, monkeypatch, keep=True, curve=True, **more):
    monkeypatch.setenv("RPO_VERBOSE", "0")
    kw = dict(use_graph=True, capacity=64, eval_fre=cfg["eval_fre"], seed=cfg["seed"])
    if curve:
        kw["eval_episodes"] = cfg["episodes"]
    if keep:
        kw["keep_best"] = cfg["rate"]
    kw.update(more)
    return _fresh(cfg["algo"], cfg["envname"], hip, DEV, cfg["n_envs"], **kw)


def _advance(tr, cfg, upto=None):
    """Train to iteration ``upto`` (default: the whole run): ``skip`` iterations without evaluation, the rest with."""
    upto = cfg["iters"] if upto is None else upto
    if tr._t < cfg["skip"]:
        tr.run_steps(cfg["skip"] - tr._t, eval=False)
    tr.run_steps(upto - tr._t, eval=True)


def _span(tr):
    flat = tr.agent.flat
    return flat.param(flat.actor_range)


def _twin(hip, cfg, monkeypatch):
    """The same run without curve mode; where the loop places its evaluation: the blocking evaluate() with the curve's seed and
    a copy of the actor's span.  -> [(step, EvalResult, span)]"""
    key = ("twin", cfg["envname"])
    if key not in _RUNS:
        b = _trainer(hip, cfg, monkeypatch, keep=False, curve=False)
        out = []

        def fake_eval(rendering=False):
            r = b.evaluate(episodes=cfg["episodes"], seed=curve_seed(b.seed, len(out)))
            out.append((b._t, r, _span(b).clone()))
            return r.summary()
        b.eval = fake_eval
        _advance(b, cfg)
        torch.cuda.synchronize()
        _RUNS[key] = (out, b.agent.flat.data.clone())
    return _RUNS[key]


def _kept(hip, cfg, monkeypatch, overlap=1):
    key = ("kept", cfg["envname"], overlap)
    if key not in _RUNS:
        a = _trainer(hip, cfg, monkeypatch, schedule=dict(eval_overlap=overlap))
        _advance(a, cfg)
        _RUNS[key] = a
    return _RUNS[key]


def _check_run(hip, cfg, monkeypatch, overlap, path):
    a = _kept(hip, cfg, monkeypatch, overlap)
    rows = a.eval_curve.rows
    kstar, taken = choose_numpy(rows, cfg["rate"])
    rates = [rate_numpy(r) for r in rows]
    print(cfg["envname"], "overlap", overlap, "rates", rates, "returns", list(rows[:, C_RET]), "taken", taken, "k*", kstar)
    best = a.best
    assert a.eval_curve_last.path == path and a._curve.overlap == bool(overlap and path == "fused")
    assert best is not None and best.point == kstar and best.step == int(rows[kstar, C_STEP])
    assert best.row.rows[0].tobytes() == rows[kstar].tobytes()
    points, _ = _twin(hip, cfg, monkeypatch)
    assert [t for t, _, _ in points] == list(rows[:, C_STEP].astype(int))
    assert torch.equal(best.params, points[kstar][2])
    return a, rows, taken, rates


@pytest.mark.parametrize("overlap", [1, 0])
def test_whole_run_fused(hip, overlap, monkeypatch):
    a, rows, taken, rates = _check_run(hip, FUSED, monkeypatch, overlap, "fused")
    assert 6 <= len(rows) <= 8
    # not vacuous: safe and unsafe points, at least two takes, at least one rejection
    assert sum(taken) >= 2 and taken.count(False) >= 1
    assert any(r <= FUSED["rate"] for r in rates) and any(r > FUSED["rate"] for r in rates)
    if overlap == 0:                                            # both forms keep the same point and the same bits
        o = _kept(hip, FUSED, monkeypatch, 1).best
        i = a.best
        assert o.point == i.point and o.row.rows.tobytes() == i.row.rows.tobytes() and torch.equal(o.params, i.params)


def test_whole_run_stepwise(hip, monkeypatch):
    a, rows, taken, rates = _check_run(hip, STEPWISE, monkeypatch, 1, "stepwise")
    assert len(rows) == 3 and sum(taken) >= 2 and taken.count(False) >= 1
    assert any(r <= STEPWISE["rate"] for r in rates) and any(r > STEPWISE["rate"] for r in rates)


def test_training_is_untouched(hip, monkeypatch):
    """keep_best=True against the same curve-mode run without it: the flat parameter buffer and the curve rows, bit for bit
    (and both against the run without curve mode)."""
    cfg = dict(FUSED, rate=True)
    a = _trainer(hip, cfg, monkeypatch)
    _advance(a, cfg)
    b = _trainer(hip, cfg, monkeypatch, keep=False)
    _advance(b, cfg)
    torch.cuda.synchronize()
    assert a.keep_best == 0.0 and b.keep_best is False and b.best is None
    assert torch.equal(a.agent.flat.data, b.agent.flat.data) and torch.equal(a.vec.internal, b.vec.internal)
    assert a.eval_curve.rows.tobytes() == b.eval_curve.rows.tobytes()
    assert torch.equal(a.agent.flat.data, _twin(hip, FUSED, monkeypatch)[1])
    kstar, _ = choose_numpy(a.eval_curve.rows, 0.0)
    assert a.best.point == kstar
    assert [(k, int(x[0])) for k, x in a._device_flags() if int(x[0])] == []


@pytest.mark.parametrize("cfg,path", [(FUSED, "fused"), (STEPWISE, "stepwise")])
def test_using_best_and_restore_best(hip, cfg, path, monkeypatch):
    a = _trainer(hip, cfg, monkeypatch)
    _advance(a, cfg)
    a.run_steps(4, eval=False)                                  # (an actor step behind the last point: live != kept)
    best = a.best
    k = best.point
    points, _ = _twin(hip, cfg, monkeypatch)
    live = _span(a).clone()
    whole = a.agent.flat.data.clone()
    assert not torch.equal(live, best.params)
    with a.using_best():
        assert torch.equal(_span(a), best.params)
        r = a.evaluate(cfg["episodes"], seed=curve_seed(a.seed, k))
        assert r.path == path
        for f in r.FIELDS:                                      # point k*'s accumulators, bit for bit
            np.testing.assert_array_equal(getattr(r, f), getattr(points[k][1], f), err_msg=f)
        out = a.act(a.vec.obs[:3].clone())
        assert out.action.shape == (3, a.kernels.action_dim)
    assert torch.equal(a.agent.flat.data, whole)
    with pytest.raises(RuntimeError, match="inside"):
        with a.using_best():
            assert torch.equal(_span(a), best.params)
            raise RuntimeError("inside")
    assert torch.equal(a.agent.flat.data, whole)
    a.restore_best()
    assert torch.equal(_span(a), best.params)
    lo, hi = a.agent.flat.actor_range
    assert torch.equal(a.agent.flat.data[:lo], whole[:lo]) and torch.equal(a.agent.flat.data[hi:], whole[hi:])
    plain = _trainer(hip, cfg, monkeypatch, keep=False)
    with pytest.raises(ValueError):
        plain.restore_best()
    with pytest.raises(ValueError):
        with plain.using_best():
            pass


def test_checkpoint(hip, tmp_path, monkeypatch):
    cfg = FUSED
    a = _kept(hip, cfg, monkeypatch, 1)
    want = a.best

    def fresh(**more):
        tr = _trainer(hip, cfg, monkeypatch, **more)
        tr.work_dir = str(tmp_path / "ckpt")
        return tr
    b = fresh()
    _advance(b, cfg, 55)                                        # points 0, 1, 2 (steps 30, 40, 50)
    mid = b.best
    b.save()
    c = fresh()
    assert c.best is None
    c.load()
    got = c.best                                                # (before any point of its own: the checkpoint's incumbent)
    assert got.point == mid.point and got.row.rows.tobytes() == mid.row.rows.tobytes() and torch.equal(got.params, mid.params)
    _advance(c, cfg)
    got = c.best
    assert got.point == want.point and got.step == want.step and got.row.rows.tobytes() == want.row.rows.tobytes()
    assert torch.equal(got.params, want.params)
    assert c.eval_curve.rows.tobytes() == a.eval_curve.rows.tobytes()
    # BestPolicy travels as an npz
    got.save(str(tmp_path / "best.npz"))
    back = BestPolicy.load(str(tmp_path / "best.npz"))
    assert back.point == got.point and back.step == got.step and back.row.rows.tobytes() == got.row.rows.tobytes()
    assert torch.equal(back.params, got.params.cpu()) and back.max_violation_rate == cfg["rate"]
    # a checkpoint written without keep_best: no incumbent
    d = fresh(keep=False)
    _advance(d, cfg, 35)                                        # one point (step 30)
    d.save()
    e = fresh()
    _advance(e, cfg, 32)
    assert e.best is not None and e.best.point == 0
    e.load()
    assert e.best is None and len(e.eval_curve) == 1 and e._t == 35
    _advance(e, cfg, 41)                                        # point 1 (step 40) is its first candidate
    assert e.best.point == 1 and e.best.step == 40
