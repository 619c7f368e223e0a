"""trainer.evaluate(obs_noise=...) on the MI355X: rpo_eval_obs_noise against the definition (oracle/philox.py, restated in
test_evaluate_noise.py) and against the composition of rpo_philox_normal launches it stands for; the fused kernel's NOISE
instances (rpo_<env>_evaluate_noisy) against the stepwise path, bit for bit; and the property the feature exists for -- the
policy and the projection read the noisy observation while the env steps the true state -- against the oracle envs.

Tolerances.  The draw: rtol 1e-5, atol 2e-5 on z (scaled by sigma), test_kernels_gpu.py's for the device normal against
oracle/philox.py (``DRAW``).  A difference of two recorded float32 observations ``noisy - clean`` additionally carries the one
rounding of the float32 sum ``o + sigma * z`` the definition asks for: 2^-24 |noisy| (``_draw_tol``).  The dynamics: the
per-step tolerances of test_evaluate_record_gpu.py (``CART_TOL`` / ``PEND_TOL``).
"""
import numpy as np
import pytest
import torch

from oracle import cartsafe as cs
from oracle import pendulum as pd
from test_evaluate_noise import SEED63, noise_z
from test_evaluate_record import RESULT_ARRAYS, _close
from test_evaluate_record_gpu import CART_TOL, PEND_TOL
from test_train_step_golden import build_trainer

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
F32 = np.float32
DRAW = (1e-5, 2e-5)                                            # (rtol, atol) on z
FUSED = [("ddpg", "cart"), ("sac", "pendulum")]                # cart-RPODDPG, pendulum-RPOSAC (the Gaussian mean head)


@pytest.fixture(scope="module")
def hip():
    from rpo_amd import ops
    assert torch.cuda.is_available()
    return ops


_TRAINERS = {}


def _trained(hip, algo, envname):
    """One trainer per configuration for the whole module (evaluate() changes no trainer state: item 7), its policy moved
    off its initialisation by 8 training steps."""
    key = (algo, envname)
    if key not in _TRAINERS:
        torch.manual_seed(5)
        tr = build_trainer(algo, envname, hip, DEV, num_envs=64, use_graph=False)
        tr.vec.reset()
        tr.run_steps(8)
        _TRAINERS[key] = tr
    return _TRAINERS[key]


def _sigma(tr, kind):
    """0.05, or a per-column sigma with one zero."""
    if kind == "scalar":
        return 0.05
    s = [0.02 * (q + 1) for q in range(tr.kernels.obs_dim)]
    s[2] = 0.0
    return s


def _run(tr, fused, **kw):
    had = "fused_eval" in tr.schedule
    was = tr.schedule.get("fused_eval")
    tr.schedule["fused_eval"] = int(fused)
    try:
        r = tr.evaluate(**kw)
    finally:
        if had:
            tr.schedule["fused_eval"] = was
        else:
            del tr.schedule["fused_eval"]
    assert r.path == ("fused" if fused else "stepwise")
    return r


def _same_bits(a, b):
    """Accumulators, trace and constraint report of two evaluations, bit for bit (NaN-safe)."""
    for f in RESULT_ARRAYS:
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), f
    assert (a.trajectory is None) == (b.trajectory is None) and (a.constraints is None) == (b.constraints is None)
    if a.trajectory is not None:
        for name in a.trajectory.ARRAYS:
            x, y = getattr(a.trajectory, name), getattr(b.trajectory, name)
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), name
    if a.constraints is not None:
        for name in a.constraints.ARRAYS:
            x, y = getattr(a.constraints, name), getattr(b.constraints, name)
            assert x.shape == y.shape and x.tobytes() == y.tobytes(), name
    np.testing.assert_array_equal(a.obs_noise, b.obs_noise)


def _draw_tol(sigma, z, noisy):
    """|(noisy - clean) - sigma z| allowed: the draw's tolerance scaled by sigma plus one float32 rounding of the sum."""
    sigma = np.asarray(sigma, dtype=np.float64)
    return sigma * (DRAW[1] + DRAW[0] * np.abs(z)) + 2.0 ** -24 * np.abs(noisy)


# ------------------------------------------------------------------------------------------------ 1. the draw
@pytest.mark.parametrize("step", [0, 1, 199])
@pytest.mark.parametrize("O", [5, 6, 57])
def test_obs_noise_kernel_is_the_definition(hip, O, step):
    n = 37
    rng = np.random.RandomState(O)
    src = torch.tensor(rng.uniform(-2, 2, size=(n + 2, O + 3)).astype(F32), device=DEV)
    sigma = rng.uniform(0.01, 2.0, size=O).astype(F32)
    sigma[[1, O - 1]] = 0.0
    sig = torch.tensor(sigma, device=DEV)
    dst = torch.full((n + 2, O + 5), 7.0, device=DEV)
    obs, out = src[:n, :O], dst[:n, :O]                         # row strides O + 3 and O + 5
    hip.eval_obs_noise(obs, sig, SEED63, step, out)
    got, o = out.cpu().numpy(), obs.cpu().numpy()
    # the numpy restatement from oracle/philox.py
    z = noise_z(SEED63, n, step, O)
    ref = o.astype(np.float64) + sigma[None, :].astype(np.float64) * z
    np.testing.assert_array_less(np.abs(got - ref), DRAW[0] * np.abs(ref) + DRAW[1] * sigma[None, :] + 1e-30)
    # the composition it stands for: rpo_philox_normal per column, then torch's multiply and add
    want = obs.clone()
    zq = torch.zeros(n, device=DEV)
    for q in range(O):
        if sigma[q] != 0:
            hip.philox_normal(zq, SEED63, 0, step, hip.STREAM_EVAL_OBS + 0x100 * q)
            want[:, q] = obs[:, q] + sig[q] * zq
    assert got.tobytes() == want.cpu().numpy().tobytes()
    assert got[:, sigma == 0].tobytes() == o[:, sigma == 0].tobytes()          # zero-sigma columns: the bits of obs
    full = dst.cpu().numpy()
    assert (full[n:] == 7.0).all() and (full[:, O:] == 7.0).all()             # rows past n, columns past obs_dim
    assert torch.equal(src[:n, :O], obs) and src.cpu().numpy()[:n, :O].tobytes() == o.tobytes()


def test_obs_noise_kernel_validates_its_arguments(hip):
    obs, out, sig = torch.zeros(4, 6, device=DEV), torch.zeros(4, 6, device=DEV), torch.zeros(6, device=DEV)
    with pytest.raises(hip.RpoHipError, match="invalid argument"):
        hip.eval_obs_noise(obs, sig, 1, 1 << 24, out)
    with pytest.raises(hip.RpoHipError, match="invalid argument"):
        hip.eval_obs_noise(obs, sig, 1, -1, out)
    with pytest.raises(hip.RpoHipError, match="invalid argument"):
        hip.eval_obs_noise(obs, sig, 1, 0, obs)                 # out is never obs
    with pytest.raises(hip.RpoHipError):
        hip.eval_obs_noise(obs, sig[:5], 1, 0, out)
    hip.eval_obs_noise(obs, sig, 1, 0, out)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 2. off means off
@pytest.mark.parametrize("algo,envname", FUSED)
def test_off_means_off(hip, algo, envname, monkeypatch):
    tr = _trained(hip, algo, envname)
    kw = dict(episodes=17, seed=13, record=True, constraints=True)
    plain_f, plain_s = _run(tr, True, **kw), _run(tr, False, **kw)
    seen, drawn = [], []
    inner, inner_noise = tr.kernels.evaluate, hip.eval_obs_noise
    monkeypatch.setattr(tr.kernels, "evaluate", lambda *a, **k: (seen.append(sorted(k)), inner(*a, **k))[1])
    monkeypatch.setattr(hip, "eval_obs_noise", lambda *a, **k: (drawn.append(1), inner_noise(*a, **k))[1])
    for off in (None, 0.0, 0, [0.0] * tr.kernels.obs_dim):
        f, s = _run(tr, True, obs_noise=off, **kw), _run(tr, False, obs_noise=off, **kw)
        assert f.obs_noise is None and s.obs_noise is None
        _same_bits(f, plain_f)
        _same_bits(s, plain_s)
    assert seen and all("noise" not in k for k in seen) and not drawn
    _run(tr, True, obs_noise=0.05, **kw)
    _run(tr, False, obs_noise=0.05, **kw)
    assert "noise" in seen[-1] and len(drawn) == 200            # (the spies do see a noisy evaluation)


# ------------------------------------------------------------------------------------------------ 3. fused == stepwise
CASES = [(1, None, True, True), (70, None, True, True), (17, None, False, False), (17, None, True, False),
         (17, None, False, True), (17, None, True, True), (12288 + 5, 4, 64, True)]


@pytest.mark.parametrize("kind", ["scalar", "percol"])
@pytest.mark.parametrize("n,horizon,record,constraints", CASES)
@pytest.mark.parametrize("algo,envname", FUSED)
def test_fused_equals_stepwise_bit_for_bit(hip, algo, envname, n, horizon, record, constraints, kind):
    """12288 + 5: the 64-lane instance with a ragged last tile (5 of its 64 lanes); the others the 16-lane instance with 1, 1
    and 6 live lanes in their last tile, over the full default horizon."""
    tr = _trained(hip, algo, envname)
    kw = dict(episodes=n, seed=SEED63, horizon=horizon, record=record, constraints=constraints, obs_noise=_sigma(tr, kind))
    a, b = _run(tr, True, **kw), _run(tr, False, **kw)
    assert a.horizon == (horizon or 200) and a.obs_noise.dtype == np.float32 and a.obs_noise.shape == (tr.kernels.obs_dim,)
    _same_bits(a, b)
    assert a.length.min() >= 1 and not a.nonfinite.any()
    clean = _run(tr, True, **dict(kw, obs_noise=None))
    assert any(getattr(a, f).tobytes() != getattr(clean, f).tobytes() for f in RESULT_ARRAYS)
    if record and constraints:                                  # the record's tail and the report describe the same steps
        R = a.trajectory.episodes
        np.testing.assert_array_equal(np.where(a.trajectory.valid, a.trajectory.ineq, 0).max(axis=1).astype(np.float64),
                                      a.constraints.ineq_max.max(axis=1)[:R])
    if kind == "percol" and record:                             # the zero column is the clean run's at step 0
        c = _run(tr, True, **dict(kw, obs_noise=None))
        assert a.trajectory.obs[:, 0, 2].tobytes() == c.trajectory.obs[:, 0, 2].tobytes()
        assert a.trajectory.obs[:, 0, 1].tobytes() != c.trajectory.obs[:, 0, 1].tobytes()


# ------------------------------------------------------------------------------------------------ 4. launch splits
@pytest.mark.parametrize("algo,envname", FUSED)
def test_launch_splits_are_invisible(hip, algo, envname, monkeypatch):
    tr = _trained(hip, algo, envname)
    kw = dict(episodes=17, seed=SEED63, record=True, constraints=True, obs_noise=0.05)
    one = _run(tr, True, **kw)
    launches = []
    inner = tr.kernels.evaluate
    monkeypatch.setattr(tr.kernels, "evaluate", lambda *a, **k: (launches.append((a[12], a[13])), inner(*a, **k))[1])
    monkeypatch.setattr(hip, "EVAL_LANE_STEPS", 17 * 3)
    split = _run(tr, True, **kw)
    assert launches[:3] == [(0, 3), (3, 3), (6, 3)] and len(launches) == 67 and launches[-1] == (198, 2)
    _same_bits(split, one)
    assert one.length.max() > 3                                 # (episodes did run on into later launches)


# ------------------------------------------------------------------------------------------------ 5. who reads what
def _replay(envname, init, actions):
    """The oracle env from ``init`` under the recorded actions [n, T, 2] -> per step (true obs, reward, max ineq, max |eq|)."""
    out = []
    state = np.asarray(init, dtype=np.float64)
    for s in range(actions.shape[1]):
        a = np.ascontiguousarray(actions[:, s])
        if envname == "cart":
            nxt, reward, _, ineq, eq = cs.step(state, a, cs.Constants(1))
            obs = state
        else:
            obs = pd.get_obs(state)
            nxt, _, reward, _, ineq, eq = pd.step(state, a)
        out.append((np.asarray(obs, dtype=np.float64), reward, ineq.max(axis=1), np.abs(eq).max(axis=1)))
        state = np.asarray(nxt, dtype=np.float64)
    return out


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("algo,envname", FUSED)
def test_the_policy_reads_the_noisy_observation_and_the_env_steps_the_true_state(hip, algo, envname, fused):
    """This is the test that fails if the cart lane steps the staged (noisy) tile: the replay of the recorded actions from the
    initial states through the oracle env is the TRUE trajectory; rewards and violations of steps 0..3 must be its, and the
    recorded observations must sit sigma * z(i, s, .) away from its states."""
    tr = _trained(hip, algo, envname)
    n, sigma, T = 17, 0.1, 4
    v = tr.base_env.make_vec(n, seed=5, max_episode_steps=tr.max_episode_steps, device=DEV, stats_cap=2)
    v.reset()
    init = v.internal.clone()
    kw = dict(episodes=n, seed=SEED63, init_states=init, record=True)
    clean, noisy = _run(tr, fused, **kw), _run(tr, fused, obs_noise=sigma, **kw)
    tj = noisy.trajectory
    O = tr.kernels.obs_dim
    # step 0: the same true state in both runs
    z0 = noise_z(SEED63, n, 0, O)
    d0 = tj.obs[:, 0].astype(np.float64) - clean.trajectory.obs[:, 0]
    np.testing.assert_array_less(np.abs(d0 - np.float64(F32(sigma)) * z0), _draw_tol(sigma, z0, tj.obs[:, 0]))
    assert np.abs(d0).min() > 0
    # steps 0..3 against the oracle's true trajectory
    tol = CART_TOL if envname == "cart" else PEND_TOL
    truth = _replay(envname, init.cpu().numpy(), tj.action[:, :T])
    assert tj.valid[:, :T].sum() > 3 * n
    for s, (obs, reward, ineq, eq) in enumerate(truth):
        live = tj.valid[:, s]
        _close(tj.reward[live, s], reward.astype(F32)[live], tol["reward"], "reward, step %d" % s)
        _close(tj.ineq[live, s], ineq[live], tol["ineq"], "ineq, step %d" % s)
        _close(tj.eq[live, s], eq[live], tol["eq"], "eq, step %d" % s)
        z = noise_z(SEED63, n, s, O)
        d = tj.obs[:, s].astype(np.float64) - obs
        for cols, rtol, atol in tol["next_obs"]:
            bound = (_draw_tol(sigma, z, tj.obs[:, s]) + atol + rtol * np.abs(obs))[:, cols]
            np.testing.assert_array_less(np.abs(d - np.float64(F32(sigma)) * z)[:, cols][live], bound[live], err_msg="obs, step %d" % s)
    # ... and the noisy policy did act differently
    assert clean.trajectory.action[:, 0].tobytes() != tj.action[:, 0].tobytes()


def test_evopf_reads_the_noisy_observation(hip):
    """EVOPF-v0 (stepwise only), sigma = 1e-3: at step 0 the recorded observation is the clean run's plus sigma * z."""
    torch.manual_seed(5)
    tr = build_trainer("ddpg", "evopf256", hip, DEV, num_envs=16, use_graph=False)
    n, sigma, O = 6, 1e-3, tr.kernels.obs_dim
    v = tr.base_env.make_vec(n, seed=SEED63, max_episode_steps=tr.max_episode_steps, device=DEV, stats_cap=2)
    v.reset()
    kw = dict(episodes=n, seed=SEED63, horizon=3, init_states=v.internal.clone(), record=True, constraints=True)
    clean, noisy = tr.evaluate(**kw), tr.evaluate(obs_noise=sigma, **kw)
    assert noisy.path == "stepwise" and noisy.obs_noise.shape == (O,)
    z0 = noise_z(SEED63, n, 0, O)
    d0 = noisy.trajectory.obs[:, 0].astype(np.float64) - clean.trajectory.obs[:, 0]
    np.testing.assert_array_less(np.abs(d0 - np.float64(F32(sigma)) * z0), _draw_tol(sigma, z0, noisy.trajectory.obs[:, 0]))
    assert (d0 != 0).mean() > 0.9                               # (a small draw can vanish in the rounding of a large entry)
    assert noisy.trajectory.action[:, 0].tobytes() != clean.trajectory.action[:, 0].tobytes()
    again = tr.evaluate(obs_noise=sigma, **kw)
    _same_bits(again, noisy)


# ------------------------------------------------------------------------------------------------ 6. determinism and keys
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("algo,envname", FUSED)
def test_determinism_and_keys(hip, algo, envname, fused):
    tr = _trained(hip, algo, envname)
    kw = dict(record=True, constraints=True, obs_noise=0.05)
    a = _run(tr, fused, episodes=70, seed=SEED63, **kw)
    _same_bits(_run(tr, fused, episodes=70, seed=SEED63, **kw), a)
    other = _run(tr, fused, episodes=70, seed=SEED63 ^ 0x10, **kw)
    assert other.trajectory.obs.tobytes() != a.trajectory.obs.tobytes()
    assert any(getattr(a, f).tobytes() != getattr(other, f).tobytes() for f in RESULT_ARRAYS)
    # keyed by the episode id, not by the tile: episode i < 17 of 70 is episode i of 17
    small = _run(tr, fused, episodes=17, seed=SEED63, **kw)
    for f in RESULT_ARRAYS:
        assert getattr(a, f)[:17].tobytes() == getattr(small, f).tobytes(), f
    for name in a.trajectory.ARRAYS:
        assert getattr(a.trajectory, name)[:17].tobytes() == getattr(small.trajectory, name).tobytes(), name
    for name in a.constraints.ARRAYS:
        assert getattr(a.constraints, name)[:17].tobytes() == getattr(small.constraints, name).tobytes(), name


# ------------------------------------------------------------------------------------------------ 7. trainer state
def test_noisy_evaluate_has_no_side_effects_on_the_device(hip, monkeypatch):
    monkeypatch.setenv("RPO_GRAPH_CYCLE", "4")

    def fresh():
        torch.manual_seed(5)
        tr = build_trainer("ddpg", "cart", hip, DEV, num_envs=512, use_graph=True)
        tr.vec.reset()
        return tr
    a = fresh()
    a.run_steps(24)
    b = fresh()
    b.run_steps(8)
    torch.cuda.synchronize()
    snap = {k: getattr(b.vec, k).clone() for k in ("internal", "ep_len", "ep_ret", "ep_count", "ctrl", "stats")}
    rows, flat = b.buffer.rows.clone(), b.agent.flat.data.clone()
    r = b.evaluate(1000, record=64, constraints=True, obs_noise=0.1)
    assert r.path == "fused" and r.obs_noise is not None
    r = _run(b, False, episodes=100, horizon=20, record=True, obs_noise=[0.1, 0.0, 0.1, 0.2, 0.1, 0.3])
    torch.cuda.synchronize()
    for k, x in snap.items():
        assert torch.equal(getattr(b.vec, k), x), k
    assert torch.equal(b.buffer.rows, rows) and torch.equal(b.agent.flat.data, flat)
    b.run_steps(16)
    torch.cuda.synchronize()
    for k in ("internal", "ep_len", "ep_ret", "ep_count", "ctrl"):
        assert torch.equal(getattr(a.vec, k), getattr(b.vec, k)), k
    assert torch.equal(a.buffer.rows, b.buffer.rows)
    assert torch.equal(a.agent.flat.data, b.agent.flat.data)
    assert torch.equal(a.agent.critic_target_flat, b.agent.critic_target_flat)


# ------------------------------------------------------------------------------------------------ 8. the distribution
# The draw is deterministic in the seed, so the bound was evaluated for this seed on the CPU first, with oracle/philox.py
# (noise_z(DIST_SEED, 4096, 0, 6): |mean| <= 0.018, |std - 1| <= 0.018 over the six columns); the test repeats that.
DIST_SEED = 20261019


@pytest.mark.parametrize("algo,envname", FUSED)
def test_the_recovered_draw_is_standard_normal(hip, algo, envname):
    tr = _trained(hip, algo, envname)
    n, sigma, O = 4096, 0.1, tr.kernels.obs_dim
    want = noise_z(DIST_SEED, n, 0, O)
    assert (np.abs(want.mean(axis=0)) < 0.05).all() and (np.abs(want.std(axis=0) - 1) < 0.05).all()
    kw = dict(episodes=n, seed=DIST_SEED, horizon=1, record=True)
    clean, noisy = _run(tr, True, **kw), _run(tr, True, obs_noise=sigma, **kw)
    z = (noisy.trajectory.obs[:, 0].astype(np.float64) - clean.trajectory.obs[:, 0]) / np.float64(F32(sigma))
    assert (np.abs(z.mean(axis=0)) < 0.05).all(), z.mean(axis=0)
    assert (np.abs(z.std(axis=0) - 1) < 0.05).all(), z.std(axis=0)
    np.testing.assert_array_less(np.abs(z - want) * np.float64(F32(sigma)), _draw_tol(sigma, want, noisy.trajectory.obs[:, 0]))


# ------------------------------------------------------------------------------------------------ the entry points
def test_noisy_entry_points_validate_sigma(hip):
    tr = _trained(hip, "ddpg", "cart")
    v = tr.base_env.make_vec(32, seed=1, max_episode_steps=tr.max_episode_steps, device=DEV, stats_cap=2)
    v.reset()
    acc = torch.zeros(32, 8, device=DEV)
    scale, base = tr._box_affine

    def run(sigma):
        tr.kernels.evaluate(tr.fused.descs["actor"], tr._gauss_policy, scale, base, v.internal, None, v.action, v.ep_len, v.ep_ret,
                            v.ep_count, v.ctrl, acc, 0, 2, tr._box_lo, tr._box_hi, tr.eval_steps, tr.eval_lr, tr.corr_eps,
                            tr.corr_momentum, v.max_episode_steps, v.viol_thresh, noise=(sigma, 3))
    for bad in ([0.1] * 5, [0.1] * 7):
        with pytest.raises(hip.RpoHipError):
            run(np.array(bad, dtype=F32))
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(hip.RpoHipError, match="invalid argument"):
            run(np.array([0.1, 0.1, bad, 0.1, 0.1, 0.1], dtype=F32))
    run(np.full(6, 0.1, dtype=F32))
    torch.cuda.synchronize()
