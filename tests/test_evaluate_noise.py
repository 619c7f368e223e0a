"""trainer.evaluate(obs_noise=...) on the CPU: the stepwise path driven by the oracle backend (``obs_noise_torch``).

The draw has one definition: z(i, s, q) = the Box-Muller normal of words 0 and 1 of Philox with key = the evaluation's seed
and counter (i, s, RPO_STREAM_EVAL_OBS + 0x100 q, 0), and the perturbed observation is the float32 product sigma[q] * z added
to the observation in float32.  ``noise_z`` / ``noisy_obs`` below restate it from oracle/philox.py; test_evaluate_noise_gpu.py
imports them.
"""
import ctypes
import types

import numpy as np
import pytest
import torch

import oracle_backend as ob
from oracle import cartsafe as cs
from oracle import philox
from rpo_amd import ops as hip_ops
from rpo_amd.algo import evaluation as ev
from test_evaluate_record import RESULT_ARRAYS, assert_arrays_equal
from test_train_step_golden import build_trainer

F32 = np.float32
SEED63 = 0x5A17C0DEFACE1234                                  # a 63-bit seed: both key words are in use
assert SEED63 >> 62 == 1 and SEED63 < 2 ** 63


def noise_z(seed, n, step, obs_dim):
    """z(i, step, q) for i < n, q < obs_dim -> float32 [n, obs_dim]."""
    z = np.zeros((n, obs_dim), dtype=F32)
    for q in range(obs_dim):
        w = philox.draw(seed, np.arange(n), step, 7 + 0x100 * q)
        z[:, q] = philox.normal(w[:, 0], w[:, 1])
    return z


def noisy_obs(obs, sigma, seed, step):
    """obs [n, obs_dim] float32 -> obs + sigma * z in float32 (multiply, then add); columns with sigma == 0 keep their bits."""
    obs = np.asarray(obs, dtype=F32)
    sigma = np.asarray(sigma, dtype=F32)
    out = (obs + (sigma[None, :] * noise_z(seed, obs.shape[0], step, obs.shape[1])).astype(F32)).astype(F32)
    out[:, sigma == 0] = obs[:, sigma == 0]
    return out


def test_stream_tag():
    assert hip_ops.STREAM_EVAL_OBS == hip_ops.CONST["RPO_STREAM_EVAL_OBS"] == 7
    assert hip_ops.CONST["RPO_ABI_VERSION"] == 6


def test_entry_points_validate_before_any_hip_call():
    """NULL sigma -> RPO_ERR_NULL; another length, a negative or a non-finite entry -> RPO_ERR_ARG; rpo_eval_obs_noise like its
    neighbours.  Everything else is NULL, so a call that got past its validation would not return these codes."""
    from rpo_amd import _lib
    lib = _lib.load()
    ARG, NULL = _lib.CONST["RPO_ERR_ARG"], _lib.CONST["RPO_ERR_NULL"]
    net = hip_ops._MlpStruct()
    head = (ctypes.byref(net), 0, 1.0, 0.0, 4)
    cart = head + (None,) * 7 + (0, 1, -1.0, 1.0, 1, 0.1, 1e-5, 0.0, None, 1, 200, 1e-3, None, 0, 0, None)
    pend = head + (None,) * 8 + (0, 1, -1.0, 1.0, 1, 0.1, 1e-5, 0.0, 200, 1e-3, None, 0, 0, None)
    for fn, args, O in ((lib.rpo_cartsafe_evaluate_noisy, cart, 6), (lib.rpo_pendulum_evaluate_noisy, pend, 5)):
        good = (ctypes.c_float * O)(*([0.1] * O))
        assert fn(*args, None, O, 3, None) == NULL
        assert fn(*args, good, O - 1, 3, None) == ARG and fn(*args, good, O + 1, 3, None) == ARG
        for bad in (-1e-3, float("nan"), float("inf")):
            sig = (ctypes.c_float * O)(*([0.1] * (O - 1) + [bad]))
            assert fn(*args, sig, O, 3, None) == ARG, bad
        assert fn(*args, good, O, 3, None) == NULL               # sigma passes: the NULL env pointers are next
        assert fn(None, *args[1:], good, O, 3, None) == NULL
    buf = (ctypes.c_float * 64)()
    p, q = ctypes.cast(buf, ctypes.c_void_p), ctypes.c_void_p(ctypes.addressof(buf) + 128)
    for bad in ((0, p, 6, 6, p, 1, 0, q, 6), (4, p, 5, 6, p, 1, 0, q, 6), (4, p, 6, 6, p, 1, 0, q, 5), (4, p, 6, 0, p, 1, 0, q, 6),
                (4, p, 4097, 4097, p, 1, 0, q, 4097), (4, p, 6, 6, p, 1, -1, q, 6), (4, p, 6, 6, p, 1, 1 << 24, q, 6),
                (4, p, 6, 6, p, 1, 0, p, 6)):
        assert lib.rpo_eval_obs_noise(*bad, None) == ARG, bad
    for bad in ((4, None, 6, 6, p, 1, 0, q, 6), (4, p, 6, 6, None, 1, 0, q, 6), (4, p, 6, 6, p, 1, 0, None, 6)):
        assert lib.rpo_eval_obs_noise(*bad, None) == NULL, bad


# ------------------------------------------------------------------------------------------------ the argument
def test_check_obs_noise_accepts_a_scalar_and_a_vector():
    assert ev.check_obs_noise(None, 6) is None
    s = ev.check_obs_noise(0.05, 6)
    assert s.dtype == np.float32 and s.shape == (6,) and (s == F32(0.05)).all()
    assert (ev.check_obs_noise(0, 5) == 0).all() and ev.check_obs_noise(0, 5).shape == (5,)
    assert (ev.check_obs_noise(2, 5) == 2).all()
    v = [0.1, 0.0, 0.2, 0.3, 0.4, 0.5]
    np.testing.assert_array_equal(ev.check_obs_noise(v, 6), np.array(v, dtype=F32))
    np.testing.assert_array_equal(ev.check_obs_noise(tuple(v), 6), np.array(v, dtype=F32))
    np.testing.assert_array_equal(ev.check_obs_noise(np.array(v), 6), np.array(v, dtype=F32))
    np.testing.assert_array_equal(ev.check_obs_noise(torch.tensor(v), 6), np.array(v, dtype=F32))


@pytest.mark.parametrize("bad", [-1e-3, float("nan"), float("inf"), True, False, np.bool_(True), "0.1", [0.1] * 5, [0.1] * 7, [],
                                 [0.1, 0.1, 0.1, 0.1, 0.1, -1e-3], [0.1, 0.1, 0.1, 0.1, 0.1, float("nan")],
                                 [0.1, 0.1, 0.1, 0.1, 0.1, float("inf")], [0.1, 0.1, 0.1, 0.1, 0.1, True], [[0.1] * 6], 1e39,
                                 [0.1, None, 0.1, 0.1, 0.1, 0.1]])
def test_check_obs_noise_refuses(bad):
    with pytest.raises(ValueError, match="obs_noise"):
        ev.check_obs_noise(bad, 6)


def test_evaluate_refuses_a_bad_obs_noise():
    torch.manual_seed(5)
    tr = build_trainer("ddpg", "cart", ob, torch.device("cpu"), num_envs=4, use_graph=False, capacity=8)
    for bad in (-1e-3, float("nan"), float("inf"), True, [0.1] * 5):
        with pytest.raises(ValueError, match="obs_noise"):
            tr.evaluate(3, horizon=2, obs_noise=bad)


# ------------------------------------------------------------------------------------------------ the draw
@pytest.mark.parametrize("step", [0, 3])
def test_obs_noise_torch_is_the_philox_normal_of_the_definition(step):
    n, O = 7, 6
    rng = np.random.RandomState(3)
    obs = rng.uniform(-1, 1, size=(n, O)).astype(F32)
    sigma = np.array([0.05, 0.1, 0.0, 1.0, 0.3, 2.5], dtype=F32)
    out = torch.full((n, O), 9.0)
    src = torch.tensor(obs)
    ev.obs_noise_torch(types.SimpleNamespace(backend=ob), src, sigma, SEED63, step, out)
    want = noisy_obs(obs, sigma, SEED63, step)
    assert out.numpy().tobytes() == want.tobytes()
    assert out.numpy()[:, 2].tobytes() == obs[:, 2].tobytes()                   # the zero column's bits
    assert src.numpy().tobytes() == obs.tobytes()                               # the source is not written
    z = noise_z(SEED63, n, step, O)
    assert np.isfinite(z).all() and len(np.unique(z)) == n * O                  # every (episode, column) has its own draw
    assert (noise_z(SEED63, n, step + 1, O) != z).all() and (noise_z(SEED63 ^ 1, n, step, O) != z).all()


# ------------------------------------------------------------------------------------------------ evaluate()
def _fresh(algo, envname):
    torch.manual_seed(5)
    tr = build_trainer(algo, envname, ob, torch.device("cpu"), num_envs=4, use_graph=False, capacity=8)
    tr.vec.reset()
    return tr


@pytest.mark.parametrize("algo,envname", [("ddpg", "cart"), ("sac", "pendulum")])
def test_off_means_off(algo, envname, monkeypatch):
    """None, 0, 0.0 and all-zero: the arrays, the trajectory and the calls of an evaluation without the argument."""
    torch.set_num_threads(1)
    tr = _fresh(algo, envname)
    calls = []
    monkeypatch.setattr(ev, "obs_noise_torch", lambda *a, **k: calls.append(a))
    seen = []
    inner = tr._eval_action
    monkeypatch.setattr(tr, "_eval_action", lambda v, **kw: (seen.append(sorted(kw)), inner(v, **kw))[1])
    plain = tr.evaluate(5, seed=9, horizon=12, record=True, constraints=True)
    for off in (None, 0, 0.0, [0.0] * tr.kernels.obs_dim):
        r = tr.evaluate(5, seed=9, horizon=12, record=True, constraints=True, obs_noise=off)
        assert_arrays_equal(r, plain)
        assert r.obs_noise is None
        for name in plain.trajectory.ARRAYS:
            assert getattr(r.trajectory, name).tobytes() == getattr(plain.trajectory, name).tobytes(), name
        for name in plain.constraints.ARRAYS:
            np.testing.assert_array_equal(getattr(r.constraints, name), getattr(plain.constraints, name), err_msg=name)
    assert not calls and all("obs" not in kw for kw in seen)


@pytest.mark.parametrize("algo,envname", [("ddpg", "cart"), ("sac", "pendulum"), ("ddpgla", "cart")])
def test_noisy_evaluation_is_reproducible_and_differs_from_clean(algo, envname):
    torch.set_num_threads(1)
    if algo.endswith("la"):
        torch.manual_seed(5)
        tr = build_trainer(algo, envname, ob, torch.device("cpu"), num_envs=4, fused=False)
    else:
        tr = _fresh(algo, envname)
    O = tr.kernels.obs_dim
    kw = dict(seed=SEED63, horizon=10, record=True)
    clean = tr.evaluate(6, **kw)
    a = tr.evaluate(6, obs_noise=0.1, **kw)
    b = tr.evaluate(6, obs_noise=0.1, **kw)
    assert a.path == "stepwise" and a.obs_noise.dtype == np.float32 and (a.obs_noise == F32(0.1)).all() and a.obs_noise.shape == (O,)
    assert_arrays_equal(a, b)
    for name in a.trajectory.ARRAYS:
        assert getattr(a.trajectory, name).tobytes() == getattr(b.trajectory, name).tobytes(), name
    assert a.trajectory.action.tobytes() != clean.trajectory.action.tobytes()
    assert any(not np.array_equal(getattr(a, f), getattr(clean, f)) for f in RESULT_ARRAYS)
    # step 0: both runs start from the same state, so the recorded observations differ by the draw alone
    np.testing.assert_array_equal(a.trajectory.obs[:, 0], noisy_obs(clean.trajectory.obs[:, 0], a.obs_noise, SEED63, 0))
    # another seed is another evaluation; a zero column of a per-column sigma keeps the clean run's bits at step 0
    sig = [0.1] * O
    sig[1] = 0.0
    c = tr.evaluate(6, obs_noise=sig, **kw)
    assert c.trajectory.obs[:, 0, 1].tobytes() == clean.trajectory.obs[:, 0, 1].tobytes()
    np.testing.assert_array_equal(c.trajectory.obs[:, 0], noisy_obs(clean.trajectory.obs[:, 0], c.obs_noise, SEED63, 0))


def test_the_policy_reads_the_noisy_observation_and_the_env_steps_the_true_state():
    """CartSafe-v0 on the oracle backend (whose step is the oracle's, rounded to float32): the recorded actions replayed from
    the initial states give the TRUE trajectory; its rewards and violations are the recorded ones, exactly, and every
    recorded observation is that true state plus sigma * z(i, s, .), bit for bit."""
    torch.set_num_threads(1)
    tr = _fresh("ddpg", "cart")
    n, H, sigma = 5, 8, 0.1
    init = torch.tensor(philox.cart_reset(21, np.arange(n), 0))
    r = tr.evaluate(n, seed=SEED63, horizon=H, init_states=init, record=True, obs_noise=sigma)
    tj = r.trajectory
    state = init.numpy().astype(F32)
    alive = np.ones(n, dtype=bool)
    checked = 0
    for s in range(H):
        assert (tj.valid[:, s] == alive).all()
        want = noisy_obs(state, r.obs_noise, SEED63, s)
        assert tj.obs[alive, s].tobytes() == want[alive].tobytes(), s
        nxt, reward, term, ineq, eq = cs.step(state.astype(np.float64), np.ascontiguousarray(tj.action[:, s]), cs.Constants(1))
        np.testing.assert_array_equal(tj.reward[alive, s], reward.astype(F32)[alive])
        np.testing.assert_array_equal(tj.ineq[alive, s], ineq.max(axis=1).astype(F32)[alive])
        np.testing.assert_array_equal(tj.eq[alive, s], np.abs(eq).max(axis=1).astype(F32)[alive])
        checked += int(alive.sum())
        alive = alive & ~tj.done[:, s]
        state = nxt.astype(F32)
    assert checked == r.length.sum() and checked > n


@pytest.mark.parametrize("algo,envname", [("ddpg", "cart"), ("sac", "pendulum")])
def test_noisy_evaluate_leaves_the_trainer_untouched(algo, envname):
    torch.set_num_threads(1)
    a = _fresh(algo, envname)
    a.run_steps(10)
    b = _fresh(algo, envname)
    b.run_steps(5)
    r = b.evaluate(5, horizon=20, record=True, constraints=True, obs_noise=0.1)
    assert r.obs_noise is not None and r.length.min() >= 1
    b.run_steps(5)
    for name in ("internal", "obs", "action", "ep_len", "ep_ret", "ep_count", "ctrl", "stats"):
        assert torch.equal(getattr(a.vec, name), getattr(b.vec, name)), name
    assert torch.equal(a.buffer.rows, b.buffer.rows)
    assert torch.equal(a.agent.flat.data, b.agent.flat.data)
    assert torch.equal(a.agent.critic_target_flat, b.agent.critic_target_flat)
    assert a._t == b._t == 10
