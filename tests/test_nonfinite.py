"""The float64 statement of non-finite rows (tests/nonfinite_f64.py) against the oracle backend, on the CPU: the whole case table
of test_nonfinite_gpu.py through ``tests/oracle_backend.py`` -- which keeps the same failure word -- and the agreement of the two on
the word, on the bad lanes and on the non-finite masks of everything the step leaves behind.  No tolerance anywhere: finite lanes
are compared bit for bit with the same step without the plant, planted lanes as masks.

The oracle backend runs the single-stage chain (actor, head, projection, step), so SpringPendulum's observation and internal state
are separate inputs here and every target of the table applies.  The reference is held against the oracle under clips="ieee" (its
own np.clip / np.maximum); that the statement the kernels are held to, clips="fmax", names the same bad lanes and the same word is
asserted beside it.
"""
import numpy as np
import pytest
import torch

import nonfinite_f64 as nf
import oracle_backend as ob
from test_train_step_golden import build_trainer

pytestmark = pytest.mark.filterwarnings("ignore::RuntimeWarning")       # (NaN and inf in numpy arithmetic: the subject)
CASES = [("ddpg", "cart"), ("sac", "cart"), ("ddpg", "pendulum"), ("sac", "pendulum")]
_H = {}


def harness(algo, envname):
    if (algo, envname) not in _H:
        torch.set_num_threads(1)
        torch.manual_seed(5)
        tr = build_trainer(algo, envname, ob, torch.device("cpu"), num_envs=nf.N, use_graph=False, capacity=16)
        assert tr.fused is not None and not tr._rollout_pipeline
        h = nf.StepHarness(tr)
        _H[(algo, envname)] = (h, h.run())
    return _H[(algo, envname)]


def _agree(a, b):
    assert np.array_equal(a["bad"], b["bad"]) and a["word"] == b["word"]


@pytest.mark.parametrize("algo,envname", CASES)
def test_lane_plants_on_the_oracle_backend(algo, envname):
    h, clean = harness(algo, envname)
    sp = h.spec
    assert int(clean["ctrl"][nf.NF_IDX]) == 0 and int(clean["ctrl"][nf.T_IDX]) == nf.T0 + 1
    ref0 = nf.vector_step(sp, h.internal0, h.obs0, h.ep_len0, nf.T0, "ieee")
    assert not ref0["bad"].any() and ref0["word"] == 0
    assert not nf.check_step("clean", clean, clean, ref0, nf.N, sp)
    wrong = []
    for name, target, plants in nf.lane_cases(sp.env):
        internal, obs = nf.planted_state(sp.env, h.internal0, h.obs0, target, plants)
        ref = nf.vector_step(sp, internal, obs, h.ep_len0, nf.T0, "ieee")
        _agree(ref, nf.vector_step(sp, internal, obs, h.ep_len0, nf.T0, "fmax"))
        # exactly the planted lanes, whatever the component and the value: rows are independent
        assert sorted(np.flatnonzero(ref["bad"])) == sorted(p[0] for p in plants), name
        assert ref["word"] == nf.T0 + 1
        wrong += nf.check_step(name, h.run(internal, obs), clean, ref, nf.N, sp)
    assert not wrong, "\n".join(wrong)


@pytest.mark.parametrize("algo,envname", CASES)
def test_parameter_plants_on_the_oracle_backend(algo, envname):
    """The diverged actor: 0 * NaN is NaN, so ONE NaN element of any layer makes every lane bad."""
    h, clean = harness(algo, envname)
    sp = h.spec
    wrong = []
    for name, field, bits in nf.param_cases(sp.gauss):
        with h.planted_param(field, bits) as index:
            out = h.run()
        ref = nf.vector_step(sp.with_param(field, index, nf.f32_of(bits)), h.internal0, h.obs0, h.ep_len0, nf.T0, "ieee")
        _agree(ref, nf.vector_step(sp.with_param(field, index, nf.f32_of(bits)), h.internal0, h.obs0, h.ep_len0, nf.T0, "fmax"))
        assert ref["bad"].all() and ref["word"] == nf.T0 + 1, name
        wrong += nf.check_step(name, out, clean, ref, nf.N, sp)
    assert not wrong, "\n".join(wrong)
    assert nf.same_bits(h.run()["rows"], clean["rows"])           # every element was put back


@pytest.mark.parametrize("algo,envname", [("ddpg", "cart"), ("sac", "pendulum")])
def test_the_word_is_sticky_and_needs_a_ctrl(algo, envname):
    """A second launch at T0 + 1 with another bad lane leaves the word; a step without a ctrl writes nothing."""
    h, clean = harness(algo, envname)
    sp = h.spec
    internal, obs = nf.planted_state(sp.env, h.internal0, h.obs0, "state", [(16, 1, nf.QNAN)])
    first = h.run(internal, obs)
    assert int(first["ctrl"][nf.NF_IDX]) == nf.T0 + 1
    internal, obs = nf.planted_state(sp.env, first["internal"], first["obs"], "state", [(63, 0, nf.NEG_QNAN)])
    h.set_state(internal, obs)
    second = h.step()
    assert int(second["ctrl"][nf.NF_IDX]) == nf.T0 + 1 and int(second["ctrl"][nf.T_IDX]) == nf.T0 + 2
    cap = second["rows"].shape[0] // nf.N
    assert np.isnan(second["rows"].reshape(cap, nf.N, -1)[nf.T0 + 1, 63, sp.cols["action"][0]])       # ... though the lane WAS bad
    # ctrl = NULL
    h.restore()
    v = h.tr.vec
    before = v.ctrl.clone()
    action = torch.zeros(nf.N, 2)
    action[3, 0] = float("nan")
    v.k.step(v.internal, None if v.obs is v.internal else v.obs, action, v.ep_len, v.ep_ret, v.ep_count, None, 1, None, None,
             v.max_episode_steps, True, v.viol_thresh, v.seed, v.env_id_base)
    assert torch.equal(v.ctrl, before)
    ref = nf.vector_step(sp, h.internal0, h.obs0, h.ep_len0, nf.T0, "ieee", has_ctrl=False)
    assert ref["word"] == 0




@pytest.mark.parametrize("algo,envname", [("ddpg", "cart"), ("sac", "pendulum")])
def test_evaluation_on_the_oracle_backend(algo, envname):
    h, _ = harness(algo, envname)
    sp, tr = h.spec, h.tr
    init = nf.eval_init(h)
    clean = tr.evaluate(nf.N, init_states=init, horizon=3, seed=1)
    ref0 = nf.evaluate(sp, init, 3, "ieee")
    assert not clean.nonfinite.any() and not ref0["nonfinite"].any()
    assert clean.length[7] == 1 and ref0["length"][7] == 1 and np.array_equal(clean.length, ref0["length"])
    for name, _, plants in nf.eval_plants(sp.env):
        bad_init, _ = nf.planted_state(sp.env, init, nf.get_obs(sp, init), "state", plants)
        r = tr.evaluate(nf.N, init_states=bad_init, horizon=3, seed=1)
        ref = nf.evaluate(sp, bad_init, 3, "ieee")
        fm = nf.evaluate(sp, bad_init, 3, "fmax")
        lanes = sorted(p[0] for p in plants)
        assert sorted(np.flatnonzero(ref["nonfinite"])) == lanes and np.array_equal(fm["nonfinite"], ref["nonfinite"]), name
        assert np.array_equal(r.nonfinite, ref["nonfinite"]), name
        assert np.array_equal(r.length, ref["length"]), name
        got = np.stack([~np.isfinite(getattr(r, k)) for k in nf.ACC_SLOTS], axis=1)
        assert np.array_equal(got, ref["nan"]), name
        keep = ~ref["nonfinite"]
        for k in clean.FIELDS:
            assert np.array_equal(getattr(r, k)[keep], getattr(clean, k)[keep]), (name, k)
    assert int(tr.vec.ctrl[nf.NF_IDX]) == 0                       # the evaluation owns its ctrl
