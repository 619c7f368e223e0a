"""The shipped trainers on the HIP kernels (MI355X): (1) the reference's recorded update steps are reproduced through
the C ABI, (2) a hipGraph-replayed run equals the eager run bit for bit, (3) several whole iterations (rollout +
scatter + sample + update) agree with the same trainer driven by the oracle backend on the CPU.

Tolerances: (1) 4 Adam steps of float32 MLPs on rocBLAS vs the reference's CPU GEMMs: parameters agree to 5e-6
absolute, losses to 1e-4 relative.  (3) float32 env physics on the GPU vs float64 in the oracle, compounded over the
iterations: parameters 2e-5 absolute, replay rows 2e-4.
"""
import functools

import numpy as np
import pytest
import torch

from test_train_step_golden import CASES, build_trainer, check_product_update, run_product_update, sd  # noqa: F401
import test_train_step_golden as tsg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from rpo_amd import ops
    assert torch.cuda.is_available()
    return ops


@pytest.mark.parametrize("fused", [True, False], ids=["fused_mlp", "torch_mlp"])
@pytest.mark.parametrize("algo,envname", CASES)
def test_update_matches_reference_on_gpu(golden, hip, algo, envname, fused, monkeypatch):
    monkeypatch.setattr(tsg, "TOL", dict(rtol=0, atol=5e-6))
    out = run_product_update(golden, algo, envname, hip, torch.device("cuda"), fused=fused)
    g, tr, closs, aloss, proxy = out
    np.testing.assert_allclose(closs, g["critic_losses"], rtol=1e-4)
    np.testing.assert_allclose(aloss, g["actor_losses"], rtol=1e-4, atol=1e-6)
    ag = tr.agent
    for name, net in (("critic4", ag.critic), ("actor4", ag.actor), ("critic_target4", ag.critic_target)):
        for k, v in sd(g, name).items():
            np.testing.assert_allclose(net.state_dict()[k].cpu().numpy(), v, rtol=0, atol=5e-6)
    np.testing.assert_allclose(ag.nju.weight.detach().cpu().numpy(), g["nju4"], rtol=1e-4, atol=1e-7)


def _run(algo, envname, backend, device, iters, n_envs, use_graph, seed_all=5, fused=True, **extra):
    torch.manual_seed(seed_all)
    tr = build_trainer(algo, envname, backend, device, fused=fused, num_envs=n_envs, use_graph=use_graph, **extra)
    tr.vec.reset()
    tr.run_steps(iters)
    if device.type == "cuda":
        torch.cuda.synchronize()
    return tr


def _stats_equal(a, b, n):
    """Per-step statistics of two runs: counters exactly, float sums over lanes to rounding (the riding rollout adds the
    lanes of a step in another association than the one-launch rollout; both are sums of the same per-lane values)."""
    from rpo_amd import ops
    S = ops.STAT
    exact = [S[k] for k in ("episodes", "length_sum", "viol_count", "terminated", "proj_iters")]
    sa, sb = ops.reduce_stats(a.vec.stats[:n]).cpu().numpy(), ops.reduce_stats(b.vec.stats[:n]).cpu().numpy()
    np.testing.assert_array_equal(sa[:, exact], sb[:, exact])
    np.testing.assert_allclose(sa, sb, rtol=2e-6, atol=1e-7)


@pytest.mark.parametrize("fused", [True, False], ids=["fused_mlp", "torch_mlp"])
@pytest.mark.parametrize("algo,envname", [("ddpg", "cart"), ("sac", "pendulum")])
def test_graph_replay_equals_eager(hip, algo, envname, fused, monkeypatch):
    dev = torch.device("cuda")
    monkeypatch.setenv("RPO_GRAPH_CYCLE", "4")                  # (24 iterations: three eager windows, the capture, two replays)
    a = _run(algo, envname, hip, dev, 24, 512, use_graph=False, fused=fused)
    b = _run(algo, envname, hip, dev, 24, 512, use_graph=True, fused=fused)
    assert any(e["graph"] is not None for e in b._graphs.entries.values())
    assert torch.equal(a.vec.internal, b.vec.internal)
    assert torch.equal(a.buffer.rows, b.buffer.rows)
    assert torch.equal(a.agent.flat.data, b.agent.flat.data)
    assert torch.equal(a.agent.nju.weight, b.agent.nju.weight)
    assert int(b.vec.ctrl[0]) == 24 == int(a.vec.ctrl[0])
    _stats_equal(a, b, 24)


@pytest.mark.parametrize("policy_fre", [3, 5, 2])
@pytest.mark.parametrize("algo,envname", [("ddpg", "cart"), ("sac", "pendulum")])
def test_graph_replay_equals_eager_for_other_policy_periods(hip, algo, envname, policy_fre, monkeypatch):
    """policy_fre 3 / 5 / 2: the single-iteration hipGraph of a critic-only iteration is captured at a position of the period
    that depends on policy_fre (the 4th execution of its key); what its first launch does on behalf of the optimiser
    launches (zeroing the inf-norm slots of BOTH optimisers) must not depend on where it was captured.  Graph replays
    (single iterations, then windows) against eager launches, bit for bit, incl. the optimiser moments that the clip enters."""
    dev = torch.device("cuda")
    out = []
    for cyc, use_graph in (("1", True), ("16", True), ("1", False)):
        monkeypatch.setenv("RPO_GRAPH_CYCLE", cyc)
        # (clip_thres far below the gradients' inf-norm: every optimiser step is clipped, so a stale maximum changes the bits)
        out.append(_run(algo, envname, hip, dev, 64, 256, use_graph=use_graph, policy_fre=policy_fre, clip_thres=1e-3))
    a, b, c = out
    assert any(e["graph"] is not None for e in a._graphs.entries.values())
    assert any(k[0] == "cycle" and e["graph"] is not None for k, e in b._graphs.entries.items())
    for other in (a, b):
        assert torch.equal(other.agent.flat.data, c.agent.flat.data)
        assert torch.equal(other.agent.critic_target_flat, c.agent.critic_target_flat)
        assert torch.equal(other.agent.nju.weight, c.agent.nju.weight)
        assert torch.equal(other.agent.actor_optim.exp_avg, c.agent.actor_optim.exp_avg)
        assert torch.equal(other.agent.critic_optim.exp_avg_sq, c.agent.critic_optim.exp_avg_sq)
        assert torch.equal(other.buffer.rows, c.buffer.rows)


@pytest.mark.parametrize("algo,envname", [("ddpg", "cart"), ("sac", "cart"), ("ddpg", "pendulum")])
def test_multi_iteration_graph_equals_single_iteration_graphs(hip, algo, envname, monkeypatch):
    """RPO_GRAPH_CYCLE: one hipGraph per 8 iterations (two policy_fre periods) against one graph per iteration and
    against eager launches; 70 iterations = 3 eager passes of the window, its capture, 4 replays and a ragged tail."""
    dev = torch.device("cuda")
    monkeypatch.setenv("RPO_GRAPH_CYCLE", "8")
    monkeypatch.setenv("RPO_SCHEDULE", "ride=0")               # (the riding rollout has its own test below)
    a = _run(algo, envname, hip, dev, 70, 256, use_graph=True)
    assert a._cycle == 8 and a._graphs.entries[("cycle", 8, True)]["graph"] is not None
    monkeypatch.setenv("RPO_GRAPH_CYCLE", "1")
    b = _run(algo, envname, hip, dev, 70, 256, use_graph=True)
    assert ("cycle", 8, True) not in b._graphs.entries
    c = _run(algo, envname, hip, dev, 70, 256, use_graph=False)
    for other in (b, c):
        assert torch.equal(a.vec.internal, other.vec.internal)
        assert torch.equal(a.buffer.rows, other.buffer.rows)
        assert torch.equal(a.agent.flat.data, other.agent.flat.data)
        assert torch.equal(a.agent.critic_target_flat, other.agent.critic_target_flat)
        assert torch.equal(a.agent.nju.weight, other.agent.nju.weight)
        assert torch.equal(a.vec.stats[:70], other.vec.stats[:70])
    assert int(a.vec.ctrl[0]) == 70 and a._t == 70 and a._updates == b._updates == 70


def test_multi_iteration_graph_with_evaluation_and_logger(hip, monkeypatch, capsys):
    """run(eval=True) over 1100 iterations (evaluations at 500 and 1000, Logger attached): graph windows of 16 iterations
    must stop at the evaluation boundaries and give the same parameters, Logger rows and evaluation lines as one graph
    per iteration."""
    from rpo_amd.utils.logger import Logger
    dev = torch.device("cuda")
    monkeypatch.setenv("RPO_VERBOSE", "1")                     # (other tests of the session switch the printing off)
    out = []
    for cyc in ("16", "1"):
        monkeypatch.setenv("RPO_GRAPH_CYCLE", cyc)
        torch.manual_seed(5)
        tr = build_trainer("ddpg", "cart", hip, dev, num_envs=256, use_graph=True)
        tr.max_epochs = 1100
        tr.logger = Logger(("epoch", "reward", "max_ineq", "max_eq"), times=1, epochs=1100)
        tr.run(eval=True)
        torch.cuda.synchronize()
        out.append((tr, capsys.readouterr().out))
    (a, ta), (b, tb) = out
    assert ("cycle", 16, True) in a._graphs.entries and not any(k[0] == "cycle" for k in b._graphs.entries)
    assert a._t == b._t == 1100 and a.logger.pointer == b.logger.pointer > 1000
    assert torch.equal(a.agent.flat.data, b.agent.flat.data) and torch.equal(a.buffer.rows, b.buffer.rows)
    for key in ("epoch", "reward", "max_ineq", "max_eq"):
        np.testing.assert_array_equal(a.logger.tracker[key], b.logger.tracker[key])
    assert ta == tb and ta.count("\n") >= 2


def test_multi_iteration_graph_of_rollouts_only(hip, monkeypatch):
    dev = torch.device("cuda")
    monkeypatch.setenv("RPO_GRAPH_CYCLE", "8")
    out = []
    for use_graph in (True, False):
        torch.manual_seed(5)
        tr = build_trainer("ddpg", "cart", hip, dev, num_envs=256, use_graph=use_graph)
        tr.vec.reset()
        tr.run_steps(70, train=False)
        torch.cuda.synchronize()
        out.append(tr)
    a, c = out
    assert a._graphs.entries[("cycle", 8, False)]["graph"] is not None and a._updates == 0
    assert torch.equal(a.vec.internal, c.vec.internal) and torch.equal(a.buffer.rows, c.buffer.rows)
    assert torch.equal(a.vec.stats[:70], c.vec.stats[:70]) and int(a.vec.ctrl[0]) == 70


@pytest.mark.parametrize("algo", ["ddpg", "sac"])
def test_multi_update_graph_in_utd_mode(hip, algo, monkeypatch):
    """updates_per_step = 23: the 22 extra updates of a vector step run as two 8-update hipGraph windows + single-update
    graphs (alignment to policy_fre, ragged tail); same bits as eager launches."""
    dev = torch.device("cuda")
    monkeypatch.setenv("RPO_GRAPH_CYCLE", "8")
    out = []
    for use_graph in (True, False):
        out.append(_run(algo, "cart", hip, dev, 6, 64, use_graph=use_graph, updates_per_step=23))
    a, c = out
    assert a._graphs.entries[("extra", 8)]["graph"] is not None and a._updates == c._updates == 6 * 23
    assert torch.equal(a.agent.flat.data, c.agent.flat.data) and torch.equal(a.buffer.rows, c.buffer.rows)
    assert torch.equal(a.agent.critic_target_flat, c.agent.critic_target_flat)
    assert int(a.agent.critic_optim.step_dev[0]) == 6 * 23
    assert int(a.agent.actor_optim.step_dev[0]) == int(c.agent.actor_optim.step_dev[0]) >= 6 * 23 // 4 - 1
    # ctrl[RPO_CTRL_UPDATES] (the Philox sub-index of the k-th update of a vector step) is advanced by the update's own last
    # stage and is back at zero when the vector step is over
    assert a._updates_inkernel and int(a._uctrl[hip.CONST["RPO_CTRL_UPDATES"]]) == 0


@pytest.mark.parametrize("algo,envname", CASES)
def test_iterations_match_oracle_backend(hip, algo, envname):
    import oracle_backend as ob
    iters, n = 8, 64
    g = _run(algo, envname, hip, torch.device("cuda"), iters, n, use_graph=False)
    c = _run(algo, envname, ob, torch.device("cpu"), iters, n, use_graph=False)
    np.testing.assert_allclose(g.buffer.rows[: iters * n].cpu().numpy(), c.buffer.rows[: iters * n].numpy(), rtol=2e-4, atol=2e-4)
    np.testing.assert_allclose(g.vec.internal.cpu().numpy(), c.vec.internal.numpy(), rtol=2e-4, atol=2e-4)
    np.testing.assert_allclose(g.agent.flat.data.cpu().numpy(), c.agent.flat.data.numpy(), rtol=0, atol=2e-5)
    np.testing.assert_allclose(g.agent.nju.weight.detach().cpu().numpy(), c.agent.nju.weight.detach().numpy(), rtol=1e-3, atol=1e-6)
    np.testing.assert_array_equal(g.vec.ep_count.cpu().numpy(), c.vec.ep_count.numpy())
    S = hip.STAT
    gs = hip.reduce_stats(g.vec.stats[:iters]).cpu().numpy()
    cs_ = hip.reduce_stats(c.vec.stats[:iters]).numpy()
    for key in ("episodes", "reward_sum", "proj_iters"):
        np.testing.assert_allclose(gs[:, S[key]], cs_[:, S[key]], rtol=1e-5)
    np.testing.assert_allclose(gs[:, S["max_ineq_sum"]], cs_[:, S["max_ineq_sum"]], rtol=1e-3, atol=1e-3)


def test_eval_and_logger_on_gpu(hip):
    from rpo_amd.utils.logger import Logger
    torch.manual_seed(3)
    tr = build_trainer("ddpg", "cart", hip, torch.device("cuda"), num_envs=256, eval_fre=20)
    tr.max_epochs = 40
    tr.logger = Logger(("epoch", "reward", "max_ineq", "max_eq"), times=1, epochs=40)
    tr.run(eval=True)
    res = tr.eval()
    assert len(res) == 10 and 1.0 <= res[0] <= 200.0 and res[5] < 1e-5       # equalities hold to round-off
    assert tr.logger.pointer > 0 and tr.logger.tracker["reward"][0] > 0
    assert 0.0 <= tr.viol_rate <= 1.0 and tr.env_steps == 40 * 256


def test_gym_api_single_env_on_gpu(hip, golden):
    """`gym.make("CartSafe-v0")` -> reset / step through the HIP kernel with n = 1, against the reference vectors."""
    import gym
    import rpo_amd.env  # noqa: F401  (registers the ids)
    np.random.seed(123)
    env = gym.make("CartSafe-v0")
    assert list(env.partial_actions) == [1]
    g = golden("cart_env_p1")
    obs = env.reset()
    assert obs.shape == (6,) and np.all(np.abs(obs) <= 0.05)
    for i in range(5):
        env.unwrapped._vec.set_internal(g["states"][i][None, :])
        o, r, d, info = env.step(g["actions"][i])
        np.testing.assert_allclose(o, g["next_states"][i], rtol=1e-4, atol=1e-4)
        assert r == 1.0 and d == bool(g["done"][i])
        np.testing.assert_allclose(info["ineq_viol"], g["ineq_viol"][i], atol=4e-6)
        np.testing.assert_allclose(info["eq_viol"], g["eq_viol"][i], atol=2e-6)
    env.close()


def _dp_worker(rank, world, port, out_dir, use_graph=True):
    import os
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, here)
    sys.path.insert(0, os.path.dirname(here))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RPO_VERBOSE="0")
    import torch.distributed as dist
    from rpo_amd import ops
    from test_train_step_golden import build_trainer
    dist.init_process_group("gloo", rank=rank, world_size=world)      # both ranks share cuda:0; gloo moves GPU tensors
    torch.manual_seed(5)
    tr = build_trainer("ddpg", "cart", ops, torch.device("cuda"), num_envs=512, use_graph=use_graph)
    assert tr.n_local == 256 and tr.vec.env_id_base == 256 * rank
    tr.vec.reset()
    tr.run_steps(13)                        # eager passes, capture of the graph segments, replays + collectives;
    tr.run_steps(27)                        # the deferred optimiser tail is flushed at the end of each call
    tr._harvest(final=True)
    torch.cuda.synchronize()
    if use_graph:
        captured = [k for k, e in tr._graphs.entries.items() if e["graph"] is not None]
        assert any(k[0] == "after" for k in captured), captured      # tail of iteration i + head of iteration i + 1
    torch.save(dict(flat=tr.agent.flat.data.cpu(), nju=tr.agent.nju.weight.data.cpu(), env_steps=float(tr.env_steps),
                    state=tr.vec.internal.cpu()), os.path.join(out_dir, "rank%d.pt" % rank))
    dist.barrier()
    dist.destroy_process_group()


def test_data_parallel_graph_segments_on_gpu(hip, tmp_path):
    """Two ranks on the one GPU (gloo carries the collectives): the hipGraph-segmented iteration with eager gradient
    all-reduces keeps the replicas bit-identical, and the lanes of rank 1 are env ids 256..511."""
    import socket
    import torch.multiprocessing as mp
    ports = []
    for _ in range(2):
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        ports.append(s.getsockname()[1])
        s.close()
    import os
    import time
    results = {}
    for use_graph in (True, False):
        # Two processes time-slicing one GPU through gloo (a stand-in for one process per GPU over RCCL) stall once in ~20
        # runs on this pool (the same test passes alone and in the other 19).  A run normally takes ~6 s: a stalled
        # attempt is ended after 60 s (exactly the ranks started here) and repeated, twice at most; three stalls in a row FAIL.
        for attempt in (0, 1, 2):
            out_dir = os.path.join(str(tmp_path), "%s%d" % ("graph" if use_graph else "eager", attempt))
            os.makedirs(out_dir)
            s_ = socket.socket()
            s_.bind(("127.0.0.1", 0))
            port = s_.getsockname()[1]
            s_.close()
            ctx = mp.spawn(_dp_worker, args=(2, port, out_dir, use_graph), nprocs=2, join=False)
            deadline = time.time() + 60
            hung = False
            while not ctx.join(timeout=2):                         # raises if a rank failed
                if time.time() > deadline:
                    for proc in ctx.processes:
                        if proc.is_alive():
                            proc.kill()
                    hung = True
                    break
            if not hung:
                break
        if hung:
            pytest.fail("two ranks sharing one GPU did not finish within 60 s, three times in a row: a hung collective path "
                        "must not pass as a skip")
        results[use_graph] = [torch.load(os.path.join(out_dir, "rank%d.pt" % r), weights_only=False) for r in (0, 1)]
        if use_graph:
            graph_dir = out_dir
    tmp_path = graph_dir
    # graph segments (with the deferred optimiser tail) == eager launches, bit for bit
    for r in (0, 1):
        assert torch.equal(results[True][r]["flat"], results[False][r]["flat"])
        assert torch.equal(results[True][r]["state"], results[False][r]["state"])
    r0 = torch.load(os.path.join(tmp_path, "rank0.pt"), weights_only=False)
    r1 = torch.load(os.path.join(tmp_path, "rank1.pt"), weights_only=False)
    assert torch.equal(r0["flat"], r1["flat"]) and torch.equal(r0["nju"], r1["nju"])
    assert r0["env_steps"] == r1["env_steps"] == 512 * 40
    assert not torch.equal(r0["state"], r1["state"])


def _rccl_worker(rank, world, port, out_dir, algo, n_total, iters):
    """One rank per GPU over RCCL (backend "nccl"); world == 1 exercises the same code path on a one-GPU box through
    the schedule's force_dist (the collective is then a self-reduce, but it is issued, captured and replayed like any other)."""
    import os
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, here)
    sys.path.insert(0, os.path.dirname(here))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RPO_VERBOSE="0", RPO_SCHEDULE="force_dist=1",
                      RPO_GRAPH_CYCLE="8")
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import torch.distributed as dist
    from rpo_amd import ops
    from test_train_step_golden import build_trainer
    torch.cuda.set_device(rank)
    dev = torch.device("cuda", rank)
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    torch.manual_seed(5 + rank)             # rank 0's initial state is broadcast at construction
    tr = build_trainer(algo, "cart", ops, dev, num_envs=n_total, use_graph=True)
    assert tr.dist.on and tr.dist.in_graph and tr.dist.world == world and tr.n_local == n_total // world
    tr.vec.reset()
    tr.run_steps(iters)
    tr._harvest(final=True)
    torch.cuda.synchronize()
    captured = [k for k, e in tr._graphs.entries.items() if e["graph"] is not None]
    # multi-iteration windows WITH the collectives inside
    assert ("cycle", 8, True) in captured or ("cycle", 8, True, "ride") in captured, captured
    assert tr._graphs.enabled                                 # no capture failure fell back to eager launches
    torch.save(dict(flat=tr.agent.flat.data.cpu(), nju=tr.agent.nju.weight.data.cpu(), env_steps=float(tr.env_steps),
                    state=tr.vec.internal.cpu(), rows=tr.buffer.rows[:64 * tr.n_local].cpu(), seed=tr.seed),
               os.path.join(out_dir, "rank%d.pt" % rank))
    dist.barrier()
    dist.destroy_process_group()


def _spawn_rccl(world, out_dir, algo, n_total, iters, budget=240):
    import os
    import socket
    import time
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.spawn(_rccl_worker, args=(world, port, out_dir, algo, n_total, iters), nprocs=world, join=False)
    deadline = time.time() + budget
    while not ctx.join(timeout=5):
        if time.time() > deadline:
            for proc in ctx.processes:
                if proc.is_alive():
                    proc.kill()
            pytest.fail("RCCL ranks did not finish within %d s" % budget)
    return [torch.load(os.path.join(out_dir, "rank%d.pt" % r), weights_only=False) for r in range(world)]


@pytest.mark.parametrize("algo", ["ddpg", "sac"])
def test_rccl_collectives_inside_the_graph_single_rank(hip, tmp_path, algo, monkeypatch):
    """The data-parallel iteration over RCCL on the one GPU of this box (world size 1, schedule force_dist=1): every gradient
    all-reduce is issued inside the hipGraph of the iteration / of the 8-iteration window.  With one rank the mean over
    ranks is the identity, so the run must equal the plain single-process run bit for bit -- which also pins that the
    data-parallel path (no in-backward inf-norm, explicit rpo_absmax) computes the same update."""
    # (round 4's RPO_DP_OVERLAP variant -- the riders' env step on a second captured branch beside the all-reduce -- was
    # measured slower, 46.7 -> 66 us per iteration, and went with round 5: DESIGN.md 7)
    (r0,) = _spawn_rccl(1, str(tmp_path), algo, 256, 70)
    monkeypatch.setenv("RPO_GRAPH_CYCLE", "8")
    torch.manual_seed(5)
    tr = build_trainer(algo, "cart", hip, torch.device("cuda"), num_envs=256, use_graph=True)
    assert not tr.dist.on and tr.seed == r0["seed"]
    tr.vec.reset()
    tr.run_steps(70)
    torch.cuda.synchronize()
    assert torch.equal(tr.vec.internal.cpu(), r0["state"])
    assert torch.equal(tr.buffer.rows[:64 * 256].cpu(), r0["rows"])
    assert torch.equal(tr.agent.flat.data.cpu(), r0["flat"]) and torch.equal(tr.agent.nju.weight.data.cpu(), r0["nju"])


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs (one rank per GPU over RCCL / xGMI)")
def test_rccl_two_ranks_one_per_gpu(hip, tmp_path):
    """Two ranks, one per GPU, RCCL all-reduce inside the graph windows: replicas stay bit-identical, lanes are sharded
    by global env id, statistics are summed over ranks."""
    r0, r1 = _spawn_rccl(2, str(tmp_path), "sac", 512, 70)
    assert torch.equal(r0["flat"], r1["flat"]) and torch.equal(r0["nju"], r1["nju"])
    assert r0["env_steps"] == r1["env_steps"] == 512 * 70 and r0["seed"] == r1["seed"]
    assert not torch.equal(r0["state"], r1["state"])


def test_wide_rollout_tiles_are_bitwise_identical(hip, monkeypatch):
    """The 64-lane-per-workgroup rollout pipeline (used from 12 288 lanes up) and the 16-lane one compute the same
    bits: same per-row arithmetic, only the work distribution differs.  Same for the wide MLP forward."""
    dev = torch.device("cuda")
    with hip.tuning(rollout_wide=0):
        a = _run("ddpg", "cart", hip, dev, 12, 1000, use_graph=False)
    with hip.tuning(rollout_wide=1):
        b = _run("ddpg", "cart", hip, dev, 12, 1000, use_graph=False)
    assert torch.equal(a.vec.internal, b.vec.internal) and torch.equal(a.buffer.rows, b.buffer.rows)
    assert torch.equal(a.agent.flat.data, b.agent.flat.data)
    # statistics are float sums over differently shaped workgroups: equal up to summation order
    np.testing.assert_allclose(hip.reduce_stats(a.vec.stats[:12]).cpu().numpy(),
                               hip.reduce_stats(b.vec.stats[:12]).cpu().numpy(), rtol=1e-5, atol=1e-9)
    # generic forward: n >= 12288 takes the streaming kernel (weights in LDS, round 5; 12 or 16 waves per workgroup) or, with
    # the switch off, the 64-row tiles of rounds 3-4; every 4096-row slice of the same input the 16-row tiles: the same bits,
    # on all 16 384 rows
    f = a.fused
    s = torch.randn(16384, 6, device=dev)
    out_n = torch.full((16384, 1), float("nan"), device=dev)
    for r0 in range(0, 16384, 4096):
        f.forward("actor", s[r0:r0 + 4096], None, out_n[r0:r0 + 4096])
    for kw in (dict(fwd_stream=1, fwd_stream_waves=12), dict(fwd_stream=1, fwd_stream_waves=16), dict(fwd_stream=0)):
        out_w = torch.full((16384, 1), float("nan"), device=dev)
        with hip.tuning(**kw):
            f.forward("actor", s, None, out_w)
        assert torch.equal(out_w, out_n), kw


@pytest.mark.parametrize("sel,n_envs", [(3, 1000), (3, 16 * 16 * 256 * 2 + 37), (4, 1000), (4, 64 * 16 * 256 + 16 * 3 + 5)],
                         ids=["16_lane_groups", "several_tiles_per_wave", "64_lane_groups", "64_lane_groups_ragged_second_pass"])
@pytest.mark.parametrize("algo,envname", CASES)
def test_streaming_rollout_equals_the_row_tile_rollout(hip, algo, envname, sel, n_envs):
    """The streaming form of the one-launch rollout (rollout_stream.hip: the actor's hidden matrix stationary in
    LDS, one wave per 16-lane tile, both layers transposed on the matrix cores, the env step as the epilogue; default from
    65 536 lanes) against the 16-lane row tiles: the same per-lane functions behind a forward that is the row-tile forward to
    the bit -- states, actions, ring rows (incl. the zeroed padding of CartSafe's 128-byte ring lines, which the row tiles
    leave untouched = zero) and therefore the parameters after the updates are EQUAL; statistics are sums over other groupings."""
    dev = torch.device("cuda")
    iters = 9
    with hip.tuning(rollout_wide=0):
        a = _run(algo, envname, hip, dev, iters, n_envs, use_graph=False, capacity=16)
    with hip.tuning(rollout_wide=sel):
        b = _run(algo, envname, hip, dev, iters, n_envs, use_graph=False, capacity=16)
    assert torch.equal(a.vec.internal, b.vec.internal) and torch.equal(a.vec.action, b.vec.action)
    assert torch.equal(a.vec.ep_len, b.vec.ep_len) and torch.equal(a.vec.ep_ret, b.vec.ep_ret)
    assert torch.equal(a.buffer.rows, b.buffer.rows)
    assert torch.equal(a.agent.flat.data, b.agent.flat.data)
    assert int(b.vec.ctrl[0]) == iters
    _stats_equal(a, b, iters)


def _assert_same(a, b, names, atol=None):
    """The named tensors of two runs: equal bit for bit, or within atol[name] where a bound is given.  Prints every figure
    before it asserts (for a run with -s)."""
    get = {"parameters": lambda t: t.agent.flat.data, "critic targets": lambda t: t.agent.critic_target_flat,
           "replay rows": lambda t: t.buffer.rows, "env state": lambda t: t.vec.internal, "obs": lambda t: t.vec.obs,
           "actions": lambda t: t.vec.action, "ep_len": lambda t: t.vec.ep_len, "ep_count": lambda t: t.vec.ep_count}
    diff = {n: float((get[n](a).double() - get[n](b).double()).abs().max()) for n in names}
    print("max |a - b|: " + ", ".join("%s %.9g" % (n, diff[n]) for n in names))
    for n in names:
        bound = (atol or {}).get(n, 0.0)
        assert torch.equal(get[n](a), get[n](b)) if bound == 0.0 else diff[n] <= bound, (n, diff[n], bound)


def _no_split_no_actor_pipeline(tr):
    """embed_dim = 256: neither the column-split update nor the actor pipelines apply, so the row-tile kernels' E = 256
    instantiations run (rollout_kernel<., 256, 256, 1>, the critic forwards / fronts / backs at <256, 256>)"""
    return tr._split_state() is None and not tr._actor_pipeline and tr.fused.descs["actor"].E == 256


# embed_256: the E = 256 instantiations, which no embed_dim = 128 case launches
_ROLLOUT_CASES = [pytest.param(a, e, n, 128, id="%s-%s-%s" % (a, e, name)) for name, n in (("16_lane_tiles", 100), ("64_lane_tiles", 12500))
                  for a, e in CASES] + [pytest.param(a, e, 100, 256, id="%s-%s-embed_256" % (a, e)) for a, e in CASES[:4]]
# The largest |difference| the parent commit left between the two forms at embed_dim = 256, case by case; the bound is twice
# that.  No entry: the parent is bitwise there, and so is the assertion.  "stats": the per-step statistics that miss rtol 1e-5
# (sums of residuals near zero).
# Where the RPOSAC differences come from (read from the code, not from a run): the two forms run the actor's forward through
# different kernels with another order of the k sums.  The pipeline runs mlp_tile_forward (fused.hip, rollout_tile: out_mode
# `gauss ? 0 : 1`).  The stepwise sequence calls FusedNets.forward, which at E = 256 and n <= 16384 hands rpo_mlp_forward scratch
# for x0 / h1 also on an inference call; with out_mode == 0 -- RPOSAC's raw heads (RPOSAC._gauss) -- that is gemm_path_ok
# (mlp_gemm.h), so the forward goes layer by layer through gemm_forward, whose hidden layer (K = 256) takes the k-split kernel:
# four quarter chains added as ((q0 + q1) + q2) + q3, not the tile kernel's one chain.  RPODDPG's proposal asks for the tanh box
# (RPODDPG._actor_out: out_mode 1), which gemm_path_ok refuses: it stays on mlp_forward_kernel<256, 256>, the same mlp_tile.h
# code as the pipeline, and is bitwise.  The update side (_CRITIC_MAX_256) differs in all four cases for the same reason: the
# generic launches' forward_multi / forward of the critics and targets (saved or scratch x0 / h1, out_mode 0) take the GEMM path,
# the pipelines mlp_tile_forward.  Both forms are held to float64 on their own by tests/test_embed256_f64_gpu.py; the figures
# below stay what they were.
_ROLLOUT_MAX_256 = {
    ("sac", "cart"): {"env state": 2.86102295e-06, "obs": 2.86102295e-06, "replay rows": 2.86102295e-06, "actions": 1.54972076e-06,
                      "parameters": 1.45286322e-07, "stats": 5.122274e-07},
    ("sac", "pendulum"): {"env state": 1.78813934e-07, "obs": 1.78813934e-07, "replay rows": 1.49011612e-06, "actions": 9.53674316e-07,
                          "parameters": 3.7252903e-08, "stats": 2.3841858e-06}}


def _twice(measured):
    return {n: 2 * v for n, v in measured.items()} if measured else {}


@pytest.mark.parametrize("algo,envname,n_envs,embed_dim", _ROLLOUT_CASES)
def test_rollout_pipeline_equals_single_stage_launches(hip, algo, envname, n_envs, embed_dim, monkeypatch):
    """rpo_<env>_rollout (actor -> head -> complete -> project -> step -> scatter in one launch) reproduces the
    sequence rpo_mlp_forward (+ rpo_philox_normal + rpo_gauss_head) + rpo_<env>_act_project + rpo_<env>_step bit for
    bit, for both envs and both policy heads; n_envs is ragged against both tile heights.

    embed_256 (rollout_kernel<., 256, 256, 1>), as measured on the parent commit:
      ddpg-cart, ddpg-pendulum   bitwise, statistics within the bound of the embed_dim = 128 cases: asserted like those
      sac-cart                   states, observations and replay rows within 2.861e-6, actions 1.550e-6, parameters 1.453e-7;
                                 statistics miss rtol 1e-5 by up to 5.12e-7 absolute
      sac-pendulum               states and observations 1.788e-7, replay rows 1.490e-6, actions 9.537e-7, parameters 3.73e-8;
                                 statistics miss rtol 1e-5 by up to 2.384e-6 absolute
    The RPOSAC cases are asserted at twice their own figures (a margin for data-dependent rounding order), the episode counters
    exactly."""
    dev = torch.device("cuda")
    iters = 10
    monkeypatch.setenv("RPO_SCHEDULE", "fused_rollout=0")
    a = _run(algo, envname, hip, dev, iters, n_envs, use_graph=False, embed_dim=embed_dim)
    assert not a._rollout_pipeline
    monkeypatch.setenv("RPO_SCHEDULE", "fused_rollout=1")
    b = _run(algo, envname, hip, dev, iters, n_envs, use_graph=False, embed_dim=embed_dim)
    assert b._rollout_pipeline
    if embed_dim == 256:
        assert b._pipelines and _no_split_no_actor_pipeline(b)
    atol = _twice(_ROLLOUT_MAX_256.get((algo, envname)) if embed_dim == 256 else None)
    _assert_same(a, b, ["env state", "obs", "actions", "replay rows", "ep_len", "ep_count", "parameters"], atol)
    np.testing.assert_allclose(hip.reduce_stats(a.vec.stats[:iters]).cpu().numpy(),
                               hip.reduce_stats(b.vec.stats[:iters]).cpu().numpy(), rtol=1e-5, atol=atol.get("stats", 1e-9))


_CRITIC_CASES = [("ddpg", "cart"), ("sac", "cart"), ("sac", "pendulum"), ("ddpg", "pendulum")]
_CRITIC_MAX_256 = {                                              # (as _ROLLOUT_MAX_256; no case is bitwise on the parent)
    ("ddpg", "cart"): {"parameters": 5.96046448e-08, "critic targets": 1.49011612e-08, "replay rows": 2.86102295e-06, "env state": 2.86102295e-06},
    ("sac", "cart"): {"parameters": 3.74391675e-07, "critic targets": 2.98023224e-08, "replay rows": 2.86102295e-06, "env state": 2.86102295e-06},
    ("sac", "pendulum"): {"parameters": 5.96046448e-08, "critic targets": 2.98023224e-08, "replay rows": 1.43051147e-06, "env state": 1.1920929e-07},
    ("ddpg", "pendulum"): {"parameters": 5.96046448e-08, "critic targets": 1.49011612e-08, "replay rows": 9.53674316e-07, "env state": 1.1920929e-07}}


# embed_256: 64 envs and a batch of 100, ragged against the 16-row tile
@pytest.mark.parametrize("algo,envname,embed_dim", [pytest.param(a, e, 128, id="%s-%s" % (a, e)) for a, e in _CRITIC_CASES] +
                         [pytest.param(a, e, 256, id="%s-%s-embed_256" % (a, e)) for a, e in _CRITIC_CASES])
def test_critic_forward_pipeline_equals_single_stage_launches(hip, algo, envname, embed_dim, monkeypatch):
    """rpo_cartsafe_{ddpg,sac}_critic_forward (sample -> policy -> projection -> target critics -> critics -> TD/Huber in
    one launch; SpringPendulum: front | batch-coupled projection | back) leaves the same bits behind as the launches it replaces: parameters, targets and replay after 16
    iterations with Philox-drawn batches and noise.

    embed_256 (the critic forwards, fronts and backs at <256, 256>): none of the four cases is bitwise on the parent commit.
    Measured there (parameters | target critics | replay rows | env states):
      ddpg-cart       5.96e-8 | 1.49e-8 | 2.861e-6 | 2.861e-6        sac-cart        3.744e-7 | 2.98e-8 | 2.861e-6 | 2.861e-6
      ddpg-pendulum   5.96e-8 | 1.49e-8 | 9.54e-7 | 1.19e-7          sac-pendulum    5.96e-8 | 2.98e-8 | 1.431e-6 | 1.19e-7
    Each case is asserted at twice its own figures (a margin for data-dependent rounding order)."""
    dev = torch.device("cuda")
    run = functools.partial(_run, embed_dim=embed_dim, **({} if embed_dim == 128 else dict(batch_size=100)))
    n_envs = 256 if embed_dim == 128 else 64
    monkeypatch.setenv("RPO_SCHEDULE", "fused_critic=0")
    a = run(algo, envname, hip, dev, 16, n_envs, use_graph=False)
    assert not a._pipelines
    monkeypatch.setenv("RPO_SCHEDULE", "fused_critic=1")
    b = run(algo, envname, hip, dev, 16, n_envs, use_graph=False)
    assert b._pipelines
    if embed_dim == 256:
        assert b._rollout_pipeline and _no_split_no_actor_pipeline(b)
    _assert_same(a, b, ["parameters", "critic targets", "replay rows", "env state"],
                 _twice(_CRITIC_MAX_256[algo, envname] if embed_dim == 256 else None))
    np.testing.assert_allclose(float(a.last_losses["critic"]), float(b.last_losses["critic"]), rtol=1e-5)


@pytest.mark.parametrize("shared", [True, False], ids=["shared_embedding", "separate_embeddings"])
def test_actor_update_pipeline_matches_single_stage_launches(hip, shared, monkeypatch):
    """rpo_cartsafe_ddpg_actor_forward / _backward (the policy step in two launches + one weights pass) against the ~18
    launches they replace.  Row-local arithmetic is shared code (bit-identical); the Lagrangian sums and, with a shared
    embedding, the first-layer reduction are associated differently -> parameters agree to 1e-7 after 24 iterations."""
    dev = torch.device("cuda")
    monkeypatch.setenv("RPO_SCHEDULE", "fused_actor=0")
    a = _run("ddpg", "cart_viol", hip, dev, 24, 256, use_graph=False, shared_param=shared)
    assert not a._actor_pipeline
    monkeypatch.setenv("RPO_SCHEDULE", "fused_actor=1")
    b = _run("ddpg", "cart_viol", hip, dev, 24, 256, use_graph=False, shared_param=shared)
    assert b._actor_pipeline
    # 1e-7 absolute, or one ulp for the few parameters above 1 (1.2e-7)
    np.testing.assert_allclose(a.agent.flat.data.cpu().numpy(), b.agent.flat.data.cpu().numpy(), rtol=1.2e-7, atol=1e-7)
    np.testing.assert_allclose(a.agent.actor_target_flat.cpu().numpy(), b.agent.actor_target_flat.cpu().numpy(), rtol=1.2e-7, atol=1e-7)
    np.testing.assert_allclose(a.agent.nju.weight.detach().cpu().numpy(), b.agent.nju.weight.detach().cpu().numpy(), rtol=1e-5, atol=1e-8)
    assert float(b.agent.nju.weight.max()) != 0.5 and torch.equal(a.buffer.rows[:256], b.buffer.rows[:256])
    np.testing.assert_allclose(float(a.last_losses["actor"]), float(b.last_losses["actor"]), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("envname", ["cart", "pendulum"])
def test_sac_actor_update_pipeline_matches_single_stage_launches(hip, envname, monkeypatch):
    """rpo_sac_actor_forward / _backward against the ~20 launches (kernels and torch elementwise ops) they replace:
    parameters agree to 1e-7 after 24 iterations (the Lagrangian sums are associated differently)."""
    dev = torch.device("cuda")
    monkeypatch.setenv("RPO_SCHEDULE", "fused_actor=0")
    a = _run("sac", envname, hip, dev, 24, 256, use_graph=False)
    assert not a._actor_pipeline
    monkeypatch.setenv("RPO_SCHEDULE", "fused_actor=1")
    b = _run("sac", envname, hip, dev, 24, 256, use_graph=False)
    assert b._actor_pipeline
    np.testing.assert_allclose(a.agent.flat.data.cpu().numpy(), b.agent.flat.data.cpu().numpy(), rtol=0, atol=1e-7)
    np.testing.assert_allclose(a.agent.critic_target_flat.cpu().numpy(), b.agent.critic_target_flat.cpu().numpy(), rtol=0, atol=1e-7)
    assert torch.equal(a.buffer.rows[:256], b.buffer.rows[:256])
    np.testing.assert_allclose(float(a.last_losses["actor"]), float(b.last_losses["actor"]), rtol=1e-5, atol=1e-6)


def test_ddpg_actor_update_pipeline_on_pendulum(hip, monkeypatch):
    """The env-generic RPODDPG actor pipelines on SpringPendulum-v0 against the single-stage launches (1e-7)."""
    dev = torch.device("cuda")
    monkeypatch.setenv("RPO_SCHEDULE", "fused_actor=0")
    a = _run("ddpg", "pendulum_viol", hip, dev, 24, 256, use_graph=False)
    assert not a._actor_pipeline
    monkeypatch.setenv("RPO_SCHEDULE", "fused_actor=1")
    b = _run("ddpg", "pendulum_viol", hip, dev, 24, 256, use_graph=False)
    assert b._actor_pipeline
    # (the two forms associate the Lagrangian sums differently: 1e-7 per step; after 24 iterations through the batch-coupled
    # projection one of 68 496 parameters sits at 2.1e-7)
    np.testing.assert_allclose(a.agent.flat.data.cpu().numpy(), b.agent.flat.data.cpu().numpy(), rtol=0, atol=4e-7)
    np.testing.assert_allclose(a.agent.nju.weight.detach().cpu().numpy(), b.agent.nju.weight.detach().cpu().numpy(), rtol=1e-5, atol=1e-8)
    np.testing.assert_allclose(float(a.last_losses["actor"]), float(b.last_losses["actor"]), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("algo,envname", [("ddpg", "cart_viol"), ("sac", "cart"), ("sac", "pendulum"), ("ddpg", "pendulum_viol")])
def test_pipelines_with_a_ragged_batch(hip, algo, envname, monkeypatch):
    """batch_size = 100 (not a multiple of the 16-row tile): critic-forward and actor-update pipelines against the
    single-stage launches."""
    dev = torch.device("cuda")
    monkeypatch.setenv("RPO_SCHEDULE", "fused_critic=0,fused_actor=0")
    a = _run(algo, envname, hip, dev, 16, 64, use_graph=False, batch_size=100)
    assert not a._pipelines and not a._actor_pipeline
    monkeypatch.setenv("RPO_SCHEDULE", "fused_critic=1,fused_actor=1")
    b = _run(algo, envname, hip, dev, 16, 64, use_graph=False, batch_size=100)
    assert b._pipelines and b._actor_pipeline
    np.testing.assert_allclose(a.agent.flat.data.cpu().numpy(), b.agent.flat.data.cpu().numpy(), rtol=0, atol=1e-7)
    np.testing.assert_allclose(a.agent.critic_target_flat.cpu().numpy(), b.agent.critic_target_flat.cpu().numpy(), rtol=0, atol=1e-7)
    np.testing.assert_allclose(float(a.last_losses["critic"]), float(b.last_losses["critic"]), rtol=1e-5)
    # the actor pipelines agree with the single-stage launches to 1e-7 (not bitwise), so do the rollouts that follow
    np.testing.assert_allclose(a.buffer.rows.cpu().numpy(), b.buffer.rows.cpu().numpy(), rtol=0, atol=1e-5)


@pytest.mark.parametrize("algo,envname,batch", [pytest.param(a, e, 256, id="%s-%s" % (a, e)) for a, e in CASES[:4]] +
                         [("ddpg", "pendulum", 272), ("sac", "pendulum", 272)])
def test_split_update_equals_row_tile_pipelines(hip, algo, envname, batch, monkeypatch):
    """The column-split update (rpo_split_*: 128 workgroups per network evaluation, head partials summed by the
    consumer, TD prologue + on-the-fly dh in the backward) against the row-tile pipelines it replaces.  Batch 272 (17 row
    tiles, SpringPendulum): one tile past the 256 rows of the wide projection kernel, the one-workgroup form of
    rpo_split_pend_head_project that no other schedule test reaches."""
    dev = torch.device("cuda")
    run = functools.partial(_run, batch_size=batch)
    monkeypatch.setenv("RPO_SCHEDULE", "split=0")
    a = run(algo, envname, hip, dev, 26, 300, use_graph=False)
    assert a._split_state() is None
    monkeypatch.setenv("RPO_SCHEDULE", "split=1")
    b = run(algo, envname, hip, dev, 26, 300, use_graph=False)
    assert b._split_state() is not None and int(b._split_state().st.batch) == batch
    c = run(algo, envname, hip, dev, 26, 300, use_graph=True)
    assert torch.equal(b.agent.flat.data, c.agent.flat.data) and torch.equal(b.buffer.rows, c.buffer.rows)   # graph == eager
    # critic update: bit for bit (3 iterations: before the first policy step)
    monkeypatch.setenv("RPO_SCHEDULE", "split=0")
    a3 = run(algo, envname, hip, dev, 3, 300, use_graph=False)
    monkeypatch.setenv("RPO_SCHEDULE", "split=1")
    b3 = run(algo, envname, hip, dev, 3, 300, use_graph=False)
    assert torch.equal(a3.agent.flat.data, b3.agent.flat.data)
    assert torch.equal(a3.agent.critic_target_flat, b3.agent.critic_target_flat)
    assert torch.equal(a3.agent.critic_optim.exp_avg_sq, b3.agent.critic_optim.exp_avg_sq)
    assert float(a3.last_losses["critic"]) == float(b3.last_losses["critic"])
    # with policy steps: d(-Q)/d action is summed over column groups instead of one 128-term chain, so the actor's
    # gradient agrees to ~1e-7 relative and the runs drift apart at that level (Adam normalises the step: 26 iterations
    # of lr 1e-4 / 3e-4 steps keep the parameters within 2e-6)
    np.testing.assert_allclose(a.agent.flat.data.cpu().numpy(), b.agent.flat.data.cpu().numpy(), rtol=0, atol=2e-6)
    np.testing.assert_allclose(a.agent.nju.weight.detach().cpu().numpy(), b.agent.nju.weight.detach().cpu().numpy(), rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(float(a.last_losses["critic"]), float(b.last_losses["critic"]), rtol=1e-4)
    np.testing.assert_allclose(float(a.last_losses["actor"]), float(b.last_losses["actor"]), rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("algo,envname", [("sac", "cart"), ("ddpg", "pendulum"), ("sac", "pendulum")])
def test_overlapped_rollout_equals_serial(hip, algo, envname, monkeypatch):
    """Inside a multi-iteration hipGraph the rollout of step t+1 runs on a second stream beside the update of step t (no
    shared embedding; forked after the sampling launch, joined before the next one; serial after policy steps).  The
    update reads its own clock, so nothing it sees moves: 70 iterations equal the serial order bit for bit."""
    # (round 5: the branch is the default where the update runs through the generic launches -- EVOPF-v0 --, never beside
    # the pipelines of the classic-control envs, where it was measured slower; here the classic-control envs on the generic
    # launches exercise it, `_overlap_enabled = False` is the serial order)
    from rpo_amd.algo.trainer import RPOTrainerBase
    dev = torch.device("cuda")
    monkeypatch.setenv("RPO_GRAPH_CYCLE", "8")
    monkeypatch.setenv("RPO_SCHEDULE", "fused_critic=0,fused_actor=0")
    a = _run(algo, envname, hip, dev, 70, 300, use_graph=True)
    assert a._overlap_ok(True) and a._graphs.entries[("cycle", 8, True, "overlap")]["graph"] is not None
    monkeypatch.setattr(RPOTrainerBase, "_overlap_enabled", False, raising=False)
    b = _run(algo, envname, hip, dev, 70, 300, use_graph=True)
    assert ("cycle", 8, True, "overlap") not in b._graphs.entries
    c = _run(algo, envname, hip, dev, 70, 300, use_graph=False)
    for other in (b, c):
        assert torch.equal(a.vec.internal, other.vec.internal)
        assert torch.equal(a.buffer.rows, other.buffer.rows)
        assert torch.equal(a.agent.flat.data, other.agent.flat.data)
        assert torch.equal(a.agent.critic_target_flat, other.agent.critic_target_flat)
        assert torch.equal(a.agent.nju.weight, other.agent.nju.weight)
        assert torch.equal(a.vec.stats[:70], other.vec.stats[:70])
    assert int(a._uctrl[0]) == 71 and int(a.vec.ctrl[0]) == 70       # the update clock runs one ahead between iterations
    # a full ring: the fork sits behind the gather, so the rollout never overwrites a slot the sampler still reads
    d = _run(algo, envname, hip, dev, 70, 64, use_graph=True, capacity=5)
    monkeypatch.setattr(RPOTrainerBase, "_overlap_enabled", True, raising=False)
    e = _run(algo, envname, hip, dev, 70, 64, use_graph=True, capacity=5)
    assert ("cycle", 8, True, "overlap") in e._graphs.entries and ("cycle", 8, True, "overlap") not in d._graphs.entries
    assert torch.equal(d.agent.flat.data, e.agent.flat.data) and torch.equal(d.buffer.rows, e.buffer.rows)


@pytest.mark.parametrize("algo,envname", [("sac", "cart"), ("ddpg", "pendulum"), ("sac", "pendulum")])
def test_ridden_rollout_equals_serial(hip, algo, envname, monkeypatch):
    """Inside a multi-iteration window the rollout of step t+1 rides on the launches of the critic update of step t
    (rpo_split_critic_fwd_a_ride / _fwd_b_ride: the actor forward of a lane range each; rpo_split_critic_bwd_b_ride:
    explore / project / step / scatter, behind fwd_a's gather); serial after policy steps.  Same arithmetic, and the update reads its own clock: 70
    iterations equal the serial order bit for bit (the per-step statistics are float sums over lanes in a different
    association: equal to rounding, the counters exactly)."""
    dev = torch.device("cuda")
    monkeypatch.setenv("RPO_GRAPH_CYCLE", "8")
    a = _run(algo, envname, hip, dev, 70, 300, use_graph=True)
    assert a._ride_ok(True) and a._graphs.entries[("cycle", 8, True, "ride")]["graph"] is not None
    monkeypatch.setenv("RPO_SCHEDULE", "ride=0")
    b = _run(algo, envname, hip, dev, 70, 300, use_graph=True)
    assert not b._ride_ok(True) and ("cycle", 8, True, "ride") not in b._graphs.entries
    c = _run(algo, envname, hip, dev, 70, 300, use_graph=False)
    for other in (b, c):
        assert torch.equal(a.vec.internal, other.vec.internal)
        assert torch.equal(a.vec.action, other.vec.action)
        assert torch.equal(a.vec.ep_len, other.vec.ep_len) and torch.equal(a.vec.ep_count, other.vec.ep_count)
        assert torch.equal(a.buffer.rows, other.buffer.rows)
        assert torch.equal(a.agent.flat.data, other.agent.flat.data)
        assert torch.equal(a.agent.critic_target_flat, other.agent.critic_target_flat)
        assert torch.equal(a.agent.nju.weight, other.agent.nju.weight)
        _stats_equal(a, other, 70)
    assert int(a._uctrl[0]) == 71 and int(a.vec.ctrl[0]) == 70 and a.vec.steps_host == 70
    # a full ring: both halves sit behind the gather, so the step never overwrites a slot the sampler still reads
    d = _run(algo, envname, hip, dev, 70, 64, use_graph=True, capacity=5)
    monkeypatch.setenv("RPO_SCHEDULE", "ride=1")
    e = _run(algo, envname, hip, dev, 70, 64, use_graph=True, capacity=5)
    assert ("cycle", 8, True, "ride") in e._graphs.entries
    assert torch.equal(d.agent.flat.data, e.agent.flat.data) and torch.equal(d.buffer.rows, e.buffer.rows)
    assert torch.equal(d.vec.internal, e.vec.internal)
    # a shared state embedding (scripts/cart_exp.py): the critic step changes the policy, nothing rides
    f = build_trainer("ddpg", "cart", hip, dev, num_envs=64, use_graph=True)
    assert f.agent.flat.sizes[1] > 0 and not f._ride_ok(True)


_FRONT_CASES = [
    ("ddpg", "cart", True, "0"), ("ddpg", "cart", False, "0"), ("sac", "cart", False, "0"), ("sac", "cart", False, "1"),
    ("ddpg", "cart", False, "1"), ("sac", "pendulum", False, "0"), ("sac", "pendulum", False, "1"), ("ddpg", "pendulum", False, "1"),
    ("ddpg", "pendulum", True, "0")]
# SpringPendulum with a projection budget past the workspace kernel's (31 > 30 steps): no rpo_split_critic_pfront, so front=1 is
# fwd_a | projection | rpo_split_critic_mid / _mid_pol (ride=0) / _mid_ride (ride=1).  Batch 128: 8 row tiles, one per XCD.
_MID_CASES = [("sac", "pendulum", False, "0"), ("ddpg", "pendulum", False, "1")]


@pytest.mark.parametrize("algo,envname,shared,ride,mid", [pytest.param(*c, False, id="%s-%s-%s-%s" % c) for c in _FRONT_CASES] +
                         [pytest.param(*c, True, id="%s-%s-%s-%s-mid" % c) for c in _MID_CASES])
def test_fused_front_launch_equals_separate_launches(hip, algo, envname, shared, ride, mid, monkeypatch):
    """CartSafe critic update: fwd_a, fwd_b and bwd_a as ONE launch (rpo_split_critic_front: the later stages wait inside the
    launch for the workgroups of their own row tile; _pol: pol_a of a policy iteration as one more plane; _ride: the actor
    forward of the next vector step in the planes behind) leaves the same bits as the separate launches, eagerly and replayed
    from graph windows; no wait ever gives up and the arrival words are zero again after every launch.  SpringPendulum: fwd_b
    and bwd_a (rpo_split_critic_mid*; the batch-coupled projection in between keeps fwd_a a launch of its own)."""
    dev = torch.device("cuda")
    monkeypatch.setenv("RPO_GRAPH_CYCLE", "8")
    extra = dict(shared_param=shared) if algo == "ddpg" else {}
    if mid:
        extra.update(batch_size=128, max_steps=31)
    runs = {}
    for front in ("0", "1"):
        monkeypatch.setenv("RPO_SCHEDULE", "ride=%s,front=%s" % (ride, front))   # (rides in the graph windows only)
        for graph in (False, True):
            runs[front, graph] = _run(algo, envname, hip, dev, 45, 300, use_graph=graph, **extra)
    a = runs["0", False]
    for key in (("1", False), ("1", True), ("0", True)):
        b = runs[key]
        assert torch.equal(a.agent.flat.data, b.agent.flat.data), key
        assert torch.equal(a.agent.critic_target_flat, b.agent.critic_target_flat), key
        assert torch.equal(a.agent.critic_optim.exp_avg_sq, b.agent.critic_optim.exp_avg_sq), key
        assert torch.equal(a.agent.nju.weight, b.agent.nju.weight), key
        assert torch.equal(a.buffer.rows, b.buffer.rows) and torch.equal(a.vec.internal, b.vec.internal), key
        assert float(a.last_losses["critic"]) == float(b.last_losses["critic"]), key
    assert runs["1", True]._front_ok() and runs["1", False]._front_ok() and not runs["0", True]._front_ok()
    assert runs["1", True]._ride_ok(True) == (ride == "1")
    assert not (mid and runs["1", True]._pfront)
    sync = runs["1", True]._split_state()._held["tile_sync"]
    assert int(sync.abs().sum()) == 0


@pytest.mark.parametrize("algo,envname", [("ddpg", "cart"), ("sac", "cart"), ("sac", "pendulum")])
def test_aborted_graph_capture_falls_back_to_eager_from_a_clean_state(hip, algo, envname, monkeypatch):
    """A hipGraph capture that fails has run the iteration's Python -- hand-over flags, the stages' argument struct, the host
    step counter -- but no launch.  `_GraphCache` restores that host state before the eager re-run: a run whose first capture
    dies in the middle of a window equals an eager run bit for bit (and warns).  (The flags are recomputed by every iteration's
    `_set_hand_overs`, so today's schedules also survive without the restore -- checked by hand; the snapshot keeps that from
    depending on which flag a future schedule forgets to recompute.)"""
    dev = torch.device("cuda")
    monkeypatch.setenv("RPO_GRAPH_CYCLE", "8")
    a = _run(algo, envname, hip, dev, 45, 300, use_graph=False)
    orig, seen = hip.SplitUpdate.run, [0]

    def failing_run(self, stage, rider=None):
        # the capture dies in the MIDDLE of a window: behind a critic update's front launch, in front of its bwd_b
        if torch.cuda.is_current_stream_capturing() and stage == "critic_bwd_b":
            seen[0] += 1
            if seen[0] == 3:
                raise RuntimeError("forced capture failure")
        return orig(self, stage, rider)
    monkeypatch.setattr(hip.SplitUpdate, "run", failing_run)
    with pytest.warns(UserWarning, match="hipGraph capture failed"):
        b = _run(algo, envname, hip, dev, 45, 300, use_graph=True)
    assert not b._graphs.enabled
    assert torch.equal(a.agent.flat.data, b.agent.flat.data)
    assert torch.equal(a.agent.critic_target_flat, b.agent.critic_target_flat)
    assert torch.equal(a.agent.critic_optim.exp_avg_sq, b.agent.critic_optim.exp_avg_sq)
    assert int(a.agent.critic_optim.step_dev[0]) == int(b.agent.critic_optim.step_dev[0])
    assert torch.equal(a.buffer.rows, b.buffer.rows) and torch.equal(a.vec.internal, b.vec.internal)
    assert int(a.vec.ctrl[0]) == int(b.vec.ctrl[0]) == 45


@pytest.mark.parametrize("algo,envname", [("ddpg", "cart"), ("sac", "cart")])
def test_tail_windows_equal_eager(hip, algo, envname, monkeypatch):
    """The last < RPO_GRAPH_CYCLE iterations of a run_steps call are one shorter graph window (whole policy_fre periods; the
    library default since round 5, bench.py's own switch before) instead of single-iteration graphs -- same launches in the
    same order: six calls of 20 iterations (a 16-iteration window + a 4-iteration one each, both captured by then) equal 120
    eager iterations bit for bit."""
    dev = torch.device("cuda")
    runs = []
    for graph in (False, True):
        torch.manual_seed(5)
        tr = build_trainer(algo, envname, hip, dev, num_envs=300, use_graph=graph)
        tr.vec.reset()
        for _ in range(6):
            tr.run_steps(20)
        torch.cuda.synchronize()
        runs.append(tr)
    a, b = runs
    keys = [k for k, e in b._graphs.entries.items() if e["graph"] is not None]
    assert any(k[:2] == ("cycle", 4) for k in keys) and any(k[:2] == ("cycle", 16) for k in keys), keys
    assert torch.equal(a.agent.flat.data, b.agent.flat.data) and torch.equal(a.agent.nju.weight, b.agent.nju.weight)
    assert torch.equal(a.buffer.rows, b.buffer.rows) and torch.equal(a.vec.internal, b.vec.internal)
    assert int(b.vec.ctrl[0]) == 120 == int(a.vec.ctrl[0])


@pytest.mark.parametrize("algo,envname,batch", [("ddpg", "cart", 250), ("sac", "cart", 128), ("sac", "pendulum", 250)])
def test_fused_front_with_other_batch_sizes(hip, algo, envname, batch, monkeypatch):
    """The fused launches at batch sizes other than 256: 250 rows (16 row tiles, the last one partly empty: its masked rows
    still count their workgroups' arrivals) and 128 rows (8 tiles: one per XCD).  Same bits as the separate launches."""
    dev = torch.device("cuda")
    monkeypatch.setenv("RPO_GRAPH_CYCLE", "8")
    runs = {}
    for front in ("0", "1"):
        monkeypatch.setenv("RPO_SCHEDULE", "front=" + front)
        runs[front] = _run(algo, envname, hip, dev, 45, 300, use_graph=True, batch_size=batch)
    a, b = runs["0"], runs["1"]
    assert b._front_ok() and not a._front_ok()
    assert torch.equal(a.agent.flat.data, b.agent.flat.data) and torch.equal(a.agent.nju.weight, b.agent.nju.weight)
    assert torch.equal(a.agent.critic_target_flat, b.agent.critic_target_flat)
    assert torch.equal(a.buffer.rows, b.buffer.rows) and torch.equal(a.vec.internal, b.vec.internal)
    assert int(b._split_state()._held["tile_sync"].abs().sum()) == 0


@pytest.mark.parametrize("algo,envname", [("ddpg", "cart"), ("sac", "cart"), ("sac", "pendulum")])
def test_large_batch_update_mode(hip, algo, envname, monkeypatch):
    """batch_size >= RPO_SPLITK_FROM (one batch of 256 * N per vector step): the update runs through the generic
    MLP kernels with the split-K weights pass; SpringPendulum batches beyond 1024 rows are projected row by row -- other
    semantics than the reference's sample-coupled batch, so the trainer refuses them unless RPO_ROWWISE_PROJECTION=1.  hipGraph
    windows == eager launches bit for bit (every reduction has a fixed order), parameters move and stay finite, and the
    first critic update equals the same update through the plain one-owner weights pass to summation round-off."""
    dev = torch.device("cuda")
    B = hip.CONST["RPO_SPLITK_FROM"]
    if envname == "pendulum":
        with pytest.raises(ValueError, match="RPO_ROWWISE_PROJECTION"):
            build_trainer(algo, envname, hip, dev, num_envs=512, use_graph=False, batch_size=B, capacity=64)
        monkeypatch.setenv("RPO_ROWWISE_PROJECTION", "1")
    a = _run(algo, envname, hip, dev, 24, 512, use_graph=True, batch_size=B, capacity=64)
    assert a.projection_mode == "row-wise"
    b = _run(algo, envname, hip, dev, 24, 512, use_graph=False, batch_size=B, capacity=64)
    assert a._large_batch and not a._pipelines and not a._actor_pipeline and a._split_state() is None
    assert all(d.splitk is not None for n, d in a.fused.descs.items() if "target" not in n)
    assert envname != "pendulum" or not a.batch_reference
    assert torch.equal(a.agent.flat.data, b.agent.flat.data) and torch.equal(a.buffer.rows, b.buffer.rows)
    assert torch.equal(a.agent.critic_target_flat, b.agent.critic_target_flat) and torch.equal(a.agent.nju.weight, b.agent.nju.weight)
    assert bool(torch.isfinite(a.agent.flat.data).all()) and int(a.agent.critic_optim.step_dev[0]) == 24
    # one update with / without the scratch buffers (same sampled batch: same seed, same clock)
    c = _run(algo, envname, hip, dev, 1, 512, use_graph=False, batch_size=B, capacity=64)
    torch.manual_seed(5)
    d = build_trainer(algo, envname, hip, dev, num_envs=512, use_graph=False, batch_size=B, capacity=64)
    for desc in d.fused.descs.values():
        desc.splitk = None
    d.vec.reset()
    d.run_steps(1)
    torch.cuda.synchronize()
    np.testing.assert_allclose(c.agent.flat.data.cpu().numpy(), d.agent.flat.data.cpu().numpy(), rtol=0, atol=2e-6)


def test_large_batch_mode_is_reproducible_run_to_run(hip):
    """One batch-2^20 update per vector step at 4096 lanes (bench.py's `large_batch`): two runs from the same seeds end with the
    same bits.  Round 4 found they did not (3e-8 on the parameters after 40 updates): rpo_*_lagrangian added its per-workgroup
    partial sums of the multiplier gradient with float atomics once the batch spanned more than one workgroup; the sums are now
    taken by one workgroup in a fixed order."""
    dev = torch.device("cuda")
    runs = []
    for _ in range(2):
        tr = _run("ddpg", "cart", hip, dev, 24, 4096, use_graph=True, batch_size=256 * 4096, capacity=32)
        runs.append((tr.agent.flat.data.clone(), tr.agent.nju.weight.detach().clone(), tr.buffer.rows.clone()))
        del tr
        torch.cuda.empty_cache()
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    assert float(runs[0][1].abs().max()) > 0.0                  # the multipliers moved: the reduction in question was exercised


def test_large_batch_graph_windows_keep_the_padding_floats_zero(hip, monkeypatch):
    """Round 6, found by the failure flag (tests/test_failure_flag.py): under hipGraph REPLAY the large-batch update was not
    what the eager launches compute.  The split-K scratch (35 MB at 2^20 rows) was zeroed by `hipMemsetAsync`, which stream
    capture turns into a memset NODE; replayed inside the trainer's windows, that node filled the buffer with a stale 16-byte
    pattern instead of zeros -- visible in the three padding floats behind the critic's head bias (which no
    kernel writes), different from run to run, NaN once in a few thousand updates (the NaN reached an action at update 2060 of a
    3000-update run: NonFiniteError).  Never with eager launches.  The scratch is now zeroed by a kernel of the library
    (mlp_bwd.h splitk_zero_kernel; -DRPO_SPLITK_ZERO=0 is the old form, tools/probe/dbg_padding.py the reproducer).
    Asserted: after 48 iterations through graph windows every padding float of the flat parameter buffer, of its gradient and
    of both optimisers' moments is exactly zero, and the parameters equal the eager run's bit for bit."""
    dev = torch.device("cuda")
    monkeypatch.setenv("RPO_GRAPH_CYCLE", "4")
    out = {}
    for use_graph in (False, True):
        tr = _run("ddpg", "cart", hip, dev, 48, 4096, use_graph=use_graph, batch_size=256 * 4096, capacity=64)
        fl = tr.agent.flat
        pad = torch.ones(fl.total, dtype=torch.bool, device=dev)
        for mod in (tr.agent.actor, tr.agent.critic, tr.agent.nju):
            for p in mod.parameters():
                o = fl.offset.get(id(p))
                if o is not None:
                    pad[o:o + p.numel()] = False
        assert int(pad.sum()) >= 3                              # (the critic's one-float head bias is followed by three)
        assert not bool(fl.data[pad].any()) and not bool(fl.grad[pad].any()), (use_graph, fl.data[pad].tolist())
        for opt, (lo, hi) in ((tr.agent.critic_optim, fl.critic_range), (tr.agent.actor_optim, fl.actor_range)):
            assert not bool(opt.exp_avg[pad[lo:hi]].any()) and not bool(opt.exp_avg_sq[pad[lo:hi]].any()), use_graph
        if use_graph:
            assert any(e["graph"] is not None for e in tr._graphs.entries.values()) and not tr._graphs.capture_failed
        out[use_graph] = (fl.data.clone(), tr.agent.nju.weight.detach().clone())
        del tr
        torch.cuda.empty_cache()
    assert torch.equal(out[False][0], out[True][0]) and torch.equal(out[False][1], out[True][1])


@pytest.mark.parametrize("algo,envname,n,extra", [("ddpg", "cart", 4096, {}), ("ddpg", "cart", 4096, dict(batch_size=256 * 4096, capacity=64)),
                                                  ("sac", "pendulum", 4096, {}), ("ddpg", "evopf256", 1024, {})])
def test_the_windows_hold_kernel_nodes_only(hip, monkeypatch, algo, envname, n, extra):
    """a hipMemsetAsync captured into the windows (a memset NODE) was replayed with a stale fill pattern.  The
    library launches kernels only (tests/test_docs.py) and the trainer issues no torch operation inside a window that the
    capture turns into a memset / memcpy node: with RPO_GRAPH_AUDIT=1 the captured hipGraph_t is kept and its nodes are counted
    by kind (hipGraphGetNodes / hipGraphNodeGetType)."""
    monkeypatch.setenv("RPO_GRAPH_AUDIT", "1")
    tr = _run(algo, envname, hip, torch.device("cuda"), 96, n, use_graph=True, **extra)
    kinds = [e.get("node_kinds") for e in tr._graphs.entries.values() if e["graph"] is not None]
    assert kinds and not tr._graphs.capture_failed
    for k in kinds:
        assert set(k) == {"kernel"} and k["kernel"] >= 16, k
