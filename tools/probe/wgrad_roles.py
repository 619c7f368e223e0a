#!/usr/bin/env python
"""Durations of the all-rows launches of the column-split update (GPU box): split_critic_bwd_b [_ride] and split_policy_e of one
policy_fre period of a workload, by bench.time_kernel (a hipGraph of back-to-back launches between one event pair), under each
value of the tuning key wgrad_staged.

    python tools/probe/wgrad_roles.py WORKLOAD [REPEATS] [OUT.json]

RPO_HIP_LIBRARY selects another build of the library: the timing-only variants that leave one role out
(KIND=ns tools/probe/build_stream_variants.sh N..., -DRPO_NS_SKIP=N, rpo_amd/csrc/nsplit_dev.h) or the parent commit's.  A library
without the key (the parent's) is timed once, as it is.  Prints one JSON line; with OUT.json appends it to that file."""
import json
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import bench
from rpo_amd import _lib, ops
from rpo_amd.algo.trainer import NonFiniteError

WANT = ("split_critic_bwd_b", "split_critic_bwd_b_ride", "split_policy_e")


def record_period(tr):
    """The launches of one policy_fre period, as bench.kernel_clinic records them."""
    graphs_on = tr._graphs.enabled
    tr._graphs.enabled = False
    tr._flush_tail()
    rec = bench.LaunchRecorder(tr)
    try:
        t0 = tr._t
        if getattr(tr, "_ride_ok", lambda d: False)(True):
            tr._sync_uclock(rollout_pending=True)
            tr._uclock_ok = True
            tr._ridden_window(t0, tr.policy_fre)
            for i in range(tr.policy_fre):
                tr._advance_host(t0 + i + 1)
            tr._updates += tr.policy_fre
        else:
            for i in range(tr.policy_fre):
                tr._iteration(False, True, (t0 + i + 1) % tr.policy_fre == 0)
                tr._advance_host(t0 + i + 1)
                tr._updates += 1
    finally:
        rec.close()
        tr._graphs.enabled = graphs_on
    torch.cuda.synchronize()
    first = {}
    for name, fn, a, kw in rec.calls:
        if name in WANT and name not in first:
            first[name] = (fn, a, kw)
    return first


def main():
    w = sys.argv[1] if len(sys.argv) > 1 else "cart_ddpg"
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    os.environ.setdefault("RPO_VERBOSE", "0")
    tr = bench.make_trainer(bench.envs_per_gpu(w), torch.device("cuda", 0), 10 ** 9, capacity=64, workload=w)
    tr.vec.reset()
    nonfinite = False
    try:
        tr.run_steps(64)
    except NonFiniteError:                                       # a timing-only library (no optimiser bookkeeping, gradients left out):
        nonfinite = True                                         # the launches are timed on the buffers as they are
    calls = record_period(tr)
    has_key = _lib.load().rpo_tuning(ops.TUNE["wgrad_staged"], -1) >= 0
    out = dict(workload=w, library=os.path.basename(_lib.LIBRARY), repeats=repeats, nonfinite_warmup=nonfinite, us={})
    for staged in ((1, 0) if has_key else (None,)):
        for name, (fn, a, kw) in sorted(calls.items()):
            def one():
                return bench.time_kernel(lambda: fn(*a, **kw))[0]
            if staged is None:
                ts = [one() for _ in range(repeats)]
            else:
                with ops.tuning(wgrad_staged=staged):
                    ts = [one() for _ in range(repeats)]
            key = name if staged is None else "%s@wgrad_staged=%d" % (name, staged)
            out["us"][key] = dict(median=float(np.median(ts)), min=min(ts), max=max(ts), all=ts)
    line = json.dumps(out)
    print(line, flush=True)
    if len(sys.argv) > 3:
        with open(sys.argv[3], "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
