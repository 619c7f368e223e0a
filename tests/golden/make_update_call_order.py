"""Record the backend / kernels calls the trainers make over a few iterations.

    python tests/golden/make_update_call_order.py                # CPU only: the oracle backend, no built library, no GPU

Runs every case of ``tests/test_update_call_order.py`` and writes ``update_call_order.json``:
``{"table": [call, ...], "cases": {case: [index into table, ...]}}``, a call being ``name(token,...)``.

The fixture was recorded with the trainers of the commit BEFORE the update skeleton of RPODDPG / RPOSAC was hoisted into
RPOTrainerBase (this script and the test copied into a checkout of that commit), so the test pins every call and its order as
they were.  Regenerate it only when a launch or its arguments are changed on purpose.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, "..", ".."), os.path.join(HERE, "..")]
import test_update_call_order as calls  # noqa: E402

if __name__ == "__main__":
    lists = {name: calls.run_case(name) for name in sorted(calls.CASES)}
    out = calls.pack(lists)
    with open(calls.FIXTURE, "w") as f:
        json.dump(out, f, indent=None, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print("wrote %s: %d cases, %d calls (%d distinct), %d bytes" % (calls.FIXTURE, len(lists), sum(map(len, lists.values())),
                                                                   len(out["table"]), os.path.getsize(calls.FIXTURE)))
    for name, c in sorted(lists.items()):
        print("  %-32s %5d calls" % (name, len(c)))
