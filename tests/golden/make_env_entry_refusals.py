"""Record the return codes of the host-side refusals of the 32 stand-alone env entry points (csrc/cartsafe.hip, pendulum.hip,
evopf.hip, act.hip).

    python tests/golden/make_env_entry_refusals.py               # needs the built library and NO GPU

Runs every candidate of the table of ``tests/test_env_entry_refusals.py`` and keeps the ones the library refuses with RPO_ERR_ARG
or RPO_ERR_NULL (an accepted candidate goes on to a launch, which without a device returns a HIP error and does nothing; with a
device it would run a kernel on host addresses, so this script refuses to start where /dev/kfd exists).  Writes
``env_entry_refusals.json`` in the layout of ``split_entry_refusals.json`` (make_split_entry_refusals.py), its keys the symbols.
Every pair (ARG defect, NULL defect) of a key is kept: none is dropped.

The fixture was recorded with the library of the commit BEFORE these entry points were put on the shared launch helper and the
shared checks (this script and the test copied into a checkout of that commit), so the test pins the order of the checks as it
was.  Regenerate it only when an entry point's validation is changed on purpose.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, "..", ".."), os.path.join(HERE, "..")]
import test_env_entry_refusals as refusals  # noqa: E402
from rpo_amd import _lib  # noqa: E402

if __name__ == "__main__":
    if refusals.HAS_GPU_NODE:
        sys.exit("/dev/kfd exists: an accepted candidate would launch a kernel on host addresses; record on a box without a GPU")
    lib, letter = _lib.load(), refusals.LETTER
    singles = refusals.run_rows(lambda key, names: [(n,) for n in names])
    kept = {key: {kind: [row[0] for row, code in codes.items() if letter.get(code) == kind] for kind in "AN"}
            for key, codes in singles.items()}
    pairs = refusals.run_rows(lambda key, names: [(a, n) for a in kept[key]["A"] for n in kept[key]["N"]])
    combos = {key: {"arg": k["A"], "null": k["N"],
                    "pairs": {a: "".join(letter.get(pairs[key][(a, n)], ".") for n in k["N"]) for a in k["A"]}}
              for key, k in kept.items()}
    out = {"all_null": {s: refusals.all_null(lib, s) for s in refusals.SYMBOLS}, "combos": combos}
    with open(refusals.FIXTURE, "w") as f:
        json.dump(out, f, indent=None, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    n_single = sum(len(k["A"]) + len(k["N"]) for k in kept.values())
    n_pairs = sum(len(s) - s.count(".") for c in combos.values() for s in c["pairs"].values())
    print("wrote %s: %d single refusals, %d pairs, %d bytes" % (refusals.FIXTURE, n_single, n_pairs, os.path.getsize(refusals.FIXTURE)))
    accepted = {s: [r[0] for r, c in codes.items() if c not in letter] for s, codes in singles.items()}
    print("accepted single candidates:", {s: a for s, a in accepted.items() if a})
