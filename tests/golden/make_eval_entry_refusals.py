"""Record the return codes of the host-side refusals of the 14 ``rpo_<env>_evaluate*`` entry points.

    python tests/golden/make_eval_entry_refusals.py              # needs the built library, no GPU

Writes ``eval_entry_refusals.json``: the id of every call of the table of ``tests/test_evaluate_entry_refusals.py`` -> the code
the library returned.  The fixture was recorded with the library of the commit BEFORE the entry points were folded onto one
validation ladder (this script and the test copied into a checkout of that commit), so the test pins the order of the checks as
it was.  Regenerate it only when an entry point's validation is changed on purpose.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, "..", ".."), os.path.join(HERE, "..")]
import test_evaluate_entry_refusals as refusals  # noqa: E402

if __name__ == "__main__":
    codes = refusals.run_table()
    with open(refusals.FIXTURE, "w") as f:
        json.dump(codes, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d calls, codes %s" % (refusals.FIXTURE, len(codes), sorted(set(codes.values()))))
