"""Record what the env kernel classes of rpo_amd/ops.py hand to the library.

    python tests/golden/make_env_binding_calls.py                # needs neither the built library nor a GPU

Runs every case of ``tests/test_env_binding_calls.py`` and writes ``env_binding_calls.json``:
``{"constructors": {case: text}, "methods": {class key: {method: {case: {"calls": [[symbol, [argument, ...]]]} | {"error": text}}}}}``;
the case ``optional_none`` also carries ``nulled``, the tensor parameters the classes accepted as None one at a time.

The fixture was recorded with the ops.py of the commit BEFORE the per-env method bodies were folded onto one base class (this
script and the test copied into a checkout of that commit), so the test pins every argument list as it was.  Regenerate it only
when a binding's argument list is changed on purpose.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, "..", ".."), os.path.join(HERE, "..")]
import test_env_binding_calls as calls  # noqa: E402

if __name__ == "__main__":
    out = calls.record(lambda key, method, results: [c[5:] for c, r in results.items() if c.startswith("none:") and "calls" in r])
    with open(calls.FIXTURE, "w") as f:
        json.dump(out, f, indent=None, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    n = sum(len(r) for m in out["methods"].values() for r in m.values())
    errors = sorted({r["error"] for m in out["methods"].values() for rs in m.values() for r in rs.values() if "error" in r})
    print("wrote %s: %d cases, %d bytes" % (calls.FIXTURE, n, os.path.getsize(calls.FIXTURE)))
    print("\n".join(errors))
