#!/usr/bin/env python3
"""Record how a library refuses the faulty calls of tests/scene_update_refusal_cases.py: (part, entry point, case, return code,
mi355pt_last_error text) into tests/golden/scene_update_refusals.json, which tests/test_scene_update_refusals.py replays on the tree's
library.  Run it on a library built from the revision whose refusals are the contract.  Part 1 needs no GPU; part 2 builds scene "1" on
the MI355X and checks after every refused call that the device arrays kept their digest.  Every case must be refused by a check.

  tools/record_scene_update_refusals.py <path/to/libmi355pt.so> [out.json]
"""
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

if __name__ == "__main__":
    argv = sys.argv[1:]
    if not argv:
        sys.exit(__doc__)
    import torch  # noqa: F401  (first, as in tests/conftest.py)
    import scene_update_refusal_cases as rc
    pkg = importlib.import_module("toy-cpu-pathtracing_amd")
    lib = os.path.abspath(argv[0])
    records = rc.Caller(pkg, lib, part=1).records()
    caller = rc.Caller(pkg, lib, part=2)
    digest = {id(sc): sc.debug_device_digest() for sc in (caller.scene, caller.multi)}

    def unchanged(entry, name, sc):
        assert sc.debug_device_digest() == digest[id(sc)], (entry, name)
    records += caller.records(unchanged)
    assert [(r["part"], r["entry"], r["case"]) for r in records] == [(p, e, n) for p in (1, 2) for e, n, _ in rc.cases(p)]
    slipped = [r for r in records if r["code"] == 0 or not r["error"]]
    assert not slipped, "not refused by a check: %s" % slipped[:5]
    out = argv[1] if len(argv) > 1 else os.path.join(ROOT, "tests", "golden", "scene_update_refusals.json")
    with open(out, "w") as fh:
        fh.write("[\n" + ",\n".join(json.dumps(r) for r in records) + "\n]\n")      # one record per line
    print("%d records -> %s" % (len(records), out))
