#!/usr/bin/env python3
"""Record how a library refuses the faulty calls of tests/temporal_refusal_cases.py: (entry point, case, return code, mi355pt_last_error
text) into tests/golden/temporal_refusals.json, which tests/test_temporal_refusals.py replays on the tree's library.  Run it on a library
built from the revision whose refusals are the contract.  Needs no GPU: every case must be refused by a check (MI355PT_E_INVALID).

  tools/record_temporal_refusals.py <path/to/libmi355pt.so> [out.json]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import temporal_refusal_cases as rc  # noqa: E402

if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    records = rc.Caller(sys.argv[1]).records()
    slipped = [r for r in records if r["code"] != rc.INVALID]
    assert not slipped, "not refused by a check: %s" % slipped[:5]
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "temporal_refusals.json")
    with open(out, "w") as fh:
        fh.write("[\n" + ",\n".join(json.dumps(r) for r in records) + "\n]\n")      # one record per line
    print("%d records -> %s" % (len(records), out))
