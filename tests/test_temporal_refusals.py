"""The refusals of the twelve mi355pt_temporal_accumulate* entry points, precedence between the checks included: every faulty call of
tests/temporal_refusal_cases.py is replayed on the tree's library and must give the return code and the mi355pt_last_error text that
tests/golden/temporal_refusals.json holds for it — recorded (tools/record_temporal_refusals.py) from the library as it was before the
entry points became calls of one driver.  Needs no GPU: every case is refused by a check."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import temporal_refusal_cases as rc  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "temporal_refusals.json")


def test_case_list_covers_every_form_group_and_pair():
    """All twelve entry points; per entry point every applicable fault alone and every pair of its groups; unique names."""
    cases = rc.cases()
    assert len({(e, n) for e, n, _ in cases}) == len(cases)
    assert len(rc.FORMS) == 12 and {e for e, _, _ in cases} == set(rc.FORMS)
    for entry in rc.FORMS:
        names = {n for e, n, _ in cases if e == entry}
        groups = rc._groups(entry)
        for g in groups:
            assert {"%s.%s" % (g, n) for n, _, needs in rc.FAULTS[g] if rc._applies(entry, needs)} <= names
        for i, g0 in enumerate(groups):
            for g1 in groups[i + 1:]:
                assert any(n.startswith(g0 + ".") and ("+" + g1 + ".") in n for n in names), (entry, g0, g1)


def test_refusals_match_the_recorded_ones(pkg):
    golden = json.load(open(GOLDEN))
    assert [(r["entry"], r["case"]) for r in golden] == [(e, n) for e, n, _ in rc.cases()], "the case list changed: record the fixture again"
    assert all(r["code"] == rc.INVALID and r["error"] for r in golden)
    got = rc.Caller(pkg.ffi.LIB_PATH).records()
    different = [(g, r) for g, r in zip(golden, got) if g != r]
    assert not different, "%d of %d refusals changed, the first: %s" % (len(different), len(golden), different[0])
