"""The refusals of mi355pt_scene_move_camera, mi355pt_scene_move_instances, mi355pt_scene_deform_meshes and the three description
setters beside them, precedence between the checks included: every faulty call of tests/scene_update_refusal_cases.py is replayed on the
tree's library and must give the return code and the mi355pt_last_error text that tests/golden/scene_update_refusals.json holds for it —
recorded (tools/record_scene_update_refusals.py) from the library as it was before the three updates shared one device step.  Part 1 needs
no GPU; part 2 runs on the built scene and holds the device arrays to their digest after every refused call."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scene_update_refusal_cases as rc  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scene_update_refusals.json")
# the single faults that must be in the list, by its names: fault -> the entry points it applies to.  Part 1: each null argument, n = 0, ids out of
# range / descending / equal, null positions, a tangent without uv, NaN and infinite positions, a negative and a NaN rebuild_above; part 2, on the built
# scene: a wrong camera position, bad ids, a singular and a non-finite transform, a tangent without uv, non-finite positions, a negative rebuild_above, a
# scene built with mi355pt_scene_build_multi
SINGLE_FAULTS_1 = {"null.s": rc.UPDATES + rc.SETTERS, "null.cam": rc.UPDATES, "null.ids": rc.UPDATES[1:2], "null.l2w": rc.UPDATES[1:2], "null.updates": (rc.UPDATES[2], rc.SETTERS[1]),
                   "null.matrix": rc.SETTERS[2:], "null.n_zero": (rc.UPDATES[1], rc.UPDATES[2], rc.SETTERS[1]), "ids.out_of_range": rc.UPDATES[1:2],
                   "id.out_of_range": (rc.SETTERS[0], rc.SETTERS[2]), "ids.descending": rc.UPDATES[1:2], "ids.equal": rc.UPDATES[1:2], "arrays.bad_geom": (rc.UPDATES[2], rc.SETTERS[1]),
                   "arrays.descending": (rc.UPDATES[2], rc.SETTERS[1]), "arrays.equal": (rc.UPDATES[2], rc.SETTERS[1]), "arrays.null_pos": (rc.UPDATES[2], rc.SETTERS[1]),
                   "arrays.tangent_without_uv": (rc.UPDATES[2], rc.SETTERS[1]), "arrays.nan_pos": (rc.UPDATES[2], rc.SETTERS[1]), "arrays.inf_pos": (rc.UPDATES[2], rc.SETTERS[1]),
                   "rebuild_above.negative": rc.UPDATES[1:], "rebuild_above.nan": rc.UPDATES[1:]}
SINGLE_FAULTS_2 = {"cam.wrong_position": rc.UPDATES[1:], "ids.out_of_range": rc.UPDATES[1:2], "ids.descending": rc.UPDATES[1:2], "arrays.bad_geom": rc.UPDATES[2:],
                   "xform.singular": rc.UPDATES[1:2], "xform.nonfinite": rc.UPDATES[1:2], "arrays.tangent_without_uv": rc.UPDATES[2:], "arrays.nan_pos": rc.UPDATES[2:],
                   "arrays.inf_pos": rc.UPDATES[2:], "rebuild_above.negative": rc.UPDATES[1:], "multi.scene": rc.UPDATES}


def golden(part):
    return [r for r in json.load(open(GOLDEN)) if r["part"] == part]


def test_case_list_covers_every_fault_and_every_pair():
    """Both parts: unique names; every single fault of SINGLE_FAULTS_1 / _2, per entry point; every pair of faults from two different groups of an
    entry point; in part 1 the unbuilt scene alone for each of the three updates and named in every other case of theirs"""
    for part, singles in ((1, SINGLE_FAULTS_1), (2, SINGLE_FAULTS_2)):
        cases = rc.cases(part)
        assert len({(e, n) for e, n, _ in cases}) == len(cases)
        names = {e: {n for x, n, _ in cases if x == e} for e in rc.UPDATES + rc.SETTERS}
        tail = {e: "+built.unbuilt" if part == 1 and e in rc.UPDATES else "" for e in names}
        for fault, entries in singles.items():
            for e in entries:
                assert fault + tail[e] in names[e], (part, e, fault)
        for e in rc.UPDATES if part == 2 else rc.UPDATES + rc.SETTERS:
            faults = [n for n, _ in rc._faults(e, part)]
            assert len(faults) >= 1 and all(n + tail[e] in names[e] for n in faults)
            for i, n0 in enumerate(faults):
                for n1 in faults[i + 1:]:
                    if n0.split(".")[0] != n1.split(".")[0]:
                        assert n0 + "+" + n1 + tail[e] in names[e], (part, e, n0, n1)
            if tail[e]:
                assert "built.unbuilt" in names[e] and all(n == "built.unbuilt" or n.endswith(tail[e]) for n in names[e])
    # two of the orders the fixture pins: the deformation checks its arrays before it asks whether the scene is built, the instance move asks first
    by_name = {(r["entry"], r["case"]): r["error"] for r in golden(1)}
    assert by_name[(rc.UPDATES[2], "arrays.bad_geom+built.unbuilt")] == "bad geom id"
    assert by_name[(rc.UPDATES[1], "ids.out_of_range+built.unbuilt")] == "scene not built"


def replay(caller, after_each=None):
    want = golden(caller.part)
    assert [(r["entry"], r["case"]) for r in want] == [(e, n) for e, n, _ in rc.cases(caller.part)], "the case list changed: record the fixture again"
    assert all(r["code"] != 0 and r["error"] for r in want)                      # no case reaches a launch
    got = caller.records(after_each)
    different = [(g, r) for g, r in zip(want, got) if g != r]
    assert not different, "%d of %d refusals changed, the first: %s" % (len(different), len(want), different[0])


def test_refusals_match_the_recorded_ones(pkg):
    replay(rc.Caller(pkg, part=1))


@pytest.mark.gpu
def test_refusals_on_a_built_scene_match_and_leave_the_device_bytes(pkg):
    caller = rc.Caller(pkg, part=2)
    before = {id(sc): sc.debug_device_digest() for sc in (caller.scene, caller.multi)}
    assert before[id(caller.scene)] == caller.scene.debug_pinned_digest(caller.cam)
    checked = []

    def unchanged(entry, name, sc):
        assert sc.debug_device_digest() == before[id(sc)], (entry, name)
        checked.append(name)
    replay(caller, unchanged)
    assert len(checked) == len(golden(2)) and any("multi.scene" in n for n in checked)
