"""The refusals of the three in-place updates of a built scene — mi355pt_scene_move_camera, mi355pt_scene_move_instances,
mi355pt_scene_deform_meshes — and of the three description setters beside them (mi355pt_scene_set_instance_dynamic,
mi355pt_scene_debug_set_mesh_vertices, mi355pt_scene_debug_set_instance_transform) as one case list, shared by
tools/record_scene_update_refusals.py (which writes tests/golden/scene_update_refusals.json from a library) and
tests/test_scene_update_refusals.py (which replays it on the tree's).

A case is an entry point and one or two FAULTS put into a call that is valid otherwise: scene "1" of the package (three meshes, the second
without uv; four instances), its camera, a real move of instances 0 and 1, a real deformation of meshes 0 and 1.  The faults fall into the
groups the entry points check in — null, ids / arrays, xform, cam, rebuild_above, multi, built — and a case's name says which it combines:
"ids.descending+rebuild_above.nan".  Every fault is a case, and every pair of faults from two different groups, so the fixture pins which
check wins: the three entry points run the same checks in three different orders.

Part 1 needs no GPU: the scene is NOT built, so for the three updates "built.unbuilt" is part of every case (and named in it); the case
"built.unbuilt" alone is the valid call on the unbuilt scene.  Part 2 runs on the scene built with the host builder, and "multi.scene" on a
second one built with mi355pt_scene_build_multi over devices [0, 0]; after every refused call the device arrays have the digest they had.
No case reaches a launch: every one is refused by a check."""
import ctypes as C
import itertools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_deform import Remeshed, deformed  # noqa: E402
from test_instance_move import applied, trs  # noqa: E402
from test_scene_lowering import _describe  # noqa: E402

F = np.float32
UPDATES = ("mi355pt_scene_move_camera", "mi355pt_scene_move_instances", "mi355pt_scene_deform_meshes")
SETTERS = ("mi355pt_scene_set_instance_dynamic", "mi355pt_scene_debug_set_mesh_vertices", "mi355pt_scene_debug_set_instance_transform")


def _set(**kw):
    return lambda a: a.update(kw)


def _ids(v):
    return lambda a: a.update(ids=v) if a["ids"] is not None else None       # (paired with a null array there is nothing to edit)


def _matrix(k, fn):
    def edit(a):
        if a["l2w"] is not None:                     # (paired with a null array there is nothing to edit)
            m = [x.copy() for x in a["l2w"]]
            fn(m[k])
            a["l2w"] = m
    return edit


def _updates(fn):
    def edit(a):
        if a["updates"] is not None:
            a["updates"] = fn([dict(u) for u in a["updates"]])
    return edit


def _update(k, **kw):
    return _updates(lambda ups: (ups[k].update(kw), ups)[1])


def _pos(k, value):
    def fn(ups):
        ups[k]["pos"] = ups[k]["pos"].copy()
        ups[k]["pos"][2, 1] = value
        return ups
    return _updates(fn)


def _singular(m):
    m[:3, 0] = 0.0


def _nonfinite(m):
    m[1, 3] = np.inf


# group -> [(name, edit)].  An edit works on the argument set of valid_args(); a fault on an array of the second update or matrix leaves
# the first one valid, so that the check has to walk to it
_ARRAYS = [("bad_geom", _update(1, geom=99)), ("descending", _updates(lambda ups: ups[::-1])),
           ("equal", _updates(lambda ups: [ups[0], ups[0]])), ("null_pos", _update(1, pos=None)),
           ("tangent_without_uv", _update(1, tangent=np.zeros((2, 3), F))), ("nan_pos", _pos(1, np.nan)), ("inf_pos", _pos(0, np.inf))]
_REBUILD = [("negative", _set(rebuild_above=-1.0)), ("nan", _set(rebuild_above=float("nan")))]
FAULTS = {
    "mi355pt_scene_move_camera": {"null": [("s", _set(s=None)), ("cam", _set(cam=None))], "multi": [("scene", _set(s="multi"))], "built": [("unbuilt", None)]},
    "mi355pt_scene_move_instances": {
        "null": [("s", _set(s=None)), ("cam", _set(cam=None)), ("ids", _set(ids=None)), ("l2w", _set(l2w=None)), ("n_zero", _set(n=0))],
        "multi": [("scene", _set(s="multi"))], "built": [("unbuilt", None)],
        "ids": [("out_of_range", _ids([0, 99])), ("descending", _ids([1, 0])), ("equal", _ids([1, 1]))],
        "cam": [("wrong_position", _set(cam="off"))], "xform": [("singular", _matrix(1, _singular)), ("nonfinite", _matrix(0, _nonfinite))],
        "rebuild_above": _REBUILD},
    "mi355pt_scene_deform_meshes": {
        "null": [("s", _set(s=None)), ("cam", _set(cam=None)), ("updates", _set(updates=None)), ("n_zero", _set(n=0))],
        "arrays": _ARRAYS, "rebuild_above": _REBUILD, "multi": [("scene", _set(s="multi"))], "built": [("unbuilt", None)],
        "cam": [("wrong_position", _set(cam="off"))]},
    "mi355pt_scene_set_instance_dynamic": {"null": [("s", _set(s=None))], "id": [("out_of_range", _set(instance=99))]},
    "mi355pt_scene_debug_set_mesh_vertices": {"null": [("s", _set(s=None)), ("updates", _set(updates=None)), ("n_zero", _set(n=0))], "arrays": _ARRAYS},
    "mi355pt_scene_debug_set_instance_transform": {"null": [("s", _set(s=None)), ("matrix", _set(l2w=None))], "id": [("out_of_range", _set(instance=99))]},
}
# part 1: what an unbuilt scene and no device can show; part 2: what takes a built scene, or is worth holding the device bytes against
PART_GROUPS = {1: ("null", "ids", "arrays", "id", "xform", "rebuild_above"), 2: ("ids", "arrays", "xform", "cam", "rebuild_above", "multi")}


def _faults(entry, part):
    return [("%s.%s" % (g, n), e) for g, fs in FAULTS[entry].items() if g in PART_GROUPS[part] for n, e in fs]


def cases(part):
    """[(entry point, case name, [edit, ...])] in a fixed order"""
    out = []
    for entry in (UPDATES + SETTERS if part == 1 else UPDATES):
        unbuilt = "+built.unbuilt" if part == 1 and entry in UPDATES else ""
        faults = _faults(entry, part)
        if unbuilt:
            out.append((entry, "built.unbuilt", []))
        out += [(entry, n + unbuilt, [e]) for n, e in faults]
        out += [(entry, n0 + "+" + n1 + unbuilt, [e0, e1]) for (n0, e0), (n1, e1) in itertools.combinations(faults, 2) if n0.split(".")[0] != n1.split(".")[0]]
    return out


class Caller:
    """calls the entry points of the library at `lib_path` (default: the tree's) with edited copies of the valid argument set"""

    def __init__(self, pkg, lib_path=None, part=1):
        self.pkg, self.part = pkg, part
        self.prod = Remeshed(pkg.Product(lib_path or pkg.ffi.LIB_PATH))
        self.lib = self.prod.lib
        self.lib.mi355pt_last_error.restype = C.c_char_p
        self.scene, self.cam = self._described()
        self.multi, self._valid = None, None
        if part == 2:
            self.scene.build(self.cam)
            self.multi, _ = self._described()
            self.prod.build_multi(self.multi, self.cam, [0, 0])
        p = np.array(self.cam.position[:], F) + np.asarray((0.3, -0.2, 0.45), F)
        self.cam_off = pkg.make_camera(tuple(float(v) for v in p), tuple(self.cam.direction[:]), tuple(self.cam.up[:]), self.cam.width, self.cam.height, self.cam.fov_deg)

    def _described(self):
        sc, cam = _describe(self.pkg, self.prod, "1")
        sc.set_bvh_builder("host")
        assert len(sc.meshes) >= 2 and len(sc.instances) >= 2 and sc.meshes[1].get("uv") is None and sc.meshes[0].get("uv") is not None
        return sc, cam

    def valid_args(self):
        """the valid argument set (the edits copy what they change)"""
        if not self._valid:
            sc = self.scene
            ups = [dict(zip(("pos", "nrm", "tangent"), deformed(sc.meshes[g])), geom=g) for g in (0, 1)]
            self._valid = {"s": "single", "cam": "at", "ids": [0, 1], "l2w": [applied(trs(), sc.instances[i][2]) for i in (0, 1)], "n": None,
                           "rebuild_above": None, "updates": ups, "instance": 0}
        return dict(self._valid)

    def call(self, entry, edits):
        """-> (return code, mi355pt_last_error text)"""
        a = self.valid_args()
        for edit in edits:
            if edit:
                edit(a)
        keep = []

        def floats(x):
            if x is None:
                return None
            keep.append(np.ascontiguousarray(x, dtype=F))
            return keep[-1].ctypes.data_as(C.POINTER(C.c_float))
        ffi = self.pkg.ffi
        s = {None: None, "single": self.scene.h.value, "multi": self.multi and self.multi.h.value}[a["s"]]
        assert a["s"] is None or s, "no such scene in this part"
        cam = {None: None, "at": C.byref(self.cam), "off": C.byref(self.cam_off)}[a["cam"]]
        prm = C.byref(ffi.InstanceMoveParams(a["rebuild_above"])) if a["rebuild_above"] is not None else None
        ups = None
        if a["updates"] is not None:
            ups = (ffi.MeshUpdate * len(a["updates"]))()
            for k, u in enumerate(a["updates"]):
                ups[k] = ffi.MeshUpdate(u["geom"], floats(u["pos"]), floats(u["nrm"]), floats(u["tangent"]))
        n_ups = a["n"] if a["n"] is not None else len(a["updates"] or [0, 0])
        cols = None if a["l2w"] is None else floats(np.stack(a["l2w"]).transpose(0, 2, 1).reshape(-1))      # column-major
        ids = None if a["ids"] is None else (C.c_uint32 * len(a["ids"]))(*a["ids"])
        n_ids = a["n"] if a["n"] is not None else len(a["ids"] or [0, 0])
        u32, ptr = C.c_uint32, C.c_void_p
        args = {"mi355pt_scene_move_camera": [ptr(s), cam, None],
                "mi355pt_scene_move_instances": [ptr(s), cam, ids, cols, u32(n_ids), prm, None],
                "mi355pt_scene_deform_meshes": [ptr(s), cam, ups, u32(n_ups), prm, None],
                "mi355pt_scene_set_instance_dynamic": [ptr(s), u32(a["instance"]), u32(1)],
                "mi355pt_scene_debug_set_mesh_vertices": [ptr(s), ups, u32(n_ups)],
                "mi355pt_scene_debug_set_instance_transform": [ptr(s), u32(a["instance"]), None if a["l2w"] is None else floats(a["l2w"][0].T.reshape(-1))]}[entry]
        fn = getattr(self.lib, entry)
        fn.restype, fn.argtypes = C.c_int, None
        rc = fn(*args)
        return int(rc), (self.lib.mi355pt_last_error() or b"").decode()

    def records(self, after_each=None):
        """after_each(entry, case name, scene handle that was called): part 2's check of the device bytes"""
        out = []
        for entry, name, edits in cases(self.part):
            code, text = self.call(entry, edits)
            out.append({"part": self.part, "entry": entry, "case": name, "code": code, "error": text})
            if after_each:
                after_each(entry, name, self.multi if "multi.scene" in name else self.scene)
        return out
