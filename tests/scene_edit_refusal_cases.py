"""The refusals and fallbacks of mi355pt_scene_edit and of its host-only twin mi355pt_scene_debug_apply_edits as one case list, shared by
tools/record_scene_edit_refusals.py (which writes tests/golden/scene_edit_refusals.json from a library) and the tests that replay it on the
tree's (tests/test_scene_edit.py part 1, tests/test_scene_edit_gpu.py part 2), in the manner of tests/scene_update_refusal_cases.py.

A case is one FAULT put into an edit that is valid otherwise, on scene 21 of the package (a spot and a directional light, an area light,
seven Lambert materials) or, for the environment faults, scene 19.  Part 1 needs no GPU: the scene is not built, so the public call ends
every valid edit with MI355PT_E_NOT_BUILT — a fault must win over that — and the twin applies it; "later_table" pins the scene first and
adds a texture after the pin.  Part 2 runs on built scenes: what only a built scene can refuse, and every reason an edit falls back for."""
import ctypes as C

import numpy as np

import scene_edit_cases as sec

F = np.float32
# the golden file's own note on what it holds and what it cannot
WHAT = ("mi355pt_scene_edit / mi355pt_scene_debug_apply_edits: (code, last_error) per case of tests/scene_edit_refusal_cases.py.  MI355PT_MOVE_UNSUPPORTED_BUILD and the wrong-device refusal are in neither part: the first needs a build with quantised 4-wide nodes, the second a second GPU, and neither can be produced on one GPU with the default build (the three other update calls' golden file has the same gap); the reason is checked through edit_fallback_reason in tests/scene_edit_plan_check.cpp.")


def _valid(pkg, sc, scene_id):
    """a valid edit of every kind the scene has"""
    f = pkg.ffi
    if scene_id == "19":
        return {"envs": {0: (2.0, sec.rot_y(30.0), None)}}
    wall = sec._first(sc, f.MAT_LAMBERT, skip=2)
    d = sec.copy_of(sc.material_descs[wall]); d.color = f.Spectrum.constant(0.4)
    a, b = sec.copy_of(sc.light_descs[0]), sec.copy_of(sc.light_descs[1])
    a.intensity = 3.0; b.intensity = 0.75
    return {"materials": {wall: d, wall + 1: sec.copy_of(sc.material_descs[wall + 1])}, "lights": {0: a, 1: b}}


def _material(fn):
    def fault(pkg, sc, e):
        k = sorted(e["materials"])[1]
        fn(pkg.ffi, e["materials"][k])
    return fault


def _light(fn):
    def fault(pkg, sc, e):
        fn(pkg.ffi, e["lights"][1])
    return fault


def _matrix(d, m):
    sec.set_matrix(d, m)


def _rekey(kind, fn):
    def fault(pkg, sc, e):
        e[kind] = fn(sc, e[kind])
    return fault


def _hidden_material(sc, mats):
    hidden = [i for i, d in enumerate(sc.material_descs) if d is None][0]
    return {hidden: next(iter(mats.values()))}


def _singular():
    m = np.eye(4, dtype=F); m[:3, 0] = 0.0
    return m


def _nan_matrix():
    m = np.eye(4, dtype=F); m[1, 3] = np.nan
    return m


# name -> (scene, fault(pkg, sc, edits) editing the dictionaries in place, or a string handled by the caller)
FAULTS = {
    "null.scene": ("21", "null_scene"), "null.cam": ("21", "null_cam"), "null.edits": ("21", "null_edits"), "null.all_counts_zero": ("21", "all_zero"),
    "null.list_with_count": ("21", "null_list"),
    "ids.material_out_of_range": ("21", _rekey("materials", lambda sc, m: {999: next(iter(m.values()))})),
    "ids.material_of_a_light": ("21", _rekey("materials", _hidden_material)),
    "ids.material_descending": ("21", "materials_descending"), "ids.material_equal": ("21", "materials_equal"),
    "ids.light_out_of_range": ("21", _rekey("lights", lambda sc, m: {2: m[0]})), "ids.light_descending": ("21", "lights_descending"),
    "ids.env_out_of_range": ("21", lambda pkg, sc, e: e.update(envs={0: (1.0, None, None)})),
    "desc.material_type": ("21", _material(lambda f, d: setattr(d, "type", 77))),
    "desc.normal_texture": ("21", _material(lambda f, d: setattr(d, "normal_tex", 99))),
    "desc.lut": ("21", _material(lambda f, d: (setattr(d, "type", f.MAT_GLASS), setattr(d, "eta", f.Spectrum.lut(99))))),
    "desc.texture_on_glass": ("21", _material(lambda f, d: (setattr(d, "type", f.MAT_GLASS), setattr(d, "eta", f.Spectrum.constant(1.5)),
                                                              setattr(d, "color", f.Spectrum.texture_albedo_srgb(0))))),
    "desc.light_kind": ("21", _light(lambda f, d: setattr(d, "kind", 0))),
    "desc.light_spectrum": ("21", _light(lambda f, d: setattr(d, "spectrum", f.Spectrum.texture_albedo_srgb(0)))),
    "later_table.texture": ("21", "later_texture"), "later_table.lut": ("21", "later_lut"),
    "finite.material_roughness": ("21", _material(lambda f, d: setattr(d, "roughness", float("nan")))),
    "finite.material_colour": ("21", _material(lambda f, d: setattr(d, "color", f.Spectrum.constant(float("inf"))))),
    "finite.light_intensity": ("21", _light(lambda f, d: setattr(d, "intensity", float("inf")))),
    "finite.light_matrix": ("21", _light(lambda f, d: _matrix(d, _nan_matrix()))),
    "singular.light_matrix": ("21", _light(lambda f, d: _matrix(d, _singular()))),
    "finite.env_intensity": ("19", lambda pkg, sc, e: e.update(envs={0: (float("nan"), None, None)})),
    "singular.env_matrix": ("19", lambda pkg, sc, e: e.update(envs={0: (1.0, _singular(), None)})),
    "finite.env_map": ("19", "nan_map"),
    "valid.scene_21": ("21", None), "valid.scene_19": ("19", None),
}


class Caller:
    """calls both entry points of the library behind `prod` with the valid edit of a scene and one fault; part 1: the scenes as described"""

    def __init__(self, pkg, prod, build=None):
        self.pkg, self.prod, self.build = pkg, prod, build
        self.lib = prod.lib
        self.lib.mi355pt_last_error.restype = C.c_char_p

    def scene(self, scene_id):
        from test_scene_lowering import _describe
        sc, cam = _describe(self.pkg, sec.Edited(self.prod), scene_id)
        sc.set_bvh_builder("host")
        if self.build:
            self.build(sc, cam)
        return sc, cam

    def raw(self, entry, sc_ptr, cam_ref, edits_ref):
        fn = getattr(self.lib, entry)
        fn.restype, fn.argtypes = C.c_int, None
        rc = fn(C.c_void_p(sc_ptr), cam_ref, edits_ref, None) if entry == "mi355pt_scene_edit" else fn(C.c_void_p(sc_ptr), edits_ref)
        return int(rc), (self.lib.mi355pt_last_error() or b"").decode() if rc else ""

    def call(self, entry, name, sc=None, cam=None):
        """-> (return code, mi355pt_last_error text, or "" after MI355PT_OK)"""
        f = self.pkg.ffi
        scene_id, fault = FAULTS[name]
        if sc is None:
            sc, cam = self.scene(scene_id)
        if name.startswith("later_table") and not self.build:
            sc.debug_pin_host_tree(cam)
        edits = _valid(self.pkg, sc, scene_id)
        if callable(fault):
            fault(self.pkg, sc, edits)
        if fault == "later_texture":
            t = sc.add_tex_rgb8(np.full((2, 2, 3), 128, np.uint8))
            sorted(edits["materials"].items())[1][1].normal_tex = t
        if fault == "later_lut":
            lut = sc.add_lut470(np.ones(470, F))
            edits["lights"][1].spectrum = f.Spectrum.lut(lut)
        if fault == "nan_map":
            rgb = sc.env_lights[0][1].copy(); rgb[1, 2, 0] = np.nan
            edits["envs"] = {0: (1.0, None, rgb)}
        se, keep = sc._scene_edits(**edits)
        if fault == "materials_descending":
            se.materials[0], se.materials[1] = sec.copy_of(se.materials[1]), sec.copy_of(se.materials[0])
        if fault == "materials_equal":
            se.materials[1] = sec.copy_of(se.materials[0])
        if fault == "lights_descending":
            se.lights[0], se.lights[1] = sec.copy_of(se.lights[1]), sec.copy_of(se.lights[0])
        if fault == "all_zero":
            se.n_materials = se.n_lights = se.n_envs = 0
        if fault == "null_list":
            se.lights = None
        return self.raw(entry, None if fault == "null_scene" else sc.h.value, None if fault == "null_cam" else C.byref(cam),
                        None if fault == "null_edits" else C.byref(se))

    def records(self, part=1):
        out = []
        for name in FAULTS:
            for entry in ("mi355pt_scene_edit", "mi355pt_scene_debug_apply_edits"):
                if entry.endswith("apply_edits") and name == "null.cam":
                    continue
                code, text = self.call(entry, name)
                out.append({"part": part, "entry": entry, "case": name, "code": code, "error": text})
        return out
