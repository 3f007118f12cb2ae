"""The edits tests/test_scene_edit.py (host form, no GPU) and tests/test_scene_edit_gpu.py (device) hold mi355pt_scene_edit to, as one case
list, and the two ways to the edited description: the edit dictionaries SceneHandle.edit / debug_apply_edits take, and Edited, a backend
whose new scenes are DESCRIBED with the edited records from the start (through the package's own scene descriptions)."""
import ctypes as C

import numpy as np

F = np.float32


def copy_of(desc):
    return type(desc).from_buffer_copy(desc)


def rot_x(deg):
    a = np.radians(deg)
    c, s = np.cos(a), np.sin(a)
    return np.array([[1, 0, 0, 0], [0, c, -s, 0], [0, s, c, 0], [0, 0, 0, 1]], F)


def rot_y(deg):
    a = np.radians(deg)
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0, s, 0], [0, 1, 0, 0], [-s, 0, c, 0], [0, 0, 0, 1]], F)


def translate(x, y, z):
    m = np.eye(4, dtype=F)
    m[:3, 3] = (x, y, z)
    return m


def set_matrix(desc, m):
    desc.local_to_world = (C.c_float * 16)(*np.ascontiguousarray(np.asarray(m, F).T.reshape(-1)))
    return desc


def matrix_of(desc):
    return np.array(desc.local_to_world[:], F).reshape(4, 4).T.copy()


def env_map(w, h, seed):
    """a small lat-long map with a bright patch: every row and column differs"""
    rng = np.random.default_rng(seed)
    m = rng.uniform(0.05, 1.0, (h, w, 3)).astype(F)
    m[h // 3, w // 2] = (6.0, 5.0, 3.0)
    return m


class Edited:
    """a backend whose new scenes take other descriptions for some material, delta-light and environment-light ids while they are
    described: materials {mat: MaterialDesc}, lights {light: LightDesc}, envs {env: (intensity, local_to_world or None, rgb or None)} —
    the dictionaries of SceneHandle.edit.  env_maps {env: rgb} replaces a map's SIZE too (a variant of the scene, not an edit)"""

    def __init__(self, backend, materials=None, lights=None, envs=None, env_maps=None):
        self._backend = backend
        self._materials, self._lights, self._envs, self._env_maps = materials or {}, lights or {}, envs or {}, env_maps or {}

    def __getattr__(self, name):
        return getattr(self._backend, name)

    def new_scene(self):
        sc = self._backend.new_scene()
        add_material, add_delta, add_env = sc.add_material, sc.add_delta_light, sc.add_environment_light
        count = {"mat": 0, "light": 0, "env": 0}

        def material_replacing(desc):
            return add_material(self._materials.get(self._next_material(sc), desc))

        def delta(kind, intensity, spectrum, local_to_world=None, angle_inner=0.0, angle_outer=0.0):
            k = count["light"]; count["light"] += 1
            sc._hidden += 1
            if k in self._lights:
                d = self._lights[k]
                return add_delta(d.kind, d.intensity, d.spectrum, matrix_of(d), d.angle_inner, d.angle_outer)
            return add_delta(kind, intensity, spectrum, local_to_world, angle_inner, angle_outer)

        def env(intensity, rgb, illuminant_lut, local_to_world=None):
            k = count["env"]; count["env"] += 1
            sc._hidden += 1
            rgb = self._env_maps.get(k, rgb)
            if k in self._envs:
                i2, m2, rgb2 = self._envs[k]
                return add_env(i2, rgb if rgb2 is None else rgb2, illuminant_lut, local_to_world if m2 is None else m2)
            return add_env(intensity, rgb, illuminant_lut, local_to_world)

        sc._hidden = 0
        sc.add_material, sc.add_delta_light, sc.add_environment_light = material_replacing, delta, env
        return sc

    @staticmethod
    def _next_material(sc):
        """the id the next add_material returns: every material and every light added so far took one"""
        return sum(d is not None for d in sc.material_descs) + sc._hidden


# ---- the cases: name -> (scene case of tests/test_scene_lowering.py, variant maps or None, edits(sc) -> dict for SceneHandle.edit) ----

def _first(sc, mat_type, skip=0):
    ids = [i for i, d in enumerate(sc.material_descs) if d is not None and d.type == mat_type]
    return ids[skip]


def point_to_spot(pkg, sc):
    """scene 2's point light: moved, brighter, and a spot light looking down"""
    d = copy_of(sc.light_descs[0])
    d.kind = pkg.ffi.LIGHT_SPOT; d.intensity = 25.0; d.angle_inner = 0.35; d.angle_outer = 0.7
    set_matrix(d, translate(0.5, 2.5, -0.3) @ rot_x(90.0))
    return {"lights": {0: d}}


def point_moved(pkg, sc):
    d = copy_of(sc.light_descs[0])
    d.intensity = 4.0
    set_matrix(d, translate(-0.8, 2.0, 0.6))
    return {"lights": {0: d}}


def several_lights(pkg, sc):
    """scene 21's spot light becomes a point light elsewhere, its directional light turns and brightens"""
    a, b = copy_of(sc.light_descs[0]), copy_of(sc.light_descs[1])
    a.kind = pkg.ffi.LIGHT_POINT; a.intensity = 12.0
    set_matrix(a, translate(-0.7, 2.8, 0.4))
    b.intensity = 1.25
    set_matrix(b, rot_y(35.0) @ rot_x(60.0))
    return {"lights": {0: a, 1: b}}


def env_turn(pkg, sc):
    """scene 19's sky: twice as bright, turned by 90 degrees of yaw"""
    return {"envs": {0: (2.0, rot_y(90.0), None)}}


def env_new_map(pkg, sc):
    """the 7 x 5 variant of scene 19: another 7 x 5 map, dimmer"""
    return {"envs": {0: (0.5, None, env_map(7, 5, seed=9))}}


def emitter_look(pkg, sc):
    """scene 3's emitter: four times the intensity, a warm constant radiance instead of D65"""
    em = _first(sc, pkg.ffi.MAT_EMISSIVE)
    d = copy_of(sc.material_descs[em])
    d.intensity = 4.0 * d.intensity
    d.color = pkg.ffi.Spectrum.rgb_albedo_srgb_linear(1.0, 0.8, 0.55)
    return {"materials": {em: d}}


def emitter_gain(gain):
    def edit(pkg, sc):
        em = _first(sc, pkg.ffi.MAT_EMISSIVE)
        d = copy_of(sc.material_descs[em])
        d.intensity = gain * d.intensity
        return {"materials": {em: d}}
    return edit


def wall_to_glass(pkg, sc):
    """scene 3's left wall (its first constant-colour Lambert material after the box's) becomes glass: another class, another feature set"""
    f = pkg.ffi
    wall = _first(sc, f.MAT_LAMBERT, skip=2)
    d = f.MaterialDesc(); d.type = f.MAT_GLASS; d.eta = f.Spectrum.constant(1.5); d.color = f.Spectrum.constant(1.0)
    d.normal_tex = f.NONE; d.thin = 0; d.roughness = 0.0
    return {"materials": {wall: d}}


def look_and_glass(pkg, sc):
    return {"materials": {**emitter_look(pkg, sc)["materials"], **wall_to_glass(pkg, sc)["materials"]}}


def coat_roughness(pkg, sc):
    """scene 17's hero: a rougher coat, which changes its coat-albedo row"""
    cc = _first(sc, pkg.ffi.MAT_CLEARCOAT)
    d = copy_of(sc.material_descs[cc])
    d.clearcoat_roughness = 0.35
    return {"materials": {cc: d}}


CASES = {
    "2:point_moved": ("2", None, point_moved), "2:point_to_spot": ("2", None, point_to_spot), "21:several_lights": ("21", None, several_lights),
    "19:env_turn": ("19", None, env_turn), "19:env_new_map": ("19", {0: env_map(7, 5, seed=4)}, env_new_map),
    "3:emitter_look": ("3", None, emitter_look), "3:wall_to_glass": ("3", None, wall_to_glass), "3:look_and_glass": ("3", None, look_and_glass),
    "17:coat_roughness": ("17", None, coat_roughness),
}
# the arrays an edit of each case reaches, name by name (everything else keeps its digest); "scalars" holds the feature bits
DIFFER = {
    "2:point_moved": {"lights"}, "2:point_to_spot": {"lights"}, "21:several_lights": {"lights"},
    "19:env_turn": {"lights", "envs"}, "19:env_new_map": {"lights", "envs", "materials", "env0.texels", "env0.marginal", "env0.conditional"},
    "3:emitter_look": {"materials"}, "3:wall_to_glass": {"materials", "tris_render", "tris_local", "scalars"},
    "3:look_and_glass": {"materials", "tris_render", "tris_local", "scalars"}, "17:coat_roughness": {"materials", "cc_albedo"},
}
LAUNCHES = {name: 1 if "glass" in name else 0 for name in CASES}


def original_edits(sc, edits):
    """the edit that puts back what `edits` replaces, from what the scene was described with"""
    back = {}
    if edits.get("materials"):
        back["materials"] = {m: copy_of(sc.material_descs[m]) for m in edits["materials"]}
    if edits.get("lights"):
        back["lights"] = {k: copy_of(sc.light_descs[k]) for k in edits["lights"]}
    if edits.get("envs"):
        back["envs"] = {k: (sc.env_lights[k][0], sc.env_lights[k][2], sc.env_lights[k][1]) for k in edits["envs"]}
    return back


def described(pkg, prod, name, edited=False, builder=None):
    """(scene, camera, edits) of a case, described and not built; edited: described with the edited records from the start"""
    from test_scene_lowering import _describe
    case, maps, make = CASES[name]
    sc, cam = _describe(pkg, Edited(prod, env_maps=maps), case)
    edits = make(pkg, sc)
    if edited:
        sc, cam = _describe(pkg, Edited(prod, env_maps=maps, **edits), case)
    if builder:
        sc.set_bvh_builder(builder)
    return sc, cam, edits
