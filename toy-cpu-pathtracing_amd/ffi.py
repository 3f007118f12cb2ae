"""ctypes view of include/mi355pt.h and a thin object wrapper over the C ABI.

This is plumbing for tests / bench / smoke: the product is libmi355pt.so (hand-written HIP for
gfx950 behind the C ABI).  There is no CPU fallback: if the shared library is missing this module
raises, and every compute entry point fails loudly when no gfx950 device is present.

`Backend` is prefix-agnostic so that the *oracle's* C entry points (oracle/libptoracle.so, prefix
`ptoracle_`, test infrastructure only) can be driven with the very same scene description — the
oracle binding itself lives in oracle/ptoracle.py, not here.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB_PATH = os.environ.get("MI355PT_LIB") or os.path.join(HERE, "csrc", "libmi355pt.so")   # env override: A/B builds while tuning

NONE = 0xFFFFFFFF
SPEC_CONSTANT, SPEC_RGB_ALBEDO_SRGB, SPEC_LUT470, SPEC_TEXTURE_ALBEDO_SRGB, SPEC_SIGMOID, SPEC_RGB_ALBEDO_SRGB_LINEAR = 0, 1, 2, 3, 4, 5
SPEC_TEXTURE_ILLUMINANT_SRGB, SPEC_TEXTURE_UNBOUNDED_SRGB = 6, 7
MAT_LAMBERT, MAT_EMISSIVE, MAT_GLASS, MAT_PLASTIC, MAT_CLEARCOAT, MAT_METAL, MAT_SIMPLE_PBR = 0, 1, 2, 3, 4, 5, 6
STRATEGY = {"pt": 0, "nee": 1, "mis": 2}
SAMPLER = {"random": 0, "sobol": 1}
AOV_NORMAL, AOV_ALBEDO, AOV_SHADING_NORMAL = 0, 1, 2      # MI355PT_AOV_*: the reference's NormalRenderer / AlbedoRenderer and the extension
AOV = {"normal": AOV_NORMAL, "albedo": AOV_ALBEDO, "shading_normal": AOV_SHADING_NORMAL}


class Spectrum(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("id", C.c_uint32), ("c", C.c_float * 3)]

    @staticmethod
    def constant(v):
        return Spectrum(SPEC_CONSTANT, 0, (C.c_float * 3)(v, 0, 0))

    @staticmethod
    def rgb_albedo_srgb(r, g, b):
        return Spectrum(SPEC_RGB_ALBEDO_SRGB, 0, (C.c_float * 3)(r, g, b))

    @staticmethod
    def rgb_albedo_srgb_linear(r, g, b):
        return Spectrum(SPEC_RGB_ALBEDO_SRGB_LINEAR, 0, (C.c_float * 3)(r, g, b))

    @staticmethod
    def lut(i):
        return Spectrum(SPEC_LUT470, i, (C.c_float * 3)(0, 0, 0))

    @staticmethod
    def texture_albedo_srgb(i):
        return Spectrum(SPEC_TEXTURE_ALBEDO_SRGB, i, (C.c_float * 3)(0, 0, 0))

    @staticmethod
    def texture_illuminant_srgb(i, illuminant_lut):
        """SpectrumParameter::texture(.., SpectrumType::Illuminant): c[0] carries the LUT470 id of presets::cie_illum_d6500()"""
        return Spectrum(SPEC_TEXTURE_ILLUMINANT_SRGB, i, (C.c_float * 3)(float(illuminant_lut), 0, 0))

    @staticmethod
    def texture_unbounded_srgb(i):
        return Spectrum(SPEC_TEXTURE_UNBOUNDED_SRGB, i, (C.c_float * 3)(0, 0, 0))


class MaterialDesc(C.Structure):
    _fields_ = [("type", C.c_uint32), ("color", Spectrum), ("normal_tex", C.c_uint32), ("normal_flip_y", C.c_uint32),
                ("intensity", C.c_float), ("eta", Spectrum), ("thin", C.c_uint32), ("roughness", C.c_float),
                ("metallic", C.c_float), ("ior", C.c_float), ("clearcoat_ior", C.c_float), ("clearcoat_roughness", C.c_float),
                ("clearcoat_thickness", C.c_float), ("clearcoat_tint", Spectrum), ("k", Spectrum),
                ("metallic_tex", C.c_uint32), ("roughness_tex", C.c_uint32), ("clearcoat_thickness_tex", C.c_uint32),
                ("intensity_tex", C.c_uint32)]

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.metallic_tex = NONE; self.roughness_tex = NONE; self.clearcoat_thickness_tex = NONE; self.intensity_tex = NONE


LIGHT_POINT, LIGHT_SPOT, LIGHT_DIRECTIONAL = 1, 2, 3


class LightDesc(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("intensity", C.c_float), ("angle_inner", C.c_float), ("angle_outer", C.c_float),
                ("spectrum", Spectrum), ("local_to_world", C.c_float * 16)]


class Camera(C.Structure):
    _fields_ = [("position", C.c_float * 3), ("direction", C.c_float * 3), ("up", C.c_float * 3),
                ("fov_deg", C.c_float), ("width", C.c_uint32), ("height", C.c_uint32)]


class Params(C.Structure):
    _fields_ = [("spp", C.c_uint32), ("seed", C.c_uint32), ("max_depth", C.c_uint32), ("strategy", C.c_uint32),
                ("sampler", C.c_uint32), ("exposure", C.c_float), ("shard_index", C.c_uint32),
                ("shard_count", C.c_uint32), ("collect_stats", C.c_uint32), ("rr_gate_slack", C.c_float), ("albedo_lut", C.c_uint32)]


class Stats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("samples", "closest_rays", "shadow_rays", "nodes_closest", "tris_closest",
                                          "nodes_shadow", "tris_shadow", "closest_hits", "bounces", "spectrum_evals",
                                          "textured_lookups")] + [("phase_cycles", C.c_uint64 * 10), ("kernel_ms", C.c_double), ("launches", C.c_uint32),
                                                ("wave_steps", C.c_uint64 * 8), ("busy_hist", C.c_uint64 * 16), ("divergence", C.c_uint64 * 12)]

    def as_dict(self):
        d = {n: getattr(self, n) for n, _ in self._fields_}
        d["phase_cycles"] = list(self.phase_cycles)
        d["wave_steps"] = list(self.wave_steps)
        d["busy_hist"] = [list(self.busy_hist)[:8], list(self.busy_hist)[8:]]
        d["divergence"] = list(self.divergence)
        return d


class DenoiseParams(C.Structure):
    """mi355pt_denoise_params (include/mi355pt_denoise.h); Product.denoise_params_default() fills it — a zeroed one is refused"""
    _fields_ = [("levels", C.c_uint32), ("sigma_color", C.c_float), ("sigma_normal", C.c_float), ("sigma_albedo", C.c_float),
                ("albedo_eps", C.c_float)]


class DenoiseVarParams(C.Structure):
    """mi355pt_denoise_var_params (include/mi355pt_denoise_var.h); Product.denoise_var_params_default() fills it — a zeroed one is refused"""
    _fields_ = [("levels", C.c_uint32), ("sigma_lum", C.c_float), ("sigma_normal", C.c_float), ("sigma_albedo", C.c_float),
                ("albedo_eps", C.c_float), ("lum_eps", C.c_float)]


class AdaptiveParams(C.Structure):
    """mi355pt_adaptive_params (include/mi355pt_adaptive.h): threshold has no default, and a zeroed struct is refused"""
    _fields_ = [("threshold", C.c_float), ("dark_eps", C.c_float), ("min_spp", C.c_uint32)]


class AdaptiveResult(C.Structure):
    """mi355pt_adaptive_result"""
    _fields_ = [("passes", C.c_uint32), ("tiles_at_max", C.c_uint32), ("total_samples", C.c_uint64)]


class GbufferFilms(C.Structure):
    """mi355pt_gbuffer_films (include/mi355pt_gbuffer.h): device or host pointers, NULL = not wanted"""
    _fields_ = [("albedo", C.c_void_p), ("shading_normal", C.c_void_p), ("position", C.c_void_p), ("hit", C.c_void_p)]


GBUFFER_FILMS = ("albedo", "shading_normal", "position", "hit")


class TemporalView(C.Structure):
    """mi355pt_temporal_view (include/mi355pt_temporal.h): how a render-space point of the current frame lands in the previous frame's image"""
    _fields_ = [("delta", C.c_float * 3), ("rows", C.c_float * 9), ("sx", C.c_float), ("sy", C.c_float), ("cx", C.c_float), ("cy", C.c_float)]


class TemporalParams(C.Structure):
    """mi355pt_temporal_params; Product.temporal_params_default() fills it — a zeroed one is refused"""
    _fields_ = [("pos_tol", C.c_float), ("normal_cos", C.c_float), ("min_weight", C.c_float), ("max_history", C.c_float)]


class TemporalFrame(C.Structure):
    """mi355pt_temporal_frame: device or host pointers; half may be NULL, length is read of the previous frame only"""
    _fields_ = [("film", C.c_void_p), ("half", C.c_void_p), ("length", C.c_void_p), ("position", C.c_void_p), ("shading_normal", C.c_void_p),
                ("hit", C.c_void_p)]


TEMPORAL_FILMS = ("film", "half", "length", "position", "shading_normal", "hit")


class TemporalRectifyParams(C.Structure):
    """mi355pt_temporal_rectify_params (include/mi355pt_temporal_rectify.h); Product.temporal_rectify_params_default() fills it — a zeroed
    one is refused"""
    _fields_ = [("radius", C.c_uint32), ("gamma", C.c_float)]


class MotionXform(C.Structure):
    """mi355pt_motion_xform (include/mi355pt_motion.h): X_prev = a X_cur + b, nrm_prev = n nrm_cur between two frames' render spaces; 96 bytes"""
    _fields_ = [("a", C.c_float * 9), ("b", C.c_float * 3), ("n", C.c_float * 9), ("pad", C.c_float * 3)]


class BudgetParams(C.Structure):
    """mi355pt_budget_params (include/mi355pt_budget.h): a zeroed struct is refused"""
    _fields_ = [("base_spp", C.c_uint32), ("max_spp", C.c_uint32), ("target_history", C.c_float)]


class BudgetMotion(C.Structure):
    """mi355pt_budget_motion: device or host pointers; all zero = the static world"""
    _fields_ = [("ids_cur", C.c_void_p), ("ids_prev", C.c_void_p), ("table", C.c_void_p), ("n_entries", C.c_uint32), ("flow", C.c_void_p)]


class UpsampleParams(C.Structure):
    """mi355pt_upsample_params (include/mi355pt_upsample.h); Product.upsample_params_default() fills it — a zeroed one is refused"""
    _fields_ = [("pos_tol", C.c_float), ("normal_cos", C.c_float), ("emitter_tol", C.c_float), ("min_weight", C.c_float), ("albedo_eps", C.c_float)]


class UpsampleGuides(C.Structure):
    """mi355pt_upsample_guides: the raw G-buffer sums of one resolution, device or host pointers; albedo may be NULL (then on both sides)"""
    _fields_ = [("albedo", C.c_void_p), ("shading_normal", C.c_void_p), ("position", C.c_void_p), ("hit", C.c_void_p)]


UPSAMPLE_GUIDES = ("albedo", "shading_normal", "position", "hit")


class DisplayParams(C.Structure):
    """mi355pt_display_params (include/mi355pt_display.h); Product.display_params_default() fills it — a zeroed one is refused"""
    _fields_ = [("tone", C.c_uint32), ("encode", C.c_uint32), ("exposure", C.c_float), ("white", C.c_float), ("log2_lum_min", C.c_int32),
                ("trim_low", C.c_uint32), ("trim_high", C.c_uint32), ("key", C.c_float), ("e_min", C.c_float), ("e_max", C.c_float), ("adapt", C.c_float)]


TONE = {"none": 0, "reinhard": 1, "reinhard-ext": 2, "aces": 3, "hable": 4}      # MI355PT_TONE_*
ENCODE = {"linear": 0, "srgb": 1}                                                # MI355PT_ENCODE_*
DISPLAY_RECORD_WORDS, DISPLAY_HIST_WORDS = 8, 258


class BloomParams(C.Structure):
    """mi355pt_bloom_params (include/mi355pt_bloom.h); Product.bloom_params_default() fills it — a zeroed one is refused"""
    _fields_ = [("levels", C.c_uint32), ("firefly", C.c_uint32), ("threshold", C.c_float), ("knee", C.c_float), ("scatter", C.c_float), ("base", C.c_float),
                ("intensity", C.c_float), ("exposure", C.c_float)]


BLOOM_MAX_LEVELS = 8


class RobustParams(C.Structure):
    """mi355pt_robust_params (include/mi355pt_robust.h); Product.robust_params_default() gives GMON with scale 1, a zeroed one is MEAN"""
    _fields_ = [("mode", C.c_uint32), ("gini_scale", C.c_float)]


ROBUST_MODE = {"mean": 0, "mom": 1, "gmon": 2}                                   # MI355PT_ROBUST_*


class MoveResult(C.Structure):
    """mi355pt_move_result (include/mi355pt_rebase.h)"""
    _fields_ = [("rebuilt", C.c_uint32), ("reason", C.c_uint32), ("launches", C.c_uint32), ("host_ms", C.c_double), ("device_ms", C.c_double)]

    def as_dict(self):
        return {"rebuilt": int(self.rebuilt), "reason": MOVE_REASON[self.reason], "launches": int(self.launches), "host_ms": float(self.host_ms),
                "device_ms": float(self.device_ms)}


MOVE_REASON = ["rebased", "same_position", "degenerate_set_changed", "instance_class_changed", "unsupported_build"]   # MI355PT_MOVE_*


# mi355pt_instance_move_result.reason: MOVE_REASON plus the two of include/mi355pt_instances.h
INSTANCE_MOVE_REASON = MOVE_REASON + ["same_transforms", "sah_degraded"]
# ... plus the one of include/mi355pt_deform.h (mi355pt_scene_deform_meshes reports through the same result struct)
DEFORM_REASON = INSTANCE_MOVE_REASON + ["same_vertices"]


class InstanceMoveParams(C.Structure):
    """mi355pt_instance_move_params (include/mi355pt_instances.h)"""
    _fields_ = [("rebuild_above", C.c_float)]


class InstanceMoveResult(C.Structure):
    """mi355pt_instance_move_result (include/mi355pt_instances.h)"""
    _fields_ = [("rebuilt", C.c_uint32), ("reason", C.c_uint32), ("launches", C.c_uint32), ("sah_built", C.c_float), ("sah_after", C.c_float),
                ("host_ms", C.c_double), ("device_ms", C.c_double)]

    def as_dict(self):
        return {"rebuilt": int(self.rebuilt), "reason": DEFORM_REASON[self.reason], "launches": int(self.launches),
                "sah_built": np.float32(self.sah_built), "sah_after": np.float32(self.sah_after), "host_ms": float(self.host_ms),
                "device_ms": float(self.device_ms)}


class MeshUpdate(C.Structure):
    """mi355pt_mesh_update (include/mi355pt_deform.h)"""
    _fields_ = [("geom", C.c_uint32), ("pos", C.POINTER(C.c_float)), ("nrm", C.POINTER(C.c_float)), ("tri_tangent", C.POINTER(C.c_float))]


# mi355pt_edit_result.reason (include/mi355pt_edit.h): "rebased" (edited in place) and "unsupported_build" of MOVE_REASON, and three of its own
EDIT_REASON = DEFORM_REASON + ["same_records", "emitter_set_changed", "table_shape_changed"]


class MaterialEdit(C.Structure):
    """mi355pt_material_edit (include/mi355pt_edit.h)"""
    _fields_ = [("mat", C.c_uint32), ("desc", MaterialDesc)]


class LightEdit(C.Structure):
    """mi355pt_light_edit (include/mi355pt_edit.h)"""
    _fields_ = [("light", C.c_uint32), ("desc", LightDesc)]


class EnvEdit(C.Structure):
    """mi355pt_env_edit (include/mi355pt_edit.h)"""
    _fields_ = [("env", C.c_uint32), ("intensity", C.c_float), ("local_to_world", C.POINTER(C.c_float)), ("rgb", C.POINTER(C.c_float))]


class SceneEdits(C.Structure):
    """mi355pt_scene_edits (include/mi355pt_edit.h)"""
    _fields_ = [("materials", C.POINTER(MaterialEdit)), ("n_materials", C.c_uint32), ("lights", C.POINTER(LightEdit)), ("n_lights", C.c_uint32),
                ("envs", C.POINTER(EnvEdit)), ("n_envs", C.c_uint32)]


class EditResult(C.Structure):
    """mi355pt_edit_result (include/mi355pt_edit.h)"""
    _fields_ = [("rebuilt", C.c_uint32), ("reason", C.c_uint32), ("launches", C.c_uint32), ("features_before", C.c_uint32), ("features_after", C.c_uint32),
                ("host_ms", C.c_double), ("device_ms", C.c_double)]

    def as_dict(self):
        return {"rebuilt": int(self.rebuilt), "reason": EDIT_REASON[self.reason], "launches": int(self.launches), "features_before": int(self.features_before),
                "features_after": int(self.features_after), "host_ms": float(self.host_ms), "device_ms": float(self.device_ms)}


def make_light_desc(kind, intensity, spectrum, local_to_world=None, angle_inner=0.0, angle_outer=0.0):
    """mi355pt_light_desc from a row-major 4 x 4 matrix, as SceneHandle.add_delta_light takes its arguments"""
    m = np.eye(4, dtype=np.float32) if local_to_world is None else np.asarray(local_to_world, dtype=np.float32)
    d = LightDesc(); d.kind = kind; d.intensity = intensity; d.angle_inner = angle_inner; d.angle_outer = angle_outer
    d.spectrum = spectrum
    d.local_to_world = (C.c_float * 16)(*np.ascontiguousarray(m.T.reshape(-1)))   # column-major
    return d


def make_camera(position, direction, up, width, height, fov_deg=45.0):
    return Camera((C.c_float * 3)(*position), (C.c_float * 3)(*direction), (C.c_float * 3)(*up), fov_deg, width, height)


def make_params(spp, strategy="mis", sampler="sobol", seed=0, max_depth=16, exposure=1.0, shard_index=0, shard_count=1,
                collect_stats=0, rr_gate_slack=0.0, albedo_lut=0):
    return Params(spp, seed, max_depth, STRATEGY[strategy], SAMPLER[sampler], exposure, shard_index, shard_count, collect_stats, rr_gate_slack,
                  albedo_lut)


def _ptr(a, ty):
    return a.ctypes.data_as(C.POINTER(ty)) if a is not None else None


# every symbol include/mi355pt.h declares (tests/test_abi.py checks the built library exports all of them) ...
DEBUG_SYMBOLS = ["debug_unlock", "scene_debug_set_lowering", "scene_debug_lowering_digest", "scene_debug_camera_candidates", "scene_debug_move_digest", "scene_debug_move_export", "scene_debug_device_digest", "scene_debug_pinned_digest", "scene_debug_pinned_export", "scene_debug_pin_host_tree", "scene_debug_set_instance_transform", "scene_debug_set_mesh_vertices", "scene_debug_apply_edits", "debug_sah_cost", "scene_export_bvh", "probe_bvh_collapse", "probe_bvh_collapse_nodes", "probe_sobol", "probe_sincos", "probe_intersect", "probe_occluded",
                 "sample_log_records", "render_sample_log", "probe_radiance", "probe_display_meter_ms",
                 "render_flow_debug", "scene_export_flow_mark", "scene_export_triangle_ids"]     # ... and include/mi355pt_debug.h
ABI_SYMBOLS = [
    "scene_create", "scene_destroy", "scene_set_rgb2spec", "scene_add_lut470", "scene_add_tex_rgb8", "scene_add_mesh",
    "scene_add_material", "scene_add_instance", "scene_add_delta_light", "scene_add_environment_light", "scene_set_bvh_builder", "scene_build", "render", "render_accum_device", "film_resolve_device",
    "render_accum_tiles_device",
    "render_aov", "render_aov_accum_device", "aov_resolve_device",
    "quantize_u8", "scene_info", "scene_build_multi", "render_multi", "coat_albedo_table",
    "last_error", "version",
]
# ... include/mi355pt_denoise.h, the denoiser block mi355pt.h includes (tests/test_denoise.py checks these the same way)
DENOISE_SYMBOLS = ["denoise_params_default", "denoise_scratch_bytes", "denoise_device", "denoise"]
# ... include/mi355pt_denoise_var.h, the variance-guided denoiser block mi355pt.h includes (tests/test_denoise_var.py)
DENOISE_VAR_SYMBOLS = ["denoise_var_params_default", "denoise_var_scratch_bytes", "denoise_var_device", "denoise_var"]
# ... and include/mi355pt_adaptive.h, the adaptive-sampling block mi355pt.h includes (tests/test_adaptive.py)
# ... and include/mi355pt_gbuffer.h, the G-buffer block mi355pt.h includes (tests/test_gbuffer.py)
GBUFFER_SYMBOLS = ["render_gbuffer_accum_device", "gbuffer_normalize_device", "render_gbuffer"]
# ... and include/mi355pt_temporal.h, the temporal-reprojection block mi355pt.h includes (tests/test_temporal.py)
TEMPORAL_SYMBOLS = ["temporal_params_default", "temporal_view_from_cameras", "temporal_accumulate_device", "temporal_accumulate"]
# ... and include/mi355pt_temporal_rectify.h, its rectified form (tests/test_temporal_rectify.py)
TEMPORAL_RECTIFY_SYMBOLS = ["temporal_rectify_params_default", "temporal_rectify_scratch_bytes", "temporal_accumulate_rectified_device",
                            "temporal_accumulate_rectified"]
# ... and include/mi355pt_upsample.h, the guided half-resolution block (tests/test_upsample.py)
UPSAMPLE_SYMBOLS = ["upsample_params_default", "upsample_low_camera", "upsample_device", "upsample"]
# ... and include/mi355pt_display.h, the display block (tests/test_display.py)
DISPLAY_SYMBOLS = ["display_params_default", "display_scratch_bytes", "display_meter_device", "display_device", "display_meter", "display"]
# ... and include/mi355pt_bloom.h, the bloom block (tests/test_bloom.py)
BLOOM_SYMBOLS = ["bloom_params_default", "bloom_scratch_bytes", "bloom_device", "bloom"]
# ... and include/mi355pt_robust.h, the robust-film block (tests/test_robust.py)
ROBUST_SYMBOLS = ["robust_params_default", "robust_combine_device", "robust_combine", "render_buckets_device", "render_robust"]
# ... and include/mi355pt_rebase.h, the camera-move block (tests/test_rebase.py)
REBASE_SYMBOLS = ["scene_move_camera"]
# ... and include/mi355pt_instances.h, the instance-move block (tests/test_instance_move.py)
INSTANCES_SYMBOLS = ["scene_set_instance_dynamic", "scene_move_instances"]
# ... and include/mi355pt_motion.h, the object-motion block (tests/test_motion.py)
MOTION_SYMBOLS = ["render_ids_device", "render_ids", "motion_table", "temporal_accumulate_motion_device", "temporal_accumulate_motion",
                  "temporal_accumulate_rectified_motion_device", "temporal_accumulate_rectified_motion"]
# ... and include/mi355pt_deform.h, the mesh-deformation block (tests/test_deform.py)
DEFORM_SYMBOLS = ["scene_deform_meshes"]
# ... and include/mi355pt_edit.h, the lights-and-materials block (tests/test_scene_edit.py)
EDIT_SYMBOLS = ["scene_edit"]
# ... and include/mi355pt_flow.h, the per-pixel motion block (tests/test_flow.py)
FLOW_SYMBOLS = ["scene_flow_mark", "scene_flow_marked", "render_flow_device", "render_flow", "temporal_accumulate_flow_device", "temporal_accumulate_flow",
                "temporal_accumulate_rectified_flow_device", "temporal_accumulate_rectified_flow"]
FLOW_DEBUG_SYMBOLS = ["render_flow_debug", "scene_export_flow_mark", "scene_export_triangle_ids"]      # include/mi355pt_debug.h
# mi355pt_flow_pixel as a NumPy record: 32 bytes
FLOW_PIXEL = np.dtype([("d", np.float32, 3), ("id", np.uint32), ("dn", np.float32, 3), ("pad", np.uint32)])
FLOW_HIT = np.dtype([("tri", np.uint32), ("b", np.float32, 3)])           # mi355pt_render_flow_debug's hit record: 16 bytes
# ... and include/mi355pt_budget.h, the sample-budget block (tests/test_budget.py)
BUDGET_SYMBOLS = ["temporal_budget_device", "temporal_budget", "render_budget_device", "film_pair_normalize_tiles_device", "film_pair_normalize_tiles",
                  "temporal_length_credit_device"]
ADAPTIVE_SYMBOLS = ["adaptive_scratch_bytes", "adaptive_step_device", "film_normalize_tiles_device", "render_adaptive_device", "render_adaptive"]


class Backend:
    """Prefix-agnostic binding of the scene-construction / probe subset shared by product and oracle."""

    def __init__(self, lib, prefix):
        self.lib, self.prefix = lib, prefix
        f = self.fn
        f("scene_create").argtypes = [C.POINTER(C.c_void_p)]
        f("scene_destroy").argtypes = [C.c_void_p]; f("scene_destroy").restype = None
        f("scene_set_rgb2spec").argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_size_t]
        f("scene_add_lut470").argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint32)]
        f("scene_add_tex_rgb8").argtypes = [C.c_void_p, C.POINTER(C.c_uint8), C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]
        f("scene_add_mesh").argtypes = [C.c_void_p] + [C.POINTER(C.c_float)] * 4 + [C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]
        f("scene_add_material").argtypes = [C.c_void_p, C.POINTER(MaterialDesc), C.POINTER(C.c_uint32)]
        f("scene_add_instance").argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_float)]
        f("scene_add_delta_light").argtypes = [C.c_void_p, C.POINTER(LightDesc)]
        f("scene_add_environment_light").argtypes = [C.c_void_p, C.c_float, C.POINTER(C.c_float), C.c_uint32, C.c_uint32, C.POINTER(C.c_float),
                                                     C.c_uint32]
        f("scene_build").argtypes = [C.c_void_p, C.POINTER(Camera)]
        f("probe_sobol").argtypes = [C.c_uint32] * 4 + [C.POINTER(C.c_uint32), C.c_uint32, C.c_char_p, C.POINTER(C.c_uint32)]
        f("probe_intersect").argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_uint32, C.POINTER(C.c_float),
                                         C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_float)]
        if prefix == "mi355pt_":                                              # (product only: the oracle IS the host libm)
            f("probe_sincos").argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]
        f("probe_occluded").argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_uint32,
                                        C.POINTER(C.c_uint8)]
        f("probe_radiance").argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(Params), C.POINTER(C.c_uint32), C.c_uint32,
                                        C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]
        f("quantize_u8").argtypes = [C.POINTER(C.c_float), C.c_size_t, C.POINTER(C.c_uint8)]

    def fn(self, name):
        return getattr(self.lib, self.prefix + name)

    def check(self, rc, what):
        if rc != 0:
            msg = ""
            if self.prefix == "mi355pt_":
                self.lib.mi355pt_last_error.restype = C.c_char_p
                msg = (self.lib.mi355pt_last_error() or b"").decode()
            raise RuntimeError(f"{self.prefix}{what} failed with code {rc}: {msg}")

    def new_scene(self):
        return SceneHandle(self)

    def probe_sincos(self, first_bits, stride, n):
        """(compared, sin mismatches, cos mismatches) of the device's sin / cos against this host's libm (include/mi355pt_debug.h)"""
        out = (C.c_uint64 * 3)()
        self.check(self.fn("probe_sincos")(first_bits, stride, n, out), "probe_sincos")
        return int(out[0]), int(out[1]), int(out[2])

    def probe_sobol(self, width, height, spp, seed, xys, pattern):
        xys = np.ascontiguousarray(xys, dtype=np.uint32).reshape(-1, 3)
        per = sum(2 if ch == "2" else 1 for ch in pattern)
        out = np.zeros((xys.shape[0], per), dtype=np.uint32)
        self.check(self.fn("probe_sobol")(width, height, spp, seed, _ptr(xys, C.c_uint32), xys.shape[0], pattern.encode(),
                                           _ptr(out, C.c_uint32)), "probe_sobol")
        return out

    def quantize_u8(self, rgb):
        rgb = np.ascontiguousarray(rgb, dtype=np.float32)
        out = np.zeros(rgb.shape, dtype=np.uint8)
        self.check(self.fn("quantize_u8")(_ptr(rgb, C.c_float), rgb.size, _ptr(out, C.c_uint8)), "quantize_u8")
        return out


class SceneHandle:
    """Owns one opaque scene; mirrors scene::Scene's construction API (scene/src/scene.rs:43-76)."""

    def __init__(self, backend):
        self.b = backend
        self.h = C.c_void_p()
        backend.check(backend.fn("scene_create")(C.byref(self.h)), "scene_create")
        self.keep = []
        self.material_descs = []       # by material id (delta / environment lights add hidden materials on the library side, after these)
        self.instances = []            # by instance id: (geometry, material, local_to_world as a row-major 4 x 4 float32 array) as described
        self.light_descs = []          # by delta-light id (the order of add_delta_light calls): the LightDesc as described
        self.env_lights = []           # by environment-light id: (intensity, rgb (h, w, 3) float32, local_to_world row-major 4 x 4) as described

    def close(self):
        if self.h:
            self.b.fn("scene_destroy")(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_rgb2spec(self, table):
        table = np.ascontiguousarray(table, dtype=np.float32)
        self.b.check(self.b.fn("scene_set_rgb2spec")(self.h, _ptr(table, C.c_float), table.size), "scene_set_rgb2spec")

    def add_lut470(self, values):
        v = np.ascontiguousarray(values, dtype=np.float32)
        assert v.size == 470
        out = C.c_uint32()
        self.b.check(self.b.fn("scene_add_lut470")(self.h, _ptr(v, C.c_float), C.byref(out)), "scene_add_lut470")
        return out.value

    def add_tex_rgb8(self, img):
        img = np.ascontiguousarray(img, dtype=np.uint8)
        h, w, c = img.shape
        assert c == 3
        out = C.c_uint32()
        self.b.check(self.b.fn("scene_add_tex_rgb8")(self.h, _ptr(img, C.c_uint8), w, h, C.byref(out)), "scene_add_tex_rgb8")
        return out.value

    def add_mesh(self, mesh):
        pos = np.ascontiguousarray(mesh["pos"], dtype=np.float32)
        nrm = np.ascontiguousarray(mesh["nrm"], dtype=np.float32)
        uv = None if mesh.get("uv") is None else np.ascontiguousarray(mesh["uv"], dtype=np.float32)
        tan = None if mesh.get("tangent") is None else np.ascontiguousarray(mesh["tangent"], dtype=np.float32)
        idx = np.ascontiguousarray(mesh["idx"], dtype=np.uint32).reshape(-1)
        out = C.c_uint32()
        self.b.check(self.b.fn("scene_add_mesh")(self.h, _ptr(pos, C.c_float), _ptr(nrm, C.c_float), _ptr(uv, C.c_float),
                                                  _ptr(tan, C.c_float), _ptr(idx, C.c_uint32), pos.shape[0], idx.size // 3,
                                                  C.byref(out)), "scene_add_mesh")
        return out.value

    def add_material(self, desc):
        out = C.c_uint32()
        self.b.check(self.b.fn("scene_add_material")(self.h, C.byref(desc), C.byref(out)), "scene_add_material")
        while len(self.material_descs) <= out.value:
            self.material_descs.append(None)
        self.material_descs[out.value] = desc
        return out.value

    def add_instance(self, geom, mat, local_to_world=None):
        m = np.eye(4, dtype=np.float32) if local_to_world is None else np.asarray(local_to_world, dtype=np.float32)
        cols = np.ascontiguousarray(m.T.reshape(-1))   # column-major
        self.b.check(self.b.fn("scene_add_instance")(self.h, geom, mat, _ptr(cols, C.c_float)), "scene_add_instance")
        self.instances.append((geom, mat, m.copy()))

    def add_delta_light(self, kind, intensity, spectrum, local_to_world=None, angle_inner=0.0, angle_outer=0.0):
        d = make_light_desc(kind, intensity, spectrum, local_to_world, angle_inner, angle_outer)
        self.b.check(self.b.fn("scene_add_delta_light")(self.h, C.byref(d)), "scene_add_delta_light")
        self.light_descs.append(d)

    def add_environment_light(self, intensity, rgb, illuminant_lut, local_to_world=None):
        rgb = np.ascontiguousarray(rgb, dtype=np.float32)
        assert rgb.ndim == 3 and rgb.shape[2] == 3
        m = np.eye(4, dtype=np.float32) if local_to_world is None else np.asarray(local_to_world, dtype=np.float32)
        cols = np.ascontiguousarray(m.T.reshape(-1))
        self.b.check(self.b.fn("scene_add_environment_light")(self.h, intensity, _ptr(rgb, C.c_float), rgb.shape[1], rgb.shape[0],
                                                              _ptr(cols, C.c_float), illuminant_lut), "scene_add_environment_light")
        self.env_lights.append((float(intensity), rgb.copy(), m.copy()))

    def set_bvh_builder(self, mode):
        """mi355pt_scene_set_bvh_builder: "auto" | "host" | "gpu" (product only; the oracle has its own BVH)."""
        fn = self.b.fn("scene_set_bvh_builder")
        fn.argtypes = [C.c_void_p, C.c_int]
        self.b.check(fn(self.h, {"auto": 0, "host": 1, "gpu": 2}[mode]), "scene_set_bvh_builder")

    def debug_set_lowering(self, mode):
        """mi355pt_scene_debug_set_lowering (include/mi355pt_debug.h): "auto" | "no_local_tris" | "general" (product only)."""
        fn = self.b.fn("scene_debug_set_lowering")
        fn.argtypes = [C.c_void_p, C.c_int]
        self.b.check(fn(self.h, {"auto": 0, "no_local_tris": 1, "general": 2}[mode]), "scene_debug_set_lowering")

    def debug_lowering_digest(self, cam):
        """mi355pt_scene_debug_lowering_digest (host only, product only) -> ({array name: FNV-1a-64 as 16 hex digits}, in upload order with
        "scalars" last, and scene_info's text without the *_ms fields)"""
        fn = self.b.fn("scene_debug_lowering_digest")
        fn.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_char_p, C.c_size_t, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
        text = C.create_string_buffer(4096); dig = (C.c_uint64 * 128)(); n = C.c_uint32(128)
        self.b.check(fn(self.h, C.byref(cam), text, 4096, dig, C.byref(n)), "scene_debug_lowering_digest")
        *names, info = text.value.decode().split("\n")
        assert len(names) == n.value
        return {nm: f"{dig[i]:016x}" for i, nm in enumerate(names)}, info

    def debug_camera_candidates(self, cam, rects, cap=16, want_tris=False):
        """mi355pt_scene_debug_camera_candidates (host only, product only): the candidate lists of csrc/camera_candidates.hpp for the pixel
        rectangles `rects` (n x 4: x0, y0, x1, y1, inclusive) -> counts (n,), overflow (n,) bool, indices (n, cap) uint32 (row r: counts[r]
        valid entries) and, on request, the lowered triangles in leaf order as (m, 3, 3) float32 render-space vertices"""
        fn = self.b.fn("scene_debug_camera_candidates")
        fn.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint8),
                       C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.POINTER(C.c_uint32)]
        r = np.ascontiguousarray(rects, dtype=np.uint32).reshape(-1, 4)
        n = r.shape[0]
        counts = np.zeros(n, np.uint32); over = np.zeros(n, np.uint8); idx = np.zeros((n, cap), np.uint32)
        nt = C.c_uint32(0)
        tris = None
        if want_tris:
            self.b.check(fn(self.h, C.byref(cam), None, 0, cap, None, None, None, None, C.byref(nt)), "scene_debug_camera_candidates")
            tris = np.zeros((nt.value, 3, 3), np.float32)
        self.b.check(fn(self.h, C.byref(cam), _ptr(r, C.c_uint32), n, cap, _ptr(counts, C.c_uint32), _ptr(over, C.c_uint8), _ptr(idx, C.c_uint32),
                        _ptr(tris, C.c_float), C.byref(nt)), "scene_debug_camera_candidates")
        return (counts, over.astype(bool), idx, tris) if want_tris else (counts, over.astype(bool), idx)

    def build(self, cam):
        self.b.check(self.b.fn("scene_build")(self.h, C.byref(cam)), "scene_build")

    def move_camera(self, cam):
        """mi355pt_scene_move_camera (include/mi355pt_rebase.h, product only): the built scene re-based to cam's position on the device ->
        {"rebuilt", "reason" (a MOVE_REASON name), "launches", "host_ms", "device_ms"}"""
        fn = self.b.fn("scene_move_camera")
        fn.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(MoveResult)]
        res = MoveResult()
        self.b.check(fn(self.h, C.byref(cam), C.byref(res)), "scene_move_camera")
        return res.as_dict()

    def set_instance_dynamic(self, instance, dynamic=True):
        """mi355pt_scene_set_instance_dynamic (include/mi355pt_instances.h, product only): before the build, mark an instance that will move"""
        fn = self.b.fn("scene_set_instance_dynamic")
        fn.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
        self.b.check(fn(self.h, instance, 1 if dynamic else 0), "scene_set_instance_dynamic")

    def move_instances(self, cam, ids, local_to_world, rebuild_above=0.0):
        """mi355pt_scene_move_instances (include/mi355pt_instances.h, product only): new local_to_world matrices (row-major 4 x 4 each, as
        add_instance takes them) for the instances `ids` (strictly ascending) of the built scene, applied on the device ->
        {"rebuilt", "reason" (an INSTANCE_MOVE_REASON name), "launches", "sah_built", "sah_after", "host_ms", "device_ms"}"""
        fn = self.b.fn("scene_move_instances")
        fn.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.c_uint32, C.POINTER(InstanceMoveParams),
                       C.POINTER(InstanceMoveResult)]
        idv = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
        m = np.asarray(local_to_world, dtype=np.float32).reshape(-1, 4, 4)
        assert m.shape[0] == idv.size
        cols = np.ascontiguousarray(m.transpose(0, 2, 1).reshape(-1))          # column-major
        prm = InstanceMoveParams(rebuild_above)
        res = InstanceMoveResult()
        self.b.check(fn(self.h, C.byref(cam), _ptr(idv, C.c_uint32), _ptr(cols, C.c_float), idv.size, C.byref(prm), C.byref(res)), "scene_move_instances")
        return res.as_dict()

    def _mesh_updates(self, meshes):
        """{geom: (pos, nrm or None, tangent or None)} -> (a ctypes array of MeshUpdate in ascending geom order, the arrays it points into)"""
        keep, ups = [], (MeshUpdate * len(meshes))()
        for k, geom in enumerate(sorted(meshes)):
            arrays = [None if a is None else np.ascontiguousarray(a, dtype=np.float32) for a in meshes[geom]]
            keep.append(arrays)
            ups[k] = MeshUpdate(geom, *[_ptr(a, C.c_float) for a in arrays])
        return ups, keep

    def deform_meshes(self, cam, meshes, rebuild_above=0.0):
        """mi355pt_scene_deform_meshes (include/mi355pt_deform.h, product only): new vertex arrays {geom: (pos (n_vert, 3), nrm (n_vert, 3) or
        None = keep, per-triangle tangent (n_tri, 3) or None = keep)} for meshes of the built scene, applied on the device -> move_instances'
        dictionary ("reason" a DEFORM_REASON name)"""
        fn = self.b.fn("scene_deform_meshes")
        fn.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(MeshUpdate), C.c_uint32, C.POINTER(InstanceMoveParams), C.POINTER(InstanceMoveResult)]
        ups, keep = self._mesh_updates(meshes)
        prm = InstanceMoveParams(rebuild_above)
        res = InstanceMoveResult()
        self.b.check(fn(self.h, C.byref(cam), ups, len(meshes), C.byref(prm), C.byref(res)), "scene_deform_meshes")
        return res.as_dict()

    def debug_set_mesh_vertices(self, meshes):
        """mi355pt_scene_debug_set_mesh_vertices (host only, product only): deform_meshes' description update alone, on an unbuilt scene"""
        fn = self.b.fn("scene_debug_set_mesh_vertices")
        fn.argtypes = [C.c_void_p, C.POINTER(MeshUpdate), C.c_uint32]
        ups, keep = self._mesh_updates(meshes)
        self.b.check(fn(self.h, ups, len(meshes)), "scene_debug_set_mesh_vertices")

    def _scene_edits(self, materials=None, lights=None, envs=None):
        """{mat: MaterialDesc}, {light: LightDesc}, {env: (intensity, local_to_world row-major 4 x 4 or None = keep, rgb (h, w, 3) or None =
        keep)} -> (a SceneEdits with each list in ascending id order, what it points into)"""
        materials, lights, envs = materials or {}, lights or {}, envs or {}
        me, le, ee, keep = (MaterialEdit * max(len(materials), 1))(), (LightEdit * max(len(lights), 1))(), (EnvEdit * max(len(envs), 1))(), []
        for k, mat in enumerate(sorted(materials)):
            me[k] = MaterialEdit(mat, materials[mat])
        for k, light in enumerate(sorted(lights)):
            le[k] = LightEdit(light, lights[light])
        for k, env in enumerate(sorted(envs)):
            intensity, l2w, rgb = envs[env]
            cols = None if l2w is None else np.ascontiguousarray(np.asarray(l2w, dtype=np.float32).T.reshape(-1))
            rgb = None if rgb is None else np.ascontiguousarray(rgb, dtype=np.float32)
            keep += [cols, rgb]
            ee[k] = EnvEdit(env, intensity, _ptr(cols, C.c_float), _ptr(rgb, C.c_float))
        keep += [me, le, ee]
        return SceneEdits(me if materials else None, len(materials), le if lights else None, len(lights), ee if envs else None, len(envs)), keep

    def edit(self, cam, materials=None, lights=None, envs=None):
        """mi355pt_scene_edit (include/mi355pt_edit.h, product only): new descriptions for materials, delta lights and environment lights
        of the built scene (_scene_edits' dictionaries), applied in place -> {"rebuilt", "reason" (an EDIT_REASON name), "launches",
        "features_before", "features_after", "host_ms", "device_ms"}"""
        fn = self.b.fn("scene_edit")
        fn.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(SceneEdits), C.POINTER(EditResult)]
        edits, keep = self._scene_edits(materials, lights, envs)
        res = EditResult()
        self.b.check(fn(self.h, C.byref(cam), C.byref(edits), C.byref(res)), "scene_edit")
        return res.as_dict()

    def debug_apply_edits(self, materials=None, lights=None, envs=None):
        """mi355pt_scene_debug_apply_edits (host only, product only): edit's description update alone, on an unbuilt scene"""
        fn = self.b.fn("scene_debug_apply_edits")
        fn.argtypes = [C.c_void_p, C.POINTER(SceneEdits)]
        edits, keep = self._scene_edits(materials, lights, envs)
        self.b.check(fn(self.h, C.byref(edits)), "scene_debug_apply_edits")

    def debug_pin_host_tree(self, cam):
        """mi355pt_scene_debug_pin_host_tree (host only, product only): what a build keeps on the host, for an unbuilt scene"""
        fn = self.b.fn("scene_debug_pin_host_tree")
        fn.argtypes = [C.c_void_p, C.POINTER(Camera)]
        self.b.check(fn(self.h, C.byref(cam)), "scene_debug_pin_host_tree")

    def debug_set_instance_transform(self, instance, local_to_world):
        """mi355pt_scene_debug_set_instance_transform (host only, product only): a new matrix (row-major 4 x 4) in the description of an unbuilt scene"""
        fn = self.b.fn("scene_debug_set_instance_transform")
        fn.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_float)]
        cols = np.ascontiguousarray(np.asarray(local_to_world, dtype=np.float32).T.reshape(-1))
        self.b.check(fn(self.h, instance, _ptr(cols, C.c_float)), "scene_debug_set_instance_transform")

    def debug_pinned_digest(self, cam):
        """mi355pt_scene_debug_pinned_digest (host only, product only): debug_lowering_digest's pair for the built scene's CURRENT description
        over the topology the built scene holds"""
        fn = self.b.fn("scene_debug_pinned_digest")
        fn.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_char_p, C.c_size_t, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
        return self._digests(lambda *a: fn(self.h, C.byref(cam), *a), "scene_debug_pinned_digest")

    def debug_pinned_export(self, cam):
        """mi355pt_scene_debug_pinned_export (host only, product only): the BVH2 of debug_pinned_digest's lowering as Product.export_bvh
        gives a built one — nodes (n, 16) uint32, triangle records (m, 12) uint32, root — and the refit plan's entries (uint32)"""
        fn = self.b.fn("scene_debug_pinned_export")
        fn.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_void_p, C.POINTER(C.c_uint32), C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_int32),
                       C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        nn, nt, ne, root = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.c_int32(0)
        self.b.check(fn(self.h, C.byref(cam), None, C.byref(nn), None, C.byref(nt), None, None, C.byref(ne)), "scene_debug_pinned_export")
        nodes = np.zeros((nn.value, 16), np.uint32); tris = np.zeros((nt.value, 12), np.uint32); entries = np.zeros(ne.value, np.uint32)
        self.b.check(fn(self.h, C.byref(cam), nodes.ctypes.data_as(C.c_void_p), C.byref(nn), tris.ctypes.data_as(C.c_void_p), C.byref(nt), C.byref(root),
                        _ptr(entries, C.c_uint32), C.byref(ne)), "scene_debug_pinned_export")
        return nodes, tris, int(root.value), entries

    def _digests(self, call, what):
        text = C.create_string_buffer(4096); dig = (C.c_uint64 * 128)(); n = C.c_uint32(128)
        self.b.check(call(text, 4096, dig, C.byref(n)), what)
        *names, info = text.value.decode().split("\n")
        assert len(names) == n.value
        return {nm: f"{dig[i]:016x}" for i, nm in enumerate(names)}, info

    def debug_move_digest(self, cam_built, cam_new):
        """mi355pt_scene_debug_move_digest (host only, product only): debug_lowering_digest's pair for the scene lowered for cam_new over the
        tree of cam_built, and the MOVE_REASON name a move from cam_built to cam_new would report"""
        fn = self.b.fn("scene_debug_move_digest")
        fn.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(Camera), C.c_char_p, C.c_size_t, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        reason = C.c_uint32(0)
        got, info = self._digests(lambda *a: fn(self.h, C.byref(cam_built), C.byref(cam_new), *a, C.byref(reason)), "scene_debug_move_digest")
        return got, info, MOVE_REASON[reason.value]

    def debug_move_export(self, cam_built, cam_new):
        """mi355pt_scene_debug_move_export (host only, product only): the tree of debug_move_digest's lowering as Product.export_bvh gives a
        built one — nodes (n, 16) uint32, triangle records (m, 12) uint32, root — and the pad's two radii (from the root record, by the
        lowering's own loop)"""
        fn = self.b.fn("scene_debug_move_export")
        fn.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(Camera), C.c_void_p, C.POINTER(C.c_uint32), C.c_void_p, C.POINTER(C.c_uint32),
                       C.POINTER(C.c_int32), C.POINTER(C.c_float)]
        nn, nt, root = C.c_uint32(0), C.c_uint32(0), C.c_int32(0)
        self.b.check(fn(self.h, C.byref(cam_built), C.byref(cam_new), None, C.byref(nn), None, C.byref(nt), None, None), "scene_debug_move_export")
        nodes = np.zeros((nn.value, 16), np.uint32); tris = np.zeros((nt.value, 12), np.uint32); radii = (C.c_float * 2)()
        self.b.check(fn(self.h, C.byref(cam_built), C.byref(cam_new), nodes.ctypes.data_as(C.c_void_p), C.byref(nn), tris.ctypes.data_as(C.c_void_p),
                        C.byref(nt), C.byref(root), radii), "scene_debug_move_export")
        return nodes, tris, int(root.value), (np.float32(radii[0]), np.float32(radii[1]))

    def debug_device_digest(self):
        """mi355pt_scene_debug_device_digest (product only): the same pair hashed from what the device holds"""
        fn = self.b.fn("scene_debug_device_digest")
        fn.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
        return self._digests(lambda *a: fn(self.h, *a), "scene_debug_device_digest")

    # ---- probes ----
    def probe_intersect(self, origins, dirs):
        o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        n = o.shape[0]
        t = np.zeros(n, np.float32); inst = np.zeros(n, np.uint32); tri = np.zeros(n, np.uint32); nrm = np.zeros((n, 3), np.float32)
        self.b.check(self.b.fn("probe_intersect")(self.h, _ptr(o, C.c_float), _ptr(d, C.c_float), n, _ptr(t, C.c_float),
                                                   _ptr(inst, C.c_uint32), _ptr(tri, C.c_uint32), _ptr(nrm, C.c_float)), "probe_intersect")
        return t, inst, tri, nrm

    def probe_occluded(self, origins, dirs, t_max):
        o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        tm = np.ascontiguousarray(t_max, dtype=np.float32).reshape(-1)
        out = np.zeros(o.shape[0], np.uint8)
        self.b.check(self.b.fn("probe_occluded")(self.h, _ptr(o, C.c_float), _ptr(d, C.c_float), _ptr(tm, C.c_float), o.shape[0],
                                                  _ptr(out, C.c_uint8)), "probe_occluded")
        return out

    def probe_radiance(self, cam, params, xys):
        xys = np.ascontiguousarray(xys, dtype=np.uint32).reshape(-1, 3)
        n = xys.shape[0]
        L = np.zeros((n, 4), np.float32); lam = np.zeros((n, 4), np.float32); pdf = np.zeros((n, 4), np.float32)
        self.b.check(self.b.fn("probe_radiance")(self.h, C.byref(cam), C.byref(params), _ptr(xys, C.c_uint32), n, _ptr(L, C.c_float),
                                                  _ptr(lam, C.c_float), _ptr(pdf, C.c_float)), "probe_radiance")
        return L, lam, pdf


class Product(Backend):
    """libmi355pt.so — the HIP product.  Raises if the extension has not been built."""

    def __init__(self, path=LIB_PATH):
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(hipcc --offload-arch=gfx950).  There is no CPU fallback for the product path.")
        lib = C.CDLL(path)
        super().__init__(lib, "mi355pt_")
        lib.mi355pt_version.restype = C.c_char_p
        lib.mi355pt_last_error.restype = C.c_char_p
        lib.mi355pt_render.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(Params), C.POINTER(C.c_float), C.POINTER(Stats)]
        lib.mi355pt_render_accum_device.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(Params), C.c_uint32, C.c_uint32,
                                                    C.c_void_p, C.c_void_p, C.POINTER(Stats)]
        lib.mi355pt_film_resolve_device.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        if hasattr(lib, "mi355pt_render_aov"):                 # (absent from an older build loaded through MI355PT_LIB)
            lib.mi355pt_render_aov.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(Params), C.c_int, C.c_uint32, C.POINTER(C.c_float),
                                               C.POINTER(Stats)]
            lib.mi355pt_render_aov_accum_device.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(Params), C.c_int, C.c_uint32, C.c_uint32,
                                                            C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(Stats)]
            lib.mi355pt_aov_resolve_device.argtypes = [C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        if hasattr(lib, "mi355pt_denoise_device"):             # (absent from an older build loaded through MI355PT_LIB)
            lib.mi355pt_denoise_params_default.argtypes = [C.POINTER(DenoiseParams)]; lib.mi355pt_denoise_params_default.restype = None
            lib.mi355pt_denoise_scratch_bytes.argtypes = [C.c_uint32, C.c_uint32]; lib.mi355pt_denoise_scratch_bytes.restype = C.c_size_t
            lib.mi355pt_denoise_device.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32,
                                                   C.POINTER(DenoiseParams), C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
            lib.mi355pt_denoise.argtypes = [C.POINTER(C.c_float), C.c_uint32, C.POINTER(C.c_float), C.c_uint32, C.POINTER(C.c_float), C.c_uint32,
                                            C.c_uint32, C.c_uint32, C.POINTER(DenoiseParams), C.POINTER(C.c_float)]
        if hasattr(lib, "mi355pt_denoise_var_device"):         # (absent from an older build loaded through MI355PT_LIB)
            lib.mi355pt_denoise_var_params_default.argtypes = [C.POINTER(DenoiseVarParams)]; lib.mi355pt_denoise_var_params_default.restype = None
            lib.mi355pt_denoise_var_scratch_bytes.argtypes = [C.c_uint32, C.c_uint32]; lib.mi355pt_denoise_var_scratch_bytes.restype = C.c_size_t
            lib.mi355pt_denoise_var_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32,
                                                       C.c_uint32, C.POINTER(DenoiseVarParams), C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
            lib.mi355pt_denoise_var.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.c_uint32,
                                                C.POINTER(C.c_float), C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(DenoiseVarParams), C.POINTER(C.c_float)]
        if hasattr(lib, "mi355pt_render_adaptive_device"):     # (absent from an older build loaded through MI355PT_LIB)
            lib.mi355pt_render_accum_tiles_device.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(Params), C.POINTER(C.c_uint32), C.c_uint32,
                                                              C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(Stats)]
            lib.mi355pt_adaptive_scratch_bytes.argtypes = [C.c_uint32, C.c_uint32]; lib.mi355pt_adaptive_scratch_bytes.restype = C.c_size_t
            lib.mi355pt_adaptive_step_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(AdaptiveParams),
                                                         C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
            lib.mi355pt_film_normalize_tiles_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
            lib.mi355pt_render_adaptive_device.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(Params), C.POINTER(AdaptiveParams)] + [C.c_void_p] * 6 + \
                [C.c_size_t, C.c_void_p, C.POINTER(AdaptiveResult)]
            lib.mi355pt_render_adaptive.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(Params), C.POINTER(AdaptiveParams), C.POINTER(C.c_float),
                                                    C.POINTER(C.c_uint32), C.POINTER(AdaptiveResult)]
        if hasattr(lib, "mi355pt_render_gbuffer"):             # (absent from an older build loaded through MI355PT_LIB)
            lib.mi355pt_render_gbuffer_accum_device.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(Params), C.c_uint32, C.c_uint32, C.c_uint32,
                                                                C.POINTER(GbufferFilms), C.c_void_p, C.POINTER(Stats)]
            lib.mi355pt_gbuffer_normalize_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
            lib.mi355pt_render_gbuffer.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(Params), C.c_uint32, C.POINTER(GbufferFilms), C.POINTER(Stats)]
        if hasattr(lib, "mi355pt_temporal_accumulate_device"):  # (absent from an older build loaded through MI355PT_LIB)
            lib.mi355pt_temporal_params_default.argtypes = [C.POINTER(TemporalParams)]; lib.mi355pt_temporal_params_default.restype = None
            lib.mi355pt_temporal_view_from_cameras.argtypes = [C.POINTER(Camera), C.POINTER(Camera), C.POINTER(TemporalView)]
            lib.mi355pt_temporal_accumulate_device.argtypes = [C.POINTER(TemporalFrame), C.c_uint32, C.POINTER(TemporalFrame), C.POINTER(TemporalView), C.c_uint32,
                                                               C.c_uint32, C.POINTER(TemporalParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
            lib.mi355pt_temporal_accumulate.argtypes = [C.POINTER(TemporalFrame), C.c_uint32, C.POINTER(TemporalFrame), C.POINTER(TemporalView), C.c_uint32,
                                                        C.c_uint32, C.POINTER(TemporalParams), C.c_void_p, C.c_void_p, C.c_void_p]
        if hasattr(lib, "mi355pt_temporal_accumulate_rectified_device"):  # (absent from an older build loaded through MI355PT_LIB)
            lib.mi355pt_temporal_rectify_params_default.argtypes = [C.POINTER(TemporalRectifyParams)]; lib.mi355pt_temporal_rectify_params_default.restype = None
            lib.mi355pt_temporal_rectify_scratch_bytes.argtypes = [C.c_uint32, C.c_uint32]; lib.mi355pt_temporal_rectify_scratch_bytes.restype = C.c_size_t
            lib.mi355pt_temporal_accumulate_rectified_device.argtypes = [C.POINTER(TemporalFrame), C.c_uint32, C.POINTER(TemporalFrame), C.POINTER(TemporalView),
                                                                         C.c_uint32, C.c_uint32, C.POINTER(TemporalParams), C.POINTER(TemporalRectifyParams),
                                                                         C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
            lib.mi355pt_temporal_accumulate_rectified.argtypes = [C.POINTER(TemporalFrame), C.c_uint32, C.POINTER(TemporalFrame), C.POINTER(TemporalView), C.c_uint32,
                                                                  C.c_uint32, C.POINTER(TemporalParams), C.POINTER(TemporalRectifyParams), C.c_void_p, C.c_void_p,
                                                                  C.c_void_p]
        if hasattr(lib, "mi355pt_upsample_device"):  # (absent from an older build loaded through MI355PT_LIB)
            lib.mi355pt_upsample_params_default.argtypes = [C.POINTER(UpsampleParams)]; lib.mi355pt_upsample_params_default.restype = None
            lib.mi355pt_upsample_low_camera.argtypes = [C.POINTER(Camera), C.POINTER(Camera)]
            lib.mi355pt_upsample_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(UpsampleGuides), C.c_uint32, C.POINTER(UpsampleGuides), C.c_uint32,
                                                    C.c_uint32, C.c_uint32, C.POINTER(UpsampleParams), C.c_void_p, C.c_void_p, C.c_void_p]
            lib.mi355pt_upsample.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(UpsampleGuides), C.c_uint32, C.POINTER(UpsampleGuides), C.c_uint32,
                                             C.c_uint32, C.c_uint32, C.POINTER(UpsampleParams), C.c_void_p, C.c_void_p]
        if hasattr(lib, "mi355pt_display_device"):  # (absent from an older build loaded through MI355PT_LIB)
            lib.mi355pt_display_params_default.argtypes = [C.POINTER(DisplayParams)]; lib.mi355pt_display_params_default.restype = None
            lib.mi355pt_display_scratch_bytes.argtypes = [C.c_uint32, C.c_uint32]; lib.mi355pt_display_scratch_bytes.restype = C.c_size_t
            lib.mi355pt_display_meter_device.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(DisplayParams), C.c_void_p, C.c_void_p, C.c_size_t,
                                                         C.c_void_p, C.c_void_p, C.c_void_p]
            lib.mi355pt_display_device.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(DisplayParams), C.c_void_p, C.c_void_p, C.c_void_p]
            lib.mi355pt_display_meter.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(DisplayParams), C.c_void_p, C.c_void_p, C.c_void_p]
            lib.mi355pt_display.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(DisplayParams), C.c_void_p, C.c_void_p]
        if hasattr(lib, "mi355pt_bloom_device"):  # (absent from an older build loaded through MI355PT_LIB)
            lib.mi355pt_bloom_params_default.argtypes = [C.POINTER(BloomParams)]; lib.mi355pt_bloom_params_default.restype = None
            lib.mi355pt_bloom_scratch_bytes.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]; lib.mi355pt_bloom_scratch_bytes.restype = C.c_size_t
            lib.mi355pt_bloom_device.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(BloomParams), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                                 C.c_void_p]
            lib.mi355pt_bloom.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(BloomParams), C.c_void_p, C.c_void_p]
        if hasattr(lib, "mi355pt_robust_combine_device"):  # (absent from an older build loaded through MI355PT_LIB)
            lib.mi355pt_robust_params_default.argtypes = [C.POINTER(RobustParams)]; lib.mi355pt_robust_params_default.restype = None
            lib.mi355pt_robust_combine_device.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(RobustParams), C.c_void_p, C.c_void_p,
                                                          C.c_void_p, C.c_void_p]
            lib.mi355pt_robust_combine.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(RobustParams), C.c_void_p, C.c_void_p, C.c_void_p]
            lib.mi355pt_render_buckets_device.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(Params), C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(Stats)]
            lib.mi355pt_render_robust.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(Params), C.c_uint32, C.POINTER(RobustParams), C.c_void_p]
        if hasattr(lib, "mi355pt_temporal_accumulate_motion_device"):  # (absent from an older build loaded through MI355PT_LIB)
            frame4 = [C.POINTER(TemporalFrame), C.c_uint32, C.POINTER(TemporalFrame), C.POINTER(TemporalView), C.c_uint32, C.c_uint32, C.POINTER(TemporalParams)]
            motion4 = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]                      # ids_cur, ids_prev, table, n_entries
            lib.mi355pt_render_ids_device.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(Params), C.c_void_p, C.c_void_p, C.POINTER(Stats)]
            lib.mi355pt_render_ids.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(Params), C.c_void_p, C.POINTER(Stats)]
            lib.mi355pt_motion_table.argtypes = [C.POINTER(Camera), C.POINTER(Camera), C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
            lib.mi355pt_temporal_accumulate_motion_device.argtypes = frame4 + motion4 + [C.c_void_p] * 4
            lib.mi355pt_temporal_accumulate_motion.argtypes = frame4 + motion4 + [C.c_void_p] * 3
            lib.mi355pt_temporal_accumulate_rectified_motion_device.argtypes = frame4 + [C.POINTER(TemporalRectifyParams), C.c_void_p, C.c_size_t] + motion4 + \
                [C.c_void_p] * 4
            lib.mi355pt_temporal_accumulate_rectified_motion.argtypes = frame4 + [C.POINTER(TemporalRectifyParams)] + motion4 + [C.c_void_p] * 3
        if hasattr(lib, "mi355pt_render_flow_device"):  # (absent from an older build loaded through MI355PT_LIB)
            frame4 = [C.POINTER(TemporalFrame), C.c_uint32, C.POINTER(TemporalFrame), C.POINTER(TemporalView), C.c_uint32, C.c_uint32, C.POINTER(TemporalParams)]
            flow3 = [C.c_void_p, C.c_void_p, C.c_void_p]                                    # ids_cur, ids_prev, flow
            lib.mi355pt_scene_flow_mark.argtypes = [C.c_void_p, C.c_void_p]
            lib.mi355pt_scene_flow_marked.argtypes = [C.c_void_p]
            lib.mi355pt_render_flow_device.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(Params), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Stats)]
            lib.mi355pt_render_flow.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(Params), C.c_void_p, C.c_void_p, C.POINTER(Stats)]
            lib.mi355pt_render_flow_debug.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(Params), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Stats)]
            lib.mi355pt_scene_export_flow_mark.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]
            lib.mi355pt_scene_export_triangle_ids.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]
            lib.mi355pt_temporal_accumulate_flow_device.argtypes = frame4 + flow3 + [C.c_void_p] * 4
            lib.mi355pt_temporal_accumulate_flow.argtypes = frame4 + flow3 + [C.c_void_p] * 3
            lib.mi355pt_temporal_accumulate_rectified_flow_device.argtypes = frame4 + [C.POINTER(TemporalRectifyParams), C.c_void_p, C.c_size_t] + flow3 + \
                [C.c_void_p] * 4
            lib.mi355pt_temporal_accumulate_rectified_flow.argtypes = frame4 + [C.POINTER(TemporalRectifyParams)] + flow3 + [C.c_void_p] * 3
        if hasattr(lib, "mi355pt_temporal_budget_device"):  # (absent from an older build loaded through MI355PT_LIB)
            probe8 = [C.POINTER(TemporalFrame), C.POINTER(TemporalFrame), C.POINTER(TemporalView), C.c_uint32, C.c_uint32, C.POINTER(TemporalParams),
                      C.POINTER(BudgetMotion), C.POINTER(BudgetParams)]
            lib.mi355pt_temporal_budget_device.argtypes = probe8 + [C.c_void_p] * 4
            lib.mi355pt_temporal_budget.argtypes = probe8 + [C.c_void_p] * 3
            lib.mi355pt_render_budget_device.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(Params), C.POINTER(BudgetParams)] + [C.c_void_p] * 5 + \
                [C.c_size_t, C.c_void_p, C.POINTER(AdaptiveResult)]
            lib.mi355pt_film_pair_normalize_tiles_device.argtypes = [C.c_void_p] * 3 + [C.c_uint32, C.c_uint32] + [C.c_void_p] * 3
            lib.mi355pt_film_pair_normalize_tiles.argtypes = [C.c_void_p] * 3 + [C.c_uint32, C.c_uint32] + [C.c_void_p] * 2
            lib.mi355pt_temporal_length_credit_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_uint32, C.c_uint32, C.c_void_p]
        if not hasattr(lib, "mi355pt_render_sample_log"):     # an older build loaded through MI355PT_LIB for an A/B timing run
            return
        lib.mi355pt_sample_log_records.argtypes = [C.POINTER(Camera), C.POINTER(Params), C.c_uint32, C.c_uint32, C.POINTER(C.c_size_t)]
        lib.mi355pt_render_sample_log.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(Params), C.c_uint32, C.c_uint32] + \
            [C.POINTER(C.c_float)] * 3 + [C.c_size_t, C.POINTER(C.c_float)]

    def version(self):
        return self.lib.mi355pt_version().decode()

    def debug_unlock(self, on=True):
        """mi355pt_debug_unlock (mi355pt_debug.h): lets params.rr_gate_slack through; returns the previous state.  The parity tests that
        relax the Russian-roulette gate switch it on for themselves (tests/conftest.py `product` fixture)."""
        if not hasattr(self.lib, "mi355pt_debug_unlock"):      # an older build loaded through MI355PT_LIB
            return True
        return bool(self.lib.mi355pt_debug_unlock(1 if on else 0))

    def scene_info(self, scene):
        buf = C.create_string_buffer(256)
        self.lib.mi355pt_scene_info.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
        self.check(self.lib.mi355pt_scene_info(scene.h, buf, 256), "scene_info")
        return buf.value.decode()

    def render(self, scene, cam, params, want_stats=False):
        """RendererImage::render -> (H, W, 3) float32 tone-mapped sRGB in [0,1] (renderer.rs:120-134)."""
        out = np.zeros((cam.height, cam.width, 3), dtype=np.float32)
        st = Stats()
        self.check(self.lib.mi355pt_render(scene.h, C.byref(cam), C.byref(params), _ptr(out, C.c_float), C.byref(st)), "render")
        return (out, st) if want_stats else out

    def render_aov(self, scene, cam, params, kind, illuminant_lut=0, want_stats=False):
        """RendererImage::<NormalRenderer | AlbedoRenderer>::render (main.rs:155-186) -> (H, W, 3) float32.  kind: AOV_NORMAL / AOV_ALBEDO /
        AOV_SHADING_NORMAL; illuminant_lut: the LUT470 id of presets()["cie_illum_d6500"] in this scene (albedo only)."""
        out = np.zeros((cam.height, cam.width, 3), dtype=np.float32)
        st = Stats()
        self.check(self.lib.mi355pt_render_aov(scene.h, C.byref(cam), C.byref(params), kind, illuminant_lut, _ptr(out, C.c_float), C.byref(st)),
                   "render_aov")
        return (out, st) if want_stats else out

    def render_aov_accum_device(self, scene, cam, params, kind, illuminant_lut, s_begin, s_end, d_accum_ptr, stream=None, stats=None):
        self.check(self.lib.mi355pt_render_aov_accum_device(scene.h, C.byref(cam), C.byref(params), kind, illuminant_lut, s_begin, s_end,
                                                            C.c_void_p(d_accum_ptr), C.c_void_p(stream or 0),
                                                            C.byref(stats) if stats is not None else None), "render_aov_accum_device")

    def aov_resolve_device(self, kind, d_accum_ptr, n_pixels, spp, d_out_ptr, stream=None):
        self.check(self.lib.mi355pt_aov_resolve_device(kind, C.c_void_p(d_accum_ptr), n_pixels, spp, C.c_void_p(d_out_ptr), C.c_void_p(stream or 0)),
                   "aov_resolve_device")

    # ---- the G-buffer pass (include/mi355pt_gbuffer.h): albedo, shading-normal, position and hit films from one primary-ray launch ----
    def render_gbuffer_accum_device(self, scene, cam, params, illuminant_lut, s_begin, s_end, films, stream=None, stats=None):
        """mi355pt_render_gbuffer_accum_device: `films` maps film names (GBUFFER_FILMS) to device pointers; a name left out or None is not wanted"""
        gf = GbufferFilms(*[C.c_void_p(films.get(k) or None) for k in GBUFFER_FILMS])
        self.check(self.lib.mi355pt_render_gbuffer_accum_device(scene.h, C.byref(cam), C.byref(params), illuminant_lut, s_begin, s_end, C.byref(gf),
                                                                C.c_void_p(stream or 0), C.byref(stats) if stats is not None else None),
                   "render_gbuffer_accum_device")

    def gbuffer_normalize_device(self, d_film_ptr, d_hit_ptr, n_pixels, d_out_ptr, stream=None):
        self.check(self.lib.mi355pt_gbuffer_normalize_device(C.c_void_p(d_film_ptr), C.c_void_p(d_hit_ptr), n_pixels, C.c_void_p(d_out_ptr),
                                                             C.c_void_p(stream or 0)), "gbuffer_normalize_device")

    def render_gbuffer(self, scene, cam, params, illuminant_lut=0, films=GBUFFER_FILMS, want_stats=False):
        """mi355pt_render_gbuffer -> {film name: (H, W, 3) float32 mean} for the names in `films` (albedo: resolved like render_aov's)"""
        out = {k: np.zeros((cam.height, cam.width, 3), dtype=np.float32) for k in films}
        gf = GbufferFilms(*[out[k].ctypes.data if k in out else None for k in GBUFFER_FILMS])
        st = Stats()
        self.check(self.lib.mi355pt_render_gbuffer(scene.h, C.byref(cam), C.byref(params), illuminant_lut, C.byref(gf), C.byref(st)), "render_gbuffer")
        return (out, st) if want_stats else out

    # ---- the denoiser (include/mi355pt_denoise.h): an a-trous filter over the linear beauty film, guided by the albedo / shading-normal films ----
    def denoise_params_default(self):
        p = DenoiseParams()
        self.lib.mi355pt_denoise_params_default(C.byref(p))
        return p

    def denoise_scratch_bytes(self, width, height):
        return int(self.lib.mi355pt_denoise_scratch_bytes(width, height))

    def denoise_device(self, d_beauty_ptr, spp_beauty, d_albedo_ptr, spp_albedo, d_normal_ptr, spp_normal, width, height, params, d_scratch_ptr,
                       scratch_bytes, d_out_ptr, stream=None):
        """mi355pt_denoise_device on device pointers (films of linear SUMS, W*H*3 f32; albedo / normal pointer None or 0 = not given);
        asynchronous on `stream`.  The output is a linear mean: resolve it with film_resolve_device(.., spp=1, ..)."""
        self.check(self.lib.mi355pt_denoise_device(C.c_void_p(d_beauty_ptr), spp_beauty, C.c_void_p(d_albedo_ptr or 0), spp_albedo,
                                                   C.c_void_p(d_normal_ptr or 0), spp_normal, width, height, C.byref(params),
                                                   C.c_void_p(d_scratch_ptr), scratch_bytes, C.c_void_p(d_out_ptr), C.c_void_p(stream or 0)),
                   "denoise_device")

    def denoise(self, beauty, spp_beauty, albedo=None, spp_albedo=0, normal=None, spp_normal=0, params=None):
        """mi355pt_denoise on host arrays (H, W, 3) of linear sums -> (H, W, 3) float32 linear mean"""
        b = np.ascontiguousarray(beauty, dtype=np.float32)
        assert b.ndim == 3 and b.shape[2] == 3
        a = None if albedo is None else np.ascontiguousarray(albedo, dtype=np.float32)
        n = None if normal is None else np.ascontiguousarray(normal, dtype=np.float32)
        assert all(g is None or g.shape == b.shape for g in (a, n))
        params = params if params is not None else self.denoise_params_default()
        out = np.zeros(b.shape, dtype=np.float32)
        self.check(self.lib.mi355pt_denoise(_ptr(b, C.c_float), spp_beauty, _ptr(a, C.c_float), spp_albedo, _ptr(n, C.c_float), spp_normal,
                                            b.shape[1], b.shape[0], C.byref(params), _ptr(out, C.c_float)), "denoise")
        return out

    # ---- the variance-guided denoiser (include/mi355pt_denoise_var.h): the film and the half film give the variance that scales its edge stop ----
    def denoise_var_params_default(self):
        p = DenoiseVarParams()
        self.lib.mi355pt_denoise_var_params_default(C.byref(p))
        return p

    def denoise_var_scratch_bytes(self, width, height):
        return int(self.lib.mi355pt_denoise_var_scratch_bytes(width, height))

    def denoise_var_device(self, d_beauty_ptr, d_half_ptr, spp_beauty, d_tile_spp_ptr, d_albedo_ptr, spp_albedo, d_normal_ptr, spp_normal, width, height, params,
                           d_scratch_ptr, scratch_bytes, d_out_ptr, stream=None):
        """mi355pt_denoise_var_device on device pointers (films of linear SUMS, W*H*3 f32; tile counts, albedo / normal pointer None or 0 = not given;
        with tile counts spp_beauty is 0); asynchronous on `stream`.  The output is a linear mean: resolve it with film_resolve_device(.., spp=1, ..)."""
        self.check(self.lib.mi355pt_denoise_var_device(C.c_void_p(d_beauty_ptr), C.c_void_p(d_half_ptr), spp_beauty, C.c_void_p(d_tile_spp_ptr or 0),
                                                       C.c_void_p(d_albedo_ptr or 0), spp_albedo, C.c_void_p(d_normal_ptr or 0), spp_normal, width, height,
                                                       C.byref(params), C.c_void_p(d_scratch_ptr), scratch_bytes, C.c_void_p(d_out_ptr), C.c_void_p(stream or 0)),
                   "denoise_var_device")

    def denoise_var(self, beauty, half, spp_beauty, tile_spp=None, albedo=None, spp_albedo=0, normal=None, spp_normal=0, params=None):
        """mi355pt_denoise_var on host arrays (H, W, 3) of linear sums (tile_spp: one uint32 per 8x8 tile, then spp_beauty = 0) -> (H, W, 3) float32
        linear mean"""
        b = np.ascontiguousarray(beauty, dtype=np.float32)
        h = np.ascontiguousarray(half, dtype=np.float32)
        assert b.ndim == 3 and b.shape[2] == 3
        a = None if albedo is None else np.ascontiguousarray(albedo, dtype=np.float32)
        n = None if normal is None else np.ascontiguousarray(normal, dtype=np.float32)
        assert all(g is None or g.shape == b.shape for g in (h, a, n))
        t = None if tile_spp is None else np.ascontiguousarray(tile_spp, dtype=np.uint32).reshape(-1)
        assert t is None or t.size == ((b.shape[0] + 7) // 8) * ((b.shape[1] + 7) // 8)
        params = params if params is not None else self.denoise_var_params_default()
        out = np.zeros(b.shape, dtype=np.float32)
        self.check(self.lib.mi355pt_denoise_var(_ptr(b, C.c_float), _ptr(h, C.c_float), spp_beauty, _ptr(t, C.c_uint32), _ptr(a, C.c_float), spp_albedo,
                                                _ptr(n, C.c_float), spp_normal, b.shape[1], b.shape[0], C.byref(params), _ptr(out, C.c_float)), "denoise_var")
        return out

    # ---- the temporal reprojection (include/mi355pt_temporal.h): the previous frame's accumulated films gathered through the hit position ----
    def temporal_params_default(self):
        p = TemporalParams()
        self.lib.mi355pt_temporal_params_default(C.byref(p))
        return p

    def temporal_view_from_cameras(self, cur, prev):
        """mi355pt_temporal_view_from_cameras (host only) -> TemporalView"""
        v = TemporalView()
        self.check(self.lib.mi355pt_temporal_view_from_cameras(C.byref(cur), C.byref(prev), C.byref(v)), "temporal_view_from_cameras")
        return v

    @staticmethod
    def _temporal_frames(cur, prev, host):
        """The `cur` / `prev` dicts of the temporal_accumulate* methods (prev None: no previous frame) -> (TemporalFrame, TemporalFrame or
        None, keep).  host False: the values are device pointers; host True: arrays, and keep = [cur's, prev's] dicts of the contiguous
        float32 arrays the frames point into, which must outlive the call"""
        frames, keep = [], []
        for frame in (cur, prev):
            if frame is None:
                frames.append(None)
            elif host:
                keep.append({k: np.ascontiguousarray(v, dtype=np.float32) for k, v in frame.items() if v is not None})
                frames.append(TemporalFrame(*[keep[-1][k].ctypes.data if k in keep[-1] else None for k in TEMPORAL_FILMS]))
            else:
                frames.append(TemporalFrame(*[C.c_void_p(frame.get(k) or None) for k in TEMPORAL_FILMS]))
        return frames[0], frames[1], keep

    @staticmethod
    def _temporal_outputs(kc):
        """The outputs of a host call on the current frame's arrays `kc` -> (h, w, out_film, out_half or None, out_length)"""
        h, w = kc["film"].shape[:2]
        return h, w, np.zeros((h, w, 3), np.float32), np.zeros((h, w, 3), np.float32) if "half" in kc else None, np.zeros((h, w), np.float32)

    def temporal_accumulate_device(self, cur, spp, prev, view, width, height, params, d_out_film_ptr, d_out_half_ptr, d_out_length_ptr, stream=None):
        """mi355pt_temporal_accumulate_device: `cur` / `prev` map film names (TEMPORAL_FILMS) to device pointers (a name left out or None is
        NULL); prev and view None = the first frame; d_out_half_ptr None or 0 without a half film"""
        fc, fp, _ = self._temporal_frames(cur, prev, host=False)
        self.check(self.lib.mi355pt_temporal_accumulate_device(C.byref(fc), spp, C.byref(fp) if fp is not None else None,
                                                               C.byref(view) if view is not None else None, width, height, C.byref(params),
                                                               C.c_void_p(d_out_film_ptr), C.c_void_p(d_out_half_ptr or 0), C.c_void_p(d_out_length_ptr),
                                                               C.c_void_p(stream or 0)), "temporal_accumulate_device")

    def temporal_accumulate(self, cur, spp, prev=None, view=None, params=None):
        """mi355pt_temporal_accumulate on host arrays: `cur` / `prev` map film names to (H, W, 3) float32 arrays ((H, W) for length)
        -> (out_film, out_half or None, out_length)"""
        fc, fp, keep = self._temporal_frames(cur, prev, host=True)
        h, w, out_film, out_half, out_len = self._temporal_outputs(keep[0])
        params = params if params is not None else self.temporal_params_default()
        self.check(self.lib.mi355pt_temporal_accumulate(C.byref(fc), spp, C.byref(fp) if fp is not None else None,
                                                        C.byref(view) if view is not None else None, w, h, C.byref(params), out_film.ctypes.data,
                                                        out_half.ctypes.data if out_half is not None else None, out_len.ctypes.data), "temporal_accumulate")
        return out_film, out_half, out_len

    # ---- its rectified form (include/mi355pt_temporal_rectify.h): the gathered history is scaled to the current frame's local mean first ----
    def temporal_rectify_params_default(self):
        p = TemporalRectifyParams()
        self.lib.mi355pt_temporal_rectify_params_default(C.byref(p))
        return p

    def temporal_rectify_scratch_bytes(self, width, height):
        return int(self.lib.mi355pt_temporal_rectify_scratch_bytes(width, height))

    def temporal_accumulate_rectified_device(self, cur, spp, prev, view, width, height, params, rectify_params, d_scratch_ptr, scratch_bytes, d_out_film_ptr,
                                             d_out_half_ptr, d_out_length_ptr, stream=None):
        """mi355pt_temporal_accumulate_rectified_device: the arguments of temporal_accumulate_device, the rectification's parameters and a
        device scratch of temporal_rectify_scratch_bytes(width, height) bytes"""
        fc, fp, _ = self._temporal_frames(cur, prev, host=False)
        self.check(self.lib.mi355pt_temporal_accumulate_rectified_device(C.byref(fc), spp, C.byref(fp) if fp is not None else None,
                                                                         C.byref(view) if view is not None else None, width, height, C.byref(params),
                                                                         C.byref(rectify_params), C.c_void_p(d_scratch_ptr), scratch_bytes,
                                                                         C.c_void_p(d_out_film_ptr), C.c_void_p(d_out_half_ptr or 0), C.c_void_p(d_out_length_ptr),
                                                                         C.c_void_p(stream or 0)), "temporal_accumulate_rectified_device")

    def temporal_accumulate_rectified(self, cur, spp, prev=None, view=None, params=None, rectify_params=None):
        """mi355pt_temporal_accumulate_rectified on host arrays, as temporal_accumulate -> (out_film, out_half or None, out_length)"""
        fc, fp, keep = self._temporal_frames(cur, prev, host=True)
        h, w, out_film, out_half, out_len = self._temporal_outputs(keep[0])
        params = params if params is not None else self.temporal_params_default()
        rectify_params = rectify_params if rectify_params is not None else self.temporal_rectify_params_default()
        self.check(self.lib.mi355pt_temporal_accumulate_rectified(C.byref(fc), spp, C.byref(fp) if fp is not None else None,
                                                                  C.byref(view) if view is not None else None, w, h, C.byref(params), C.byref(rectify_params),
                                                                  out_film.ctypes.data, out_half.ctypes.data if out_half is not None else None,
                                                                  out_len.ctypes.data), "temporal_accumulate_rectified")
        return out_film, out_half, out_len

    # ---- object motion vectors (include/mi355pt_motion.h): the ID pass, the motion table and the motion-aware twins of the accumulation ----
    def render_ids_device(self, scene, cam, params, d_ids_ptr, stream=None, stats=None):
        """mi355pt_render_ids_device: instance + 1 of the closest hit through every pixel centre (0: a miss) into W x H u32 on the device"""
        self.check(self.lib.mi355pt_render_ids_device(scene.h, C.byref(cam), C.byref(params), C.c_void_p(d_ids_ptr), C.c_void_p(stream or 0),
                                                      C.byref(stats) if stats is not None else None), "render_ids_device")

    def render_ids(self, scene, cam, params):
        """mi355pt_render_ids -> (H, W) uint32"""
        ids = np.zeros((cam.height, cam.width), np.uint32)
        self.check(self.lib.mi355pt_render_ids(scene.h, C.byref(cam), C.byref(params), ids.ctypes.data, None), "render_ids")
        return ids

    def motion_table(self, cur_cam, prev_cam, l2w_cur, l2w_prev):
        """mi355pt_motion_table (host only): l2w_cur / l2w_prev are n matrices (row-major 4 x 4 each, as add_instance takes them)
        -> (n + 1, 24) float32, one row per mi355pt_motion_xform (a 0:9, b 9:12, n 12:21, pad 21:24); entry 0 is the static one"""
        mc, mp = (np.ascontiguousarray(np.asarray(m, np.float32).reshape(-1, 4, 4).transpose(0, 2, 1)).reshape(-1, 16) for m in (l2w_cur, l2w_prev))   # column-major
        assert mc.shape == mp.shape
        out = np.zeros((mc.shape[0] + 1, 24), np.float32)
        self.check(self.lib.mi355pt_motion_table(C.byref(cur_cam), C.byref(prev_cam), mc.ctypes.data, mp.ctypes.data, mc.shape[0], out.ctypes.data), "motion_table")
        return out

    def temporal_accumulate_motion_device(self, cur, spp, prev, view, width, height, params, d_ids_cur_ptr, d_ids_prev_ptr, d_table_ptr, n_entries,
                                          d_out_film_ptr, d_out_half_ptr, d_out_length_ptr, rectify_params=None, d_scratch_ptr=None, scratch_bytes=0, stream=None):
        """mi355pt_temporal_accumulate_motion_device or, with rectify_params (and a scratch), mi355pt_temporal_accumulate_rectified_motion_device:
        the arguments of their twins plus the current ids, the previous ids (None: no id test of the taps) and the table, all device pointers"""
        fc, fp, _ = self._temporal_frames(cur, prev, host=False)
        head = (C.byref(fc), spp, C.byref(fp) if fp is not None else None, C.byref(view) if view is not None else None, width, height, C.byref(params))
        tail = (C.c_void_p(d_ids_cur_ptr), C.c_void_p(d_ids_prev_ptr or 0), C.c_void_p(d_table_ptr), n_entries, C.c_void_p(d_out_film_ptr),
                C.c_void_p(d_out_half_ptr or 0), C.c_void_p(d_out_length_ptr), C.c_void_p(stream or 0))
        if rectify_params is None:
            self.check(self.lib.mi355pt_temporal_accumulate_motion_device(*head, *tail), "temporal_accumulate_motion_device")
        else:
            self.check(self.lib.mi355pt_temporal_accumulate_rectified_motion_device(*head, C.byref(rectify_params), C.c_void_p(d_scratch_ptr), scratch_bytes, *tail),
                       "temporal_accumulate_rectified_motion_device")

    def temporal_accumulate_motion(self, cur, spp, prev, view, ids_cur, ids_prev, table, params=None, rectify_params=None):
        """mi355pt_temporal_accumulate_motion (or, with rectify_params, mi355pt_temporal_accumulate_rectified_motion) on host arrays, as
        temporal_accumulate; ids (H, W) uint32, table (n_entries, 24) float32 -> (out_film, out_half or None, out_length)"""
        fc, fp, keep = self._temporal_frames(cur, prev, host=True)
        h, w, out_film, out_half, out_len = self._temporal_outputs(keep[0])
        ic = np.ascontiguousarray(ids_cur, dtype=np.uint32)
        ip = np.ascontiguousarray(ids_prev, dtype=np.uint32) if ids_prev is not None else None
        tab = np.ascontiguousarray(table, dtype=np.float32).reshape(-1, 24)
        params = params if params is not None else self.temporal_params_default()
        head = (C.byref(fc), spp, C.byref(fp) if fp is not None else None, C.byref(view) if view is not None else None, w, h, C.byref(params))
        tail = (ic.ctypes.data, ip.ctypes.data if ip is not None else None, tab.ctypes.data, tab.shape[0], out_film.ctypes.data,
                out_half.ctypes.data if out_half is not None else None, out_len.ctypes.data)
        if rectify_params is None:
            self.check(self.lib.mi355pt_temporal_accumulate_motion(*head, *tail), "temporal_accumulate_motion")
        else:
            self.check(self.lib.mi355pt_temporal_accumulate_rectified_motion(*head, C.byref(rectify_params), *tail), "temporal_accumulate_rectified_motion")
        return out_film, out_half, out_len

    # ---- per-pixel motion vectors (include/mi355pt_flow.h): the mark, the flow pass and the flow-aware twins of the accumulation ----
    def scene_flow_mark(self, scene, stream=None):
        """mi355pt_scene_flow_mark: the scene keeps a copy of its current render-space triangle positions (asynchronous on `stream`)"""
        self.check(self.lib.mi355pt_scene_flow_mark(scene.h, C.c_void_p(stream or 0)), "scene_flow_mark")

    def scene_flow_marked(self, scene):
        return bool(self.lib.mi355pt_scene_flow_marked(scene.h))

    def render_flow_device(self, scene, cam, params, d_flow_ptr, d_ids_ptr=None, stream=None, stats=None):
        """mi355pt_render_flow_device: W x H mi355pt_flow_pixel records (and, with d_ids_ptr, the ID pass's u32) on the device"""
        self.check(self.lib.mi355pt_render_flow_device(scene.h, C.byref(cam), C.byref(params), C.c_void_p(d_flow_ptr), C.c_void_p(d_ids_ptr or 0),
                                                       C.c_void_p(stream or 0), C.byref(stats) if stats is not None else None), "render_flow_device")

    def render_flow(self, scene, cam, params, want_ids=True):
        """mi355pt_render_flow -> ((H, W) FLOW_PIXEL records, (H, W) uint32 or None)"""
        flow = np.zeros((cam.height, cam.width), FLOW_PIXEL)
        ids = np.zeros((cam.height, cam.width), np.uint32) if want_ids else None
        self.check(self.lib.mi355pt_render_flow(scene.h, C.byref(cam), C.byref(params), flow.ctypes.data, ids.ctypes.data if want_ids else None, None), "render_flow")
        return flow, ids

    def render_flow_debug(self, scene, cam, params):
        """mi355pt_render_flow_debug (include/mi355pt_debug.h) -> ((H, W) FLOW_PIXEL, (H, W) uint32, (H, W) FLOW_HIT): the records, the ids and
        the hits {tri, b0, b1, b2} the records were computed from"""
        flow = np.zeros((cam.height, cam.width), FLOW_PIXEL)
        ids = np.zeros((cam.height, cam.width), np.uint32)
        hits = np.zeros((cam.height, cam.width), FLOW_HIT)
        self.check(self.lib.mi355pt_render_flow_debug(scene.h, C.byref(cam), C.byref(params), flow.ctypes.data, ids.ctypes.data, hits.ctypes.data, None),
                   "render_flow_debug")
        return flow, ids, hits

    def scene_export_flow_mark(self, scene):
        """mi355pt_scene_export_flow_mark (include/mi355pt_debug.h) -> (n_tris, 12) float32: the mark's 48-byte records (p0 p1 p2 in words 0 - 8)"""
        n = C.c_uint32(0)
        self.check(self.lib.mi355pt_scene_export_flow_mark(scene.h, None, C.byref(n)), "scene_export_flow_mark")
        out = np.zeros((n.value, 12), np.float32)
        self.check(self.lib.mi355pt_scene_export_flow_mark(scene.h, out.ctypes.data, C.byref(n)), "scene_export_flow_mark")
        return out

    def scene_export_triangle_ids(self, scene):
        """mi355pt_scene_export_triangle_ids (include/mi355pt_debug.h) -> (n_tris, 2) uint32: (instance, triangle inside its mesh) per leaf-order triangle"""
        n = C.c_uint32(0)
        self.check(self.lib.mi355pt_scene_export_triangle_ids(scene.h, None, C.byref(n)), "scene_export_triangle_ids")
        out = np.zeros((n.value, 2), np.uint32)
        self.check(self.lib.mi355pt_scene_export_triangle_ids(scene.h, out.ctypes.data, C.byref(n)), "scene_export_triangle_ids")
        return out

    def temporal_accumulate_flow_device(self, cur, spp, prev, view, width, height, params, d_ids_cur_ptr, d_ids_prev_ptr, d_flow_ptr, d_out_film_ptr,
                                        d_out_half_ptr, d_out_length_ptr, rectify_params=None, d_scratch_ptr=None, scratch_bytes=0, stream=None):
        """mi355pt_temporal_accumulate_flow_device or, with rectify_params (and a scratch), mi355pt_temporal_accumulate_rectified_flow_device:
        the arguments of their twins plus the current ids (None without previous ids), the previous ids (None: no id test of the taps) and
        the flow records, all device pointers"""
        fc, fp, _ = self._temporal_frames(cur, prev, host=False)
        head = (C.byref(fc), spp, C.byref(fp) if fp is not None else None, C.byref(view) if view is not None else None, width, height, C.byref(params))
        tail = (C.c_void_p(d_ids_cur_ptr or 0), C.c_void_p(d_ids_prev_ptr or 0), C.c_void_p(d_flow_ptr), C.c_void_p(d_out_film_ptr),
                C.c_void_p(d_out_half_ptr or 0), C.c_void_p(d_out_length_ptr), C.c_void_p(stream or 0))
        if rectify_params is None:
            self.check(self.lib.mi355pt_temporal_accumulate_flow_device(*head, *tail), "temporal_accumulate_flow_device")
        else:
            self.check(self.lib.mi355pt_temporal_accumulate_rectified_flow_device(*head, C.byref(rectify_params), C.c_void_p(d_scratch_ptr), scratch_bytes, *tail),
                       "temporal_accumulate_rectified_flow_device")

    def temporal_accumulate_flow(self, cur, spp, prev, view, ids_cur, ids_prev, flow, params=None, rectify_params=None):
        """mi355pt_temporal_accumulate_flow (or, with rectify_params, mi355pt_temporal_accumulate_rectified_flow) on host arrays, as
        temporal_accumulate; ids (H, W) uint32 or None, flow (H, W) FLOW_PIXEL -> (out_film, out_half or None, out_length)"""
        fc, fp, keep = self._temporal_frames(cur, prev, host=True)
        h, w, out_film, out_half, out_len = self._temporal_outputs(keep[0])
        ic = np.ascontiguousarray(ids_cur, dtype=np.uint32) if ids_cur is not None else None
        ip = np.ascontiguousarray(ids_prev, dtype=np.uint32) if ids_prev is not None else None
        fl = np.ascontiguousarray(flow, dtype=FLOW_PIXEL)
        assert fl.shape == (h, w)
        params = params if params is not None else self.temporal_params_default()
        head = (C.byref(fc), spp, C.byref(fp) if fp is not None else None, C.byref(view) if view is not None else None, w, h, C.byref(params))
        tail = (ic.ctypes.data if ic is not None else None, ip.ctypes.data if ip is not None else None, fl.ctypes.data, out_film.ctypes.data,
                out_half.ctypes.data if out_half is not None else None, out_len.ctypes.data)
        if rectify_params is None:
            self.check(self.lib.mi355pt_temporal_accumulate_flow(*head, *tail), "temporal_accumulate_flow")
        else:
            self.check(self.lib.mi355pt_temporal_accumulate_rectified_flow(*head, C.byref(rectify_params), *tail), "temporal_accumulate_rectified_flow")
        return out_film, out_half, out_len

    # ---- the sample budget by reprojected history (include/mi355pt_budget.h): probe, driver, pair normalise, length credit ----
    @staticmethod
    def budget_params(base_spp, max_spp, target_history):
        return BudgetParams(base_spp, max_spp, target_history)

    @staticmethod
    def budget_motion(ids_cur=None, ids_prev=None, table=None, n_entries=0, flow=None):
        """mi355pt_budget_motion from pointers (ints; None = NULL)"""
        return BudgetMotion(ids_cur or None, ids_prev or None, table or None, n_entries, flow or None)

    def temporal_budget_device(self, cur, prev, view, width, height, params, motion, budget, d_pred_ptr, d_tile_len_ptr, d_tile_spp_ptr, stream=None):
        """mi355pt_temporal_budget_device: `cur` / `prev` as temporal_accumulate_device takes them (film and half are not read); motion a
        BudgetMotion of device pointers or None; d_pred_ptr None or 0: P is not wanted"""
        fc, fp, _ = self._temporal_frames(cur, prev, host=False)
        self.check(self.lib.mi355pt_temporal_budget_device(C.byref(fc), C.byref(fp) if fp is not None else None, C.byref(view) if view is not None else None,
                                                           width, height, C.byref(params), C.byref(motion) if motion is not None else None, C.byref(budget),
                                                           C.c_void_p(d_pred_ptr or 0), C.c_void_p(d_tile_len_ptr), C.c_void_p(d_tile_spp_ptr),
                                                           C.c_void_p(stream or 0)), "temporal_budget_device")

    def temporal_budget(self, cur, prev, view, budget, params=None, ids_cur=None, ids_prev=None, table=None, flow=None):
        """mi355pt_temporal_budget on host arrays: `cur` / `prev` map film names to arrays (position, shading_normal, hit; length of prev);
        ids (H, W) uint32 or None, table (n_entries, 24) float32 or None, flow (H, W) FLOW_PIXEL or None
        -> (P (H, W) float32, tile_len (tiles_y, tiles_x) float32, tile_spp (tiles_y, tiles_x) uint32)"""
        fc, fp, keep = self._temporal_frames(cur, prev, host=True)
        h, w = keep[0]["hit"].shape[:2]
        ty, tx = (h + 7) // 8, (w + 7) // 8
        pred, tile_len, tile_spp = np.zeros((h, w), np.float32), np.zeros((ty, tx), np.float32), np.zeros((ty, tx), np.uint32)
        params = params if params is not None else self.temporal_params_default()
        ic = np.ascontiguousarray(ids_cur, dtype=np.uint32) if ids_cur is not None else None
        ip = np.ascontiguousarray(ids_prev, dtype=np.uint32) if ids_prev is not None else None
        tab = np.ascontiguousarray(table, dtype=np.float32).reshape(-1, 24) if table is not None else None
        fl = np.ascontiguousarray(flow, dtype=FLOW_PIXEL) if flow is not None else None
        data = lambda a: a.ctypes.data if a is not None else None   # noqa: E731
        motion = BudgetMotion(data(ic), data(ip), data(tab), tab.shape[0] if tab is not None else 0, data(fl))
        self.check(self.lib.mi355pt_temporal_budget(C.byref(fc), C.byref(fp) if fp is not None else None, C.byref(view) if view is not None else None, w, h,
                                                    C.byref(params), C.byref(motion), C.byref(budget), pred.ctypes.data, tile_len.ctypes.data,
                                                    tile_spp.ctypes.data), "temporal_budget")
        return pred, tile_len, tile_spp

    def render_budget_device(self, scene, cam, params, budget, d_tile_spp_ptr, d_film_ptr, d_half_ptr, d_list_ptr, d_scratch_ptr, scratch_bytes, stream=None):
        """mi355pt_render_budget_device -> AdaptiveResult (passes, tiles_at_max, total_samples)"""
        res = AdaptiveResult()
        self.check(self.lib.mi355pt_render_budget_device(scene.h, C.byref(cam), C.byref(params), C.byref(budget), C.c_void_p(d_tile_spp_ptr),
                                                         C.c_void_p(d_film_ptr), C.c_void_p(d_half_ptr), C.c_void_p(d_list_ptr), C.c_void_p(d_scratch_ptr),
                                                         scratch_bytes, C.c_void_p(stream or 0), C.byref(res)), "render_budget_device")
        return res

    def film_pair_normalize_tiles_device(self, d_film_ptr, d_half_ptr, d_tile_spp_ptr, width, height, d_out_film_ptr, d_out_half_ptr, stream=None):
        self.check(self.lib.mi355pt_film_pair_normalize_tiles_device(C.c_void_p(d_film_ptr), C.c_void_p(d_half_ptr), C.c_void_p(d_tile_spp_ptr), width, height,
                                                                     C.c_void_p(d_out_film_ptr), C.c_void_p(d_out_half_ptr), C.c_void_p(stream or 0)),
                   "film_pair_normalize_tiles_device")

    def film_pair_normalize_tiles(self, film, half, tile_spp):
        """mi355pt_film_pair_normalize_tiles on host arrays -> (out_film, out_half): a film pair with spp = 2"""
        f, hf = np.ascontiguousarray(film, dtype=np.float32), np.ascontiguousarray(half, dtype=np.float32)
        ts = np.ascontiguousarray(tile_spp, dtype=np.uint32)
        h, w = f.shape[:2]
        out_film, out_half = np.zeros_like(f), np.zeros_like(hf)
        self.check(self.lib.mi355pt_film_pair_normalize_tiles(f.ctypes.data, hf.ctypes.data, ts.ctypes.data, w, h, out_film.ctypes.data, out_half.ctypes.data),
                   "film_pair_normalize_tiles")
        return out_film, out_half

    def temporal_length_credit_device(self, d_length_ptr, d_tile_spp_ptr, base_spp, max_history, width, height, stream=None):
        self.check(self.lib.mi355pt_temporal_length_credit_device(C.c_void_p(d_length_ptr), C.c_void_p(d_tile_spp_ptr), base_spp, max_history, width, height,
                                                                  C.c_void_p(stream or 0)), "temporal_length_credit_device")

    # ---- guided half-resolution rendering (include/mi355pt_upsample.h): a film traced at W/2 x H/2 rebuilt at W x H through both G-buffers ----
    def upsample_params_default(self):
        p = UpsampleParams()
        self.lib.mi355pt_upsample_params_default(C.byref(p))
        return p

    def upsample_low_camera(self, full):
        """mi355pt_upsample_low_camera (host only) -> Camera of width / 2 x height / 2"""
        low = Camera()
        self.check(self.lib.mi355pt_upsample_low_camera(C.byref(full), C.byref(low)), "upsample_low_camera")
        return low

    def upsample_device(self, d_low_film_ptr, d_low_half_ptr, spp, low_guides, spp_albedo_low, full_guides, spp_albedo_full, width, height, params,
                        d_out_film_ptr, d_out_half_ptr, stream=None):
        """mi355pt_upsample_device: low_guides / full_guides map guide names (UPSAMPLE_GUIDES) to device pointers (a name left out or None is
        NULL); width and height are the FULL size; d_low_half_ptr and d_out_half_ptr None or 0 without a half film"""
        gl = UpsampleGuides(*[C.c_void_p(low_guides.get(k) or None) for k in UPSAMPLE_GUIDES])
        gf = UpsampleGuides(*[C.c_void_p(full_guides.get(k) or None) for k in UPSAMPLE_GUIDES])
        self.check(self.lib.mi355pt_upsample_device(C.c_void_p(d_low_film_ptr), C.c_void_p(d_low_half_ptr or 0), spp, C.byref(gl), spp_albedo_low, C.byref(gf),
                                                    spp_albedo_full, width, height, C.byref(params), C.c_void_p(d_out_film_ptr), C.c_void_p(d_out_half_ptr or 0),
                                                    C.c_void_p(stream or 0)), "upsample_device")

    def upsample(self, low_film, low_half, spp, low_guides, spp_albedo_low, full_guides, spp_albedo_full, params=None):
        """mi355pt_upsample on host arrays: low_film / low_half (h, w, 3) float32 sums (low_half may be None), the guides map names to
        (h, w, 3) / (H, W, 3) arrays -> (out_film, out_half or None), (H, W, 3)"""
        def host(g):
            keep = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in g.items() if v is not None and k in UPSAMPLE_GUIDES}
            return keep, UpsampleGuides(*[keep[k].ctypes.data if k in keep else None for k in UPSAMPLE_GUIDES])
        kl, gl = host(low_guides)
        kf, gf = host(full_guides)
        b = np.ascontiguousarray(low_film, dtype=np.float32)
        hf = None if low_half is None else np.ascontiguousarray(low_half, dtype=np.float32)
        h, w = kf["hit"].shape[:2]
        assert b.shape == (h // 2, w // 2, 3) and kl["hit"].shape == b.shape
        params = params if params is not None else self.upsample_params_default()
        out_film = np.zeros((h, w, 3), np.float32)
        out_half = np.zeros((h, w, 3), np.float32) if hf is not None else None
        self.check(self.lib.mi355pt_upsample(b.ctypes.data, hf.ctypes.data if hf is not None else None, spp, C.byref(gl), spp_albedo_low, C.byref(gf),
                                             spp_albedo_full, w, h, C.byref(params), out_film.ctypes.data,
                                             out_half.ctypes.data if out_half is not None else None), "upsample")
        return out_film, out_half

    # ---- the display stage (include/mi355pt_display.h): histogram auto-exposure, tone curves, encoding ----
    def display_params_default(self):
        p = DisplayParams()
        self.lib.mi355pt_display_params_default(C.byref(p))
        return p

    def display_scratch_bytes(self, width, height):
        return int(self.lib.mi355pt_display_scratch_bytes(width, height))

    def display_meter_device(self, d_film_ptr, width, height, spp, params, d_prev_record_ptr, d_scratch_ptr, scratch_bytes, d_record_ptr, d_hist_ptr=None, stream=None):
        """mi355pt_display_meter_device: d_prev_record_ptr None or 0 = no previous record (it may equal d_record_ptr); d_hist_ptr None = not wanted"""
        self.check(self.lib.mi355pt_display_meter_device(C.c_void_p(d_film_ptr), width, height, spp, C.byref(params), C.c_void_p(d_prev_record_ptr or 0),
                                                         C.c_void_p(d_scratch_ptr), scratch_bytes, C.c_void_p(d_record_ptr), C.c_void_p(d_hist_ptr or 0),
                                                         C.c_void_p(stream or 0)), "display_meter_device")

    def display_device(self, d_film_ptr, width, height, spp, params, d_record_ptr, d_out_ptr, stream=None):
        """mi355pt_display_device: d_record_ptr None or 0 = the constant params.exposure"""
        self.check(self.lib.mi355pt_display_device(C.c_void_p(d_film_ptr), width, height, spp, C.byref(params), C.c_void_p(d_record_ptr or 0), C.c_void_p(d_out_ptr),
                                                   C.c_void_p(stream or 0)), "display_device")

    def probe_display_meter_ms(self, d_film_ptr, width, height, spp, params, d_scratch_ptr, scratch_bytes, d_record_ptr):
        """mi355pt_probe_display_meter_ms (include/mi355pt_debug.h) -> (ms of the block histograms, ms of the finish)"""
        out = (C.c_float * 2)()
        self.lib.mi355pt_probe_display_meter_ms.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(DisplayParams), C.c_void_p, C.c_size_t, C.c_void_p,
                                                            C.POINTER(C.c_float)]
        self.check(self.lib.mi355pt_probe_display_meter_ms(C.c_void_p(d_film_ptr), width, height, spp, C.byref(params), C.c_void_p(d_scratch_ptr), scratch_bytes,
                                                           C.c_void_p(d_record_ptr), out), "probe_display_meter_ms")
        return float(out[0]), float(out[1])

    def display_meter(self, film, spp, params=None, prev_record=None, want_hist=True):
        """mi355pt_display_meter on a host (H, W, 3) float32 film of sums -> (record: 8 uint32, hist: 258 uint32 or None)"""
        f = np.ascontiguousarray(film, dtype=np.float32)
        h, w = f.shape[:2]
        params = params if params is not None else self.display_params_default()
        prev = None if prev_record is None else np.ascontiguousarray(prev_record, dtype=np.uint32)
        record = np.zeros(DISPLAY_RECORD_WORDS, np.uint32)
        hist = np.zeros(DISPLAY_HIST_WORDS, np.uint32) if want_hist else None
        self.check(self.lib.mi355pt_display_meter(f.ctypes.data, w, h, spp, C.byref(params), prev.ctypes.data if prev is not None else None, record.ctypes.data,
                                                  hist.ctypes.data if hist is not None else None), "display_meter")
        return record, hist

    def display(self, film, spp, params=None, record=None):
        """mi355pt_display on a host (H, W, 3) float32 film of sums -> (H, W, 3) float32; record None = the constant params.exposure"""
        f = np.ascontiguousarray(film, dtype=np.float32)
        h, w = f.shape[:2]
        params = params if params is not None else self.display_params_default()
        rec = None if record is None else np.ascontiguousarray(record, dtype=np.uint32)
        out = np.zeros((h, w, 3), np.float32)
        self.check(self.lib.mi355pt_display(f.ctypes.data, w, h, spp, C.byref(params), rec.ctypes.data if rec is not None else None, out.ctypes.data), "display")
        return out

    # ---- the bloom stage (include/mi355pt_bloom.h): bright pass, blur pyramid, composite; in front of the display stage ----
    def bloom_params_default(self):
        p = BloomParams()
        self.lib.mi355pt_bloom_params_default(C.byref(p))
        return p

    def bloom_scratch_bytes(self, width, height, levels):
        return int(self.lib.mi355pt_bloom_scratch_bytes(width, height, levels))

    def bloom_device(self, d_film_ptr, width, height, spp, params, d_record_ptr, d_scratch_ptr, scratch_bytes, d_out_ptr, stream=None):
        """mi355pt_bloom_device: d_record_ptr None or 0 = the constant params.exposure; d_out_ptr may be d_film_ptr"""
        self.check(self.lib.mi355pt_bloom_device(C.c_void_p(d_film_ptr), width, height, spp, C.byref(params), C.c_void_p(d_record_ptr or 0),
                                                            C.c_void_p(d_scratch_ptr), scratch_bytes, C.c_void_p(d_out_ptr), C.c_void_p(stream or 0)), "bloom_device")

    def bloom(self, film, spp, params=None, record=None):
        """mi355pt_bloom on a host (H, W, 3) float32 film of sums -> (H, W, 3) float32 film of spp 1; record None = the constant params.exposure"""
        f = np.ascontiguousarray(film, dtype=np.float32)
        h, w = f.shape[:2]
        params = params if params is not None else self.bloom_params_default()
        rec = None if record is None else np.ascontiguousarray(record, dtype=np.uint32)
        out = np.zeros((h, w, 3), np.float32)
        self.check(self.lib.mi355pt_bloom(f.ctypes.data, w, h, spp, C.byref(params), rec.ctypes.data if rec is not None else None, out.ctypes.data), "bloom")
        return out

    # ---- the robust film (include/mi355pt_robust.h): K bucket films, a per-pixel trimmed mean chosen by their Gini coefficient ----
    def robust_params_default(self):
        p = RobustParams()
        self.lib.mi355pt_robust_params_default(C.byref(p))
        return p

    def robust_params(self, mode="gmon", gini_scale=1.0):
        return RobustParams(ROBUST_MODE[mode], gini_scale)

    def robust_combine_device(self, d_buckets_ptr, n_buckets, spp_bucket, width, height, params, d_out_ptr, d_out_half_ptr=None, d_out_trim_ptr=None, stream=None):
        """mi355pt_robust_combine_device: d_out_half_ptr None or 0 = single output; d_out_trim_ptr None or 0 = not wanted"""
        self.check(self.lib.mi355pt_robust_combine_device(C.c_void_p(d_buckets_ptr), n_buckets, spp_bucket, width, height, C.byref(params), C.c_void_p(d_out_ptr),
                                                          C.c_void_p(d_out_half_ptr or 0), C.c_void_p(d_out_trim_ptr or 0), C.c_void_p(stream or 0)),
                   "robust_combine_device")

    def robust_combine(self, buckets, spp_bucket, params=None, pair=False, want_trim=True):
        """mi355pt_robust_combine on a host (K, H, W, 3) float32 stack of sums -> (out, out_half or None, trim (H, W, 2) uint8 or None)"""
        b = np.ascontiguousarray(buckets, dtype=np.float32)
        k, h, w = b.shape[:3]
        params = params if params is not None else self.robust_params_default()
        out = np.zeros((h, w, 3), np.float32)
        half = np.zeros((h, w, 3), np.float32) if pair else None
        trim = np.zeros((h, w, 2), np.uint8) if want_trim else None
        self.check(self.lib.mi355pt_robust_combine(b.ctypes.data, k, spp_bucket, w, h, C.byref(params), out.ctypes.data, half.ctypes.data if pair else None,
                                                   trim.ctypes.data if want_trim else None), "robust_combine")
        return out, half, trim

    def render_buckets_device(self, scene, cam, params, n_buckets, d_buckets_ptr, stream=None, stats=None):
        self.check(self.lib.mi355pt_render_buckets_device(scene.h, C.byref(cam), C.byref(params), n_buckets, C.c_void_p(d_buckets_ptr), C.c_void_p(stream or 0),
                                                          C.byref(stats) if stats is not None else None), "render_buckets_device")

    def render_robust(self, scene, cam, params, n_buckets, robust_params=None):
        """mi355pt_render_robust -> (H, W, 3) float32, tone-mapped and sRGB-encoded like render()"""
        rp = robust_params if robust_params is not None else self.robust_params_default()
        out = np.zeros((cam.height, cam.width, 3), np.float32)
        self.check(self.lib.mi355pt_render_robust(scene.h, C.byref(cam), C.byref(params), n_buckets, C.byref(rp), out.ctypes.data), "render_robust")
        return out

    def render_accum_device(self, scene, cam, params, s_begin, s_end, d_accum_ptr, stream=None, stats=None):
        self.check(self.lib.mi355pt_render_accum_device(scene.h, C.byref(cam), C.byref(params), s_begin, s_end, C.c_void_p(d_accum_ptr),
                                                        C.c_void_p(stream or 0), C.byref(stats) if stats is not None else None),
                   "render_accum_device")

    # ---- adaptive sampling (include/mi355pt_adaptive.h) and the tile-list render it is built on ----
    def render_accum_tiles_device(self, scene, cam, params, tiles, s_begin, s_end, d_accum_ptr, stream=None, stats=None):
        """mi355pt_render_accum_tiles_device: `tiles` is a host sequence of frame tile indices (strictly ascending)"""
        t = np.ascontiguousarray(tiles, dtype=np.uint32).reshape(-1)
        self.check(self.lib.mi355pt_render_accum_tiles_device(scene.h, C.byref(cam), C.byref(params), _ptr(t, C.c_uint32), t.size, s_begin, s_end,
                                                              C.c_void_p(d_accum_ptr), C.c_void_p(stream or 0),
                                                              C.byref(stats) if stats is not None else None), "render_accum_tiles_device")

    def adaptive_scratch_bytes(self, width, height):
        return int(self.lib.mi355pt_adaptive_scratch_bytes(width, height))

    def adaptive_step_device(self, d_film_ptr, d_half_ptr, width, height, d_tile_spp_ptr, d_tile_err_ptr, params, level_spp, max_spp, d_scratch_ptr,
                             scratch_bytes, d_list_ptr, d_count_ptr, stream=None):
        """mi355pt_adaptive_step_device on device pointers; asynchronous on `stream`"""
        self.check(self.lib.mi355pt_adaptive_step_device(C.c_void_p(d_film_ptr), C.c_void_p(d_half_ptr), width, height, C.c_void_p(d_tile_spp_ptr),
                                                         C.c_void_p(d_tile_err_ptr), C.byref(params), level_spp, max_spp, C.c_void_p(d_scratch_ptr),
                                                         scratch_bytes, C.c_void_p(d_list_ptr), C.c_void_p(d_count_ptr), C.c_void_p(stream or 0)),
                   "adaptive_step_device")

    def film_normalize_tiles_device(self, d_film_ptr, d_tile_spp_ptr, width, height, d_mean_ptr, stream=None):
        self.check(self.lib.mi355pt_film_normalize_tiles_device(C.c_void_p(d_film_ptr), C.c_void_p(d_tile_spp_ptr), width, height, C.c_void_p(d_mean_ptr),
                                                                C.c_void_p(stream or 0)), "film_normalize_tiles_device")

    def render_adaptive_device(self, scene, cam, params, adaptive, d_film_ptr, d_half_ptr, d_tile_spp_ptr, d_tile_err_ptr, d_list_ptr, d_scratch_ptr,
                               scratch_bytes, stream=None):
        """mi355pt_render_adaptive_device -> AdaptiveResult (passes, tiles_at_max, total_samples)"""
        res = AdaptiveResult()
        self.check(self.lib.mi355pt_render_adaptive_device(scene.h, C.byref(cam), C.byref(params), C.byref(adaptive), C.c_void_p(d_film_ptr),
                                                           C.c_void_p(d_half_ptr), C.c_void_p(d_tile_spp_ptr), C.c_void_p(d_tile_err_ptr),
                                                           C.c_void_p(d_list_ptr), C.c_void_p(d_scratch_ptr), scratch_bytes, C.c_void_p(stream or 0),
                                                           C.byref(res)), "render_adaptive_device")
        return res

    def render_adaptive(self, scene, cam, params, adaptive):
        """mi355pt_render_adaptive -> ((H, W, 3) float32 tone-mapped sRGB, (tiles_y, tiles_x) uint32 samples per tile, AdaptiveResult)"""
        out = np.zeros((cam.height, cam.width, 3), dtype=np.float32)
        spp = np.zeros(((cam.height + 7) // 8, (cam.width + 7) // 8), dtype=np.uint32)
        res = AdaptiveResult()
        self.check(self.lib.mi355pt_render_adaptive(scene.h, C.byref(cam), C.byref(params), C.byref(adaptive), _ptr(out, C.c_float),
                                                    _ptr(spp, C.c_uint32), C.byref(res)), "render_adaptive")
        return out, spp, res

    def render_sample_log(self, scene, cam, params, s_begin, s_end, want_accum=False):
        """mi355pt_render_sample_log: every finished path of the production launch(es) for [s_begin, s_end) of the shard in `params`.
        Returns L, lambda, pdf as (tiles_of_shard, 64, s_end - s_begin, 4) arrays (pixel (y & 7) * 8 + (x & 7) inside its 8x8 tile;
        tile k of the shard is frame tile shard_index + k * shard_count) and, on request, the (H, W, 3) linear film sums."""
        n = C.c_size_t()
        self.check(self.lib.mi355pt_sample_log_records(C.byref(cam), C.byref(params), s_begin, s_end, C.byref(n)), "sample_log_records")
        ns = s_end - s_begin
        shape = (n.value // (64 * ns), 64, ns, 4)
        L = np.zeros(shape, np.float32); lam = np.zeros(shape, np.float32); pdf = np.zeros(shape, np.float32)
        acc = np.zeros((cam.height, cam.width, 3), np.float32) if want_accum else None
        self.check(self.lib.mi355pt_render_sample_log(scene.h, C.byref(cam), C.byref(params), s_begin, s_end, _ptr(L, C.c_float),
                                                      _ptr(lam, C.c_float), _ptr(pdf, C.c_float), n.value, _ptr(acc, C.c_float)), "render_sample_log")
        return (L, lam, pdf, acc) if want_accum else (L, lam, pdf)

    def export_bvh(self, scene):
        """mi355pt_scene_export_bvh -> (nodes (n, 16) uint32 view of the 64-B records, tris (m, 12) uint32 view of the 48-B records, root)"""
        fn = self.lib.mi355pt_scene_export_bvh
        fn.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32), C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_int32)]
        nn, nt, root = C.c_uint32(0), C.c_uint32(0), C.c_int32(0)
        self.check(fn(scene.h, None, C.byref(nn), None, C.byref(nt), C.byref(root)), "scene_export_bvh")
        nodes = np.zeros((nn.value, 16), np.uint32); tris = np.zeros((nt.value, 12), np.uint32)
        self.check(fn(scene.h, nodes.ctypes.data, C.byref(nn), tris.ctypes.data, C.byref(nt), C.byref(root)), "scene_export_bvh")
        return nodes, tris, root.value

    def debug_sah_cost(self, nodes, root, entries):
        """mi355pt_debug_sah_cost (host only): the SAH cost of an exported BVH2 over the refit plan's entries, in the fixed order of
        csrc/instance_move_plan.hpp -> numpy float32"""
        fn = self.lib.mi355pt_debug_sah_cost
        fn.argtypes = [C.c_void_p, C.c_uint32, C.c_int32, C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_float)]
        nodes = np.ascontiguousarray(nodes, dtype=np.uint32).reshape(-1, 16); entries = np.ascontiguousarray(entries, dtype=np.uint32).reshape(-1)
        out = C.c_float(0.0)
        self.check(fn(nodes.ctypes.data_as(C.c_void_p), nodes.shape[0], root, _ptr(entries, C.c_uint32), entries.size, C.byref(out)), "debug_sah_cost")
        return np.float32(out.value)

    def probe_bvh_collapse(self, tri_pos, rays_od):
        """mi355pt_probe_bvh_collapse (host-only) -> (info dict, rays whose leaf sets differ between the BVH2 and the collapsed BVH4)"""
        tri = np.ascontiguousarray(tri_pos, dtype=np.float32).reshape(-1, 9); rays = np.ascontiguousarray(rays_od, dtype=np.float32).reshape(-1, 6)
        info = np.zeros(4, np.uint32); mism = C.c_uint32(0)
        fn = self.lib.mi355pt_probe_bvh_collapse
        fn.argtypes = [C.POINTER(C.c_float), C.c_uint32, C.POINTER(C.c_float), C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        self.check(fn(_ptr(tri, C.c_float), tri.shape[0], _ptr(rays, C.c_float), rays.shape[0], _ptr(info, C.c_uint32), C.byref(mism)), "probe_bvh_collapse")
        return dict(nodes2=int(info[0]), nodes4=int(info[1]), depth2=int(info[2]), max_stack4=int(info[3])), mism.value

    def probe_bvh_collapse_nodes(self, nodes, root, n_tris):
        """mi355pt_probe_bvh_collapse_nodes (host-only): the collapse + validation SceneImpl::build runs, on a caller-supplied BVH2
        ((n, 16) uint32 view of the 64-B records, as export_bvh returns).  Raises RuntimeError when the tree is refused."""
        nodes = np.ascontiguousarray(nodes, dtype=np.uint32).reshape(-1, 16)
        info = np.zeros(4, np.uint32)
        fn = self.lib.mi355pt_probe_bvh_collapse_nodes
        fn.argtypes = [C.c_void_p, C.c_uint32, C.c_int32, C.c_uint32, C.POINTER(C.c_uint32)]
        self.check(fn(nodes.ctypes.data, nodes.shape[0], root, n_tris, _ptr(info, C.c_uint32)), "probe_bvh_collapse_nodes")
        return dict(nodes2=int(info[0]), nodes4=int(info[1]), dp=bool(info[2]), max_stack4=int(info[3]))

    def coat_albedo_table(self, alpha, r0):
        """mi355pt_coat_albedo_table: the 64-entry E(cos theta) table behind params.albedo_lut (host-only)."""
        out = np.zeros(64, np.float32)
        self.lib.mi355pt_coat_albedo_table.argtypes = [C.c_float, C.c_float, C.POINTER(C.c_float)]
        self.check(self.lib.mi355pt_coat_albedo_table(alpha, r0, _ptr(out, C.c_float)), "coat_albedo_table")
        return out

    def build_multi(self, scene, cam, device_ids):
        """mi355pt_scene_build_multi: replicate the (described, not yet built) scene on the listed devices."""
        ids = (C.c_int * len(device_ids))(*device_ids)
        self.lib.mi355pt_scene_build_multi.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_int, C.POINTER(C.c_int)]
        self.check(self.lib.mi355pt_scene_build_multi(scene.h, C.byref(cam), len(device_ids), ids), "scene_build_multi")

    def render_multi(self, scene, cam, params):
        """mi355pt_render_multi -> (H, W, 3) float32, the frame mi355pt_render returns, rendered by all devices of the scene."""
        out = np.zeros((cam.height, cam.width, 3), dtype=np.float32)
        self.lib.mi355pt_render_multi.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(Params), C.POINTER(C.c_float)]
        self.check(self.lib.mi355pt_render_multi(scene.h, C.byref(cam), C.byref(params), _ptr(out, C.c_float)), "render_multi")
        return out

    def film_resolve_device(self, d_accum_ptr, n_pixels, spp, d_out_ptr, stream=None):
        self.check(self.lib.mi355pt_film_resolve_device(C.c_void_p(d_accum_ptr), n_pixels, spp, C.c_void_p(d_out_ptr),
                                                        C.c_void_p(stream or 0)), "film_resolve_device")
