"""Roulette-doomed paths ended before their last ray is traced (csrc/path_end_plan.hpp, pt_kernel_body.inc EARLY PATH END) against the same
library with MI355PT_NO_EARLY_PATH_END=1, which takes the same decision in the same place — the roulette draw made by the pass that spawned
the ray — and traces every ray.  A skipped ray is one the sample's L cannot depend on, so the per-sample logs (L, lambda, pdf of every
finished path) must be equal as bit patterns.  A pixel's samples reach the film tile in another order, so each film is held to ITS OWN log
within the bound of tests/test_film_log_gpu.py, (n_s + K) u A_pixel (1 + 1e-3) + 1e-37 (sensor_reference.reconcile_bound).  The values are tied
to the builds before this change by tests/test_tail_queue_order_gpu.py's recorded digests, which both settings of the switch must keep.

Every case renders 64 x 48 in four launch shapes: sample indices [0, 64) and [64, 128) of a 1 024-spp job (8x8 items), [0, 256) of it
(4x4 items), and the whole job of a 64-spp render.

The count (mi355pt_stats.wave_steps[7] of a production launch that is given a stats block, the debug switch on as in the whole suite) shows
that rays are skipped at all: 0 with the switch set or with an environment light in the scene; on scene 3 under MIS at least 0.25 of the
`bounces` an instrumented launch (collect_stats = 2) of the same shape counts — the oracle, instrumented on the CPU at 240 x 135, finds 0.347
of all bounce rays doomed and out of the emitter's reach; the margin is for the small frame —; with max_depth = 1, where every bounce ray is
doomed by its depth, at least 0.9 of them."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sensor_reference as sr  # noqa: E402
from test_deform import EMITTER3, Remeshed, deformed  # noqa: E402
from test_film_log import K_ROUNDINGS  # noqa: E402
from test_instance_move import applied, describe, trs  # noqa: E402
from test_rebase import moved  # noqa: E402
from test_rebase_gpu import STEP  # noqa: E402

pytestmark = pytest.mark.gpu

TEX_SIZE = 128
SWITCH = "MI355PT_NO_EARLY_PATH_END"
W, H = 64, 48
# (spp, sample range)
SHAPES = [(1024, (0, 64)), (1024, (64, 128)), (1024, (0, 256)), (64, (0, 64))]
FEAT_ENV = 128
EMITTER_I = EMITTER3[1]

# name: (scene, strategy, sampler, max_depth, rr_gate_slack, what happens to the built scene, smallest count / bounces or None)
CASES = {
    "scene3_mis_sobol": (3, "mis", "sobol", 16, 0.0, None, 0.25),
    "scene3_nee_sobol": (3, "nee", "sobol", 16, 0.0, None, None),
    "scene3_mis_random": (3, "mis", "random", 16, 0.0, None, None),             # the generic mode's kernel
    "scene3_depth1": (3, "mis", "sobol", 1, 0.0, None, 0.9),
    "scene3_depth2": (3, "mis", "sobol", 2, 0.0, None, None),
    "scene3_rr_slack": (3, "mis", "sobol", 16, 0.25, None, None),
    "scene11_mis": (11, "mis", "sobol", 16, 0.0, None, None),                   # rough glass: NaN samples, the zero-term rule
    "scene8_mis": (8, "mis", "sobol", 16, 0.0, None, None),                     # smooth glass: specular samples
    "scene29_mis": (29, "mis", "sobol", 16, 0.0, None, None),                   # several lights, two of them environment lights: no skip
    "scene31_mis": (31, "mis", "sobol", 16, 0.0, None, None),                   # a textured emitter: the all-features kernel (two queues), no early end
    "scene19_mis": (19, "mis", "sobol", 16, 0.0, None, None),                   # an environment light: no skip
    "scene21_mis": (21, "mis", "sobol", 16, 0.0, None, None),                   # delta lights beside the area light: empty boxes in the list
    "scene0_two_area_lights": (0, "mis", "sobol", 16, 0.0, "two_lights", 0.2),   # a second emitter: two boxes, both tested by every doomed ray
    "scene3_tiles": (3, "mis", "sobol", 16, 0.0, "tiles", None),
    "scene3_camera_move": (3, "mis", "sobol", 16, 0.0, "camera", None),
    "scene3_emitter_move": (3, "mis", "sobol", 16, 0.0, "instance", None),
    "scene3_emitter_deform": (3, "mis", "sobol", 16, 0.0, "deform", None),
}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def accum(product, pkg, sc, cam, prm, rng, tiles=False):
    """the film sums of one production launch and the rays it skipped (wave_steps[7])"""
    import torch
    a = torch.zeros((cam.height, cam.width, 3), dtype=torch.float32, device="cuda")
    st = pkg.ffi.Stats()
    if tiles:
        n_tiles = ((cam.width + 7) // 8) * ((cam.height + 7) // 8)
        product.render_accum_tiles_device(sc, cam, prm, np.arange(n_tiles, dtype=np.uint32), rng[0], rng[1], a.data_ptr(), None, st)
    else:
        product.render_accum_device(sc, cam, prm, rng[0], rng[1], a.data_ptr(), None, st)
    torch.cuda.synchronize()
    return a.cpu().numpy(), int(st.wave_steps[7])


def bounces(product, pkg, sc, cam, prm, rng):
    """the bounce rays an instrumented launch of the same shape counts"""
    import torch
    a = torch.zeros((cam.height, cam.width, 3), dtype=torch.float32, device="cuda")
    st = pkg.ffi.Stats()
    q = pkg.ffi.Params.from_buffer_copy(prm)
    q.collect_stats = 2
    product.render_accum_device(sc, cam, q, rng[0], rng[1], a.data_ptr(), None, st)
    torch.cuda.synchronize()
    return int(st.bounces)


def own_log_reference(pkg, prm, log):
    """what the film of a log's launch must hold: per pixel of the frame the sum of the log's sensor responses and the pixel's absolute mass"""
    L, lam, pdf = log
    tiles_x = (W + 7) // 8
    tiles, pix = np.arange(L.shape[0]), np.arange(64)
    xs = (tiles % tiles_x)[:, None] * 8 + (pix % 8)[None, :]
    ys = (tiles // tiles_x)[:, None] * 8 + (pix // 8)[None, :]
    inside = (xs < W) & (ys < H)
    value, mass = sr.sensor_reference(L[inside], lam[inside], pdf[inside], pkg.scenes.cmf_xyz(), exposure=prm.exposure)
    with np.errstate(invalid="ignore"):
        return xs[inside], ys[inside], value.sum(axis=1), mass.sum(axis=1)


def own_log_residual(ref, film, n_s):
    """(largest |film - reference| in units of u A_pixel, all within the bound?, pixels left out) over the pixels whose samples are finite"""
    xs, ys, want, a_pixel = ref
    got = film[ys, xs].astype(np.float64)
    bad = ~np.isfinite(want)
    assert not np.isfinite(got[bad]).any(), "a non-finite sample left its pixel's film finite"
    keep = ~bad.any(axis=1)
    resid = np.abs(got[keep] - want[keep])
    bound = sr.reconcile_bound(n_s, K_ROUNDINGS, a_pixel[keep])
    units = resid / (sr.U * np.maximum(a_pixel[keep], 1e-300))
    return float(units.max()), bool((resid <= bound).all()), int((~keep).sum())


def build_case(product, pkg, scene_id, what):
    """(scene, camera) built, and updated in place when the case says so"""
    if what in ("camera", "instance", "deform"):
        sc, cam = describe(pkg, Remeshed(product), str(scene_id), dynamic=[EMITTER_I])
        sc.build(cam)
        if what == "camera":
            cam = moved(pkg, cam, STEP)
            res = sc.move_camera(cam)
        elif what == "instance":
            res = sc.move_instances(cam, [EMITTER_I], [applied(trs((0.3, -0.2, 0.45), 0.4, (1.1, 0.9, 1.0)), sc.instances[EMITTER_I][2])])
        else:
            res = sc.deform_meshes(cam, {EMITTER_I: deformed(sc.meshes[EMITTER_I], amp=0.2)})
        assert res["rebuilt"] == 0, res                     # in place: the boxes were rewritten by the update step, not by an upload
        return sc, cam
    sc = product.new_scene()
    if what == "two_lights":
        # the room's ceiling light and an upright panel beside the hero, facing the room: no environment light, two area lights
        from importlib import import_module
        ffi, assets = pkg.ffi, import_module(pkg.__name__ + ".assets")
        cam = pkg.scenes.load_scene(sc, scene_id, W, H, tex_size=TEX_SIZE, build=False)
        panel = assets.load_obj_semantics(dict(pos=np.array([[-1.5, 0.8, -0.5], [-1.5, 0.8, 0.5], [-1.5, 1.8, 0.5], [-1.5, 1.8, -0.5]], np.float32),
                                               nrm=np.array([[1, 0, 0]] * 4, np.float32), uv=np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32),
                                               idx=np.array([[0, 1, 2], [0, 2, 3]], np.uint32)))
        em = ffi.MaterialDesc(); em.type = ffi.MAT_EMISSIVE; em.normal_tex = ffi.NONE; em.intensity = 4.0
        em.color = pkg.scenes.Spectrum.lut(sc.add_lut470(pkg.scenes.presets()["cie_illum_d6500"]))
        sc.add_instance(sc.add_mesh(panel), sc.add_material(em))
        sc.build(cam)
        return sc, cam
    return sc, pkg.scenes.load_scene(sc, scene_id, W, H, tex_size=TEX_SIZE)


@pytest.mark.parametrize("name", list(CASES))
def test_skipping_doomed_rays_leaves_every_sample_as_it_was(product, pkg, monkeypatch, name):
    scene_id, strategy, sampler, max_depth, slack, what, least = CASES[name]
    sc, cam = build_case(product, pkg, scene_id, what)
    has_env = (int(re.search(r"features=(\d+)", product.scene_info(sc)).group(1)) & FEAT_ENV) != 0
    for spp, rng in SHAPES:
        n_s = rng[1] - rng[0]
        prm = pkg.make_params(spp, strategy, sampler, max_depth=max_depth, rr_gate_slack=slack)
        monkeypatch.setenv(SWITCH, "1")
        *ref_log, ref_film = product.render_sample_log(sc, cam, prm, rng[0], rng[1], want_accum=True)
        ref_accum, ref_count = accum(product, pkg, sc, cam, prm, rng, tiles=what == "tiles")
        monkeypatch.delenv(SWITCH)
        *log, film = product.render_sample_log(sc, cam, prm, rng[0], rng[1], want_accum=True)
        new_accum, count = accum(product, pkg, sc, cam, prm, rng, tiles=what == "tiles")
        n_bounce = bounces(product, pkg, sc, cam, prm, rng)
        assert ref_log[0].shape[1:] == (64, n_s, 4)
        # the samples
        for field, a, b in zip(("L", "lambda", "pdf"), ref_log, log):
            assert np.array_equal(bits(a), bits(b)), f"{name} {spp} {rng} {field}: {int((bits(a) != bits(b)).sum())} values differ"
        # every film against its own log — one reference: the two logs have just been found equal bit for bit.  (The tile-list entry point
        # has no log: its film is held to the shard launch's.)
        reference = own_log_reference(pkg, prm, log)
        worst = 0.0
        for which, f in (("switch set", ref_film), ("switch unset", film), ("switch set, counted launch", ref_accum), ("switch unset, counted launch", new_accum)):
            units, ok, left_out = own_log_residual(reference, f, n_s)
            worst = max(worst, units)
            assert ok, f"{name} {spp} {rng} {which}: largest difference {units:.2f} u A, bound {n_s + K_ROUNDINGS}"
        assert float(np.nan_to_num(film).mean()) > 0.0
        print(f"{name} spp {spp} range {rng}: skipped {count} of {n_bounce} bounce rays ({count / max(n_bounce, 1):.3f}), with the switch {ref_count}; "
              f"films within {worst:.2f} u A of their logs (bound {n_s + K_ROUNDINGS}), {left_out} pixels with a non-finite sample")
        # the count
        assert ref_count == 0
        if has_env:
            assert count == 0
        if least is not None:
            assert count >= least * n_bounce, (count, n_bounce)
        if what in ("camera", "instance", "deform", "tiles", "two_lights"):
            assert count > 0                                  # the moved emitter's box still turns rays away; the tile-list kernel counts too
