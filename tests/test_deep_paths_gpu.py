"""Deep paths (max_depth up to the 1000 that mi355pt_params accepts) and the instrumented kernels' films, against the oracle.

Every other parity test renders at max_depth <= 16, where a path's sampler dimensions stay inside the kernels' 136-entry murmur table and
Sobol prefix tables (csrc/layout.hpp HASH_TABLE_DIMS) and its depth inside 8 bits.  Scenes 34-36 (scenes.py) are a closed box of white
Lambert walls (albedo exactly 1: no roulette) with a small emitter, so that paths bounce tens to hundreds of times; 35 adds a spectrum
texture on the floor (the class the collect_stats = 2 kernel defers), 36 a clearcoat block (the clearcoat kernels).
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

from test_parity_gpu import FRAME_BAR

pytestmark = pytest.mark.gpu

ORACLE_THREADS = min(os.cpu_count() or 1, 16)
DEEP_SCENES = (34, 35, 36)
# Bars, from one measured run of every case below (the frame bar of test_parity_gpu.FRAME_BAR holds unchanged for deep paths):
#   frames, 46 scene / strategy / depth cases up to depth 1000: RMSE 2.6e-8 ... 6.0e-8, no pixel off by 0.01;
#   per-sample radiance at depth 300: 180 000 of 180 000 samples within 1e-3 (no roulette gate flipped after hundreds of bounces), so the
#   bar is PER_SAMPLE_MIN's 0.9995;
#   instrumented films: collect_stats = 2 (production-form traversal) differs from the production film by the summation order only, at most
#   1.24e-5 of a pixel (scene 30) -> bar 5e-5, and its bounce count equals the oracle's exactly in every case.  collect_stats = 1 walks the
#   BVH2 with plain per-lane traversals, which resolve a ray through a shared edge of two triangles differently now and then (scene 34: the
#   emitter's border with the ceiling): pixels up to 0.022 apart, film sums 3.6e-6, bounces 4.1e-6 (50 of 12.1 M) -> bars 0.05 / 2e-5 / 1e-5.
#   The depth wrap of the deferral record (fixed) showed as +786 / +1 315 bounces and pixels 0.15 / 0.11 apart on scene 35 at depth 256 / 300.
DEEP_PER_SAMPLE_MIN = 0.9995
STATS2_FILM_REL = 5e-5
STATS1_FILM_REL, STATS1_SUM_REL, STATS1_BOUNCES_REL = 0.05, 2e-5, 1e-5


def _log(rec):
    if os.environ.get("MI355PT_DEEP_LOG"):
        with open(os.environ["MI355PT_DEEP_LOG"], "a") as f:
            f.write(json.dumps(rec) + "\n")


def _pair(product, oracle, pkg, scene_id, w, h, tex_size=128):
    out = {}
    for name, be in (("gpu", product), ("cpu", oracle)):
        sc = be.new_scene()
        out[name] = (sc, pkg.scenes.load_scene(sc, scene_id, w, h, tex_size=tex_size))
    oracle.set_faithful(out["cpu"][0], False)
    return out


def _frame_diff(g, c):
    with np.errstate(invalid="ignore"):
        assert np.array_equal(np.isnan(g), np.isnan(c))
        d = np.nan_to_num(g - c)
    return float(np.sqrt(np.mean(d ** 2))), int((np.abs(d).max(axis=2) > 0.01).sum())


DEEP_FRAME_CASES = [(s, st, "sobol", d) for s in DEEP_SCENES for st in ("pt", "nee", "mis") for d in (17, 255, 256, 300, 1000)] + \
                   [(34, "mis", "random", 300)]


@pytest.mark.parametrize("scene_id,strategy,sampler,max_depth", DEEP_FRAME_CASES)
def test_deep_frames_match_the_oracle(product, oracle, pkg, scene_id, strategy, sampler, max_depth):
    """Depth 17 is the first whose sampler dimensions pass the 136-entry tables (device murmur hash, full-length Sobol digit loop); 255 / 256
    straddle an 8-bit depth; 1000 is the largest depth the library accepts.  Same paths on both sides: the frame-test bar."""
    w, h, spp = (32, 24, 16) if max_depth == 1000 else (64, 48, 16)
    pair = _pair(product, oracle, pkg, scene_id, w, h)
    prm = pkg.make_params(spp, strategy, sampler, max_depth=max_depth)
    g = product.render(pair["gpu"][0], pair["gpu"][1], prm)
    c = oracle.render(pair["cpu"][0], pair["cpu"][1], prm, threads=ORACLE_THREADS)
    rmse, off = _frame_diff(g, c)
    _log(dict(test="frame", scene=scene_id, strategy=strategy, sampler=sampler, max_depth=max_depth, rmse=rmse, off=off, mean=float(c.mean())))
    assert c.mean() > 0.05
    assert rmse <= FRAME_BAR[0] and off <= FRAME_BAR[1], (rmse, off)


@pytest.mark.parametrize("scene_id,strategy", [(s, st) for s in DEEP_SCENES for st in ("pt", "nee", "mis")])
def test_deep_per_sample_radiance(product, oracle, pkg, scene_id, strategy):
    """Per-sample spectral radiance at max_depth = 300 (the per-sample log of the production launch against the oracle's trace):
    wavelengths and their pdfs bit-equal, the radiance within 1e-3 for DEEP_PER_SAMPLE_MIN of the samples."""
    w, h, spp = 64, 48, 64
    pair = _pair(product, oracle, pkg, scene_id, w, h)
    rng = np.random.default_rng(1000 + scene_id)
    n = 20000
    xys = np.stack([rng.integers(0, w, n), rng.integers(0, h, n), rng.integers(0, spp, n)], 1).astype(np.uint32)
    prm = pkg.make_params(spp, strategy, "sobol", max_depth=300)
    Lg, lg, pg = pair["gpu"][0].probe_radiance(pair["gpu"][1], prm, xys)
    Lc, lc, pc = pair["cpu"][0].probe_radiance(pair["cpu"][1], prm, xys)
    assert np.array_equal(lg, lc) and np.array_equal(pg, pc)
    close = np.all(np.abs(Lg - Lc) <= 1e-3 * np.abs(Lc) + 1e-4, axis=1)
    _log(dict(test="per_sample", scene=scene_id, strategy=strategy, close=float(close.mean()), n_far=int((~close).sum()),
              far=xys[~close][:8].tolist()))
    assert close.mean() >= DEEP_PER_SAMPLE_MIN, close.mean()
    assert abs(float(Lg.mean()) - float(Lc.mean())) <= 1e-3 * float(Lc.mean())


def _accum(product, pkg, pair, prm, spp, stats=None):
    import torch
    cam = pair["gpu"][1]
    a = torch.zeros((cam.height, cam.width, 3), dtype=torch.float32, device="cuda")
    product.render_accum_device(pair["gpu"][0], cam, prm, 0, spp, a.data_ptr(), None, stats=stats)
    torch.cuda.synchronize()
    return a.cpu().numpy()


# (scene, max_depth): the scenes of both instrumented instantiations and of the deferred classes (textured Lambert: 3; clearcoat: 17, 19;
# the textured emitter: 30), and the textured deep box past depth 256, where the deferral record used to wrap the depth at 8 bits
STATS_CASES = [(0, 16), (3, 16), (17, 16), (19, 16), (30, 16), (35, 256), (35, 300), (34, 300)]


@pytest.mark.parametrize("collect_stats", [1, 2])
@pytest.mark.parametrize("scene_id,max_depth", STATS_CASES)
def test_instrumented_kernels_render_the_production_frame(product, oracle, pkg, scene_id, max_depth, collect_stats):
    """collect_stats = 1 (canonical traversal) and = 2 (production-form traversal, deferral on) run instantiations of their own, with their
    own shading stage (no tail queue), and bench.py --full builds its byte model from their counters.  Their film must be the production
    film of the same arguments up to the float summation order inside a pixel (the order in which a tile's paths finish; collect_stats = 1
    also up to its own tie-breaking, see the bars above), their sample count W*H*spp, and their bounce count the oracle's for the same
    samples — a path that came back from a queue with a wrong depth runs past max_depth and adds bounces whatever the image noise."""
    w, h, spp = 64, 48, 64
    pair = _pair(product, oracle, pkg, scene_id, w, h)
    prm0 = pkg.make_params(spp, "mis", "sobol", max_depth=max_depth)
    ref = _accum(product, pkg, pair, prm0, spp)
    st = pkg.ffi.Stats()
    film = _accum(product, pkg, pair, pkg.make_params(spp, "mis", "sobol", max_depth=max_depth, collect_stats=collect_stats), spp, stats=st)
    g = st.as_dict()
    oracle.counters(pair["cpu"][0], reset=True)
    oracle.render_accum(pair["cpu"][0], pair["cpu"][1], prm0, 0, spp, threads=ORACLE_THREADS, counters=True)
    c = oracle.counters(pair["cpu"][0])
    rel = np.abs(film - ref) / (np.abs(ref) + 1e-3 * spp)
    _log(dict(test="stats", scene=scene_id, max_depth=max_depth, collect_stats=collect_stats, film_max_rel=float(rel.max()),
              film_equal=bool(np.array_equal(film, ref)), bounces_gpu=int(g["bounces"]), bounces_oracle=int(c["bounces"]),
              samples=int(g["samples"]), film_sum=float(film.sum()), ref_sum=float(ref.sum())))
    assert g["samples"] == c["samples"] == w * h * spp
    assert np.isfinite(ref).all() and ref.mean() > 0.01 * spp
    if collect_stats == 2:
        assert float(rel.max()) <= STATS2_FILM_REL, float(rel.max())
        assert g["bounces"] == c["bounces"], (g["bounces"], c["bounces"])
    else:
        assert float(rel.max()) <= STATS1_FILM_REL, float(rel.max())
        assert abs(float(film.sum()) - float(ref.sum())) <= STATS1_SUM_REL * float(ref.sum())
        assert abs(int(g["bounces"]) - int(c["bounces"])) <= STATS1_BOUNCES_REL * c["bounces"], (g["bounces"], c["bounces"])


def test_depth_zero_sees_only_emission(product, oracle, pkg):
    """max_depth = 0: the camera ray's own hit and nothing else — in the deep box a black frame but for the emitter."""
    pair = _pair(product, oracle, pkg, 34, 64, 48)
    prm = pkg.make_params(16, "mis", "sobol", max_depth=0)
    g = product.render(pair["gpu"][0], pair["gpu"][1], prm)
    c = oracle.render(pair["cpu"][0], pair["cpu"][1], prm, threads=ORACLE_THREADS)
    rmse, off = _frame_diff(g, c)
    assert rmse <= FRAME_BAR[0] and off <= FRAME_BAR[1], (rmse, off)
    lit = (c > 0).any(axis=2)
    assert 0 < lit.sum() < 0.1 * lit.size                                  # the emitter covers a few percent of the frame
    assert not g[~lit].any() and (g[lit].max(axis=1) > 0).all()


def test_max_depth_limit(product, pkg):
    """1000 is accepted, 1001 is refused with MI355PT_E_INVALID (include/mi355pt.h)."""
    sc = product.new_scene()
    cam = pkg.scenes.load_scene(sc, 34, 16, 16)
    out = np.zeros((16, 16, 3), np.float32)
    fn = product.lib.mi355pt_render
    for depth, rc in ((1000, 0), (1001, -1)):
        got = fn(sc.h, C.byref(cam), C.byref(pkg.make_params(4, "mis", "sobol", max_depth=depth)), out.ctypes.data_as(C.POINTER(C.c_float)), None)
        assert got == rc, (depth, got)
    assert np.isfinite(out).all()
