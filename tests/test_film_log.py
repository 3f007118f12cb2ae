"""What tests/test_film_log_gpu.py judges the path kernels' films with, made trustworthy without a GPU.

a. tests/sensor_reference.py (the float64 restatement of Sensor::add_sample) against the oracle's Sensor: the oracle's film is the per-pixel
   sum of sensor_reference over the oracle's own per-sample radiance, to the bound derived in test_film_log_gpu.py.
b. The f32 XYZ -> sRGB matrix of csrc/launch_plan.hpp (what film_rgb multiplies with) against the float64 matrix, entry by entry: the `m` of
   the bound's K = 11 + m.
c. The launch-shape cases of test_film_log_gpu.py (SHAPE_CASES, below) reach every pixel-block size, split and unsplit sample ranges and a
   job of two launches, for every plausible count of resident waves: the GPU test cannot silently stop exercising a shape when
   plan_launch changes."""
import os
import subprocess

import numpy as np
import pytest

import sensor_reference as sr
from test_launch_plan import planner  # noqa: F401  (the host plan checker, tests/launch_plan_check.cpp, as a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANDOM, SOBOL = 0, 1

# b: every entry of the f32 matrix lies within M_MATRIX * u * |M64| of the float64 one.  The measured deviation rounded up to the next integer:
M_MATRIX = 15                                # measured 14.39 (entry [2][0]; the others 0.57 ... 10.86): two f32 3x3 inversions
# roundings of film_rgb on a term of a sample's absolute mass (11, counted in test_film_log_gpu.py's docstring) + the matrix
K_ROUNDINGS = 11 + M_MATRIX

# ---- c: the launch shapes of test_film_log_gpu.test_launch_shapes_reconcile ----
FRAME_W, FRAME_H = 44, 20                    # 6 x 3 tiles, ragged right (4 of 8 columns) and bottom (4 of 8 rows)
# the sparse shard of the long ranges: frame tiles 3, 10 and 17 — two whole tiles and the 4 x 4 corner tile, ragged on both sides
SPARSE = (3, 7)                              # (shard_index, shard_count)
WHOLE = (0, 1)
# (id, width, height, spp, begin, end, sampler, exposure, (shard_index, shard_count), block_log2 of every launch or None, other)
SHAPE_CASES = [
    ("spp8", FRAME_W, FRAME_H, 8, 0, 8, "sobol", 1.0, WHOLE, 3, "unsplit"),
    ("spp128-offset", FRAME_W, FRAME_H, 128, 24, 88, "sobol", 1.0, WHOLE, 3, ""),
    ("spp256", FRAME_W, FRAME_H, 256, 0, 256, "sobol", 1.0, SPARSE, 2, ""),
    ("spp1024", FRAME_W, FRAME_H, 1024, 0, 1024, "sobol", 1.0, SPARSE, 1, ""),
    # single-pixel work items.  (Whether they also take the sample-prefix tables depends on the chunk size, i.e. on the resident waves of
    # the device: sample_prefix_digits > 0 needs chunks of 4^m >= 64 samples — 256 waves give that here, 512 and more do not.  The true-size
    # configs of test_parity_gpu.py reach them.)
    ("spp4096", FRAME_W, FRAME_H, 4096, 0, 4096, "sobol", 1.0, SPARSE, 0, ""),
    # a range of 200 indices across sample index 4096 is ONE launch (for_each_launch_range only breaks up ranges longer than 4096) ...
    ("spp8192-straddle", FRAME_W, FRAME_H, 8192, 4000, 4200, "sobol", 1.0, SPARSE, 2, ""),
    # ... so the job of two launches that accumulate into one film is the same begin with a long range: [4000, 4096) then [4096, 8192)
    ("spp8192-two-launches", FRAME_W, FRAME_H, 8192, 4000, 8192, "sobol", 1.0, SPARSE, None, "two launches"),
    ("spp256-random", FRAME_W, FRAME_H, 256, 0, 256, "random", 1.0, SPARSE, 3, ""),
    ("spp64-exposure", FRAME_W, FRAME_H, 64, 0, 64, "sobol", 0.37, WHOLE, 3, ""),
    ("spp64-8x8", 8, 8, 64, 0, 64, "sobol", 1.0, WHOLE, 3, ""),
    ("spp64-9x1", 9, 1, 64, 0, 64, "sobol", 1.0, WHOLE, 3, ""),
]
SHAPE_IDS = [c[0] for c in SHAPE_CASES]
# scene 3: the TEX class under mis / sobol; scene 17: the clearcoat class under nee / sobol (the `random` case keeps the strategy)
SHAPE_SCENES = [(3, "mis"), (17, "nee")]
WAVE_COUNTS = [256 << i for i in range(7)]   # 256 ... 16384 resident waves (a MI355X holds 256 CUs x 4 SIMDs x 3-4 waves of these kernels)


def shard_tiles(w, h, shard):
    """frame tile indices of the shard, in the log's order"""
    return np.arange(shard[0], ((w + 7) // 8) * ((h + 7) // 8), shard[1])


def test_shape_cases_cover_the_launch_shapes(planner):  # noqa: F811
    assert WAVE_COUNTS[0] == 256 and WAVE_COUNTS[-1] == 16384
    tiles = shard_tiles(FRAME_W, FRAME_H, SPARSE)
    assert list(tiles) == [3, 10, 17]                                           # 2-3 tiles, one of them ragged
    for waves in WAVE_COUNTS:
        plans = planner([(w, h, spp, SOBOL if sampler == "sobol" else RANDOM, shard[0], shard[1], b, e, waves, 0)
                         for _, w, h, spp, b, e, sampler, _, shard, _, _ in SHAPE_CASES])
        blocks, split, unsplit, two = set(), False, False, False
        for case, (n_tiles, launches) in zip(SHAPE_CASES, plans):
            name, w, h, spp, b, e, sampler, _, shard, block_log2, other = case
            assert n_tiles == len(shard_tiles(w, h, shard)), (waves, name)
            assert launches[0]["begin"] == b and launches[-1]["end"] == e, (waves, name)
            for r in launches:
                blocks.add(r["block_log2"])
                split |= r["chunks"] > 1
                unsplit |= r["chunks"] == 1
                if block_log2 is not None:
                    assert r["block_log2"] == block_log2, (waves, name, r)
            if other == "unsplit":
                assert len(launches) == 1 and launches[0]["chunks"] == 1, (waves, name, launches)
            if other == "two launches":
                assert [(r["begin"], r["end"]) for r in launches] == [(4000, 4096), (4096, 8192)], (waves, name)
                assert [r["block_log2"] for r in launches] == [3, 0], (waves, name)
                two = True
            else:
                assert len(launches) == 1, (waves, name)
        assert blocks == {0, 1, 2, 3} and split and unsplit and two, (waves, blocks, split, unsplit, two)


# ---- b ----
@pytest.fixture(scope="module")
def f32_matrices(tmp_path_factory):
    """tests/srgb_matrix_check.cpp built with plain g++ and run: {"product": (3, 3) f32 row-major, "oracle": the oracle's}"""
    exe = str(tmp_path_factory.mktemp("film_log") / "srgb_matrix_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "toy-cpu-pathtracing_amd", "csrc"),
                    "-I", os.path.join(ROOT, "oracle"), "-o", exe, os.path.join(ROOT, "tests", "srgb_matrix_check.cpp")], check=True)
    out = {}
    for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines():
        tag, *vals = line.split()
        out[tag] = np.array(vals, dtype=np.float32).reshape(3, 3)
    return out


def test_float64_matrix_is_the_srgb_matrix():
    """the derivation itself: white (D65 at Y = 1) maps to RGB (1, 1, 1), each primary to its own axis, and the rows are the published
    IEC 61966-2-1 matrix to its four printed decimals"""
    M = sr.xyz_to_srgb()

    def xyz(x, y):
        return np.array([x / y, 1.0, (1.0 - x - y) / y])
    assert np.allclose(M @ xyz(0.3127, 0.3290), 1.0, rtol=0, atol=1e-14)
    for ch, (x, y) in enumerate(((0.64, 0.33), (0.30, 0.60), (0.15, 0.06))):
        rgb = M @ xyz(x, y)
        assert rgb[ch] > 0 and np.allclose(np.delete(rgb, ch), 0.0, rtol=0, atol=1e-14)
    published = np.array([[3.2406, -1.5372, -0.4986], [-0.9689, 1.8758, 0.0415], [0.0557, -0.2040, 1.0570]])
    assert np.abs(M - published).max() < 5e-4                                   # (the standard rounds its own primaries' matrix)


def test_f32_matrix_is_within_m_roundings_of_the_float64_matrix(f32_matrices):
    M64 = sr.xyz_to_srgb()
    M32 = f32_matrices["product"].astype(np.float64)
    dev = np.abs(M32 - M64) / (sr.U * np.abs(M64))
    print("deviation of the f32 matrix in units of u * |M64|:\n", dev)
    assert dev.max() <= M_MATRIX, dev
    assert M_MATRIX - 1 < dev.max()                                             # M_MATRIX is the measured value rounded up, not a loose cap
    # the oracle's Sensor multiplies with the same nine floats: (a) below judges it with the same K
    assert np.array_equal(f32_matrices["oracle"].view(np.uint32), f32_matrices["product"].view(np.uint32))


# ---- a ----
def test_absolute_mass_bounds_the_value():
    rng = np.random.default_rng(7)
    L = rng.standard_normal((500, 4)) * 3.0                                     # (negative radiance too: the mass is of magnitudes)
    lam = rng.uniform(360.0, 830.0, (500, 4))
    pdf = np.full((500, 4), 1.0 / 470.0)
    pdf[::3, 1:] = 0.0
    pdf[::3, 0] /= 4.0
    cmf = np.abs(rng.standard_normal((3, 470))).astype(np.float32)
    v, a = sr.sensor_reference(L, lam, pdf, cmf, exposure=0.5)
    assert (np.abs(v) <= a * (1 + 1e-12)).all() and (a > 0).all()
    # a terminated sample reads wavelength 0 only, with four times the weight
    L1 = L.copy(); L1[::3, 1:] = 1e30
    v1, _ = sr.sensor_reference(L1, lam, pdf, cmf, exposure=0.5)
    assert np.array_equal(v1, v)
    # index 470 wraps to 0 (sensor.rs:55-60)
    e = np.array([[1.0, 0, 0, 0]]); p = np.array([[1.0, 0, 0, 0]])
    assert np.array_equal(sr.sensor_reference(e, [[830.0, 0, 0, 0]], p, cmf)[0], sr.sensor_reference(e, [[360.5, 0, 0, 0]], p, cmf)[0])
    # non-finite radiance stays non-finite
    Ln = L.copy(); Ln[5, 2] = np.nan
    vn, _ = sr.sensor_reference(Ln, lam, pdf, cmf)
    assert np.isnan(vn[5]).all() and np.isfinite(np.delete(vn, 5, axis=0)).all()


@pytest.mark.parametrize("scene_id", [3, 17])
def test_sensor_reference_sums_to_the_oracles_film(pkg, oracle, scene_id):
    """Scenes 3 and 17 at 24 x 16, 16 spp, mis / sobol.  The oracle's render_accum adds Sensor::add_sample's f32 values in sample order; its
    film equals the float64 sum of sensor_reference over the oracle's probe_radiance of every (x, y, s) within (n_s + K) u A (1 + 1e-3).
    (The oracle divides by the pdf where film_rgb multiplies with a folded reciprocal: one rounding fewer, inside the same K.)
    Measured: the largest residual is 4.6 u A in both scenes, where the bound is 42."""
    w, h, spp = 24, 16, 16
    sc = oracle.new_scene()
    cam = pkg.scenes.load_scene(sc, scene_id, w, h, tex_size=64)
    oracle.set_faithful(sc, False)
    prm = pkg.make_params(spp, "mis", "sobol")
    film, _ = oracle.render_accum(sc, cam, prm, 0, spp, threads=min(os.cpu_count() or 1, 16))
    ys, xs, ss = np.meshgrid(np.arange(h), np.arange(w), np.arange(spp), indexing="ij")
    L, lam, pdf = sc.probe_radiance(cam, prm, np.stack([xs.ravel(), ys.ravel(), ss.ravel()], 1).astype(np.uint32))
    assert np.isfinite(L).all()
    value, mass = sr.sensor_reference(L.reshape(h, w, spp, 4), lam.reshape(h, w, spp, 4), pdf.reshape(h, w, spp, 4), oracle.cmf)
    want, a_pixel = value.sum(axis=2), mass.sum(axis=2)
    resid = np.abs(film.astype(np.float64) - want)
    bound = sr.reconcile_bound(spp, K_ROUNDINGS, a_pixel)
    print(f"scene {scene_id}: largest residual {np.max(resid / (sr.U * np.maximum(a_pixel, 1e-300))):.3f} u A, bound {spp + K_ROUNDINGS} u A; film mean {film.mean():.4f}")
    assert film.mean() > 0.01 * spp
    assert (resid <= bound).all(), float((resid / bound).max())
    # the bound is sharp enough to see one sample: dropping any single sample of a pixel moves it by far more
    drop = np.abs(value).max(axis=2)
    assert np.median(drop / bound) > 100.0


# ---- the resolve reference (test_film_log_gpu.py c) ----
def oracle_resolve_error(oracle):
    """E: the largest deviation, in f32 ulps of the float64 result, of the oracle's own f32 Sensor::to_rgb from sr.resolve_reference over the
    resolve test's inputs and sample counts.  Also asserts that both have their NaN in the same places."""
    _, pool = sr.resolve_inputs()
    pad = np.resize(pool, -(-pool.size // 3) * 3)                               # whole pixels
    worst = 0.0
    for spp in sr.RESOLVE_SPP:
        got = oracle.film_resolve(pad.reshape(-1, 3), spp).ravel()
        want = sr.resolve_reference(pad, spp)
        assert np.array_equal(np.isnan(got), np.isnan(want)), spp
        ok = ~np.isnan(want)
        worst = max(worst, float(sr.ulp_distance(got[ok], want[ok]).max()))
    return worst


def test_resolve_reference_and_the_oracles_resolve(oracle):
    special, pool = sr.resolve_inputs()
    assert pool.size == special.size * 256 + 4096
    for v in range(special.size):                                               # every special value in every residue class of a block
        at = np.arange(v, special.size * 256, special.size)
        assert np.array_equal(pool[at].view(np.uint32), np.full(256, special[v:v + 1].view(np.uint32)[0], np.uint32))
        assert np.array_equal(np.sort(at % 256), np.arange(256))
    want = sr.resolve_reference(special, 1)
    nan = np.isnan(want)
    assert nan.sum() == 1 and np.isposinf(special[nan]).all()                   # inf / (1 + inf); a NaN or a negative sum is clipped to 0
    assert (want[(special <= 0) | np.isnan(special)] == 0.0).all()
    assert ((want[~nan] >= 0.0) & (want[~nan] <= 1.0)).all()
    e = oracle_resolve_error(oracle)
    print(f"oracle's f32 resolve against the float64 reference: E = {e:.3f} ulp")
    assert np.isfinite(e)
