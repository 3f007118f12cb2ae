"""Every path kernel's film reconciled with its own per-sample log, and resolve_kernel value by value.

The suite compares the path kernels per sample (spectral radiance against the oracle: the sample log) and per frame (resolved, tone-mapped
frames at FRAME_BAR).  Between the two lie film_rgb (csrc/pt_path.hpp, the restatement of Sensor::add_sample), the hand-out of (pixel, sample)
pairs to lanes, the LDS film tile, the write-back, combine_kernel over split sample ranges and the accumulation over several launches.
mi355pt_render_sample_log returns every finished path's L[4], lambda[4], pdf[4] AND the linear film sums of the same launch, so the film must be
the sum of the sensor responses of the logged samples:

  completeness     every (pixel, sample) of the frame has a record (pdf[0] is 1/470 or 1/1880, never the memset's zero), its live wavelengths
                   lie in [360, 830), and the records of tile pixels outside the frame are untouched;
  reconciliation   per pixel and channel  |film - sum_s sensor_reference(record)| <= (n_s + K) u A_pixel (1 + 1e-3) + 1e-37,
                   u = 2^-24, A_pixel the pixel's absolute mass (tests/sensor_reference.py), the right side float64.

The bound is derived, not fitted.  film_rgb rounds a term  exposure * M[ch][j] * cmf_j * L[k] / pdf[k] / 4  of the mass at most 11 times: two
in the folded reciprocal of the pdf (the rounding of 1/470 itself is shared with the logged pdf, so one of them is slack), one for L * inv_pdf
(the / 4 is exact), one for c * cmf, three adds into X (the first add, to 0, is exact), one matrix multiply and two adds, one for the exposure
(the closing 0 + x is exact).  The kernels are compiled without contraction; a fused multiply-add would only remove roundings.  The f32 matrix
differs from the float64 one by at most m = 15 u per entry (measured on the host, tests/test_film_log.py).  K = 11 + m = 26.  Adding the n_s
values of a pixel in any order and grouping — LDS atomics in hand-out order, one partial film per chunk, combine_kernel over the chunks, the
film's += per launch — rounds n_s - 1 times on partial sums no larger than the mass: (n_s - 1) u A.  Second-order terms are below
(n_s + K) u < 3e-4 of the first-order ones at n_s = 4192, inside the factor 1 + 1e-3.
At n_s = 64 the bound is 5e-6 of the pixel's mass, where one average sample is 1.6e-2 of it: a sample dropped, counted twice or added to the
neighbouring pixel fails it by orders of magnitude.  At n_s = 4096 the bound reaches the size of one average sample: there the completeness
check carries the detection of a dropped sample, and the reconciliation still catches duplicates and misplaced samples larger than the bound
(a chunk slot added twice, a tile written one row off).

a. the 66 cases of tests/kernel_matrix.py (every production shard kernel), 44 x 20, 64 spp;  b. the launch shapes plan_launch produces
(test_film_log.SHAPE_CASES, whose coverage test_film_log.py pins without a GPU);  c. resolve_kernel against a float64 reference.
The tile-list twins need no case: test_kernel_matrix_gpu.test_tile_list_kernel_is_bit_equal_to_its_shard_twin carries the result over.
MI355PT_FRAME_LOG=<file>: one line per case (profiles/film_log_parity.jsonl is such a run: the largest residual of any case is 9.0 u A, at
n_s = 4096 where the bound is 4122; 2.3 ... 8 u A elsewhere; resolve_kernel's largest deviation is 7.4 ulp, the oracle's own E)."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_matrix as km  # noqa: E402
import sensor_reference as sr  # noqa: E402
from test_film_log import FRAME_H, FRAME_W, K_ROUNDINGS, SHAPE_CASES, SHAPE_IDS, SHAPE_SCENES, oracle_resolve_error, shard_tiles  # noqa: E402

pytestmark = pytest.mark.gpu

TEX_SIZE = 64
PDF0 = np.float32(1.0) / (np.float32(830.0) - np.float32(360.0))               # the wavelength pdf, and a quarter of it once the
PDF0_TERM = PDF0 / np.float32(4.0)                                              # secondary wavelengths are terminated
LEFT_OUT_CAP = 0                                                                # pixels with a non-finite sample: none in any case here


def log_line(rec):
    print(json.dumps(rec))
    if os.environ.get("MI355PT_FRAME_LOG"):
        with open(os.environ["MI355PT_FRAME_LOG"], "a") as f:
            f.write(json.dumps(rec) + "\n")


@pytest.fixture(scope="module")
def selector(tmp_path_factory):
    return km.compile_selector(tmp_path_factory.mktemp("film_log_gpu"))


@pytest.fixture(scope="module")
def lowered(pkg, product):
    cache = {}

    def get(scene):
        if scene not in cache:
            cache[scene] = km.lowered_features(pkg, product, scene)
        return cache[scene]
    return get


@pytest.fixture(scope="module")
def scenes(pkg, product, oracle):
    """(backend "gpu" | "cpu", scene id, width, height) -> (scene, camera), built once and shared by the scene's cases"""
    cache = {}

    def get(name, scene, w, h):
        if (name, scene, w, h) not in cache:
            sc = (product if name == "gpu" else oracle).new_scene()
            cache[(name, scene, w, h)] = (sc, pkg.scenes.load_scene(sc, scene, w, h, tex_size=TEX_SIZE))
            if name == "cpu":
                oracle.set_faithful(sc, False)
        return cache[(name, scene, w, h)]
    return get


def reconcile(pkg, product, gpu, w, h, prm, s_begin, s_end, shard, case, key):
    """render_sample_log of the range on the shard; asserts completeness and reconciliation; returns the logged record"""
    sc, cam = gpu
    n_s = s_end - s_begin
    L, lam, pdf, film = product.render_sample_log(sc, cam, prm, s_begin, s_end, want_accum=True)
    tiles = shard_tiles(w, h, shard)
    tiles_x = (w + 7) // 8
    assert L.shape == lam.shape == pdf.shape == (len(tiles), 64, n_s, 4) and film.shape == (h, w, 3)
    pix = np.arange(64)
    xs = (tiles % tiles_x)[:, None] * 8 + (pix % 8)[None, :]                    # (tiles, 64): the log's pixel (y & 7) * 8 + (x & 7)
    ys = (tiles // tiles_x)[:, None] * 8 + (pix // 8)[None, :]
    inside = (xs < w) & (ys < h)
    assert inside.any(axis=1).all()

    # completeness
    p0 = pdf[..., 0]
    full, term = p0 == PDF0, p0 == PDF0_TERM
    assert (full | term)[inside].all(), f"{int((~(full | term))[inside].sum())} (pixel, sample) pairs of the frame have no record"
    assert (pdf[..., 1:][full] == PDF0).all() and (pdf[..., 1:][term] == 0.0).all()
    live = pdf != 0.0
    assert ((lam[live] >= 360.0) & (lam[live] < 830.0)).all()
    for a in (L, lam, pdf):
        assert not a[~inside].view(np.uint32).any(), "a record of a pixel outside the frame was written"

    # reconciliation
    value, mass = sr.sensor_reference(L[inside], lam[inside], pdf[inside], pkg.scenes.cmf_xyz(), exposure=prm.exposure)    # (pixels, n_s, 3)
    with np.errstate(invalid="ignore"):
        want, a_pixel = value.sum(axis=1), mass.sum(axis=1)
    got = film[ys[inside], xs[inside]].astype(np.float64)                       # (pixels, 3)
    bad = ~np.isfinite(want)                                                    # channels a non-finite sample reaches
    assert not np.isfinite(got[bad]).any(), "a non-finite sample left its pixel's film finite"
    left_out = bad.any(axis=1)
    keep = ~left_out
    resid = np.abs(got[keep] - want[keep])
    bound = sr.reconcile_bound(n_s, K_ROUNDINGS, a_pixel[keep])
    units = resid / (sr.U * np.maximum(a_pixel[keep], 1e-300))
    worst = np.unravel_index(np.argmax(resid / bound), resid.shape) if resid.size else None
    rec = dict(case=case, kernel=dict(mode=km.MODE_NAMES[key[2]], set=key[3]), n_s=n_s, tiles=len(tiles), pixels=int(inside.sum()),
               max_residual_uA=round(float(units.max()), 3), bound_uA=n_s + K_ROUNDINGS, left_out=int(left_out.sum()),
               terminated=int(term[inside].sum()), film_mean=float(f"{got[keep].mean():.4e}"))
    log_line(rec)
    # nothing outside the shard's pixels was touched (the film starts at zero)
    rest = np.ones((h, w), bool)
    rest[ys[inside], xs[inside]] = False
    assert not film[rest].view(np.uint32).any()
    assert left_out.sum() <= LEFT_OUT_CAP, int(left_out.sum())
    # no case is black — a black film reconciles with anything.  (Linear mean per sample; the darkest case, scene 31 under nee / random, has 1.5e-3.)
    assert got[keep].mean() > 2e-4 * n_s
    if not (resid <= bound).all():
        p, ch = worst
        px, py = xs[inside][keep][p], ys[inside][keep][p]
        one = np.abs(value[keep][p, :, ch])
        near = int(np.argmin(np.abs(one - resid[p, ch])))
        raise AssertionError(f"pixel ({px}, {py}) channel {ch}: film {got[keep][p, ch]!r}, log {want[keep][p, ch]!r}, residual {resid[p, ch]:.6e} = "
                             f"{units[p, ch]:.1f} u A (bound {n_s + K_ROUNDINGS}); the pixel's sample closest in size: index {s_begin + near}, |rgb| {one[near]:.6e}")
    return rec


def oracle_has_no_non_finite_sample(pkg, cpu, w, h, prm, s_begin, s_end, shard):
    """The cap of 0 pixels left out rests on the scenes having no NaN sample: the oracle's own radiance of every (pixel, sample) of the case"""
    sc, cam = cpu
    tiles = shard_tiles(w, h, shard)
    tiles_x = (w + 7) // 8
    pix = np.arange(64)
    xs = ((tiles % tiles_x)[:, None] * 8 + (pix % 8)[None, :]).ravel()
    ys = ((tiles // tiles_x)[:, None] * 8 + (pix // 8)[None, :]).ravel()
    ok = (xs < w) & (ys < h)
    xs, ys = xs[ok], ys[ok]
    s = np.arange(s_begin, s_end)
    xys = np.stack([np.repeat(xs, s.size), np.repeat(ys, s.size), np.tile(s, xs.size)], 1).astype(np.uint32)
    Lc, _, _ = sc.probe_radiance(cam, prm, xys)
    return bool(np.isfinite(Lc).all())


@pytest.mark.parametrize("fset,scene,strategy,sampler", km.CASES, ids=km.CASE_IDS)
def test_shard_kernel_film_is_the_sum_of_its_sample_log(product, pkg, selector, lowered, scenes, fset, scene, strategy, sampler):
    pair = {name: scenes(name, scene, FRAME_W, FRAME_H) for name in ("gpu", "cpu")}
    # the kernel this launch takes is the one tests/test_kernel_matrix.py counted for the case
    assert km.info_features(product.scene_info(pair["gpu"][0])) == lowered(scene)
    key = km.case_key(selector, False, lowered(scene), strategy, sampler)
    assert key[:2] == (0, 0) and key[3] == fset
    prm = pkg.make_params(64, strategy, sampler)
    assert oracle_has_no_non_finite_sample(pkg, pair["cpu"], FRAME_W, FRAME_H, prm, 0, 64, (0, 1))
    reconcile(pkg, product, pair["gpu"], FRAME_W, FRAME_H, prm, 0, 64, (0, 1), f"set{fset}-scene{scene}-{strategy}-{sampler}", key)


@pytest.mark.parametrize("scene,strategy", SHAPE_SCENES, ids=[f"scene{s}-{st}" for s, st in SHAPE_SCENES])
@pytest.mark.parametrize("shape", SHAPE_CASES, ids=SHAPE_IDS)
def test_launch_shapes_reconcile(product, pkg, selector, lowered, scenes, shape, scene, strategy):
    name, w, h, spp, s_begin, s_end, sampler, exposure, shard, _, _ = shape
    gpu = scenes("gpu", scene, w, h)
    assert km.info_features(product.scene_info(gpu[0])) == lowered(scene)
    key = km.case_key(selector, False, lowered(scene), strategy, sampler)
    prm = pkg.make_params(spp, strategy, sampler, exposure=exposure, shard_index=shard[0], shard_count=shard[1])
    reconcile(pkg, product, gpu, w, h, prm, s_begin, s_end, shard, f"{name}-scene{scene}-{strategy}", key)


# ---- c: resolve_kernel ----
RESOLVE_PIXELS = (1, 85, 86, 175_000)        # 85 / 86: the last size below and the first above one block of 256 values; 175 000 pixels are
GUARD = 1024                                 # 525 000 values > 2048 blocks x 256 threads: the grid-stride loop takes a second trip
SENTINEL = np.float32(-123.25)


@pytest.fixture(scope="module")
def resolve_tolerance(oracle):
    """E + 4 ulp: E the oracle's own f32 deviation from the float64 reference over these inputs, measured now on the CPU; 4 for the device's
    powf and division differing from the host's"""
    e = oracle_resolve_error(oracle)
    return e, e + 4.0


@pytest.mark.parametrize("spp", sr.RESOLVE_SPP)
@pytest.mark.parametrize("n_pixels", RESOLVE_PIXELS)
def test_resolve_kernel_value_by_value(product, resolve_tolerance, n_pixels, spp):
    import torch
    e_oracle, tol = resolve_tolerance
    special, pool = sr.resolve_inputs()
    n_values = 3 * n_pixels
    # a film too small to hold every special value takes them in as many launches as it needs
    offsets = range(0, special.size, n_values) if n_values < special.size else [0]
    worst = 0.0
    for off in offsets:
        film = np.resize(np.roll(pool, -off), n_values)
        d_film = torch.from_numpy(np.concatenate([film, np.full(GUARD, 7.0, np.float32)])).cuda()
        d_out = torch.full((n_values + GUARD,), float(SENTINEL), dtype=torch.float32, device="cuda")
        product.film_resolve_device(d_film.data_ptr(), n_pixels, spp, d_out.data_ptr())
        torch.cuda.synchronize()
        out, film_after = d_out.cpu().numpy(), d_film.cpu().numpy()
        assert np.array_equal(out[n_values:].view(np.uint32), np.full(GUARD, SENTINEL).view(np.uint32))       # the guard band stays as written
        assert np.array_equal(film_after[:n_values].view(np.uint32), film.view(np.uint32)) and (film_after[n_values:] == 7.0).all()
        got, want = out[:n_values], sr.resolve_reference(film, spp)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        ok = ~np.isnan(want)
        ulps = sr.ulp_distance(got[ok], want[ok])
        worst = max(worst, float(ulps.max()))
        assert ulps.max() <= tol, (float(film[ok][np.argmax(ulps)]), float(got[ok][np.argmax(ulps)]), float(want[ok][np.argmax(ulps)]), float(ulps.max()), tol)
    log_line(dict(case=f"resolve-{n_pixels}px-{spp}spp", kernel="resolve_kernel", n_values=n_values, launches=len(offsets),
                  max_ulp=round(worst, 3), oracle_ulp_E=round(e_oracle, 3), tolerance_ulp=round(tol, 3)))
