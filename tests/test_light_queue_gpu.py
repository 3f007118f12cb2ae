"""Emitter hits evaluated 64 at a time from the wave's light-hit queue (csrc/pt_kernel.hpp LIGHT-HIT QUEUE, tail_queue_plan.hpp lq_*) against
the same library with MI355PT_NO_LIGHT_QUEUE=1, which evaluates every emitter hit in place, in the front of its vertex.  A sample's
arithmetic does not depend on where it is evaluated, so the per-sample logs (L, lambda, pdf of every finished path) must be equal as bit
patterns.  A pixel's samples reach the film tile in another order, so the linear film sums may differ in the last bits: they must agree
within the bound tests/test_film_log_gpu.py uses between a film and the sum of its own log, (n_s + K) u A_pixel (1 + 1e-3) + 1e-37
(sensor_reference.reconcile_bound; A_pixel from the log).  Both renders in one process, tex_size 128.

The cases are the smallest shapes at which the queue can go wrong:
  scene3_16x16x1024    the benchmark's own item shape: 2x2 blocks over all 1 024 indices
  scene3_64x48x64      8x8-tile items, the sample range split into chunks
  scene3_13x7x3        a ragged frame and a pool smaller than a wave ([0, 3) of spp = 4): only the pass at the end of the item, fewer records than lanes
  scene3_depth0        max_depth = 0: every non-zero sample is a camera ray on the emitter — 64 pushes at once against a non-empty stack
  scene34_32x24x16     the deep box at max_depth = 1000
  scene29_32x24x16     several lights: the multi-light weight
  scene31_32x24x16     a textured emitter
  scene0_nee_64x48x64  NEE: an emitter reached by a non-specular bounce contributes nothing and is neither queued nor evaluated — same logs
  scene3_tiles         64x48x64 through the tile-list entry point (film only: that entry point has no log; A_pixel from the shard launch's log)
  scene17_nee_64x48x64 the clearcoat kernels, which have no light-hit queue: the switch must change nothing, the film is bit-equal
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sensor_reference as sr  # noqa: E402
from test_film_log import K_ROUNDINGS  # noqa: E402

pytestmark = pytest.mark.gpu

TEX_SIZE = 128
SWITCH = "MI355PT_NO_LIGHT_QUEUE"

# name: (scene, strategy, width, height, spp, sample range, max_depth, through the tile list, film must be bit-equal)
CASES = {
    "scene3_16x16x1024": (3, "mis", 16, 16, 1024, (0, 1024), 16, False, False),
    "scene3_64x48x64": (3, "mis", 64, 48, 64, (0, 64), 16, False, False),
    "scene3_13x7x3": (3, "mis", 13, 7, 4, (0, 3), 16, False, False),
    "scene3_depth0": (3, "mis", 64, 48, 16, (0, 16), 0, False, False),
    "scene34_32x24x16": (34, "mis", 32, 24, 16, (0, 16), 1000, False, False),
    "scene29_32x24x16": (29, "mis", 32, 24, 16, (0, 16), 16, False, False),
    "scene31_32x24x16": (31, "mis", 32, 24, 16, (0, 16), 16, False, False),
    "scene0_nee_64x48x64": (0, "nee", 64, 48, 64, (0, 64), 16, False, False),
    "scene3_tiles": (3, "mis", 64, 48, 64, (0, 64), 16, True, False),
    "scene17_nee_64x48x64": (17, "nee", 64, 48, 64, (0, 64), 16, False, True),
}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def render_tiles(product, sc, cam, prm, rng):
    import torch
    a = torch.zeros((cam.height, cam.width, 3), dtype=torch.float32, device="cuda")
    n_tiles = ((cam.width + 7) // 8) * ((cam.height + 7) // 8)
    product.render_accum_tiles_device(sc, cam, prm, np.arange(n_tiles, dtype=np.uint32), rng[0], rng[1], a.data_ptr(), None)
    torch.cuda.synchronize()
    return a.cpu().numpy()


def pixel_mass(pkg, prm, log, w, h):
    """(h, w, 3) float64: A_pixel, the absolute mass of every pixel's logged samples per channel (tests/sensor_reference.py), the whole frame as one shard"""
    L, lam, pdf = log
    tiles_x = (w + 7) // 8
    tiles, pix = np.arange(L.shape[0]), np.arange(64)
    xs = (tiles % tiles_x)[:, None] * 8 + (pix % 8)[None, :]
    ys = (tiles // tiles_x)[:, None] * 8 + (pix // 8)[None, :]
    inside = (xs < w) & (ys < h)
    _, mass = sr.sensor_reference(L[inside], lam[inside], pdf[inside], pkg.scenes.cmf_xyz(), exposure=prm.exposure)
    a = np.zeros((h, w, 3), np.float64)
    a[ys[inside], xs[inside]] = mass.sum(axis=1)
    return a


@pytest.mark.parametrize("name", list(CASES))
def test_queued_and_in_place_emitter_hits_give_the_same_samples(product, pkg, monkeypatch, name):
    scene_id, strategy, w, h, spp, rng, max_depth, tiles, bit_equal = CASES[name]
    n_s = rng[1] - rng[0]
    sc = product.new_scene()
    cam = pkg.scenes.load_scene(sc, scene_id, w, h, tex_size=TEX_SIZE)
    prm = pkg.make_params(spp, strategy, "sobol", max_depth=max_depth)
    monkeypatch.setenv(SWITCH, "1")
    *ref_log, ref_film = product.render_sample_log(sc, cam, prm, rng[0], rng[1], want_accum=True)
    if tiles:
        ref_film = render_tiles(product, sc, cam, prm, rng)
    monkeypatch.delenv(SWITCH)
    *log, film = product.render_sample_log(sc, cam, prm, rng[0], rng[1], want_accum=True)
    if tiles:
        film = render_tiles(product, sc, cam, prm, rng)
    assert ref_log[0].shape[1:] == (64, n_s, 4) and film.shape == ref_film.shape == (h, w, 3)
    for f in (ref_film, film):
        assert np.isfinite(f).all() and float(f.mean()) > 0.0                              # the launch rendered something
    if not tiles:
        for what, a, b in zip(("L", "lambda", "pdf"), ref_log, log):
            assert np.array_equal(bits(a), bits(b)), f"{what}: {int((bits(a) != bits(b)).sum())} values differ"
    if max_depth == 0:
        # the only light a path of depth 0 can carry is the emitter's own, seen by the camera ray: such samples exist, so the queue was used
        lit = (log[0] != 0.0).any(axis=-1)
        print(f"{name}: {int(lit.sum())} samples of {lit.size} are camera rays on the emitter, in {int(lit.any(axis=2).sum())} pixels")
        assert lit.any(axis=2).sum() > 0
    a_pixel = pixel_mass(pkg, prm, ref_log, w, h)
    bound = sr.reconcile_bound(n_s, K_ROUNDINGS, a_pixel)
    resid = np.abs(film.astype(np.float64) - ref_film.astype(np.float64))
    n_diff = int((bits(ref_film) != bits(film)).sum())
    with np.errstate(divide="ignore", invalid="ignore"):
        units = np.where(a_pixel > 0.0, resid / (sr.U * a_pixel), 0.0)
    print(f"{name}: film mean {float(film.mean()):.5f}, {n_diff} of {film.size} film values differ, largest difference {float(units.max()):.2f} u A "
          f"(bound {n_s + K_ROUNDINGS})")
    if bit_equal:
        assert n_diff == 0, f"film: {n_diff} values differ"
    assert (resid <= bound).all(), f"film: largest difference {float(units.max()):.2f} u A, bound {n_s + K_ROUNDINGS}"
