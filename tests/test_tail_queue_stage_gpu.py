"""Tail-queue records handed to the pass through LDS (csrc/tail_queue_plan.hpp staging, pt_kernel_body.inc) against the same library with
MI355PT_NO_QUEUE_STAGING=1, which sends every record through the global stack as before: the record -> lane mapping is the same, so a
pixel's samples reach the film tile in the same order and the linear film sums (render_accum_device) must be equal as bit patterns, and
the per-sample logs (L, lambda, pdf of every finished path) too.  Both renders in one process, tex_size 128.

The cases are the smallest shapes at which the queue code can go wrong:
  scene3_16x16x1024   the benchmark's own item shape: 2x2 blocks over all 1 024 indices (~130 pushes and pops per item)
  scene3_64x48x64     8x8-tile items, the sample range split into chunks
  scene3_13x7x3       a ragged frame and a pool smaller than a wave: drain passes only, more free lanes than records ([0, 3) of spp = 4)
  scene34_32x24x16    the deep box at max_depth = 1000: long-lived records at the bottom of the global stack, the depth bits
  scene0_nee_64x48x64 another kernel with one queue (NEE)
  scene3_tiles        64x48x64 through the tile-list entry point, the list naming every tile (film only: that entry point has no log)
  scene17_64x48x64    the clearcoat kernels' two queues, which do not stage: the switch must change nothing
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TEX_SIZE = 128
SWITCH = "MI355PT_NO_QUEUE_STAGING"

# name: (scene, strategy, width, height, spp, sample range, max_depth, through the tile list)
CASES = {
    "scene3_16x16x1024": (3, "mis", 16, 16, 1024, (0, 1024), 16, False),
    "scene3_64x48x64": (3, "mis", 64, 48, 64, (0, 64), 16, False),
    "scene3_13x7x3": (3, "mis", 13, 7, 4, (0, 3), 16, False),
    "scene34_32x24x16": (34, "mis", 32, 24, 16, (0, 16), 1000, False),
    "scene0_nee_64x48x64": (0, "nee", 64, 48, 64, (0, 64), 16, False),
    "scene3_tiles": (3, "mis", 64, 48, 64, (0, 64), 16, True),
    "scene17_64x48x64": (17, "nee", 64, 48, 64, (0, 64), 16, False),
}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def render(product, sc, cam, prm, rng, tiles):
    """(linear film sums, per-sample log or None) of one launch"""
    import torch
    a = torch.zeros((cam.height, cam.width, 3), dtype=torch.float32, device="cuda")
    if tiles:
        n_tiles = ((cam.width + 7) // 8) * ((cam.height + 7) // 8)
        product.render_accum_tiles_device(sc, cam, prm, np.arange(n_tiles, dtype=np.uint32), rng[0], rng[1], a.data_ptr(), None)
    else:
        product.render_accum_device(sc, cam, prm, rng[0], rng[1], a.data_ptr(), None)
    torch.cuda.synchronize()
    log = None if tiles else product.render_sample_log(sc, cam, prm, rng[0], rng[1])
    return a.cpu().numpy(), log


@pytest.mark.parametrize("name", list(CASES))
def test_staged_and_global_records_give_the_same_film_and_samples(product, pkg, monkeypatch, name):
    scene_id, strategy, w, h, spp, rng, max_depth, tiles = CASES[name]
    sc = product.new_scene()
    cam = pkg.scenes.load_scene(sc, scene_id, w, h, tex_size=TEX_SIZE)
    prm = pkg.make_params(spp, strategy, "sobol", max_depth=max_depth)
    monkeypatch.setenv(SWITCH, "1")
    ref_film, ref_log = render(product, sc, cam, prm, rng, tiles)
    monkeypatch.delenv(SWITCH)
    film, log = render(product, sc, cam, prm, rng, tiles)
    assert np.isfinite(ref_film).all() and float(ref_film.mean()) > 0.0                    # the launch rendered something
    n_film = int((bits(ref_film) != bits(film)).sum())
    print(f"{name}: film mean {float(film.mean()):.5f}, {n_film} of {film.size} film values differ")
    assert np.array_equal(bits(ref_film), bits(film)), f"film: {n_film} values differ"
    if not tiles:
        assert ref_log[0].shape[1:] == (64, rng[1] - rng[0], 4)
        for what, a, b in zip(("L", "lambda", "pdf"), ref_log, log):
            assert np.array_equal(bits(a), bits(b)), f"{what}: {int((bits(a) != bits(b)).sum())} values differ"
