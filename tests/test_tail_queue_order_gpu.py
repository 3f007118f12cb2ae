"""The tail queue pops newest-first (a stack): nothing a sample computes may depend on when its vertex is shaded.

Per-sample values are compared bit for bit with the build BEFORE the order change: tests/golden/tail_queue_sample_log_digests.json holds one
sha256 per case of the per-sample log (L[4], lambda[4], pdf[4] per (tile, pixel, sample) slot) as that build rendered it, with its version()
string.  The films of that build are fixtures too: a pixel's samples reach the film tile in another order now, so the float sums differ in
the last bits and the films are compared at the project's frame bar (tests/test_parity_gpu.py FRAME_BAR), not bit for bit.

The cases are the smallest shapes at which the queue code can go wrong (tex_size 128 throughout):
  scene3_64x48x64    one queue, 8x8-tile items, the sample range split into chunks
  scene3_16x16x1024  the benchmark's own item shape: 2x2 blocks over all 1 024 indices, 4 096 pairs per item (~130 pushes and pops per item)
  scene17_64x48x64   the clearcoat kernels' two queues: the class-2-first rule and the shared drain passes
  scene3_13x7x3      a ragged frame and a pool smaller than a wave: drain passes only, more free lanes than queued records.  The per-sample
                     log needs a power-of-two spp (the sample index is read back from the Morton index), so the three samples are the range
                     [0, 3) of spp = 4
  scene34_32x24x16   the deep box at max_depth = 1000: long-lived records at the bottom of the stack, the depth bits of the record
"""
import hashlib
import json
import os

import numpy as np
import pytest

from test_parity_gpu import FRAME_BAR

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DIGESTS = os.path.join(GOLDEN, "tail_queue_sample_log_digests.json")
TEX_SIZE = 128

# name: (scene, strategy, width, height, spp, sample range, max_depth)
LOG_CASES = {
    "scene3_64x48x64": (3, "mis", 64, 48, 64, (0, 64), 16),
    "scene3_16x16x1024": (3, "mis", 16, 16, 1024, (0, 1024), 16),
    "scene17_64x48x64": (17, "nee", 64, 48, 64, (0, 64), 16),
    "scene3_13x7x3": (3, "mis", 13, 7, 4, (0, 3), 16),
    "scene34_32x24x16": (34, "mis", 32, 24, 16, (0, 16), 1000),
}
FILM_CASES = ("scene3_64x48x64", "scene17_64x48x64")


def film_fixture(name):
    return os.path.join(GOLDEN, f"tail_queue_film_{name}.npy")


def load_case(product, pkg, name):
    scene_id, strategy, w, h, spp, rng, max_depth = LOG_CASES[name]
    sc = product.new_scene()
    cam = pkg.scenes.load_scene(sc, scene_id, w, h, tex_size=TEX_SIZE)
    return sc, cam, spp, strategy, rng, max_depth


def render_log(product, pkg, name, s_range=None, shard_index=0, shard_count=1):
    sc, cam, spp, strategy, rng, max_depth = load_case(product, pkg, name)
    prm = pkg.make_params(spp, strategy, "sobol", max_depth=max_depth, shard_index=shard_index, shard_count=shard_count)
    s0, s1 = s_range or rng
    return product.render_sample_log(sc, cam, prm, s0, s1)


def log_digest(log):
    h = hashlib.sha256()
    for a in log:
        h.update(np.ascontiguousarray(a, dtype=np.float32).tobytes())
    return h.hexdigest()


def render_film(product, pkg, name):
    """The film of a case through render_accum_device, rendered twice: (linear sums, linear sums again, the tone-mapped frame of the first)"""
    import torch
    sc, cam, spp, strategy, rng, max_depth = load_case(product, pkg, name)
    prm = pkg.make_params(spp, strategy, "sobol", max_depth=max_depth)
    sums = []
    for _ in range(2):
        a = torch.zeros((cam.height, cam.width, 3), dtype=torch.float32, device="cuda")
        product.render_accum_device(sc, cam, prm, rng[0], rng[1], a.data_ptr(), None)
        torch.cuda.synchronize()
        sums.append(a)
    out = torch.empty_like(sums[0])
    product.film_resolve_device(sums[0].data_ptr(), cam.width * cam.height, rng[1] - rng[0], out.data_ptr(), None)
    torch.cuda.synchronize()
    return sums[0].cpu().numpy(), sums[1].cpu().numpy(), out.cpu().numpy()


@pytest.fixture(scope="module")
def golden():
    with open(DIGESTS) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def c2_log(product, pkg):
    """the whole-frame log of the 16x16x1024 case, rendered once"""
    log = render_log(product, pkg, "scene3_16x16x1024")
    for a in log:
        a.setflags(write=False)
    return log


@pytest.mark.parametrize("name", list(LOG_CASES))
def test_per_sample_values_are_those_of_the_fifo_build(product, pkg, golden, c2_log, name):
    log = c2_log if name == "scene3_16x16x1024" else render_log(product, pkg, name)
    L = log[0]
    s0, s1 = LOG_CASES[name][5]
    assert L.shape[1:] == (64, s1 - s0, 4) and np.isfinite(L).all() and float(L.mean()) > 0.0
    d = log_digest(log)
    print(name, d, "recorded by", golden["version"])
    assert d == golden["logs"][name], (name, d)


def test_sample_ranges_and_shards_render_the_same_samples(product, pkg, c2_log):
    """Another schedule, the same samples: two sample ranges (other chunks, other item pools) and two shards (other tiles per launch)"""
    name = "scene3_16x16x1024"
    halves = [render_log(product, pkg, name, s_range=r) for r in ((0, 512), (512, 1024))]
    for k in range(3):
        assert np.array_equal(np.concatenate([halves[0][k], halves[1][k]], axis=2).view(np.uint32), c2_log[k].view(np.uint32)), k
    shards = [render_log(product, pkg, name, shard_index=i, shard_count=2) for i in (0, 1)]
    for k in range(3):
        whole = np.empty_like(c2_log[k])
        whole[0::2], whole[1::2] = shards[0][k], shards[1][k]          # tile k of shard i is frame tile i + 2 k
        assert np.array_equal(whole.view(np.uint32), c2_log[k].view(np.uint32)), k


@pytest.mark.parametrize("name", FILM_CASES)
def test_films_are_identical_from_run_to_run_and_match_the_fifo_build(product, pkg, name):
    a, b, g = render_film(product, pkg, name)
    assert np.isfinite(a).all() and a.mean() > 0.0
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    c = np.load(film_fixture(name))
    assert c.shape == g.shape and c.mean() > 0.05
    rmse = float(np.sqrt(np.mean((g - c) ** 2)))
    off = int((np.abs(g - c).max(axis=2) > 0.01).sum())
    print(name, "rmse", rmse, "off", off, "bit-equal", bool(np.array_equal(g, c)))
    assert rmse <= FRAME_BAR[0] and off <= FRAME_BAR[1], (rmse, off)
