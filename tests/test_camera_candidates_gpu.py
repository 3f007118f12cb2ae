"""Camera-ray hits from the work item's candidate list (csrc/camera_candidates.hpp, pt_kernel_body.inc) against the cooperative traversal:
one library, the switch MI355PT_NO_CAMERA_LISTS off and on, the same launch twice.  The per-sample log (L, lambda, pdf of every finished
path, written by the production kernel) and the linear film must be equal bit for bit.

Tiny frames make every pixel's pyramid of directions huge and the hero overflows any cap, so the cases are sparse shards of the true
1920 x 1080 frame (plus one tiny ragged frame, which exercises exactly that fallback).  For the first three cases the lists really are in
use: through mi355pt_scene_debug_camera_candidates (the same walk on the host) at least 90 % of the case's work items have a list within
the kernels' cap and at least one has three or more triangles."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 1920, 1080
TILES = ((W + 7) // 8) * ((H + 7) // 8)
TEX_SIZE = 128
CAP = 16

# name: (scene, strategy, width, height, spp, sample range, shard_index, shard_count, lists must be in use)
CASES = {
    "scene3_mis_2x2_items": (3, "mis", W, H, 1024, (0, 1024), 3, 4001, True),
    "scene10_mis_single_pixel_items": (10, "mis", W, H, 4096, (0, 4096), 22000, TILES, True),
    "scene17_nee_general_lowering": (17, "nee", W, H, 16384, (0, 4096), 1500, 4001, True),
    "scene3_mis_ragged_9x5": (3, "mis", 9, 5, 1024, (0, 1024), 0, 1, False),
    "scene19_environment_misses": (19, "mis", W, H, 1024, (0, 1024), 0, 4001, False),
}


def block_log2(n_samples):
    """launch_plan.hpp plan_launch_over for a Sobol launch of n_samples indices"""
    b = 3
    while b > 0 and (n_samples << (2 * (b - 1))) >= 2048:
        b -= 1
    return b


def item_rects(width, height, n_samples, shard_index, shard_count):
    """the pixel blocks of the shard's work items (inclusive rectangles; blocks wholly outside a ragged frame have no paths and are left out)"""
    bs = 1 << block_log2(n_samples)
    tiles_x, tiles_y = (width + 7) // 8, (height + 7) // 8
    out = []
    for t in range(shard_index, tiles_x * tiles_y, shard_count):
        tx, ty = t % tiles_x, t // tiles_x
        for by in range(0, 8, bs):
            for bx in range(0, 8, bs):
                x0, y0 = tx * 8 + bx, ty * 8 + by
                if x0 < width and y0 < height:
                    out.append((x0, y0, x0 + bs - 1, y0 + bs - 1))
    return np.array(out, np.uint32)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("name", list(CASES))
def test_lists_and_traversal_give_the_same_samples_and_film(product, pkg, monkeypatch, name):
    scene_id, strategy, w, h, spp, (s0, s1), shard_index, shard_count, in_use = CASES[name]
    sc = product.new_scene()
    cam = pkg.scenes.load_scene(sc, scene_id, w, h, tex_size=TEX_SIZE)
    counts, over, _ = sc.debug_camera_candidates(cam, item_rects(w, h, s1 - s0, shard_index, shard_count), cap=CAP)
    print(f"{name}: {counts.size} work items, {int((~over).sum())} with a list within {CAP}, longest {int(counts[~over].max(initial=0))}, "
          f"empty {int(((counts == 0) & ~over).sum())}")
    if in_use:
        assert (~over).mean() >= 0.9
        assert (counts[~over] >= 3).any()
    if name == "scene3_mis_ragged_9x5":
        assert over.any() and not over.all()             # the fallback and the lists side by side
    if name == "scene19_environment_misses":
        assert ((counts == 0) & ~over).any()             # items whose camera rays can hit nothing: an empty list, got = false
    prm = pkg.make_params(spp, strategy, "sobol", shard_index=shard_index, shard_count=shard_count)
    monkeypatch.setenv("MI355PT_NO_CAMERA_LISTS", "1")
    ref = product.render_sample_log(sc, cam, prm, s0, s1, want_accum=True)
    monkeypatch.delenv("MI355PT_NO_CAMERA_LISTS")
    got = product.render_sample_log(sc, cam, prm, s0, s1, want_accum=True)
    assert float(np.nansum(ref[3])) > 0.0                                    # the launch rendered something
    for what, a, b in zip(("L", "lambda", "pdf", "film"), ref, got):
        assert np.array_equal(bits(a), bits(b)), f"{what}: {int((bits(a) != bits(b)).sum())} values differ"
