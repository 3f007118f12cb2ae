"""Every compiled production path kernel launched and compared, over the case table of tests/kernel_matrix.py (66 cases: one scene per compiled
feature set under all six strategy / sampler pairs; tests/test_kernel_matrix.py shows without a GPU that they reach each of the 88 kernels).

a. The shard kernel pt_kernel<false, set, mode> renders the oracle's frame, in the arrangement and to the bar of
   test_parity_gpu.test_frames_match_the_oracle_sample_for_sample (64 x 48, 64 spp, tex_size 128, the oracle's own roulette gate; FRAME_BAR).
b. The tile-list kernel pt_kernel_tiles<set, mode> over the list of all tiles is bit-equal to that shard kernel, in the arrangement of
   test_adaptive_gpu.test_list_of_all_tiles_is_bit_equal_to_the_plain_render (44 x 20 = 6 x 3 tiles, ragged right and bottom, samples
   [0, 16), tex_size 64).  No oracle: a makes the shard twin trustworthy, b carries that over.
The instrumented kernels are test_deep_paths_gpu.STATS_CASES'.  MI355PT_FRAME_LOG=<file>: a appends one line per case
(profiles/kernel_matrix.jsonl is such a run)."""
import json
import os
import sys

import numpy as np
import pytest

from test_parity_gpu import FRAME_BAR

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_matrix as km  # noqa: E402

pytestmark = pytest.mark.gpu

ORACLE_THREADS = min(os.cpu_count() or 1, 16)
MEAN_FLOOR = 0.01                           # of the oracle's resolved frame (the darkest case, scene 31, has 0.022): no case may turn black
TW, TH, T_SAMPLES, T_TILES = 44, 20, 16, 6 * 3


@pytest.fixture(scope="module")
def selector(tmp_path_factory):
    return km.compile_selector(tmp_path_factory.mktemp("kernel_matrix_gpu"))


@pytest.fixture(scope="module")
def lowered(pkg, product):
    """scene -> the feature mask of its host lowering, as test_kernel_matrix.py reads it"""
    cache = {}

    def get(scene):
        if scene not in cache:
            cache[scene] = km.lowered_features(pkg, product, scene)
        return cache[scene]
    return get


@pytest.fixture(scope="module")
def frame_pairs(pkg, product, oracle):
    """scene -> {"gpu": (scene, camera), "cpu": (scene, camera)} at 64 x 48, built once and shared by the scene's six pairs"""
    cache = {}

    def get(scene):
        if scene not in cache:
            pair = {}
            for name, be in (("gpu", product), ("cpu", oracle)):
                sc = be.new_scene()
                pair[name] = (sc, pkg.scenes.load_scene(sc, scene, 64, 48, tex_size=128))
            oracle.set_faithful(pair["cpu"][0], False)
            cache[scene] = pair
        return cache[scene]
    return get


@pytest.fixture(scope="module")
def tile_scenes(pkg, product):
    """scene -> (scene, camera) at 44 x 20, built once and shared by the scene's six pairs"""
    cache = {}

    def get(scene):
        if scene not in cache:
            sc = product.new_scene()
            cache[scene] = (sc, pkg.scenes.load_scene(sc, scene, TW, TH, tex_size=64))
        return cache[scene]
    return get


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("fset,scene,strategy,sampler", km.CASES, ids=km.CASE_IDS)
def test_shard_kernel_renders_the_oracles_frame(product, oracle, pkg, selector, lowered, frame_pairs, fset, scene, strategy, sampler):
    pair = frame_pairs(scene)
    # the kernel this launch takes is the one the completeness test counted for the case
    assert km.info_features(product.scene_info(pair["gpu"][0])) == lowered(scene)
    key = km.case_key(selector, False, lowered(scene), strategy, sampler)
    assert key[:2] == (0, 0) and key[3] == fset
    prm = pkg.make_params(64, strategy, sampler)
    g = product.render(pair["gpu"][0], pair["gpu"][1], prm)
    c = oracle.render(pair["cpu"][0], pair["cpu"][1], prm, threads=ORACLE_THREADS)
    with np.errstate(invalid="ignore"):
        nan_g, nan_c = np.isnan(g), np.isnan(c)
        d = np.nan_to_num(g - c)
    rmse = float(np.sqrt(np.mean(d ** 2)))
    off = int((np.abs(d).max(axis=2) > 0.01).sum())
    mean = float(c.mean())                                   # (no NaN pixel in the oracle's frame of any case: a NaN fails the floor)
    rec = dict(set=fset, mode=km.MODE_NAMES[key[2]], scene=scene, strategy=strategy, sampler=sampler, rmse=float(f"{rmse:.3e}"), off=off,
               nan_px=int(nan_g.any(axis=2).sum()), nan_equal=bool(np.array_equal(nan_g, nan_c)), oracle_mean=round(mean, 4))
    print(json.dumps(rec))
    if os.environ.get("MI355PT_FRAME_LOG"):
        with open(os.environ["MI355PT_FRAME_LOG"], "a") as f:
            f.write(json.dumps(rec) + "\n")
    assert mean >= MEAN_FLOOR, mean
    assert np.array_equal(nan_g, nan_c)                     # (the reference accumulates NaN samples: the same pixels on both sides)
    assert rmse <= FRAME_BAR[0] and off <= FRAME_BAR[1], (rmse, off)


@pytest.mark.parametrize("fset,scene,strategy,sampler", km.CASES, ids=km.CASE_IDS)
def test_tile_list_kernel_is_bit_equal_to_its_shard_twin(product, pkg, selector, lowered, tile_scenes, fset, scene, strategy, sampler):
    import torch
    sc, cam = tile_scenes(scene)
    assert km.info_features(product.scene_info(sc)) == lowered(scene)
    key = km.case_key(selector, True, lowered(scene), strategy, sampler)
    assert key[:2] == (1, 0) and key[3] == fset
    prm = pkg.make_params(64, strategy, sampler)
    ref = torch.zeros((TH, TW, 3), dtype=torch.float32, device="cuda")
    product.render_accum_device(sc, cam, prm, 0, T_SAMPLES, ref.data_ptr(), None)
    film = torch.zeros((TH, TW, 3), dtype=torch.float32, device="cuda")
    product.render_accum_tiles_device(sc, cam, prm, np.arange(T_TILES), 0, T_SAMPLES, film.data_ptr(), None)
    torch.cuda.synchronize()
    ref, film = ref.cpu().numpy(), film.cpu().numpy()
    assert ref.mean() > 0.01 * T_SAMPLES * 0.1
    assert np.array_equal(bits(film), bits(ref))
