"""Completeness of tests/kernel_matrix.py's case table, without a GPU: every case's scene lowered on the host (csrc/scene_lower.cpp), its
feature mask fed with the case's sampler and strategy through the host-compiled selector (csrc/launch_plan.hpp select_kernel).  The kernels
reached must be EXACTLY the production kernels the selector's own lists span — so a twelfth feature set or a fifth mode fails here until the
table grows, and so does a scene whose materials change under a table row."""
import itertools
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_matrix as km  # noqa: E402


@pytest.fixture(scope="module")
def selector(tmp_path_factory):
    return km.compile_selector(tmp_path_factory.mktemp("kernel_matrix"))


@pytest.fixture(scope="module")
def features(pkg):
    prod = pkg.Product()
    return {scene: km.lowered_features(pkg, prod, scene) for scene in sorted(set(c[1] for c in km.CASES))}


def test_cases_reach_every_production_kernel_and_no_other(selector, features):
    expected = set(itertools.product((0, 1), (0,), selector["modes"], selector["sets"]))
    assert len(expected) == 2 * len(selector["modes"]) * len(selector["sets"]) == 88
    reached = {}
    for fset, scene, strategy, sampler in km.CASES:
        for tiles in (0, 1):
            key = km.case_key(selector, tiles, features[scene], strategy, sampler)
            assert key[3] == fset, (scene, features[scene], key)          # the scene selects the set its row says
            reached.setdefault(key, []).append((scene, strategy, sampler))
    assert set(reached) == expected, (sorted(expected - set(reached)), sorted(set(reached) - expected))


def test_every_set_carries_all_six_pairs(selector):
    assert sorted(km.PRIMARY) == sorted(selector["sets"])                  # one row per compiled set
    assert len(set(km.PRIMARY.values())) == len(km.PRIMARY)               # ... each with a scene of its own
    assert len(km.PAIRS) == len(set(km.PAIRS)) == 6
    assert {(st, sa) for st, sa in km.PAIRS} == set(itertools.product(km.STRATEGY, km.SAMPLER))
    assert len(km.CASES) == len(set(km.CASES)) == 6 * len(selector["sets"]) == len(km.CASE_IDS) == len(set(km.CASE_IDS))
    for fset, scene in km.PRIMARY.items():
        assert sorted((st, sa) for f, s, st, sa in km.CASES if (f, s) == (fset, scene)) == sorted(km.PAIRS), fset


def test_no_case_is_skipped_or_expected_to_fail():
    """the table holds plain tuples, and the GPU tests are parametrised over the table itself with no mark but that"""
    import test_kernel_matrix_gpu as gpu
    assert all(type(c) is tuple and len(c) == 4 for c in km.CASES)
    assert gpu.pytestmark.name == "gpu"
    for fn in (gpu.test_shard_kernel_renders_the_oracles_frame, gpu.test_tile_list_kernel_is_bit_equal_to_its_shard_twin):
        marks = getattr(fn, "pytestmark", [])
        assert [m.name for m in marks] == ["parametrize"], fn.__name__
        assert marks[0].args[1] is km.CASES and marks[0].kwargs.get("ids") is km.CASE_IDS, fn.__name__
    src = open(gpu.__file__).read()
    for word in ("skip", "xfail", "importorskip"):
        assert word not in src, word
