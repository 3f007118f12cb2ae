"""Which path kernel a launch takes (csrc/launch_plan.hpp select_kernel) without a GPU: the selector compiled for the host and compared, over
every input it can get, with a restatement of the rules as the plain launcher, the tile-list launcher and the occupancy query each spelled
them out before they shared one lookup, and the single list of compiled feature sets against its two classes."""
import itertools
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_matrix import compile_selector  # noqa: E402

TEX, DIEL, CC, MLIGHT, ROUGH, METAL, DELTA, ENV, EMTEX = (1 << i for i in range(9))
STD, ALL = 255, 511
GENERIC, MIS_SOBOL, NEE_SOBOL, PT = 0, 1, 2, 3
RANDOM, SOBOL = 0, 1
S_PT, S_NEE, S_MIS = 0, 1, 2
# the order the feature sets were tried in while the clearcoat sets stood among the plain ones
INTERLEAVED = [0, TEX, DIEL, METAL, DIEL | ROUGH, DELTA | MLIGHT, CC, CC | TEX, STD & ~CC, STD, ALL]


def former_key(tiles, stats, feat, sampler, strategy):
    if stats:      # two instrumented variants, both generic-mode kernels
        return (tiles, 1, GENERIC, STD & ~CC if feat & (CC | EMTEX) == 0 else ALL)
    if sampler == SOBOL and strategy == S_MIS:
        mode = MIS_SOBOL
    elif sampler == SOBOL and strategy == S_NEE:
        mode = NEE_SOBOL
    elif strategy == S_PT:
        mode = PT
    else:
        mode = GENERIC
    return (tiles, 0, mode, next(s for s in INTERLEAVED if feat & ~s == 0))


@pytest.fixture(scope="module")
def selector(tmp_path_factory):
    return compile_selector(tmp_path_factory.mktemp("kernel_select"))


def test_feature_sets_are_one_list_in_two_classes(selector):
    sets, plain, cc = selector["sets"], selector["plain"], selector["cc"]
    assert len(sets) == 11 and len(set(sets)) == 11
    assert sets == plain + cc                                   # the plain sets first, then the clearcoat sets; every entry in exactly one class
    assert not set(plain) & set(cc)
    assert all(s & CC == 0 for s in plain) and all(s & CC for s in cc)
    assert sorted(sets) == sorted(INTERLEAVED)
    assert selector["modes"] == [GENERIC, MIS_SOBOL, NEE_SOBOL, PT]


def test_select_kernel_is_the_former_rules(selector):
    keys = selector["k"]
    inputs = list(itertools.product((0, 1), (0, 1), range(512), (RANDOM, SOBOL), (S_PT, S_NEE, S_MIS)))
    assert len(keys) == len(inputs) == 2 * 2 * 512 * 2 * 3
    plain, cc = set(selector["plain"]), set(selector["cc"])
    for inp in inputs:
        tiles, stats = inp[:2]
        key = keys[inp]
        assert key[3] in (cc if key[3] & CC else plain), (inp, key)
        if tiles and stats:
            # no instrumented tile-list kernel exists (the API refuses the combination): the key must go on saying what was asked for, so that
            # the lookup finds nothing, rather than name some kernel that exists
            assert key[:2] == (1, 1), (inp, key)
            continue
        assert key == former_key(*inp), (inp, key)
