"""The launch shape of the tile-list kernels (csrc/launch_plan.hpp plan_launch_tiles) without a GPU, in the manner of test_launch_plan.py and
over its grid of sizes, spp, samplers and resident waves: a list of ALL tiles gets plan_launch's whole-frame plan field for field (which is
what makes that list bit-equal to mi355pt_render_accum_device), and for shorter lists the invariants hold that lane_job_tiles and the
per-chunk film slots (pt_kernel_tiles.hpp, pt_kernels_tiles.hip) rely on."""
import itertools
import os
import subprocess

import pytest

import test_launch_plan as lp

ROOT = lp.ROOT
RANDOM, SOBOL = lp.RANDOM, lp.SOBOL
FIELDS = ("begin", "end", "spp", "seed", "max_depth", "strategy", "sampler", "sample_begin", "sample_end", "log2_spp", "n_base4_digits", "tiles_x",
          "tiles_y", "block_log2", "chunks", "chunk_size", "n_work", "sample_prefix_digits", "n_tiles", "grid", "partial_floats")


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tile_plan") / "tile_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "toy-cpu-pathtracing_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "tile_plan_check.cpp")], check=True)

    def run(cases):
        """cases: (w, h, spp, sampler, s_begin, s_end, waves, n_list) -> per case (tiles of the frame, [(list plan, frame plan)] per launch)"""
        text = "".join(" ".join(str(int(v)) for v in c) + "\n" for c in cases)
        r = subprocess.run([exe], input=text, capture_output=True, text=True, check=True)
        out = []
        for line in r.stdout.splitlines():
            tag, *vals = line.split()
            if tag == "case":
                out.append((int(vals[0]), []))
            elif tag == "l":
                out[-1][1].append([dict(zip(FIELDS, map(int, vals))), None])
            else:
                out[-1][1][-1][1] = dict(zip(FIELDS, map(int, vals)))
        assert len(out) == len(cases)
        return out
    return run


def list_sizes(total):
    return sorted({n for n in (1, 5, total // 2, total) if 1 <= n <= total})


def grid_cases():
    for w, h, spp, sampler, waves in itertools.product(lp.SIZES, lp.SIZES, lp.SPPS, (RANDOM, SOBOL), lp.WAVES):
        total = ((w + 7) // 8) * ((h + 7) // 8)
        ranges = [(0, spp)]
        if spp >= 48:
            ranges.append((16, 48))
        if spp > 4096:
            ranges.append((spp - 4096, spp))
        for (b, e), n_list in itertools.product(ranges, list_sizes(total)):
            yield (w, h, spp, sampler, b, e, waves, n_list)


def test_tile_plan_matches_frame_plan_and_keeps_the_invariants(planner):
    cases = list(grid_cases())
    assert len(cases) > 4000
    seen_full = seen_short = 0
    for case, (total, launches) in zip(cases, planner(cases)):
        w, h, spp, sampler, s_begin, s_end, waves, n_list = case
        assert total == ((w + 7) // 8) * ((h + 7) // 8), case
        log2_spp = spp.bit_length() - 1
        nb4 = (max(w, h) - 1).bit_length() + (log2_spp + 1) // 2
        odd = log2_spp & 1
        assert launches[0][0]["begin"] == s_begin and launches[-1][0]["end"] == s_end, case
        assert all(a[0]["end"] == b[0]["begin"] for a, b in zip(launches, launches[1:])), case
        for r, frame in launches:
            ctx = (case, r)
            if n_list == total:                                   # the list of all tiles: the whole-frame plan, field for field
                assert r == frame, (case, r, frame)
                seen_full += 1
            else:
                seen_short += 1
            b, e, n = r["begin"], r["end"], r["end"] - r["begin"]
            assert n > 0 and (r["sample_begin"], r["sample_end"]) == (b, e), ctx
            # what does not depend on the number of tiles is the frame's
            for k in ("spp", "seed", "max_depth", "strategy", "sampler", "log2_spp", "n_base4_digits", "tiles_x", "tiles_y"):
                assert r[k] == frame[k], (k, ctx)
            assert (r["log2_spp"], r["n_base4_digits"], r["tiles_x"] * r["tiles_y"], r["n_tiles"]) == (log2_spp, nb4, total, n_list), ctx
            bl, chunks, cs, pre = r["block_log2"], r["chunks"], r["chunk_size"], r["sample_prefix_digits"]
            # n_work = items x chunks (lane_job_tiles: work -> (item, chunk), item -> (position in the list, block)), and the grid
            assert bl <= 3 and r["n_work"] == n_list * (64 >> (2 * bl)) * chunks and r["grid"] == min(r["n_work"], waves), ctx
            # the chunks cover the range
            assert chunks >= 1 and chunks & (chunks - 1) == 0 and chunks <= n and cs == -(-n // chunks), ctx
            assert (chunks - 1) * cs < n <= chunks * cs, ctx
            # one slot per listed tile and chunk
            assert r["partial_floats"] == (n_list * chunks * 192 if chunks > 1 else 0), ctx
            if sampler == RANDOM:
                assert bl == 3 and pre == 0, ctx
            # the prefix tables' conditions
            if sampler == SOBOL:
                assert n <= 4096 and (e - 1) // 4096 == b // 4096, ctx
                if bl < 3:
                    hi_shift = 2 * ((log2_spp + 1) // 2 + bl) - odd
                    assert hi_shift >= 6 and 2 * nb4 - odd <= hi_shift + 27, ctx
            if pre > 0:
                m = log2_spp // 2 - pre
                assert sampler == SOBOL and bl == 0 and odd == 0, ctx
                assert m >= 3 and cs == 4 ** m and b % cs == 0 and n % chunks == 0 and 2 * nb4 <= 2 * m + 27, ctx
    assert seen_full > 1000 and seen_short > 1000


def test_tile_plan_pinned_shapes(planner):
    """By hand from the code: 18 tiles of a 44 x 20 frame at 16 samples on 4 096 waves are 18 whole-tile items in 2 chunks of 8 (the
    GPU tests' frame); 4 of its tiles split the same range likewise; a single tile of a 1080p frame at 1 024 spp is 16 blocks of 2 x 2
    pixels in 128 chunks of 8 samples (16 x 128 items still leave waves without one, so chunks go down to 8 samples)."""
    (_, ((r, f),)), = planner([(44, 20, 64, SOBOL, 0, 16, 4096, 18)])
    assert r == f and (r["block_log2"], r["chunks"], r["chunk_size"], r["n_work"]) == (3, 2, 8, 36)
    (_, ((r, _),)), = planner([(44, 20, 64, SOBOL, 0, 16, 4096, 4)])
    assert (r["block_log2"], r["chunks"], r["chunk_size"], r["n_work"], r["partial_floats"]) == (3, 2, 8, 8, 4 * 2 * 192)
    (_, ((r, _),)), = planner([(1920, 1080, 1024, SOBOL, 0, 1024, 4096, 1)])
    assert (r["block_log2"], r["chunks"], r["chunk_size"], r["n_work"]) == (1, 128, 8, 2048)
