"""The launch shape (csrc/launch_plan.hpp) without a GPU: the host arithmetic that decides the pixel block and sample chunk of a work item,
the Sobol prefix digits and the split of long sample ranges, compiled for the host and checked against what the kernels' lane_job and
prefix-table code (pt_kernel.hpp) rely on."""
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANDOM, SOBOL = 0, 1
SIZES = (1, 7, 8, 9, 64, 100, 1920, 4096, 16384)
SPPS = (1, 3, 8, 64, 512, 1024, 2048, 4096, 16384)
SHARDS = ((0, 1), (2, 3), (4000, 4001))          # (shard_index, shard_count)
WAVES = (64, 4096)
FIELDS = ("begin", "end", "sample_begin", "sample_end", "log2_spp", "n_base4_digits", "block_log2", "chunks", "chunk_size", "n_work",
          "sample_prefix_digits", "tiles_total", "n_tiles", "grid", "partial_floats")


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("launch_plan") / "launch_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "toy-cpu-pathtracing_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "launch_plan_check.cpp")], check=True)

    def run(cases):
        """cases: (w, h, spp, sampler, shard_index, shard_count, s_begin, s_end, waves, aov) -> per case (tiles of the shard, [launch dict])"""
        text = "".join(" ".join(str(int(v)) for v in c) + "\n" for c in cases)
        r = subprocess.run([exe], input=text, capture_output=True, text=True, check=True)
        out = []
        for line in r.stdout.splitlines():
            tag, *vals = line.split()
            if tag == "case":
                out.append((int(vals[0]), []))
            else:
                out[-1][1].append(dict(zip(FIELDS, map(int, vals))))
        assert len(out) == len(cases)
        return out
    return run


def grid_cases():
    for w, h, spp, sampler, (si, sc), waves, aov in itertools.product(SIZES, SIZES, SPPS, (RANDOM, SOBOL), SHARDS, WAVES, (0, 1)):
        ranges = [(0, spp)]
        if spp >= 48:
            ranges.append((16, 48))
        if spp > 4096:
            ranges.append((spp - 4096, spp))
        for b, e in ranges:
            yield (w, h, spp, sampler, si, sc, b, e, waves, aov)


def test_launch_plan_invariants(planner):
    cases = list(grid_cases())
    assert len(cases) > 2000
    for case, (tiles, launches) in zip(cases, planner(cases)):
        w, h, spp, sampler, si, sc, s_begin, s_end, waves, aov = case
        tiles_total = ((w + 7) // 8) * ((h + 7) // 8)
        log2_spp = spp.bit_length() - 1
        nb4 = (max(w, h) - 1).bit_length() + (log2_spp + 1) // 2
        odd = log2_spp & 1
        # I6
        assert tiles == len(range(si, tiles_total, sc)), case
        # I5
        assert launches[0]["begin"] == s_begin and launches[-1]["end"] == s_end, case
        assert all(a["end"] == b["begin"] for a, b in zip(launches, launches[1:])), case
        if sampler == RANDOM:
            assert len(launches) == 1, case
        for r in launches:
            ctx = (case, r)
            b, e, n = r["begin"], r["end"], r["end"] - r["begin"]
            assert n > 0 and (r["sample_begin"], r["sample_end"]) == (b, e), ctx
            assert (r["log2_spp"], r["n_base4_digits"], r["tiles_total"], r["n_tiles"]) == (log2_spp, nb4, tiles_total, tiles), ctx
            if sampler == SOBOL:
                assert n <= 4096 and (e - 1) // 4096 == b // 4096, ctx           # no multiple of 4096 strictly inside
            bl, chunks, cs, pre = r["block_log2"], r["chunks"], r["chunk_size"], r["sample_prefix_digits"]
            # I1
            assert bl <= 3 and r["n_work"] == tiles * (64 >> (2 * bl)) * chunks and r["grid"] == min(r["n_work"], waves), ctx
            # I2
            assert chunks >= 1 and chunks & (chunks - 1) == 0 and chunks <= n and cs == -(-n // chunks), ctx
            assert r["partial_floats"] == (tiles * chunks * 192 if chunks > 1 else 0), ctx
            if aov:
                assert chunks == 1, ctx
            if sampler == RANDOM:
                assert bl == 3 and pre == 0, ctx
            # I3
            if sampler == SOBOL and bl < 3:
                hi_shift = 2 * ((log2_spp + 1) // 2 + bl) - odd
                assert hi_shift >= 6 and 2 * nb4 - odd <= hi_shift + 27, ctx
            # I4
            if pre > 0:
                m = log2_spp // 2 - pre
                assert sampler == SOBOL and bl == 0 and odd == 0, ctx
                assert m >= 3 and cs == 4 ** m and b % cs == 0 and n % chunks == 0 and 2 * nb4 <= 2 * m + 27, ctx


def test_launch_plan_pinned_shapes(planner):
    """Plans worked out by hand from the code: a change of any of them changes the frames' bits (block size, chunking, prefix digits)."""
    def one(w, h, spp, waves=4096):
        return planner([(w, h, spp, SOBOL, 0, 1, 0, spp, waves, 0)])[0][1]

    def pick(r, *keys):
        return tuple(r[k] for k in keys)
    (r,) = one(1920, 1080, 1024)
    assert pick(r, "block_log2", "chunks", "n_work", "sample_prefix_digits") == (1, 1, 518400, 0)
    rs = one(1920, 1080, 16384)
    assert [(r["begin"], r["end"]) for r in rs] == [(0, 4096), (4096, 8192), (8192, 12288), (12288, 16384)]
    for r in rs:
        assert pick(r, "block_log2", "chunks", "n_work", "sample_prefix_digits") == (0, 1, 2073600, 1)
    (r,) = one(8, 16384, 4096)
    assert r["block_log2"] == 1                                                      # the 27-bit rule
    (r,) = one(64, 48, 8)
    assert pick(r, "block_log2", "chunks", "n_work") == (3, 1, 48)
    (r,) = one(64, 48, 64)
    assert pick(r, "block_log2", "chunks", "chunk_size", "n_work") == (3, 8, 8, 384)
