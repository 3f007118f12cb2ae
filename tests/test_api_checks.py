"""The pure argument predicates of csrc/api_checks.hpp (overlap, misaligned, all_finite_positive, frame_side_too_large / frame_too_large,
scratch_verdict) without a GPU and without HIP.  tests/api_checks_check.cpp compiles against that header alone and stops at the first
violation: overlap against "some byte lies in both" over every placement of two ranges of 0 .. 4 bytes in a window of 12 and with null
pointers; misaligned over the addresses 0 .. 63 for the alignments 4 and 16; the finite-and-positive predicate on 0, -0, the smallest
denormal, NaN, +-inf and 1; the frame bounds at 2^24 and 2^24 + 1, at 65536 x 65535, 65536 x 65536 and at 0; the scratch verdict's
outcomes and their precedence (missing, then too small, then misaligned).  The refusals built on them are tested per stage."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PLACEMENTS = sum(13 - n for n in range(5))                  # a range of 0 .. 4 bytes inside a window of 12
OVERLAP_CASES = PLACEMENTS ** 2 + 5 * (2 * PLACEMENTS + 5)  # every pair; one side null at every length, both null
MISALIGNED_CASES, FINITE_CASES, FRAME_CASES, SCRATCH_CASES = 2 * 64, 11, 12, 9


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("api_checks") / "api_checks_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "toy-cpu-pathtracing_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "api_checks_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    tag, n = r.stdout.split()
    assert tag == "ok"
    return int(n)


def test_every_case_holds(cases):
    """3600 overlap placements, 128 addresses, and the listed values of the other three predicates: none violated, none skipped"""
    assert OVERLAP_CASES == 3600
    assert cases == OVERLAP_CASES + MISALIGNED_CASES + FINITE_CASES + FRAME_CASES + SCRATCH_CASES
