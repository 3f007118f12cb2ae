"""The tail queue's index arithmetic (csrc/tail_queue_plan.hpp) without a GPU: tests/tail_queue_plan_check.cpp runs a wave's schedule —
front, push, pass, drain — on the header's functions for seeded random sequences and stops at the first violation of what
pt_kernel_body.inc relies on: every pushed record popped exactly once, no live slot overwritten, no slot index at the capacity, at most 127
records waiting with one queue and 191 in both together with two, consecutive ranks on consecutive slots, and the newest records first (a
pass that follows a push takes the records just pushed before any older one)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("pushes", "pops", "passes", "max1", "max2", "max_total", "fresh_passes", "drain_passes")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tail_queue_plan") / "tail_queue_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "toy-cpu-pathtracing_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "tail_queue_plan_check.cpp")], check=True)

    def run(two_queues, capacity, seed, items=200):
        r = subprocess.run([exe, str(int(two_queues)), str(capacity), str(seed), str(items)], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        tag, *vals = r.stdout.split()
        assert tag == "ok"
        return dict(zip(FIELDS, map(int, vals)))
    return run


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_one_queue_of_128(checker, seed):
    """The kernels without the clearcoat code: one stack of PT_TAILQ_RING1 = 128 entries"""
    r = checker(False, 128, seed)
    assert r["pushes"] == r["pops"] > 100000 and r["max2"] == 0
    assert r["max1"] == 127                                                  # the bound is reached, never passed
    assert r["drain_passes"] > 0 and r["fresh_passes"] > 0.9 * r["passes"]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_two_queues_of_256(checker, seed):
    """The clearcoat kernels: two stacks of QUEUE_RING = 256 entries, the class with its own queue first"""
    r = checker(True, 256, seed)
    assert r["pushes"] == r["pops"] > 100000
    assert 127 < r["max_total"] <= 191 and r["max1"] < 256 and r["max2"] < 256
    assert r["drain_passes"] > 0 and r["fresh_passes"] > 0.9 * r["passes"]
