"""The light-hit queue's index arithmetic (csrc/tail_queue_plan.hpp: lq_push_slot, lq_pass_due, lq_pass_take, lq_pop_slot) without a GPU.
tests/light_queue_check.cpp enumerates every count waiting (0 .. 127) and every number of pushing lanes (0 .. 64) on a model of the stack
and stops at the first violation of what pt_kernel_body.inc relies on: push slots are distinct, consecutive, on top of the waiting records
and inside the stack; a due pass pops exactly the newest min(64, count) records, each once, and leaves the others in slots [0, count); the
pass at the end of a work item empties the stack; the count never exceeds 127.  It then replays a long random schedule of pushes, passes
and ends of items on the same model."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def result(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("light_queue") / "light_queue_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "toy-cpu-pathtracing_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "light_queue_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    tag, *vals = r.stdout.split()
    assert tag == "ok"
    return dict(zip(("cases", "passes", "max_count"), map(int, vals)))


def test_every_count_and_push(result):
    """128 counts x 65 pushes, none violating the properties above, with passes among them"""
    assert result["cases"] == 128 * 65
    assert result["passes"] > result["cases"]


def test_the_bound_is_reached_and_never_passed(result):
    """63 left by a pass and 64 pushed: 127 records wait at the most, inside the 128 slots"""
    assert result["max_count"] == 127
