"""The tail queue's staging arithmetic (csrc/tail_queue_plan.hpp: tq_stage_pushes, tq_stage_push_index, tq_stage_pop) without a GPU.
tests/tail_queue_stage_check.cpp enumerates every count waiting before a push (0 .. 127), every number of pushing lanes (0 .. 64) and
draining on and off, and stops at the first violation of what pt_kernel_body.inc relies on: an iteration stages exactly when a pass follows
its push; that pass takes every staged record and leaves none in LDS; each rank pops the slot, and so the record, that tq_push_slot /
tq_pass_take / tq_pop_slot give with everything in the global stack, and the count ends where it ends there; staged LDS indices are distinct
and below 64.  It then replays the steady cadence of the benchmark's kernel (a push of 43 records after a pass, of 62 otherwise, a pass at
64) on the plan and reports how many records were staged."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def result(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tail_queue_stage") / "tail_queue_stage_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "toy-cpu-pathtracing_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "tail_queue_stage_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    tag, *vals = r.stdout.split()
    assert tag == "ok"
    return dict(zip(("cases", "staged_cases", "cadence_pushes", "cadence_staged"), map(int, vals)))


def test_every_count_push_and_drain_state(result):
    """128 counts x 65 pushes x draining on / off, none violating the properties above; staging happens in a good part of them"""
    assert result["cases"] == 128 * 65 * 2
    assert 0 < result["staged_cases"] < result["cases"]


def test_steady_cadence_stages_most_records(result):
    """Three pushes of 43 and one of 62 per cycle, one of the 43 without a pass: 148 of 191 records never leave the CU"""
    share = result["cadence_staged"] / result["cadence_pushes"]
    print(f"staged share of the steady cadence: {share:.4f}")
    assert share > 0.70
