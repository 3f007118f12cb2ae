"""The early end of roulette-doomed paths (csrc/path_end_plan.hpp) without a GPU.

tests/path_end_check.cpp holds the header's three pure functions to restatements of what they replace: the box test to the traversals'
watertight triangle test (whenever a triangle of a light is hit, the light's padded box must be reachable: rays at edges and vertices,
axis-parallel directions, origins on a box face, flat boxes, coordinates from 1 to 60 000, render-space and shifted local vertices), the
decision and the zero-term test to the front's own statements on random and adversarial values.  It is built a second time with
-fsanitize=address,undefined and run as its own executable.  The host side of the boxes and the per-launch switch are checked here too."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "toy-cpu-pathtracing_amd", "csrc")
FIELDS = ("lights", "rays", "hits", "edge_hits", "axis_hits", "far", "far_away", "decisions", "doomed", "nonzero_terms")


def build_checker(tmp_path_factory, name, extra):
    exe = str(tmp_path_factory.mktemp(name) / "path_end_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror"] + extra +
                   ["-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "path_end_check.cpp")], check=True)

    def run(seed):
        r = subprocess.run([exe, str(seed)], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        tag, *vals = r.stdout.split()
        assert tag == "ok", r.stdout
        return dict(zip(FIELDS, map(int, vals)))
    return run


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return build_checker(tmp_path_factory, "path_end", [])


@pytest.fixture(scope="module")
def checker_sanitized(tmp_path_factory):
    return build_checker(tmp_path_factory, "path_end_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_no_hit_on_a_light_is_turned_away_and_the_decision_is_the_fronts(checker, seed):
    r = checker(seed)
    assert r["lights"] == 4 * 3 * 2 * 6                                   # scales x kinds x vertex forms x repetitions
    assert r["hits"] > 40000 and r["edge_hits"] > 20000 and r["axis_hits"] > 5000     # the brute force found what the box must let through
    assert r["far_away"] > 0.9 * r["far"]                                  # and the box is a test, not a constant: rays sent past it are turned away
    assert r["decisions"] > 1_000_000 and 0.2 * r["decisions"] < r["doomed"] < 0.9 * r["decisions"]
    assert r["nonzero_terms"] > 100000                                     # inf / NaN throughputs and weights were among the inputs


def test_the_functions_are_clean_under_address_and_undefined_behaviour_sanitizers(checker_sanitized):
    r = checker_sanitized(4)
    assert r["hits"] > 40000 and r["decisions"] > 1_000_000


def test_the_header_is_pure_and_the_switch_is_per_launch(tmp_path):
    """path_end_plan.hpp compiles alone with a host compiler (no HIP in it); the switch follows MI355PT_NO_LIGHT_QUEUE's rules; the new flag
    shares a dword with queue_stage and light_queue, so the device's scene record keeps its size"""
    src = tmp_path / "t.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include <cstdlib>\n#include "path_end_plan.hpp"\n#include "launch_plan.hpp"\n'
                   "using namespace pt;\n"
                   "static_assert(offsetof(DevScene, early_path_end) / 4 == offsetof(DevScene, queue_stage) / 4 && "
                   "offsetof(DevScene, light_queue) / 4 == offsetof(DevScene, queue_stage) / 4, \"one dword\");\n"
                   "static_assert(sizeof(DevScene) == offsetof(DevScene, queue_stage) + 4, \"the flags' dword is the record's last\");\n"
                   "int main() {\n"
                   "    const KernelKey prod{false, false, MODE_MIS_SOBOL, 1u}, inst{false, true, MODE_GENERIC, 251u};\n"
                   "    std::printf(\"%d %d %d %d\\n\", (int)early_path_end_enabled(), (int)use_early_path_end(prod, true), (int)use_early_path_end(prod, false),\n"
                   "                (int)use_early_path_end(inst, true));\n"
                   "    return 0;\n}\n")
    exe = str(tmp_path / "t")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)], check=True)
    text = open(os.path.join(CSRC, "path_end_plan.hpp")).read()
    assert "hip" not in text.lower().replace("no hip in it", "")
    env = {k: v for k, v in os.environ.items() if k != "MI355PT_NO_EARLY_PATH_END"}
    for value, enabled in ((None, 1), ("1", 0), ("0", 1), ("", 1), ("yes", 0)):
        e = dict(env) if value is None else dict(env, MI355PT_NO_EARLY_PATH_END=value)
        out = subprocess.run([exe], env=e, capture_output=True, text=True, check=True).stdout.split()
        assert out == [str(enabled), "1", "0", "0"], (value, out)
