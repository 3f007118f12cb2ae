"""The case table behind "every compiled production path kernel is launched and compared" (tests/test_kernel_matrix.py without a GPU,
tests/test_kernel_matrix_gpu.py on one), and the host-compiled kernel selector both they and tests/test_kernel_select.py ask.

csrc/launch_plan.hpp compiles every feature set of FEATURE_SETS in every MODE_*, once for the shard launch (pt_kernel<false, set, mode>) and once
for the tile-list launch (pt_kernel_tiles<set, mode>).  A scene runs the first set that covers its features, so a kernel is reached only by a
scene that lowers to exactly its set's class: one PRIMARY scene per set, each under all six (strategy, sampler) pairs.  MODE_PT is reached under
both samplers and MODE_GENERIC under both strategies, because the kernel reads the choice at run time."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEX, DIEL, CC, MLIGHT, ROUGH, METAL, DELTA, ENV, EMTEX = (1 << i for i in range(9))
STD, ALL = 255, 511
MODE_NAMES = {0: "generic", 1: "mis_sobol", 2: "nee_sobol", 3: "pt"}
STRATEGY = {"pt": 0, "nee": 1, "mis": 2}                       # MI355PT_STRATEGY_* / MI355PT_SAMPLER_* (include/mi355pt.h)
SAMPLER = {"random": 0, "sobol": 1}
PAIRS = [(st, sa) for st in ("mis", "nee", "pt") for sa in ("sobol", "random")]

# compiled feature set -> the scene that selects it.  (Scenes 1 and 2 select DELTA | MLIGHT too, but have point lights only: their frame
# under `pt` is exactly black, and a black frame compares nothing.  Scene 11 selects DIEL | ROUGH and matches the oracle under all six pairs,
# but its rough SF11 glass makes NaN samples under MIS below 370 nm like the reference's (tests/test_parity_gpu.py
# test_other_scenes_radiance_parity): the unresolved 44 x 20 film of the tile-list test has NaN pixels, on the oracle too, and a mean with a
# NaN in it is no brightness floor.  Scene 12, rough BK7 glass, has none.)  Other scenes of the same set, should one have to be replaced:
# 0: 34; TEX: 4, 5, 35; DIEL: 9, 10, 13; METAL: 6; DIEL|ROUGH: 14; STD&~CC: 29; CC: 16, 20, 36; CC|TEX: 15, 22; ALL: 30, 32.
PRIMARY = {
    0: 0,
    TEX: 3,
    DIEL: 8,
    METAL: 7,
    DIEL | ROUGH: 12,
    DELTA | MLIGHT: 21,
    STD & ~CC: 27,
    CC: 17,
    CC | TEX: 18,
    STD: 19,
    ALL: 31,
}
# (feature set, scene, strategy, sampler)
CASES = [(fset, scene, st, sa) for fset, scene in PRIMARY.items() for st, sa in PAIRS]
CASE_IDS = [f"set{fset}-scene{scene}-{st}-{sa}" for fset, scene, st, sa in CASES]


def compile_selector(tmp_dir):
    """tests/kernel_select_check.cpp built with plain g++ and run: {"k": {(tiles, stats, feat, sampler, strategy): (tiles, stats, mode, set)},
    "sets": [...], "plain": [...], "cc": [...], "modes": [...]}"""
    exe = os.path.join(str(tmp_dir), "kernel_select_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "toy-cpu-pathtracing_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "kernel_select_check.cpp")], check=True)
    out = {"k": {}}
    for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines():
        tag, *vals = line.split()
        vals = list(map(int, vals))
        if tag == "k":
            out["k"][tuple(vals[:5])] = tuple(vals[5:])
        else:
            out[tag] = vals
    return out


def info_features(info):
    """the feature mask at the end of scene_info's / debug_lowering_digest's text"""
    return int(re.search(r" features=(\d+)", info).group(1))


def lowered_features(pkg, prod, scene_id):
    """what the scene lowers to on the host, nothing built or uploaded (as tests/test_scene_lowering.py describes its cases)"""
    sc = prod.new_scene()
    cam = pkg.scenes.load_scene(sc, scene_id, 64, 48, tex_size=16, build=False)
    return info_features(sc.debug_lowering_digest(cam)[1])


def case_key(selector, tiles, features, strategy, sampler):
    """the production kernel (tiles, stats, mode, set) a launch of the case takes"""
    return selector["k"][(int(tiles), 0, features, SAMPLER[sampler], STRATEGY[strategy])]
