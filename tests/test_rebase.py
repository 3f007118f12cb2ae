"""Moving the camera of a built scene (include/mi355pt_rebase.h), without a GPU: the ABI surface; csrc/rebase_plan.hpp on its own
(tests/rebase_plan_check.cpp, also under the host sanitizers); and the HOST form of the move — mi355pt_scene_debug_move_digest lowers the
scene for a new camera over the tree of the built one and refits every box with the functions the kernels call — against the recorded
digests of tests/golden/scene_lowering_digests.json, against the render-space vertices tests/geometry_stress.py computes on its own, and
against the tree validator.  tests/test_rebase_gpu.py holds the device to these digests byte for byte."""
import copy
import ctypes
import os
import platform
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geometry_stress as gs  # noqa: E402
from test_scene_lowering import CASES, GOLDEN, LIBM_ARRAYS, _describe  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "toy-cpu-pathtracing_amd", "csrc")
F = np.float32
FLT_MAX = np.finfo(F).max
FAR_STEP = (2000.0, -3.0, 0.125)
# arrays no camera translation can reach: a move must leave their bytes alone
CAMERA_FREE = re.compile(r"tris_local|cc_albedo|materials|light_uvs|luts|cmf|rgb2spec|z_nodes|texels|textures|env\d+\.\w+")


def moved(pkg, cam, step, times=1):
    """cam translated by `step`, `times` times, each sum rounded to float32 like a caller's own camera path"""
    p = np.array(cam.position[:], F)
    for _ in range(times):
        p = (p + np.asarray(step, F)).astype(F)
    return pkg.make_camera(tuple(float(v) for v in p), tuple(cam.direction[:]), tuple(cam.up[:]), cam.width, cam.height, cam.fov_deg)


def compared(names):
    """the digest names this machine's libm lets us compare with the recorded ones (tests/test_scene_lowering.py has the same caveat)"""
    same_libc = list(platform.libc_ver()) == GOLDEN["libc_ver"]
    return [n for n in names if same_libc or not LIBM_ARRAYS.fullmatch(n)]


def test_rebase_abi_surface(pkg):
    """the header declares one entry point, the library exports it, ffi.REBASE_SYMBOLS mirrors it; mi355pt.h includes the header right after
    the robust film's and ahead of the variance-guided denoiser's; the result struct is 32 bytes in C, ctypes and the generated Rust text"""
    f = pkg.ffi
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(f.ROOT, "include", "mi355pt_rebase.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(mi355pt_[a-z0-9_]+)\s*\(", hdr)))
    assert declared == sorted("mi355pt_" + s for s in f.REBASE_SYMBOLS) == ["mi355pt_scene_move_camera"]
    lib = ctypes.CDLL(f.LIB_PATH)
    assert all(hasattr(lib, n) for n in declared)
    main = open(os.path.join(f.ROOT, "include", "mi355pt.h")).read()
    includes = re.findall(r'#include "(mi355pt_\w+\.h)"', main)
    assert includes.index("mi355pt_robust.h") + 1 == includes.index("mi355pt_rebase.h") and includes[-1] == "mi355pt_denoise_var.h"
    assert "mi355pt_scene_move_camera" not in re.sub(r"/\*.*?\*/", "", main, flags=re.S)           # declared in its own header only
    assert re.search(r"MI355PT_MOVE_REBASED = 0,\s*MI355PT_MOVE_SAME_POSITION = 1,\s*MI355PT_MOVE_DEGENERATE_SET_CHANGED = 2,\s*"
                     r"MI355PT_MOVE_INSTANCE_CLASS_CHANGED = 3,\s*MI355PT_MOVE_UNSUPPORTED_BUILD = 4", hdr)
    assert f.MOVE_REASON == ["rebased", "same_position", "degenerate_set_changed", "instance_class_changed", "unsupported_build"]
    assert ctypes.sizeof(f.MoveResult) == 32 and f.MoveResult.host_ms.offset == 16 and f.MoveResult.device_ms.offset == 24
    rs = open(os.path.join(f.ROOT, "bindings", "rust", "mi355pt_sys.rs")).read()
    assert "pub fn mi355pt_scene_move_camera(s: *mut Scene, cam: *const Camera, out: *mut MoveResult) -> i32;" in rs
    assert re.search(r"pub struct MoveResult \{\s*pub rebuilt: u32,\s*pub reason: u32,\s*pub launches: u32,\s*pub host_ms: f64,\s*pub device_ms: f64,\s*\}", rs)
    assert subprocess.call([sys.executable, os.path.join(f.ROOT, "tools", "gen_rust_binding.py"), "--check"]) == 0


def test_move_refusals_without_a_device(pkg):
    """null arguments and an unbuilt scene are refused before anything asks for a device"""
    prod = pkg.Product()
    sc, cam = _describe(pkg, prod, "1")
    fn = prod.lib.mi355pt_scene_move_camera
    fn.argtypes = [ctypes.c_void_p, ctypes.POINTER(pkg.ffi.Camera), ctypes.POINTER(pkg.ffi.MoveResult)]
    assert fn(None, ctypes.byref(cam), None) == -1 and fn(sc.h, None, None) == -1                 # MI355PT_E_INVALID
    with pytest.raises(RuntimeError, match="scene not built"):
        sc.move_camera(cam)


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    """tests/rebase_plan_check.cpp built with plain g++ (rebase_plan.hpp needs no HIP) and, a second time, with the host sanitizers"""
    def build(name, extra):
        exe = str(tmp_path_factory.mktemp(name) / "rebase_plan_check")
        subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror"] + extra +
                       ["-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "rebase_plan_check.cpp")], check=True)
        return exe
    return build("plain", []), build("sanitized", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def test_plan_header_is_pure(plan_check):
    text = open(os.path.join(CSRC, "rebase_plan.hpp")).read()
    assert not re.search(r"#\s*include\s*[<\"]hip|getenv|chrono|clock_gettime|gettimeofday", text)


# (seed, triangles): 0 = the edge shapes (a root that is a leaf, the wrapped single leaf, a one-node tree, broken links); sizes around the
# leaf size, around 1024 and one large
@pytest.mark.parametrize("seed,n_tris", [(1, 0), (2, 2), (3, 5), (4, 8), (5, 9), (6, 100), (7, 1023), (8, 1024), (9, 1025), (10, 2049), (11, 20000)])
def test_plan_on_synthetic_trees(plan_check, seed, n_tris):
    """height groups partition the used (node, side) pairs with every child in a lower group, the slot map covers exactly the used slots and
    names the box the slot carries, the refit gives exact boxes and the padded slots, pad radius from the root record = the loop over the
    slots — the stand-alone program's own checks, run plain and under AddressSanitizer + UBSan"""
    for exe in plan_check:
        r = subprocess.run([exe, str(seed), str(n_tris)], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr


@pytest.mark.parametrize("case", CASES)
def test_same_camera_reproduces_the_recorded_lowering(pkg, case):
    """the pinned lowering for the SAME camera goes through the whole refit — every BVH2 box from the triangles, every 4-wide slot from its
    source, the pad from the root record — and must give the digests recorded from the builders themselves, name by name: host refit and
    re-pad reproduce both trees' boxes byte for byte (signed zeros included: camera x = 0 against vertices at x = 0 in the Cornell scenes)"""
    prod = pkg.Product()
    sc, cam = _describe(pkg, prod, case)
    gold = GOLDEN["cases"][case]
    got, info, reason = sc.debug_move_digest(cam, cam)
    assert reason == "same_position"
    assert list(got) == list(gold["digests"]) and info == gold["info"]
    for name in compared(got):
        assert got[name] == gold["digests"][name], (case, name)


@pytest.mark.parametrize("case", CASES)
def test_round_trip_and_chain(pkg, case):
    """cam -> cam + (2000, -3, 0.125) -> cam as two pinned moves gives the recorded digests again, and three steps of (0.1, 0, -0.2) give
    the digests of one move to the end position: a move is computed from the description and the tree, never from the previous position's
    records, so nothing drifts.  (On the host that holds by construction of the call; the device repeats both in tests/test_rebase_gpu.py.)
    Away from home the camera-dependent arrays differ from the recorded ones and every camera-free array keeps its bytes."""
    prod = pkg.Product()
    sc, cam = _describe(pkg, prod, case)
    gold = GOLDEN["cases"][case]["digests"]
    far = moved(pkg, cam, FAR_STEP)
    away, _, reason = sc.debug_move_digest(cam, far)
    assert reason == "rebased" and list(away) == list(gold)
    assert away["tris_render"] != gold["tris_render"] and away["nodes"] != gold["nodes"] and away["nodes4"] != gold["nodes4"] and away["instances"] != gold["instances"]
    for name in compared(away):
        if CAMERA_FREE.fullmatch(name):
            assert away[name] == gold[name], (case, name)
    back, _, reason = sc.debug_move_digest(cam, cam)                            # the second move, to the position the tree was built for
    assert reason == "same_position"
    for name in compared(back):
        assert back[name] == gold[name], (case, name)
    step = (0.1, 0.0, -0.2)
    chain = [sc.debug_move_digest(cam, moved(pkg, cam, step, k)) for k in (1, 2, 3)]
    assert [c[2] for c in chain] == ["rebased"] * 3
    assert chain[0][0]["tris_render"] != chain[1][0]["tris_render"] != chain[2][0]["tris_render"]
    end = pkg.make_camera(tuple(moved(pkg, cam, step, 3).position[:]), tuple(cam.direction[:]), tuple(cam.up[:]), cam.width, cam.height, cam.fov_deg)
    assert sc.debug_move_digest(cam, end)[0] == chain[2][0]


def _leaf(link):
    c = int(link) & 0xFFFFFFFF
    return (c & 0x7FFFFFFF) >> 3, (c & 7) + 1


def check_exported_tree(nodes, tris, root, input_tris=None):
    """gs.validate_bvh with equal boxes; the wrapped single leaf (one node whose second child is the empty point box) by hand"""
    links = nodes[:, 12:14].view(np.int32)
    if nodes.shape[0] == 1 and links[0, 0] == links[0, 1] and links[0, 0] < 0:
        f = nodes.view(F)[0]
        first, count = _leaf(links[0, 0])
        v = gs.tri_vertices(tris)[first:first + count].reshape(-1, 3)
        assert first == 0 and count == tris.shape[0]
        assert np.array_equal(f[[0, 4, 8]], v.min(axis=0)) and np.array_equal(f[[2, 6, 10]], v.max(axis=0))
        assert np.all(f[[1, 5, 9, 3, 7, 11]] == FLT_MAX)
        return
    gs.validate_bvh(nodes, tris, root, input_tris=input_tris, equal_boxes=True)


@pytest.mark.parametrize("case", CASES + ["25"])
def test_pinned_tree_of_the_scenes(pkg, case):
    """the moved tree of every lowering case (and scene 25, the other root that is a leaf): same links as at home, exact boxes, and the
    pad's radius from the root record equals pad_nodes4's own loop"""
    prod = pkg.Product()
    sc, cam = _describe(pkg, prod, case)
    n0, t0, r0, rad0 = sc.debug_move_export(cam, cam)
    far = moved(pkg, cam, (0.25, -3.0, 17.5))
    n1, t1, r1, rad1 = sc.debug_move_export(cam, far)
    assert r1 == r0 and np.array_equal(n1[:, 12:16], n0[:, 12:16]) and np.array_equal(t1[:, 9:], t0[:, 9:])      # links, pads; instance, flags, class
    assert not np.array_equal(t1[:, :9], t0[:, :9])
    for nodes, tris, root, rad in ((n0, t0, r0, rad0), (n1, t1, r1, rad1)):
        check_exported_tree(nodes, tris, root)
        assert rad[0] == rad[1] and rad[0] > 0.0
    if case in ("24", "25"):
        assert n0.shape[0] == 1


@pytest.mark.parametrize("name", gs.NAMES)
def test_pinned_lowering_on_stress_families(pkg, name):
    """adversarial geometry (counts around 1024, the world at 2000 units, x 1e3, x 1e-3, five TRS instances): at a new camera offset the
    pinned lowering's render-space vertices are Family.render32() for that offset as a multiset of records, the tree validates with
    equal boxes, and the pad radius from the root record equals the lowering's"""
    prod = pkg.Product()
    fam = gs.family(name)
    sc, cam, _ = gs.build_scene(prod, name, build=False, width=64, height=48)
    there = copy.copy(fam)
    there.offset = (fam.offset + (np.array([0.3, -0.2, 0.1], F) * F(fam.scale)).astype(F)).astype(F)
    cam2 = pkg.make_camera(tuple(float(v) for v in there.offset), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), 64, 48)
    got, info, reason = sc.debug_move_digest(cam, cam2)
    assert reason == "rebased" and "degenerate=0" in info
    nodes, tris, root, rad = sc.debug_move_export(cam, cam2)
    want = there.render32()
    assert gs.same_multiset(gs.tri_vertices(tris).reshape(-1, 9), want.reshape(-1, 9))
    gs.validate_bvh(nodes, tris, root, input_tris=want, equal_boxes=True)
    assert rad[0] == rad[1] and rad[0] > 0.0
    home_nodes, _, home_root, _ = sc.debug_move_export(cam, cam)
    assert home_root == root and np.array_equal(home_nodes[:, 12:14], nodes[:, 12:14])


def sliver_scene(pkg, backend, build=False):
    """two instances at different translations (so the triangle array is in render space) of ordinary triangles, one of them with a triangle
    whose edges are 1e-5 long: next to the camera it has a cross product, 4000 units away one float32 ulp is 2.4e-4 and its three vertices
    round to one point -> (scene, camera at home, camera 4000 away)"""
    sc = backend.new_scene()
    sc.set_rgb2spec(pkg.scenes.srgb_table())
    d = pkg.ffi.MaterialDesc(); d.type = pkg.ffi.MAT_LAMBERT; d.color = pkg.ffi.Spectrum.constant(0.7); d.normal_tex = pkg.ffi.NONE
    mat = sc.add_material(d)
    base = gs._soup(24, seed=77)
    sliver = np.array([[[0.1, 0.2, -3.0], [0.10001, 0.2, -3.0], [0.1, 0.20001, -3.0]]], F)
    g0 = sc.add_mesh(gs._mesh_dict(np.concatenate([base[:12], sliver])))
    g1 = sc.add_mesh(gs._mesh_dict(base[12:]))
    m0, m1 = np.eye(4, dtype=F), np.eye(4, dtype=F)
    m0[:3, 3] = (0.0, 0.0, 0.0); m1[:3, 3] = (0.5, 0.25, 0.0)
    sc.add_instance(g0, mat, m0); sc.add_instance(g1, mat, m1)
    sc.add_lut470(pkg.scenes.presets()["cie_illum_d6500"])
    sc.add_environment_light(1.0, np.ones((8, 16, 3), dtype=F), 0)
    cam = pkg.make_camera((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), 64, 48)
    if build:
        sc.build(cam)
    return sc, cam, moved(pkg, cam, (4000.0, 4000.0, 4000.0))


def test_fallback_when_the_degenerate_set_changes(pkg):
    prod = pkg.Product()
    sc, cam, far = sliver_scene(pkg, prod)
    _, info_home = sc.debug_lowering_digest(cam)
    _, info_far = sc.debug_lowering_digest(far)
    assert "tri_space=render" in info_home and "degenerate=0" in info_home and "degenerate=1" in info_far
    got, info, reason = sc.debug_move_digest(cam, far)
    assert reason == "degenerate_set_changed"
    fresh, fresh_info = sc.debug_lowering_digest(far)                         # a move that rebuilds gives the fresh lowering
    assert got == fresh and info == fresh_info
    back, _, reason_back = sc.debug_move_digest(far, cam)                     # ... and so does the way back: the left-out triangle returns
    assert reason_back == "degenerate_set_changed" and back == sc.debug_lowering_digest(cam)[0]
    near = moved(pkg, cam, (0.5, 0.0, 0.25))
    assert sc.debug_move_digest(cam, near)[2] == "rebased"
