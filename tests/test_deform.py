"""Deforming meshes of a built scene (include/mi355pt_deform.h), without a GPU: the ABI surface; the refusals that need no device;
csrc/deform_plan.hpp on its own (tests/deform_plan_check.cpp, also under the host sanitizers); and the HOST form of the deformation —
mi355pt_scene_debug_set_mesh_vertices updates the description of a pinned scene, mi355pt_scene_debug_pinned_digest lowers it over the kept
topology and refits every box with the functions the kernels call — against the tree validator and a fresh lowering of a scene described
with the deformed mesh from the start.  tests/test_deform_gpu.py holds the device to these digests byte for byte."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geometry_stress as gs  # noqa: E402
from test_instance_move import describe  # noqa: E402
from test_rebase import check_exported_tree  # noqa: E402
from test_scene_lowering import CASES  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "toy-cpu-pathtracing_amd", "csrc")
F = np.float32

# the mesh each case deforms (one mesh per instance in the package's scenes, so the geom id is the instance id): a wall, the emitter and
# the 12-triangle box of scene 3's room, the 20 k-triangle hero of scene 17, the textured emitter of scene 31, the ONE mesh of "instanced"
WALL, EMITTER3, BOX, HERO17, EMITTER31, SHARED = ("3", 2), ("3", 7), ("3", 1), ("17", 0), ("31", 7), ("instanced", 0)


class Remeshed:
    """a backend whose new scenes record the meshes they are given (sc.meshes, by geom id, as given) and take other vertex arrays for some
    geom ids while they are described: the way to a scene DESCRIBED with a deformed mesh from the start, through the package's own scene
    descriptions.  replace: {geom: (pos, nrm or None, tangent or None)}"""

    def __init__(self, backend, replace=None):
        self._backend, self._replace = backend, replace or {}

    def __getattr__(self, name):
        return getattr(self._backend, name)

    def new_scene(self):
        sc = self._backend.new_scene()
        add, replace = sc.add_mesh, self._replace
        sc.meshes = []

        def add_mesh(mesh):
            m = dict(mesh)
            if len(sc.meshes) in replace:
                pos, nrm, tan = replace[len(sc.meshes)]
                m["pos"] = pos
                if nrm is not None:
                    m["nrm"] = nrm
                if tan is not None:
                    m["tangent"] = tan
            sc.meshes.append(m)
            return add(m)
        sc.add_mesh = add_mesh
        return sc


def arrays_of(mesh):
    """(pos, nrm, tangent or None) of a recorded mesh: what puts it back"""
    return (np.asarray(mesh["pos"], F).reshape(-1, 3), np.asarray(mesh["nrm"], F).reshape(-1, 3),
            None if mesh.get("tangent") is None else np.asarray(mesh["tangent"], F).reshape(-1, 3))


def deformed(mesh, seed=1, amp=0.03):
    """a seeded smooth displacement of a recorded mesh: every position moves by amp x the mesh's largest extent x sin(k . p + phase) per
    axis, with wavelengths of half to twice the extent — far too smooth and too small to collapse a triangle; the normals are bent by a
    cosine field and handed over UNnormalised (the library normalises), the tangents (a mesh with uv) likewise"""
    rng = np.random.default_rng(seed)
    pos, nrm, tan = arrays_of(mesh)
    p = pos.astype(np.float64)
    ext = float((p.max(axis=0) - p.min(axis=0)).max())
    k = rng.uniform(0.5, 2.0, (3, 3)) * (2.0 * np.pi / ext)
    ph = rng.uniform(0.0, 2.0 * np.pi, 3)
    wave = p @ k.T + ph
    new_pos = (p + amp * ext * np.sin(wave)).astype(F)
    new_nrm = (nrm.astype(np.float64) + 0.25 * np.cos(wave)).astype(F)
    new_tan = None
    if tan is not None:
        c = p[np.asarray(mesh["idx"], np.uint32).reshape(-1, 3)].mean(axis=1)
        new_tan = (tan.astype(np.float64) + 0.1 * np.sin(c @ k.T + ph)).astype(F)
    return new_pos, new_nrm, new_tan


def test_deform_abi_surface(pkg):
    """the header declares one entry point, the library exports it, ffi.DEFORM_SYMBOLS mirrors it; mi355pt.h includes the header right
    after the object-motion block's and ahead of the variance-guided denoiser's and declares nothing itself; the struct has the header's
    layout in ctypes and in the generated Rust text; the new reason is numbered after the instance move's; the debug header declares the
    host-only twin"""
    f = pkg.ffi
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(f.ROOT, "include", "mi355pt_deform.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(mi355pt_[a-z0-9_]+)\s*\(", hdr)))
    assert declared == sorted("mi355pt_" + s for s in f.DEFORM_SYMBOLS) == ["mi355pt_scene_deform_meshes"]
    lib = ctypes.CDLL(f.LIB_PATH)
    assert all(hasattr(lib, n) for n in declared) and hasattr(lib, "mi355pt_scene_debug_set_mesh_vertices")
    main = open(os.path.join(f.ROOT, "include", "mi355pt.h")).read()
    includes = re.findall(r'#include "(mi355pt_\w+\.h)"', main)
    assert includes.index("mi355pt_motion.h") + 1 == includes.index("mi355pt_deform.h") and includes[-1] == "mi355pt_denoise_var.h"
    assert "mi355pt_scene_deform_meshes" not in re.sub(r"/\*.*?\*/", "", main, flags=re.S)
    assert re.search(r"enum \{ MI355PT_MOVE_SAME_VERTICES = 7 \};", hdr)
    assert f.DEFORM_REASON == f.INSTANCE_MOVE_REASON + ["same_vertices"] and len(f.DEFORM_REASON) == 8
    assert re.search(r"typedef struct mi355pt_mesh_update \{\s*uint32_t geom;\s*const float\* pos;\s*const float\* nrm;\s*const float\* tri_tangent;\s*\} mi355pt_mesh_update;", hdr)
    p = ctypes.sizeof(ctypes.c_void_p)
    assert ctypes.sizeof(f.MeshUpdate) == 4 * p and (f.MeshUpdate.geom.offset, f.MeshUpdate.pos.offset, f.MeshUpdate.nrm.offset, f.MeshUpdate.tri_tangent.offset) == (0, p, 2 * p, 3 * p)
    rs = open(os.path.join(f.ROOT, "bindings", "rust", "mi355pt_sys.rs")).read()
    assert ("pub fn mi355pt_scene_deform_meshes(s: *mut Scene, cam: *const Camera, updates: *const MeshUpdate, n: u32, "
            "p: *const InstanceMoveParams, out: *mut InstanceMoveResult) -> i32;") in rs
    assert re.search(r"pub struct MeshUpdate \{\s*pub geom: u32,\s*pub pos: \*const f32,\s*pub nrm: \*const f32,\s*pub tri_tangent: \*const f32,\s*\}", rs)
    assert "pub const MI355PT_MOVE_SAME_VERTICES: u32 = 7;" in rs
    assert subprocess.call([sys.executable, os.path.join(f.ROOT, "tools", "gen_rust_binding.py"), "--check"]) == 0
    dbg = re.sub(r"/\*.*?\*/", "", open(os.path.join(f.ROOT, "include", "mi355pt_debug.h")).read(), flags=re.S)
    assert "int mi355pt_scene_debug_set_mesh_vertices(mi355pt_scene* s, const mi355pt_mesh_update* updates, uint32_t n);" in dbg
    text = open(os.path.join(f.ROOT, "include", "mi355pt_deform.h")).read()
    assert "launches = 6 + the number of node heights" in text and "LIMITS." in text and "mi355pt_motion.h" in text


def test_refusals_without_a_device(pkg):
    """null arguments, n = 0, ids out of order or out of range, a null position array, a tangent for a mesh without uv and a non-finite
    position are refused with MI355PT_E_INVALID, and an unbuilt scene with MI355PT_E_NOT_BUILT — all before anything asks for a device, the
    description left as it was; the debug twin applies the same checks of the arrays"""
    f = pkg.ffi
    prod = Remeshed(pkg.Product())
    sc, cam = describe(pkg, prod, "3")
    before = sc.debug_lowering_digest(cam)
    fn = prod.lib.mi355pt_scene_deform_meshes
    fn.argtypes = [ctypes.c_void_p, ctypes.POINTER(f.Camera), ctypes.POINTER(f.MeshUpdate), ctypes.c_uint32, ctypes.POINTER(f.InstanceMoveParams),
                   ctypes.POINTER(f.InstanceMoveResult)]
    good = {g: deformed(sc.meshes[g]) for g in (0, 1, 2)}
    ups, keep = sc._mesh_updates({1: good[1]})
    assert fn(None, ctypes.byref(cam), ups, 1, None, None) == -1 and fn(sc.h, None, ups, 1, None, None) == -1            # MI355PT_E_INVALID
    assert fn(sc.h, ctypes.byref(cam), None, 1, None, None) == -1 and fn(sc.h, ctypes.byref(cam), ups, 0, None, None) == -1
    with pytest.raises(RuntimeError, match="code -3.*scene not built"):
        sc.deform_meshes(cam, {1: good[1]})
    with pytest.raises(RuntimeError, match="code -1.*bad geom id"):
        sc.deform_meshes(cam, {len(sc.meshes): good[1]})
    two, keep2 = sc._mesh_updates({1: good[1], 2: good[2]})
    two[0], two[1] = two[1], two[0]
    assert fn(sc.h, ctypes.byref(cam), two, 2, None, None) == -1 and b"strictly ascending" in prod.lib.mi355pt_last_error()
    two[0] = two[1]
    assert fn(sc.h, ctypes.byref(cam), two, 2, None, None) == -1 and b"strictly ascending" in prod.lib.mi355pt_last_error()
    with pytest.raises(RuntimeError, match="code -1.*null vertex positions"):
        sc.deform_meshes(cam, {1: (None, good[1][1], None)})
    assert sc.meshes[1].get("uv") is None and sc.meshes[0].get("uv") is not None                # the box has no uv, the hero has
    with pytest.raises(RuntimeError, match="code -1.*without uv"):
        sc.deform_meshes(cam, {1: (good[1][0], None, np.zeros((12, 3), F))})
    for bad_value in (np.nan, np.inf):
        bad = good[1][0].copy(); bad[5, 1] = bad_value
        with pytest.raises(RuntimeError, match="code -1.*non-finite vertex position"):
            sc.deform_meshes(cam, {0: good[0], 1: (bad, None, None)})
        with pytest.raises(RuntimeError, match="code -1.*non-finite vertex position"):
            sc.debug_set_mesh_vertices({0: good[0], 1: (bad, None, None)})
    with pytest.raises(RuntimeError, match="code -1.*rebuild_above"):
        sc.deform_meshes(cam, {1: good[1]}, rebuild_above=-1.0)
    with pytest.raises(RuntimeError, match="code -1.*bad geom id"):
        sc.debug_set_mesh_vertices({99: good[1]})
    assert sc.debug_lowering_digest(cam) == before                                               # nothing reached the description


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    """tests/deform_plan_check.cpp built with plain g++ (the header needs no HIP) and, a second time, with the host sanitizers"""
    def build(name, extra):
        exe = str(tmp_path_factory.mktemp(name) / "deform_plan_check")
        subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror"] + extra +
                       ["-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "deform_plan_check.cpp")], check=True)
        return exe
    return build("plain", []), build("sanitized", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def test_plan_header_is_pure(plan_check):
    text = open(os.path.join(CSRC, "deform_plan.hpp")).read()
    assert not re.search(r"#\s*include\s*[<\"]hip|getenv|chrono|clock_gettime|gettimeofday|scene\.hpp|layout\.hpp", text)


# (seed, meshes): none; one; a few; many
@pytest.mark.parametrize("seed,n", [(1, 0), (2, 1), (3, 2), (4, 7), (5, 40), (6, 200)])
def test_plan_layout(plan_check, seed, n):
    """disjoint staging ranges in the updates' order, the per-instance table, the moved mask, the device's table and a host restatement of
    the kernel's gather, the refusals, the same-bytes test — the stand-alone program's own checks, plain and under ASan + UBSan"""
    for exe in plan_check:
        r = subprocess.run([exe, str(seed), str(n)], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr


@pytest.mark.parametrize("case", CASES)
def test_pinned_digest_at_unchanged_arrays(pkg, case):
    """the debug twin given every mesh's own arrays changes nothing: the pinned digests stay the lowering's, name by name"""
    prod = Remeshed(pkg.Product())
    sc, cam = describe(pkg, prod, case)
    want = sc.debug_lowering_digest(cam)
    sc.debug_pin_host_tree(cam)
    sc.debug_set_mesh_vertices({g: arrays_of(m) for g, m in enumerate(sc.meshes)})
    assert sc.debug_pinned_digest(cam) == want


def tri_rows(tris):
    return np.ascontiguousarray(tris[:, :9]).view(F)


@pytest.mark.parametrize("case,geom", [WALL, EMITTER3, BOX, HERO17, EMITTER31, SHARED, ("3:general", 2)])
def test_pinned_tree_after_a_deformation(pkg, case, geom):
    """a mesh of a pinned scene takes a smooth displacement (positions, normals, tangents where it has uv): the pinned export keeps every
    link and every (instance, flags, class) word, has exact boxes over the NEW triangles (check_exported_tree), only triangles of instances
    of that mesh moved, and exactly the arrays a deformation can reach differ from the pin's; its triangles, as a multiset of records, and
    its tree-order-free arrays are those of a fresh lowering of a scene DESCRIBED with the deformed mesh; the old arrays restore the digests"""
    prod = Remeshed(pkg.Product())
    sid = case.partition(":")[0]
    sc, cam = describe(pkg, prod, case)
    sc.debug_pin_host_tree(cam)
    home = sc.debug_pinned_digest(cam)
    assert home == sc.debug_lowering_digest(cam)
    local_mode = "tri_space=local" in home[1]
    assert local_mode == (case in ("3", "31"))                                     # the Cornell rooms in their default lowering: the local-triangle mode
    n0, t0, r0, ent0 = sc.debug_pinned_export(cam)
    new = deformed(sc.meshes[geom])
    sc.debug_set_mesh_vertices({geom: new})
    n1, t1, r1, ent1 = sc.debug_pinned_export(cam)
    assert r1 == r0 and np.array_equal(n1[:, 12:16], n0[:, 12:16]) and np.array_equal(t1[:, 9:], t0[:, 9:]) and np.array_equal(ent0, ent1)
    moved_rows = (t1[:, :9] != t0[:, :9]).any(axis=1)
    users = {i for i, inst in enumerate(sc.instances) if inst[0] == geom}
    assert moved_rows.any() and set(t1[moved_rows, 9].tolist()) == users and (len(users) == 5) == (sid == "instanced")
    check_exported_tree(n1, t1, r1)
    got = sc.debug_pinned_digest(cam)
    differ = {n for n in got[0] if got[0][n] != home[0][n]}
    emitter = (sid, geom) in (EMITTER3, EMITTER31)
    assert differ == {"nodes", "nodes4", "tris_render", "tris_local", "shade"} | ({"lights", "light_tris"} if emitter else set()), differ
    assert got[1] == home[1]
    s2, _ = describe(pkg, Remeshed(pkg.Product(), {geom: new}), case)
    fresh = s2.debug_lowering_digest(cam)
    for name in ("instances", "lights", "light_tris", "light_uvs", "materials", "texels"):
        assert got[0][name] == fresh[0][name], name
    s2.debug_pin_host_tree(cam)
    _, t2, _, _ = s2.debug_pinned_export(cam)
    assert gs.same_multiset(tri_rows(t1), tri_rows(t2)) and sorted(map(tuple, t1[:, 9:].tolist())) == sorted(map(tuple, t2[:, 9:].tolist()))
    sc.debug_set_mesh_vertices({geom: arrays_of(sc.meshes[geom])})
    assert sc.debug_pinned_digest(cam) == home


def test_partial_arrays_keep_the_rest(pkg):
    """positions alone keep normals and tangents; normals alone (positions as they are) change the shading records only"""
    prod = Remeshed(pkg.Product())
    sc, cam = describe(pkg, prod, "3")
    sc.debug_pin_host_tree(cam)
    home = sc.debug_pinned_digest(cam)[0]
    pos, nrm, tan = deformed(sc.meshes[0])
    old = arrays_of(sc.meshes[0])
    sc.debug_set_mesh_vertices({0: (old[0], nrm, tan)})
    got = sc.debug_pinned_digest(cam)[0]
    assert {n for n in got if got[n] != home[n]} == {"shade"}
    sc.debug_set_mesh_vertices({0: (pos, None, None)})
    at_once = describe(pkg, prod, "3")[0]
    at_once.debug_pin_host_tree(cam)
    at_once.debug_set_mesh_vertices({0: (pos, nrm, tan)})
    assert sc.debug_pinned_digest(cam) == at_once.debug_pinned_digest(cam) and sc.debug_pinned_digest(cam)[0]["tris_local"] != home["tris_local"]
