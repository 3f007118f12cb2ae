#!/usr/bin/env python3
"""What a mesh deformation costs (include/mi355pt_deform.h) against what it replaces, on one GPU, in one process, and what a refit does
to the tree of a mesh that is bent.

TIMING.  For scene 3 in its default lowering (the local-triangle mode; the hero deforms), scene 17 (the hero deforms) and the 512 x 257
blob mesh of tests/test_bvh_gpu.py under the GPU builder (262 k triangles; the blob deforms), at 1920 x 1080: two scenes of the same
description are built at the same camera.  After WARMUP rounds, RUNS rounds ALTERNATE between
  build    the wall time of the whole mi355pt_scene_build call — lowering, tree, collapse, every hipMalloc and hipMemcpy: what a caller
           pays per frame to change vertices without the deform call (the build is of the undeformed scene: the same work); and
  deform   mi355pt_scene_deform_meshes on the other scene to the round's pose, positions and normals: its host_ms (wall time of the
           call, the upload of the new arrays included) and device_ms (HIP events around its launches), with `launches`.
The pose of round k is a wave y += 0.01 extent sin(2 pi x / extent + 0.1 k) with area-weighted vertex normals, so no call finds
unchanged arrays.  After the last round the deformed scene's device digests are compared with the host's pinned lowering
(mi355pt_scene_debug_pinned_digest): the timed calls computed the right bytes.  For the "one extra streaming pass" comparison a third
scene of the same description, the deformed mesh's instance marked dynamic, takes mi355pt_scene_move_instances in the same rounds.

TREE QUALITY.  The hero of scene 17 bent — y += a extent sin(pi (x - x_min) / extent), a from 1 % to 50 % —: sah_after / sah_built as the
call reports them, and the device time of a 4-spp MIS frame on the refit tree against the same frame on a scene described with the bent
mesh and built (median of RUNS each, alternating).

Writes one JSON object to profiles/deform_rate.json (or the path given).  Needs a GPU; reads nothing outside the repository.
usage: tools/deform_rate.py [RUNS (default 20, at least 20)] [OUTPUT.json]"""
import importlib, json, os, statistics, sys, time
import numpy as np
import torch  # first: see tests/conftest.py
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("toy-cpu-pathtracing_amd")
W, H, WARMUP, SPP = 1920, 1080, 3, 4
RUNS = max(20, int(sys.argv[1])) if len(sys.argv) > 1 else 20
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "deform_rate.json")
prod = pkg.Product()
F = np.float32


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "runs": len(ms)}


def describe(name, replace=None):
    """(scene, camera, deformed mesh = its instance); the scene records the meshes it is given (sc.meshes); replace: {geom: (pos, nrm)} to
    describe the scene with instead"""
    sc = prod.new_scene()
    add = sc.add_mesh
    sc.meshes = []

    def add_mesh(mesh):
        m = dict(mesh)
        if replace and len(sc.meshes) in replace:
            m["pos"], m["nrm"] = replace[len(sc.meshes)]
        sc.meshes.append(m)
        return add(m)
    sc.add_mesh = add_mesh
    if name == "blob512x257":
        m = pkg.assets.load_obj_semantics(pkg.assets.blob_mesh(512, 257, seed=3, lobes=(14, 0.30, 8.0, 60, 0.05, 60.0), center=(0.0, 1.2, -1.0), scale=1.0))
        sc.set_rgb2spec(pkg.scenes.srgb_table())
        g = sc.add_mesh(m)
        d = pkg.ffi.MaterialDesc(); d.type = pkg.ffi.MAT_LAMBERT; d.color = pkg.ffi.Spectrum.constant(0.7); d.normal_tex = pkg.ffi.NONE
        sc.add_instance(g, sc.add_material(d))
        pkg.scenes._room(sc, pkg.scenes.presets())
        sc.set_bvh_builder("gpu")
        return sc, pkg.ffi.make_camera((0.0, 3.15221, 6.0), (0.0, -0.9, -3.2), (0.0, 1.0, 0.0), W, H), 0
    return sc, pkg.scenes.load_scene(sc, int(name), W, H, build=False), 0


def normals(pos, idx, old):
    """area-weighted vertex normals (float64 accumulation); a vertex without area keeps its old normal"""
    p = pos.astype(np.float64)
    n = np.cross(p[idx[:, 1]] - p[idx[:, 0]], p[idx[:, 2]] - p[idx[:, 0]])
    acc = np.zeros_like(p)
    for k in range(3):
        np.add.at(acc, idx[:, k], n)
    ln = np.linalg.norm(acc, axis=1, keepdims=True)
    return np.where(ln > 0.0, acc / np.where(ln > 0.0, ln, 1.0), old.astype(np.float64)).astype(F)


def displaced(mesh, dy):
    """(pos, nrm) of the mesh with y moved by dy(x, extent, x_min)"""
    pos = np.asarray(mesh["pos"], F).reshape(-1, 3)
    idx = np.asarray(mesh["idx"], np.uint32).reshape(-1, 3)
    p = pos.astype(np.float64)
    ext = float((p.max(axis=0) - p.min(axis=0)).max())
    p[:, 1] += dy(p[:, 0], ext, float(p[:, 0].min()))
    new = p.astype(F)
    return new, normals(new, idx, np.asarray(mesh["nrm"], F).reshape(-1, 3))


def wave(k):
    return lambda x, ext, x0: 0.01 * ext * np.sin(2.0 * np.pi * x / ext + 0.1 * k)


def bend(a):
    return lambda x, ext, x0: a * ext * np.sin(np.pi * (x - x0) / ext)


def pose(t, ry, l2w):
    c, s = np.cos(ry), np.sin(ry)
    x = np.eye(4)
    x[:3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
    x[:3, 3] = t
    return (x.astype(F).astype(np.float64) @ np.asarray(l2w, np.float64)).astype(F)


def frame_ms(sc, cam):
    film = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    prm = pkg.make_params(SPP, "mis", "sobol")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(); prod.render_accum_device(sc, cam, prm, 0, SPP, film.data_ptr()); e1.record(); e1.synchronize()
    return e0.elapsed_time(e1)


result = {"library": prod.version(), "device": torch.cuda.get_device_name(0), "frame": [W, H], "frame_spp": SPP, "warmup": WARMUP, "runs": RUNS, "scenes": {}}
for name in ("3", "17", "blob512x257"):
    (s_build, cam, geom), (s_deform, _, _), (s_move, _, _) = describe(name), describe(name), describe(name)
    s_move.set_instance_dynamic(geom)
    s_build.build(cam); s_deform.build(cam); s_move.build(cam)
    info = prod.scene_info(s_deform)
    home = s_move.instances[geom][2]
    poses = [displaced(s_deform.meshes[geom], wave(k)) for k in range(1, WARMUP + RUNS + 1)]      # (made ahead: not part of any timing)
    build_ms, host_ms, device_ms, move_device_ms, launches, rebuilt, ratio = [], [], [], [], set(), 0, []
    for k in range(1, WARMUP + RUNS + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s_build.build(cam)
        torch.cuda.synchronize()
        b = (time.perf_counter() - t0) * 1e3
        r = s_deform.deform_meshes(cam, {geom: (poses[k - 1][0], poses[k - 1][1], None)})
        m = s_move.move_instances(cam, [geom], [pose((0.01 * k, 0.0, -0.02 * k), 0.01 * k, home)])
        if k > WARMUP:
            build_ms.append(b); host_ms.append(r["host_ms"]); device_ms.append(r["device_ms"]); launches.add(r["launches"]); rebuilt += r["rebuilt"]
            move_device_ms.append(m["device_ms"])
            ratio.append(float(r["sah_after"]) / float(r["sah_built"]) if r["sah_built"] else 0.0)
    got, want = s_deform.debug_device_digest()[0], s_deform.debug_pinned_digest(cam)[0]
    frames = [frame_ms(s_deform, cam) for _ in range(WARMUP + RUNS)][WARMUP:]
    mesh = s_deform.meshes[geom]
    row = {"scene_info": info, "deformed_mesh": geom, "mesh_vertices": int(np.asarray(mesh["pos"]).reshape(-1, 3).shape[0]),
           "mesh_triangles": int(np.asarray(mesh["idx"]).size // 3), "build_wall": spread(build_ms), "deform_host": spread(host_ms),
           "deform_device": spread(device_ms), "deform_launches": sorted(launches), "deforms_that_rebuilt": rebuilt,
           "instance_move_device_same_run": spread(move_device_ms), "frame_4spp_device": spread(frames),
           "build_over_deform": round(statistics.median(build_ms) / statistics.median(host_ms), 2),
           "deform_device_minus_instance_move_device_ms": round(statistics.median(device_ms) - statistics.median(move_device_ms), 4),
           "sah_after_over_built_last": round(ratio[-1], 6),
           "device_bytes_equal_pinned_lowering": got == want, "arrays_that_differ": [n for n in want if got[n] != want[n]]}
    result["scenes"][name] = row
    print(name, json.dumps(row), flush=True)

quality = {}
for a in (0.01, 0.02, 0.05, 0.1, 0.2, 0.35, 0.5):
    sc, cam, geom = describe("17")
    sc.build(cam)
    new = displaced(sc.meshes[geom], bend(a))
    r = sc.deform_meshes(cam, {geom: (new[0], new[1], None)})
    fresh, _, _ = describe("17", {geom: new})
    fresh.build(cam)
    refit_ms, fresh_ms = [], []
    for k in range(WARMUP + RUNS):
        x, y = frame_ms(sc, cam), frame_ms(fresh, cam)
        if k >= WARMUP:
            refit_ms.append(x); fresh_ms.append(y)
    quality[f"{a:g}"] = {"amplitude_over_extent": a, "rebuilt": r["rebuilt"], "reason": r["reason"], "sah_built": float(r["sah_built"]), "sah_after": float(r["sah_after"]),
                         "sah_after_over_built": round(float(r["sah_after"]) / float(r["sah_built"]), 6) if r["sah_built"] else None,
                         "frame_4spp_refit_tree": spread(refit_ms), "frame_4spp_fresh_build": spread(fresh_ms),
                         "refit_over_fresh": round(statistics.median(refit_ms) / statistics.median(fresh_ms), 4)}
    print("17 bend", a, json.dumps(quality[f"{a:g}"]), flush=True)
result["tree_quality_scene17_hero_bend"] = quality
os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
with open(OUT, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print("wrote", OUT)
