#!/usr/bin/env python3
"""What an instance move costs (include/mi355pt_instances.h) against what it replaces, on one GPU, in one process, and what a refit does
to the tree.

TIMING.  For scene 3 in general lowering (the box moves), scene 17 (the hero moves) and the 512 x 257 blob mesh of tests/test_bvh_gpu.py
under the GPU builder (262 k triangles; the blob moves), at 1920 x 1080: two scenes of the same description, the moved instance marked
dynamic, are built at the same camera.  After WARMUP rounds, RUNS rounds ALTERNATE between
  build   the wall time of the whole mi355pt_scene_build call — lowering, tree, collapse, every hipMalloc and hipMemcpy: what a caller
          pays per frame to move an object without the move call (the description cannot be edited, so the build is of the unmoved scene:
          the same work); and
  move    mi355pt_scene_move_instances on the other scene to the round's pose: its host_ms (wall time of the call) and device_ms (HIP
          events around its launches), with `launches`.
The pose of round k is T(k * (0.01, 0, -0.02)) . R_y(k * 0.01 rad) on the left of the described matrix, so no call finds an unchanged
matrix.  After the last round the moved scene's device digests are compared with the host's pinned lowering
(mi355pt_scene_debug_pinned_digest): the timed calls computed the right bytes.

TREE QUALITY.  The hero of scene 17 carried by 0.1, 1 and 10 scene units along x, and 1 unit along +y (the pose that lifts it through
the top of the room's box): sah_after / sah_built as the move reports them, and the device time of a 4-spp MIS frame on the refit tree
against the same frame on a scene described with the moved matrix and built (median of RUNS each, alternating).

Writes one JSON object to profiles/instance_move_rate.json (or the path given).  Needs a GPU; reads nothing outside the repository.
usage: tools/instance_move_rate.py [RUNS (default 20, at least 20)] [OUTPUT.json]"""
import importlib, json, os, statistics, sys, time
import numpy as np
import torch  # first: see tests/conftest.py
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("toy-cpu-pathtracing_amd")
W, H, WARMUP, SPP = 1920, 1080, 3, 4
RUNS = max(20, int(sys.argv[1])) if len(sys.argv) > 1 else 20
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "instance_move_rate.json")
prod = pkg.Product()
F = np.float32


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "runs": len(ms)}


def describe(name, matrices=None):
    """(scene, camera, moved instance); matrices: {instance: local_to_world} to describe the scene with instead"""
    sc = prod.new_scene()
    if matrices:
        add = sc.add_instance
        sc.add_instance = lambda geom, mat, l2w=None: add(geom, mat, matrices.get(len(sc.instances), l2w))
    if name == "blob512x257":
        m = pkg.assets.load_obj_semantics(pkg.assets.blob_mesh(512, 257, seed=3, lobes=(14, 0.30, 8.0, 60, 0.05, 60.0), center=(0.0, 1.2, -1.0), scale=1.0))
        sc.set_rgb2spec(pkg.scenes.srgb_table())
        g = sc.add_mesh(m)
        d = pkg.ffi.MaterialDesc(); d.type = pkg.ffi.MAT_LAMBERT; d.color = pkg.ffi.Spectrum.constant(0.7); d.normal_tex = pkg.ffi.NONE
        sc.add_instance(g, sc.add_material(d))
        pkg.scenes._room(sc, pkg.scenes.presets())
        sc.set_bvh_builder("gpu")
        return sc, pkg.ffi.make_camera((0.0, 3.15221, 6.0), (0.0, -0.9, -3.2), (0.0, 1.0, 0.0), W, H), 0
    cam = pkg.scenes.load_scene(sc, int(name.partition(":")[0]), W, H, build=False)
    if name == "3:general":
        sc.debug_set_lowering("general")
        return sc, cam, 1
    return sc, cam, 0


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
for name in ("3:general", "17", "blob512x257"):
    (s_build, cam, inst), (s_move, _, _) = describe(name), describe(name)
    s_build.set_instance_dynamic(inst); s_move.set_instance_dynamic(inst)
    s_build.build(cam); s_move.build(cam)
    info = prod.scene_info(s_move)
    home = s_move.instances[inst][2]
    build_ms, host_ms, device_ms, launches, rebuilt, ratio = [], [], [], set(), 0, []
    for k in range(1, WARMUP + RUNS + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s_build.build(cam)
        torch.cuda.synchronize()
        b = (time.perf_counter() - t0) * 1e3
        r = s_move.move_instances(cam, [inst], [pose((0.01 * k, 0.0, -0.02 * k), 0.01 * k, home)])
        if k > WARMUP:
            build_ms.append(b); host_ms.append(r["host_ms"]); device_ms.append(r["device_ms"]); launches.add(r["launches"]); rebuilt += r["rebuilt"]
            ratio.append(float(r["sah_after"]) / float(r["sah_built"]) if r["sah_built"] else 0.0)
    got, want = s_move.debug_device_digest()[0], s_move.debug_pinned_digest(cam)[0]
    frames = [frame_ms(s_move, cam) for _ in range(WARMUP + RUNS)][WARMUP:]
    row = {"scene_info": info, "moved_instance": inst, "build_wall": spread(build_ms), "move_host": spread(host_ms), "move_device": spread(device_ms),
           "move_launches": sorted(launches), "moves_that_rebuilt": rebuilt, "frame_4spp_device": spread(frames),
           "build_over_move": round(statistics.median(build_ms) / statistics.median(host_ms), 2),
           "sah_after_over_built_last": round(ratio[-1], 6),
           "device_bytes_equal_pinned_lowering": got == want, "arrays_that_differ": [n for n in want if got[n] != want[n]]}
    result["scenes"][name] = row
    print(name, json.dumps(row), flush=True)

quality = {}
for label, t in (("x+0.1", (0.1, 0.0, 0.0)), ("x+1", (1.0, 0.0, 0.0)), ("x+10", (10.0, 0.0, 0.0)), ("y+1", (0.0, 1.0, 0.0))):
    sc, cam, inst = describe("17")
    sc.set_instance_dynamic(inst); sc.build(cam)
    new = pose(t, 0.0, sc.instances[inst][2])
    r = sc.move_instances(cam, [inst], [new])
    fresh, _, _ = describe("17", {inst: new})
    fresh.set_instance_dynamic(inst); fresh.build(cam)
    refit_ms, fresh_ms = [], []
    for k in range(WARMUP + RUNS):
        a, b = frame_ms(sc, cam), frame_ms(fresh, cam)
        if k >= WARMUP:
            refit_ms.append(a); fresh_ms.append(b)
    quality[label] = {"step": list(t), "rebuilt": r["rebuilt"], "sah_built": float(r["sah_built"]), "sah_after": float(r["sah_after"]),
                      "sah_after_over_built": round(float(r["sah_after"]) / float(r["sah_built"]), 6),
                      "frame_4spp_refit_tree": spread(refit_ms), "frame_4spp_fresh_build": spread(fresh_ms),
                      "refit_over_fresh": round(statistics.median(refit_ms) / statistics.median(fresh_ms), 4)}
    print("17", label, json.dumps(quality[label]), flush=True)
result["tree_quality_scene17_hero"] = quality
os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print("wrote", OUT)
