#!/usr/bin/env python3
"""What a camera move costs (include/mi355pt_rebase.h) against what it replaces, on one GPU, in one process.

For scene 3, scene 17 and the 512 x 257 blob mesh of tests/test_bvh_gpu.py (262 k triangles: the GPU builder's territory), at 1920 x 1080:
two scenes of the same description are built at the same camera.  After WARMUP rounds, RUNS rounds ALTERNATE between
  build   the wall time of the whole mi355pt_scene_build call at the next camera position — lowering, tree, collapse, every hipMalloc and
          hipMemcpy: what a moving-camera loop pays per frame without the move; and
  move    mi355pt_scene_move_camera to the same position on the other scene: its host_ms (wall time of the call) and device_ms (HIP events
          around its launches), with `launches`.
The camera steps by (0.05, 0, -0.1) per round, so no call finds an unchanged position.  Beside them the time of a 4-spp MIS frame of the moved
scene (HIP events around mi355pt_render_accum_device, median of RUNS), for scale.  After the last round the moved scene's device digests are
compared with the host's pinned lowering (mi355pt_scene_debug_move_digest): the timed calls computed the right bytes.

Writes one JSON object to profiles/rebase_rate.json (or the path given).  Needs a GPU; reads nothing outside the repository.
usage: tools/rebase_rate.py [RUNS (default 20, at least 20)] [OUTPUT.json]"""
import importlib, json, os, statistics, sys, time
import numpy as np
import torch  # first: see tests/conftest.py
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("toy-cpu-pathtracing_amd")
W, H, WARMUP, SPP = 1920, 1080, 3, 4
RUNS = max(20, int(sys.argv[1])) if len(sys.argv) > 1 else 20
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "rebase_rate.json")
STEP = np.array([0.05, 0.0, -0.1], np.float32)
prod = pkg.Product()


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "runs": len(ms)}


def describe(name):
    sc = prod.new_scene()
    if name == "blob512x257":
        m = pkg.assets.load_obj_semantics(pkg.assets.blob_mesh(512, 257, seed=3, lobes=(14, 0.30, 8.0, 60, 0.05, 60.0), center=(0.0, 1.2, -1.0), scale=1.0))
        sc.set_rgb2spec(pkg.scenes.srgb_table())
        g = sc.add_mesh(m)
        d = pkg.ffi.MaterialDesc(); d.type = pkg.ffi.MAT_LAMBERT; d.color = pkg.ffi.Spectrum.constant(0.7); d.normal_tex = pkg.ffi.NONE
        sc.add_instance(g, sc.add_material(d))
        pkg.scenes._room(sc, pkg.scenes.presets())
        return sc, pkg.ffi.make_camera((0.0, 3.15221, 6.0), (0.0, -0.9, -3.2), (0.0, 1.0, 0.0), W, H)
    return sc, pkg.scenes.load_scene(sc, int(name), W, H, build=False)


def at(cam, k):
    p = np.array(cam.position[:], np.float32) + np.float32(k) * STEP
    return pkg.make_camera(tuple(float(v) for v in p), tuple(cam.direction[:]), tuple(cam.up[:]), cam.width, cam.height, cam.fov_deg)


result = {"library": prod.version(), "device": torch.cuda.get_device_name(0), "frame": [W, H], "frame_spp": SPP, "warmup": WARMUP, "runs": RUNS, "scenes": {}}
for name in ("3", "17", "blob512x257"):
    (s_build, cam), (s_move, _) = describe(name), describe(name)
    s_build.build(cam); s_move.build(cam)
    info = prod.scene_info(s_move)
    build_ms, host_ms, device_ms, launches, rebuilt = [], [], [], set(), 0
    for k in range(1, WARMUP + RUNS + 1):
        c = at(cam, k)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s_build.build(c)
        torch.cuda.synchronize()
        b = (time.perf_counter() - t0) * 1e3
        r = s_move.move_camera(c)
        if k > WARMUP:
            build_ms.append(b); host_ms.append(r["host_ms"]); device_ms.append(r["device_ms"]); launches.add(r["launches"]); rebuilt += r["rebuilt"]
    last = at(cam, WARMUP + RUNS)
    got, want = s_move.debug_device_digest()[0], s_move.debug_move_digest(cam, last)[0]
    film = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    prm = pkg.make_params(SPP, "mis", "sobol")
    frame_ms = []
    for k in range(WARMUP + RUNS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(); prod.render_accum_device(s_move, last, prm, 0, SPP, film.data_ptr()); e1.record(); e1.synchronize()
        if k >= WARMUP:
            frame_ms.append(e0.elapsed_time(e1))
    row = {"scene_info": info, "build_wall": spread(build_ms), "move_host": spread(host_ms), "move_device": spread(device_ms),
           "move_launches": sorted(launches), "moves_that_rebuilt": rebuilt, "frame_4spp_device": spread(frame_ms),
           "build_over_move": round(statistics.median(build_ms) / statistics.median(host_ms), 2),
           "device_bytes_equal_pinned_lowering": got == want, "arrays_that_differ": [n for n in want if got[n] != want[n]]}
    result["scenes"][name] = row
    print(name, json.dumps(row), flush=True)
os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print("wrote", OUT)
