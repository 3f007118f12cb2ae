#!/usr/bin/env python3
"""What an edit of lights and materials costs (include/mi355pt_edit.h) against what it replaces, on one GPU, in one process.

For scene 3 (the emitter's intensity; a wall between Lambert and glass: a class change, one launch), scene 17 (the hero's coat roughness:
one coat-albedo row integrated on the host), scene 19 with a 1024 x 512 sky (its intensity alone; the whole map replaced: three tables
lowered and uploaded) and the 512 x 257 blob mesh of tests/test_bvh_gpu.py in scene 3's room under the GPU builder (262 k triangles; the
emitter's intensity, and the blob between Lambert and glass), at 1920 x 1080: two scenes of the same description are built at the same
camera.  After WARMUP rounds, RUNS rounds ALTERNATE between
  build    the wall time of the whole mi355pt_scene_build call — what a caller pays to change a light or a material without the edit
           call (the build is of the unedited scene: the same work); and
  edit     mi355pt_scene_edit on the other scene to the round's value: its host_ms (wall time of the call, lowering and uploads
           included) and device_ms (HIP events around its launch, 0 without one), with `launches`.
The value of round k differs from round k - 1's, so no call finds unchanged records.  After the last round the edited scene's device
digests are compared with the host's pinned lowering (mi355pt_scene_debug_pinned_digest): the timed calls computed the right bytes.

Writes one JSON object to profiles/scene_edit_rate.json (or the path given).  Needs a GPU; reads nothing outside the repository.
usage: tools/scene_edit_rate.py [RUNS (default 20, at least 20)] [OUTPUT.json]"""
import importlib, json, os, statistics, sys, time
import numpy as np
import torch  # first: see tests/conftest.py
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("toy-cpu-pathtracing_amd")
f = pkg.ffi
W, H, WARMUP = 1920, 1080, 3
RUNS = max(20, int(sys.argv[1])) if len(sys.argv) > 1 else 20
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "scene_edit_rate.json")
prod = pkg.Product()
F = np.float32


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "runs": len(ms)}


def copy_of(d):
    return type(d).from_buffer_copy(d)


def describe(name):
    sc = prod.new_scene()
    if name == "blob512x257":
        m = pkg.assets.load_obj_semantics(pkg.assets.blob_mesh(512, 257, seed=3, lobes=(14, 0.30, 8.0, 60, 0.05, 60.0), center=(0.0, 1.2, -1.0), scale=1.0))
        sc.set_rgb2spec(pkg.scenes.srgb_table())
        d = f.MaterialDesc(); d.type = f.MAT_LAMBERT; d.color = f.Spectrum.constant(0.7); d.normal_tex = f.NONE
        sc.add_instance(sc.add_mesh(m), sc.add_material(d))
        pkg.scenes._room(sc, pkg.scenes.presets())
        sc.set_bvh_builder("gpu")
        return sc, f.make_camera((0.0, 3.15221, 6.0), (0.0, -0.9, -3.2), (0.0, 1.0, 0.0), W, H)
    if name == "19":                                      # scene 19 with a 1024 x 512 sky: the map a replacement has to lower and upload
        add = sc.add_environment_light
        sc.add_environment_light = lambda intensity, rgb, lut, l2w=None: add(intensity, pkg.assets.sky_envmap(1024, 512, seed=5), lut, l2w)
    return sc, pkg.scenes.load_scene(sc, int(name), W, H, build=False)


def first(sc, mat_type, skip=0):
    return [i for i, d in enumerate(sc.material_descs) if d is not None and d.type == mat_type][skip]


def glass():
    d = f.MaterialDesc(); d.type = f.MAT_GLASS; d.eta = f.Spectrum.constant(1.5); d.color = f.Spectrum.constant(1.0); d.normal_tex = f.NONE
    return d


def emitter_intensity(sc):
    em = first(sc, f.MAT_EMISSIVE)

    def edit(k):
        d = copy_of(sc.material_descs[em]); d.intensity = 10.0 + 0.25 * k
        return {"materials": {em: d}}
    return edit


def class_flip(sc, mat):
    return lambda k: {"materials": {mat: glass() if k % 2 else copy_of(sc.material_descs[mat])}}


def coat(sc):
    cc = first(sc, f.MAT_CLEARCOAT)

    def edit(k):
        d = copy_of(sc.material_descs[cc]); d.clearcoat_roughness = 0.05 + 0.01 * k
        return {"materials": {cc: d}}
    return edit


MAPS = {}
CASES = [("3", "emitter_intensity", emitter_intensity), ("3", "wall_class_change", lambda sc: class_flip(sc, first(sc, f.MAT_LAMBERT, 2))),
         ("17", "coat_roughness", coat), ("19", "env_intensity", lambda sc: lambda k: {"envs": {0: (1.0 + 0.05 * k, None, None)}}),
         ("19", "env_map_1024x512", lambda sc: lambda k: {"envs": {0: (1.0, None, MAPS.setdefault(k % 2, pkg.assets.sky_envmap(1024, 512, seed=6 + k % 2)))}}),
         ("blob512x257", "emitter_intensity", emitter_intensity), ("blob512x257", "blob_class_change", lambda sc: class_flip(sc, 0))]

result = {"library": prod.version(), "device": torch.cuda.get_device_name(0), "frame": [W, H], "warmup": WARMUP, "runs": RUNS, "cases": {}}
for name, what, make in CASES:
    (s_build, cam), (s_edit, _) = describe(name), describe(name)
    s_build.build(cam); s_edit.build(cam)
    edit = make(s_edit)
    edits = [edit(k) for k in range(1, WARMUP + RUNS + 1)]          # (made ahead: not part of any timing)
    build_ms, host_ms, device_ms, launches, rebuilt, reasons = [], [], [], set(), 0, set()
    for k in range(1, WARMUP + RUNS + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s_build.build(cam)
        torch.cuda.synchronize()
        b = (time.perf_counter() - t0) * 1e3
        r = s_edit.edit(cam, **edits[k - 1])
        if k > WARMUP:
            build_ms.append(b); host_ms.append(r["host_ms"]); device_ms.append(r["device_ms"]); launches.add(r["launches"]); rebuilt += r["rebuilt"]; reasons.add(r["reason"])
    got, want = s_edit.debug_device_digest()[0], s_edit.debug_pinned_digest(cam)[0]
    row = {"scene_info": prod.scene_info(s_edit), "build_wall": spread(build_ms), "edit_host": spread(host_ms), "edit_device": spread(device_ms),
           "edit_launches": sorted(launches), "edit_reasons": sorted(reasons), "edits_that_rebuilt": rebuilt,
           "build_over_edit": round(statistics.median(build_ms) / statistics.median(host_ms), 2),
           "device_bytes_equal_pinned_lowering": got == want, "arrays_that_differ": [n for n in want if got[n] != want[n]]}
    result["cases"][f"{name}:{what}"] = row
    print(name, what, json.dumps(row), flush=True)
os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
with open(OUT, "w") as fh:
    json.dump(result, fh, indent=1)
    fh.write("\n")
print("wrote", OUT)
