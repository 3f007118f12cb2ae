#!/usr/bin/env python3
"""Rate of the G-buffer pass on one GPU against the two AOV launches it replaces, in one process: scene 3 at 1920x1080, 64 spp, ZSobol
(the guide films of the denoise paths).  Four launches ALTERNATE round by round, so that drift of the machine falls on all of them alike:
  (a) the albedo AOV launch            mi355pt_render_aov_accum_device(MI355PT_AOV_ALBEDO)
  (b) the shading-normal AOV launch    mi355pt_render_aov_accum_device(MI355PT_AOV_SHADING_NORMAL)
  (c) the G-buffer launch with those two films
  (d) the G-buffer launch with all four films
WARMUP rounds, then ROUNDS timed rounds; device-event time from stats.kernel_ms; the median per launch.  The condition is (c) < (a) + (b):
the fused pass traces one of the two sets of rays.  No ratio is fixed in advance: (c) / ((a) + (b)) and (d) / (c) are recorded as they come
out.  Prints one JSON line and writes it to profiles/gbuffer_rate.json (or the path given with --out); exit status 1 when the condition
fails.  Needs a GPU; reads neither the oracle nor anything outside the repository.
usage: tools/gbuffer_rate.py [--rounds 30] [--warmup 5] [--out FILE]"""
import argparse, importlib, json, os, statistics, sys
import torch  # first: see tests/conftest.py
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("toy-cpu-pathtracing_amd")
ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gbuffer_rate.json"))
args = ap.parse_args()
W, H, SPP = 1920, 1080, 64
prod = pkg.Product(); sc = prod.new_scene()
cam = pkg.scenes.load_scene(sc, 3, W, H, build=False)
d65 = sc.add_lut470(pkg.scenes.presets()["cie_illum_d6500"])
sc.build(cam)
films = torch.zeros((4, H, W, 3), device="cuda")            # sums keep growing over the rounds: the time does not depend on their values
ptr = {k: films[i].data_ptr() for i, k in enumerate(pkg.ffi.GBUFFER_FILMS)}
prm = pkg.make_params(SPP, "mis", "sobol")
launches = {
    "a_aov_albedo": lambda st: prod.render_aov_accum_device(sc, cam, prm, pkg.ffi.AOV_ALBEDO, d65, 0, SPP, ptr["albedo"], None, stats=st),
    "b_aov_shading_normal": lambda st: prod.render_aov_accum_device(sc, cam, prm, pkg.ffi.AOV_SHADING_NORMAL, d65, 0, SPP, ptr["shading_normal"], None, stats=st),
    "c_gbuffer_two_films": lambda st: prod.render_gbuffer_accum_device(sc, cam, prm, d65, 0, SPP, {k: ptr[k] for k in ("albedo", "shading_normal")}, None, st),
    "d_gbuffer_four_films": lambda st: prod.render_gbuffer_accum_device(sc, cam, prm, d65, 0, SPP, ptr, None, st),
}
ms = {k: [] for k in launches}
for r in range(args.warmup + args.rounds):
    for k, launch in launches.items():
        st = pkg.ffi.Stats(); launch(st)
        if r >= args.warmup:
            ms[k].append(st.kernel_ms)
out = {"config": f"scene3 {W}x{H}, {SPP} spp, zsobol, launches alternating in one process, median of {args.rounds} after {args.warmup} warm-up rounds",
       "library": prod.version()}
for k, v in ms.items():
    out[k] = {"ms": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "spread": round((max(v) - min(v)) / statistics.median(v), 4)}
a, b, c, d = (out[k]["ms"] for k in launches)
out["c_over_a_plus_b"] = round(c / (a + b), 4)
out["d_over_c"] = round(d / c, 4)
out["condition_c_below_a_plus_b"] = bool(c < a + b)
line = json.dumps(out)
print(line, flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(line + "\n")
sys.exit(0 if out["condition_c_below_a_plus_b"] else 1)
