#!/usr/bin/env python3
"""Rate of the AOV kernel on one GPU against the path kernel doing strictly more work, in one process: scene 3 at 1920x1080, 1024 spp,
ZSobol (the frame bench.py times) through mi355pt_render_aov_accum_device for each AOV kind, and through mi355pt_render_accum_device with
strategy pt and max_depth 1 (the camera vertex, one BSDF sample, a second ray).  One warm-up launch, then REPEATS timed launches each;
device-event time from stats.kernel_ms.  Prints one JSON line: Msamples/s per kind (median), the path kernel's figure, the ratios and the
spread (max - min) / median over the repeats.  Needs a GPU; reads neither the oracle nor anything outside the repository."""
import importlib, json, os, statistics, sys
import torch  # first: see tests/conftest.py
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("toy-cpu-pathtracing_amd")
W, H, SPP = 1920, 1080, 1024
REPEATS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
prod = pkg.Product(); sc = prod.new_scene()
cam = pkg.scenes.load_scene(sc, 3, W, H, build=False)
d65 = sc.add_lut470(pkg.scenes.presets()["cie_illum_d6500"])
sc.build(cam)
film = torch.zeros((H, W, 3), device="cuda")


def timed(launch):
    ms = []
    for i in range(REPEATS + 1):
        st = pkg.ffi.Stats(); launch(st)
        if i: ms.append(st.kernel_ms)                      # (the first launch warms up: code object load, launch scratch)
    rate = [W * H * SPP / m / 1e3 for m in ms]
    return {"Msamples_s": round(statistics.median(rate), 1), "min": round(min(rate), 1), "max": round(max(rate), 1),
            "spread": round((max(rate) - min(rate)) / statistics.median(rate), 4)}


out = {"config": f"scene3 {W}x{H}, {SPP} spp, zsobol, one launch of {SPP} sample indices, {REPEATS} timed launches after one warm-up", "library": prod.version()}
prm_pt = pkg.make_params(SPP, "pt", "sobol", max_depth=1)
prm = pkg.make_params(SPP, "mis", "sobol")
out["path_pt_depth1"] = timed(lambda st: prod.render_accum_device(sc, cam, prm_pt, 0, SPP, film.data_ptr(), None, stats=st))
for name, kind in pkg.ffi.AOV.items():
    out[name] = timed(lambda st, kind=kind: prod.render_aov_accum_device(sc, cam, prm, kind, d65, 0, SPP, film.data_ptr(), None, stats=st))
    out[name]["ratio_to_path"] = round(out[name]["Msamples_s"] / out["path_pt_depth1"]["Msamples_s"], 3)
    out[name]["slowest_over_paths_fastest"] = round(out[name]["min"] / out["path_pt_depth1"]["max"], 3)
# once more at the end: drift of the box over the run shows as a difference between the two path-kernel figures
out["path_pt_depth1_again"] = timed(lambda st: prod.render_accum_device(sc, cam, prm_pt, 0, SPP, film.data_ptr(), None, stats=st))
print(json.dumps(out), flush=True)
