#!/usr/bin/env python3
"""Time of the bloom stage (include/mi355pt_bloom.h, csrc/pt_kernels_bloom.hip) on one GPU beside what it stands next to, in one process, on a
1920x1080 film of scene 3 at 16 spp (mis, ZSobol), six levels, default parameters.  After WARMUP calls of each, RUNS calls of each,
ALTERNATING, each bracketed by HIP events:
  bloom                    mi355pt_bloom_device as a whole (12 launches); also with the weights off, and in place;
  bloom_3_levels           the same frame with three levels: the difference to six is what the launches of levels 4 .. 6 cost, on levels
                           of 120 x 68 records and fewer — launch latency, the most a fused tail could save;
  bloom_tiny               a 2 x 2 frame with six levels: twelve launches that move nothing, the price of a launch itself;
  copy_stage_bytes         a device-to-device copy that moves the bytes the stage must move (half of them read, half written): the film
                           twice and the output once, every level written by its reduction, read by the next, read and rewritten by its mix
                           and read by the expansion below it;
  display                  mi355pt_display_device (REINHARD + sRGB) on the same film;
  denoise_var              the 5-level variance-guided filter (mi355pt_denoise_var_device) on the same film with its half film and guides.
Writes one JSON object to profiles/bloom_rate.json (or the path given): medians, spread, ratios.
  tools/bloom_rate.py --calls N              N calls of the whole stage and nothing else: the program of a `rocprofv3 --kernel-trace` run
  tools/bloom_rate.py --merge-trace CSV JSON  adds the per-launch split of that run's kernel trace (the 12 launches of a call, in order) to JSON
Needs a GPU; reads nothing outside the repository.
usage: tools/bloom_rate.py [RUNS (default 30, at least 20)] [OUTPUT.json]"""
import csv, importlib, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SPP, GUIDE_SPP, LEVELS, WARMUP = 1920, 1080, 16, 64, 6, 5


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "spread": round((max(ms) - min(ms)) / statistics.median(ms), 4), "runs": len(ms)}


def merge_trace(csv_path, json_path):
    rows = [r for r in csv.DictReader(open(csv_path)) if "bloom_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per_call = 2 * LEVELS
    assert rows and len(rows) % per_call == 0, (len(rows), per_call)
    calls = [rows[i:i + per_call] for i in range(0, len(rows), per_call)][WARMUP:]
    split = []
    for k in range(per_call):
        us = [(int(c[k]["End_Timestamp"]) - int(c[k]["Start_Timestamp"])) / 1e3 for c in calls]
        name = calls[0][k]["Kernel_Name"]
        split.append({"launch": k, "kernel": name[name.index("bloom_"):].split("(")[0][:48], "median_us": round(statistics.median(us), 2), "min_us": round(min(us), 2)})
    span = [(int(c[-1]["End_Timestamp"]) - int(c[0]["Start_Timestamp"])) / 1e3 for c in calls]
    res = json.load(open(json_path))
    busy = sum(s["median_us"] for s in split)
    res["kernel_trace"] = {"source": "rocprofv3 --kernel-trace around `tools/bloom_rate.py --calls N` in a run of its own (its timings are not the events' above)",
                           "calls": len(calls), "launches": split, "sum_of_kernel_medians_us": round(busy, 2), "first_start_to_last_end_median_us": round(statistics.median(span), 2),
                           "levels_4_to_6_kernels_us": round(sum(s["median_us"] for s in split[3:9]), 2)}
    json.dump(res, open(json_path, "w"), indent=1)
    print(json.dumps(res["kernel_trace"]), flush=True)


if len(sys.argv) > 3 and sys.argv[1] == "--merge-trace":
    merge_trace(sys.argv[2], sys.argv[3])
    sys.exit(0)

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the product: see tests/conftest.py)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bloom_reference as br  # noqa: E402
pkg = importlib.import_module("toy-cpu-pathtracing_amd")
prod = pkg.Product()
sc = prod.new_scene()
cam = pkg.scenes.load_scene(sc, 3, W, H, build=False)
d65 = sc.add_lut470(pkg.scenes.presets()["cie_illum_d6500"])
sc.build(cam)
film = {k: torch.zeros((H, W, 3), device="cuda") for k in ("half", "albedo", "normal", "out", "in_place")}
prm, guide = pkg.make_params(SPP, "mis", "sobol"), pkg.make_params(GUIDE_SPP, "mis", "sobol")
prod.render_accum_device(sc, cam, prm, 0, SPP // 2, film["half"].data_ptr(), None)
film["beauty"] = film["half"].clone()
prod.render_accum_device(sc, cam, prm, SPP // 2, SPP, film["beauty"].data_ptr(), None)
torch.cuda.synchronize()
bp = prod.bloom_params_default()
assert bp.levels == LEVELS
need = prod.bloom_scratch_bytes(W, H, LEVELS)
scratch = torch.empty(need, dtype=torch.uint8, device="cuda")


def bloom(params=bp, out="out", w=W, h=H, src="beauty"):
    prod.bloom_device(film[src].data_ptr(), w, h, SPP, params, None, scratch.data_ptr(), need, film[out].data_ptr())


if len(sys.argv) > 2 and sys.argv[1] == "--calls":
    for _ in range(WARMUP + int(sys.argv[2])):
        bloom()
        torch.cuda.synchronize()
    sys.exit(0)

RUNS = max(20, int(sys.argv[1])) if len(sys.argv) > 1 else 30
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "bloom_rate.json")
prod.render_aov_accum_device(sc, cam, guide, pkg.ffi.AOV_ALBEDO, d65, 0, GUIDE_SPP, film["albedo"].data_ptr(), None)
prod.render_aov_accum_device(sc, cam, guide, pkg.ffi.AOV_SHADING_NORMAL, d65, 0, GUIDE_SPP, film["normal"].data_ptr(), None)
torch.cuda.synchronize()
sizes = br.level_sizes(W, H, LEVELS)
n = [w * h for w, h in sizes]
stage_bytes = 36 * n[0] + 16 * sum(n[1:]) + 16 * sum(n[1:LEVELS]) + 32 * sum(n[1:LEVELS]) + 16 * sum(n[1:])
copy_src, copy_dst = torch.empty(stage_bytes // 2, dtype=torch.uint8, device="cuda"), torch.empty(stage_bytes // 2, dtype=torch.uint8, device="cuda")
plain, three = prod.bloom_params_default(), prod.bloom_params_default()
plain.firefly, three.levels = 0, 3
dp, vp = prod.display_params_default(), prod.denoise_var_params_default()
need_var = prod.denoise_var_scratch_bytes(W, H)
scratch_var = torch.empty(need_var, dtype=torch.uint8, device="cuda")
calls = [("bloom", bloom), ("bloom_no_firefly", lambda: bloom(plain)), ("bloom_in_place", lambda: bloom(out="in_place", src="in_place")), ("bloom_3_levels", lambda: bloom(three)),
         ("bloom_tiny", lambda: bloom(w=2, h=2)), ("copy_stage_bytes", lambda: copy_dst.copy_(copy_src)),
         ("display", lambda: prod.display_device(film["beauty"].data_ptr(), W, H, SPP, dp, None, film["out"].data_ptr())),
         ("denoise_var", lambda: prod.denoise_var_device(film["beauty"].data_ptr(), film["half"].data_ptr(), SPP, None, film["albedo"].data_ptr(), GUIDE_SPP,
                                                         film["normal"].data_ptr(), GUIDE_SPP, W, H, vp, scratch_var.data_ptr(), need_var, film["out"].data_ptr(), None))]
ms = {name: [] for name, _ in calls}
for i in range(WARMUP + RUNS):
    film["in_place"].copy_(film["beauty"])
    for name, fn in calls:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(); fn(); e1.record(); e1.synchronize()
        if i >= WARMUP: ms[name].append(e0.elapsed_time(e1))
bloom()
torch.cuda.synchronize()
f = film["beauty"].cpu().numpy()
want = br.bloom(f, SPP, br.params())
assert np.array_equal(br.bits(film["out"].cpu().numpy()), br.bits(want.out))           # what was timed is what the restatement gives
assert np.array_equal(br.bits(film["in_place"].cpu().numpy()), br.bits(want.out))
res = {name: spread(v) for name, v in ms.items()}
med = {name: r["median_ms"] for name, r in res.items()}
result = {"config": f"{W}x{H} film of scene 3 at {SPP} spp, {LEVELS} levels, default parameters; {RUNS} timed calls of each, alternating, after {WARMUP} warm-up calls of each, "
                    "HIP events around each call",
          "library": prod.version(), "launches_per_call": 2 * LEVELS, "level_sizes": sizes, "scratch_bytes": need, "stage_bytes": stage_bytes, **res,
          "bloom_over": {k: round(med["bloom"] / med[k], 4) for k in ("copy_stage_bytes", "display", "denoise_var")},
          "GB_s": {"bloom": round(stage_bytes / (med["bloom"] * 1e-3) / 1e9, 1), "copy_stage_bytes": round(stage_bytes / (med["copy_stage_bytes"] * 1e-3) / 1e9, 1)},
          "small_levels": {"levels_4_to_6_ms": round(med["bloom"] - med["bloom_3_levels"], 4), "share_of_the_call": round((med["bloom"] - med["bloom_3_levels"]) / med["bloom"], 4),
                           "six_empty_launches_ms": round(med["bloom_tiny"] / 2, 4),
                           "note": "levels 4 .. 6 are 120 x 68 records and fewer: their six launches cost what six launches cost; a fused tail would save at most that share"}}
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
json.dump(result, open(OUT, "w"), indent=1)
print(json.dumps(result), flush=True)
