#!/usr/bin/env python3
"""Time of the variance-guided denoiser (mi355pt_denoise_var_device, csrc/pt_kernels_denoise_var.hip) on one GPU beside the shipped filter
(mi355pt_denoise_device) on the same frame, in one process: scene 3 at 1920x1080, half film [0, 8) and film [0, 16) (mis, ZSobol), albedo
and shading-normal films at 64 spp, default parameters (5 levels) for both.  After WARMUP calls of each, RUNS calls of each whole filter
(prepass + 5 levels), ALTERNATING, each bracketed by HIP events on the stream it runs on.  Writes one JSON object to
profiles/denoise_var_rate.json (or the path given): medians, spread, the ratio of the two medians, the bytes the new filter MUST move (a
level: three 16-B records read, one written; the prepass reads four films and writes three records) and the rate that figure gives over the
measured time — a floor on the traffic, not a counter reading: the eight one-word loads of the 3 x 3 variance filter come from rows that
the level reads anyway.  Needs a GPU; reads nothing outside the repository.
usage: tools/denoise_var_rate.py [RUNS (default 30, at least 20)] [OUTPUT.json]"""
import importlib, json, os, statistics, sys, time
import torch  # first: see tests/conftest.py
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("toy-cpu-pathtracing_amd")
W, H, SPP, GUIDE_SPP, WARMUP = 1920, 1080, 16, 64, 5
RUNS = max(20, int(sys.argv[1])) if len(sys.argv) > 1 else 30
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "denoise_var_rate.json")
prod = pkg.Product(); sc = prod.new_scene()
cam = pkg.scenes.load_scene(sc, 3, W, H, build=False)
d65 = sc.add_lut470(pkg.scenes.presets()["cie_illum_d6500"])
sc.build(cam)
film = {k: torch.zeros((H, W, 3), device="cuda") for k in ("half", "albedo", "normal", "out_var", "out_shipped")}
prm, guide = pkg.make_params(SPP, "mis", "sobol"), pkg.make_params(GUIDE_SPP, "mis", "sobol")
prod.render_accum_device(sc, cam, prm, 0, SPP // 2, film["half"].data_ptr(), None)
film["beauty"] = film["half"].clone()
prod.render_accum_device(sc, cam, prm, SPP // 2, SPP, film["beauty"].data_ptr(), None)
prod.render_aov_accum_device(sc, cam, guide, pkg.ffi.AOV_ALBEDO, d65, 0, GUIDE_SPP, film["albedo"].data_ptr(), None)
prod.render_aov_accum_device(sc, cam, guide, pkg.ffi.AOV_SHADING_NORMAL, d65, 0, GUIDE_SPP, film["normal"].data_ptr(), None)
torch.cuda.synchronize()
vp, dp = prod.denoise_var_params_default(), prod.denoise_params_default()
need_var, need = prod.denoise_var_scratch_bytes(W, H), prod.denoise_scratch_bytes(W, H)
scratch = torch.empty(max(need_var, need), dtype=torch.uint8, device="cuda")


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "spread": round((max(ms) - min(ms)) / statistics.median(ms), 4), "runs": len(ms)}


def variance_guided():
    prod.denoise_var_device(film["beauty"].data_ptr(), film["half"].data_ptr(), SPP, None, film["albedo"].data_ptr(), GUIDE_SPP, film["normal"].data_ptr(),
                            GUIDE_SPP, W, H, vp, scratch.data_ptr(), need_var, film["out_var"].data_ptr(), None)   # the null stream = torch's current stream here


def shipped():
    prod.denoise_device(film["beauty"].data_ptr(), SPP, film["albedo"].data_ptr(), GUIDE_SPP, film["normal"].data_ptr(), GUIDE_SPP, W, H, dp,
                        scratch.data_ptr(), need, film["out_shipped"].data_ptr(), None)


ms = {"variance_guided": [], "shipped": []}
host_ms = {"variance_guided": [], "shipped": []}
for i in range(WARMUP + RUNS):
    for name, fn in (("variance_guided", variance_guided), ("shipped", shipped)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        e0.record(); fn(); e1.record(); e1.synchronize()
        t1 = time.perf_counter()
        if i >= WARMUP: ms[name].append(e0.elapsed_time(e1)); host_ms[name].append((t1 - t0) * 1e3)
# the host clock around the same call + synchronise is an upper bound of the event time (launch overhead on top): events that did not
# bracket the kernels would show as an event time far BELOW it
for name in ms:
    assert statistics.median(ms[name]) > 0.2 * statistics.median(host_ms[name]), (name, statistics.median(ms[name]), statistics.median(host_ms[name]))
assert bool(torch.isfinite(film["out_var"]).all()) and bool(torch.isfinite(film["out_shipped"]).all())
level_bytes = 64 * W * H
prepass_bytes = (4 * 12 + 3 * 16) * W * H                    # four films read, three records written
moved = vp.levels * level_bytes - 16 * W * H + 12 * W * H + prepass_bytes   # (the last level writes the 12-B film pixel, not a record)
v, s = spread(ms["variance_guided"]), spread(ms["shipped"])
out = {"config": f"scene3 {W}x{H}, film {SPP} spp and half film {SPP // 2} spp mis zsobol, guides {GUIDE_SPP} spp, {vp.levels} levels, default parameters of "
                 f"both filters; {RUNS} timed calls of each, alternating, after {WARMUP} warm-up calls of each, HIP events around each call",
       "library": prod.version(), "variance_guided": v, "shipped": s,
       "host_clock_median_ms": {k: round(statistics.median(x), 4) for k, x in host_ms.items()},
       "variance_guided_over_shipped": round(v["median_ms"] / s["median_ms"], 4),
       "bytes_per_level_that_must_move": level_bytes, "bytes_per_pixel_per_level": 64, "bytes_whole_filter_that_must_move": moved,
       "GB_s_over_required_bytes": round(moved / (v["median_ms"] * 1e-3) / 1e9, 1),
       "Mpixels_s": round(W * H / (v["median_ms"] * 1e-3) / 1e6, 1)}
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
json.dump(out, open(OUT, "w"), indent=1)
print(json.dumps(out), flush=True)
