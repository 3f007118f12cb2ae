#!/usr/bin/env python3
"""Time of the denoiser (mi355pt_denoise_device, csrc/pt_kernels_denoise.hip) on one GPU beside the render it cleans up, in one process:
scene 3 at 1920x1080, beauty film at 16 spp (mis, ZSobol), albedo and shading-normal films at 64 spp, default parameters (5 levels).
After WARMUP calls, RUNS calls of the whole filter (prepass + 5 levels), each bracketed by HIP events on the stream it runs on; the
16-spp beauty render of the same frame is timed the same number of times by its own device events (stats.kernel_ms), the two guide films
once each.  Writes one JSON object to profiles/denoise_rate.json (or the path given): medians, spread, the bytes a level MUST move (64 B
per pixel: three 16-B records read, one written) and the rate that figure gives over the measured time — a floor on the traffic, not a
counter reading.  Needs a GPU; reads nothing outside the repository.
usage: tools/denoise_rate.py [RUNS (default 30, at least 20)] [OUTPUT.json]"""
import importlib, json, os, statistics, sys, time
import torch  # first: see tests/conftest.py
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("toy-cpu-pathtracing_amd")
W, H, SPP, GUIDE_SPP, WARMUP = 1920, 1080, 16, 64, 5
RUNS = max(20, int(sys.argv[1])) if len(sys.argv) > 1 else 30
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "denoise_rate.json")
prod = pkg.Product(); sc = prod.new_scene()
cam = pkg.scenes.load_scene(sc, 3, W, H, build=False)
d65 = sc.add_lut470(pkg.scenes.presets()["cie_illum_d6500"])
sc.build(cam)
film = {k: torch.zeros((H, W, 3), device="cuda") for k in ("beauty", "albedo", "normal", "out")}
prm, guide = pkg.make_params(SPP, "mis", "sobol"), pkg.make_params(GUIDE_SPP, "mis", "sobol")


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "spread": round((max(ms) - min(ms)) / statistics.median(ms), 4), "runs": len(ms)}


beauty_ms = []
for i in range(RUNS + 1):                                   # the last pass leaves exactly one 16-spp film behind for the filter
    film["beauty"].zero_()
    st = pkg.ffi.Stats(); prod.render_accum_device(sc, cam, prm, 0, SPP, film["beauty"].data_ptr(), None, stats=st)
    if i: beauty_ms.append(st.kernel_ms)
guide_ms = {}
for name, kind in (("albedo", pkg.ffi.AOV_ALBEDO), ("normal", pkg.ffi.AOV_SHADING_NORMAL)):
    st = pkg.ffi.Stats(); prod.render_aov_accum_device(sc, cam, guide, kind, d65, 0, GUIDE_SPP, film[name].data_ptr(), None, stats=st)
    guide_ms[name] = round(st.kernel_ms, 4)
dp = prod.denoise_params_default()
need = prod.denoise_scratch_bytes(W, H)
scratch = torch.empty(need, dtype=torch.uint8, device="cuda")


def denoise():
    prod.denoise_device(film["beauty"].data_ptr(), SPP, film["albedo"].data_ptr(), GUIDE_SPP, film["normal"].data_ptr(), GUIDE_SPP, W, H, dp,
                        scratch.data_ptr(), need, film["out"].data_ptr(), None)   # the null stream = torch's current stream here


den_ms, host_ms = [], []
for i in range(WARMUP + RUNS):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    e0.record(); denoise(); e1.record(); e1.synchronize()
    t1 = time.perf_counter()
    if i >= WARMUP: den_ms.append(e0.elapsed_time(e1)); host_ms.append((t1 - t0) * 1e3)
# the host clock around the same call + synchronise is an upper bound of the event time (launch overhead on top): events that did not
# bracket the kernels would show as an event time far BELOW it
assert statistics.median(den_ms) > 0.2 * statistics.median(host_ms), (statistics.median(den_ms), statistics.median(host_ms))
assert bool(torch.isfinite(film["out"]).all())
level_bytes = 64 * W * H
prepass_bytes = (3 * 12 + 3 * 16) * W * H                    # three films read, three records written
moved = dp.levels * level_bytes - 16 * W * H + 12 * W * H + prepass_bytes   # (the last level writes the 12-B film pixel, not a record)
d, b = spread(den_ms), spread(beauty_ms)
out = {"config": f"scene3 {W}x{H}, beauty {SPP} spp mis zsobol, guides {GUIDE_SPP} spp, {dp.levels} levels, default sigmas; "
                 f"{RUNS} timed calls after {WARMUP} warm-up calls, HIP events around each call",
       "library": prod.version(), "denoise": d, "denoise_host_clock_median_ms": round(statistics.median(host_ms), 4), "beauty_render_16spp": b, "guide_render_64spp_ms": guide_ms,
       "denoise_over_beauty_render": round(d["median_ms"] / b["median_ms"], 4),
       "bytes_per_level_that_must_move": level_bytes, "bytes_per_pixel_per_level": 64, "bytes_whole_filter_that_must_move": moved,
       "GB_s_over_required_bytes": round(moved / (d["median_ms"] * 1e-3) / 1e9, 1),
       "Mpixels_s": round(W * H / (d["median_ms"] * 1e-3) / 1e6, 1)}
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
json.dump(out, open(OUT, "w"), indent=1)
print(json.dumps(out), flush=True)
