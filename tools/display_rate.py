#!/usr/bin/env python3
"""Time of the display stage (include/mi355pt_display.h, csrc/pt_kernels_display.hip) on one GPU beside the resolve it stands next to and a
plain copy, in one process, on a 1920x1080 film of three contents:
  rendered     scene 3 at 4 spp (mis, ZSobol);
  constant     one value everywhere — every lane of every wave of the meter's first launch on ONE histogram word, the LDS worst case;
  loguniform   the log-uniform frame of tests/display_reference.py without its special values: 64 different bins per wave, mostly.
Per content, after WARMUP calls of each, RUNS calls of each, ALTERNATING: the meter's two launches one by one
(mi355pt_probe_display_meter_ms: a HIP event between them), mi355pt_display_meter_device as a whole, mi355pt_display_device (REINHARD + sRGB,
the resolve's work; ACES + sRGB; REINHARD_EXT + linear), mi355pt_film_resolve_device (resolve_kernel) and a device-to-device copy of the
film's bytes (read once, written once: what the display and the resolve must move; the meter only reads), each bracketed by HIP events.
Writes one JSON object to profiles/display_rate.json (or the path given): medians, spread, the ratios to the copy and to resolve_kernel, and
the meter against the 5-level variance-guided filter of profiles/denoise_var_rate.json.
Needs a GPU; reads nothing outside the repository.
usage: tools/display_rate.py [RUNS (default 30, at least 20)] [OUTPUT.json]"""
import importlib, json, os, statistics, sys, time
import numpy as np
import torch  # first: see tests/conftest.py
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import display_reference as dr  # noqa: E402
pkg = importlib.import_module("toy-cpu-pathtracing_amd")
W, H, SPP, WARMUP = 1920, 1080, 4, 5
RUNS = max(20, int(sys.argv[1])) if len(sys.argv) > 1 else 30
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "display_rate.json")
prod = pkg.Product()

sc = prod.new_scene()
cam = pkg.scenes.load_scene(sc, 3, W, H)
rendered = torch.zeros((H, W, 3), device="cuda")
prod.render_accum_device(sc, cam, pkg.make_params(SPP, "mis", "sobol", seed=0), 0, SPP, rendered.data_ptr())
torch.cuda.synchronize()
films = {"rendered": rendered,
         "constant": torch.from_numpy(dr.frame(W, H, "constant", spp=SPP)[0]).cuda(),
         "loguniform": torch.from_numpy(dr.frame(W, H, "loguniform", spp=SPP, specials=False)[0]).cuda()}
need = prod.display_scratch_bytes(W, H)
scratch = torch.zeros(need, dtype=torch.uint8, device="cuda")
record = torch.zeros(8, dtype=torch.int32, device="cuda")
out = torch.full((H, W, 3), float("nan"), device="cuda")
copy_dst = torch.empty((H, W, 3), device="cuda")
meter_p = prod.display_params_default()


def display_params(tone, encode):
    p = prod.display_params_default()
    p.tone, p.encode = pkg.ffi.TONE[tone], pkg.ffi.ENCODE[encode]
    return p


DISPLAYS = {"display_reinhard_srgb": display_params("reinhard", "srgb"), "display_aces_srgb": display_params("aces", "srgb"),
            "display_reinhard_ext_linear": display_params("reinhard-ext", "linear")}


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "spread": round((max(ms) - min(ms)) / statistics.median(ms), 4), "runs": len(ms)}


result = {"config": f"{W}x{H} film of {SPP} spp; {RUNS} timed calls of each, alternating, after {WARMUP} warm-up calls of each, HIP events around each call "
                    f"(the meter's two launches: an event between them, mi355pt_probe_display_meter_ms)",
          "library": prod.version(), "film_bytes": W * H * 12, "meter_scratch_bytes": need, "meter_rows": need // (258 * 4)}
filter_ms = json.load(open(os.path.join(ROOT, "profiles", "denoise_var_rate.json")))["variance_guided"]["median_ms"]
for content, film in films.items():
    calls = [("meter_device", lambda: prod.display_meter_device(film.data_ptr(), W, H, SPP, meter_p, None, scratch.data_ptr(), need, record.data_ptr()))]
    calls += [(n, (lambda p=p: prod.display_device(film.data_ptr(), W, H, SPP, p, record.data_ptr(), out.data_ptr()))) for n, p in DISPLAYS.items()]
    calls += [("resolve_kernel", lambda: prod.film_resolve_device(film.data_ptr(), W * H, SPP, out.data_ptr())), ("copy_film_bytes", lambda: copy_dst.copy_(film))]
    ms = {n: [] for n, _ in calls}
    ms["meter_hist_launch"], ms["meter_finish_launch"] = [], []
    for i in range(WARMUP + RUNS):
        torch.cuda.synchronize()
        a, b = prod.probe_display_meter_ms(film.data_ptr(), W, H, SPP, meter_p, scratch.data_ptr(), need, record.data_ptr())
        if i >= WARMUP: ms["meter_hist_launch"].append(a); ms["meter_finish_launch"].append(b)
        for name, fn in calls:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record(); fn(); e1.record(); e1.synchronize()
            if i >= WARMUP: ms[name].append(e0.elapsed_time(e1))
    torch.cuda.synchronize()
    rec = record.cpu().numpy().view(np.uint32)
    want, _, _ = dr.meter(film.cpu().numpy(), SPP)
    assert np.array_equal(rec, want), (content, rec, want)                 # what was timed is what the restatement gives
    assert bool(torch.isfinite(out).all())
    res = {n: spread(v) for n, v in ms.items()}
    med = {n: r["median_ms"] for n, r in res.items()}
    res["record"] = {"E": float(dr.from_bits(rec[:1])[0]), "L_avg": float(dr.from_bits(rec[2:3])[0]), "N": int(rec[3]), "below": int(rec[4]), "above": int(rec[5])}
    res["over_copy"] = {n: round(med[n] / med["copy_film_bytes"], 4) for n in med if n != "copy_film_bytes"}
    res["over_resolve_kernel"] = {n: round(med[n] / med["resolve_kernel"], 4) for n in med if n != "resolve_kernel"}
    res["GB_s"] = {"meter_hist_launch_read": round(W * H * 12 / (med["meter_hist_launch"] * 1e-3) / 1e9, 1),
                   "copy_read_plus_write": round(2 * W * H * 12 / (med["copy_film_bytes"] * 1e-3) / 1e9, 1),
                   "display_reinhard_srgb_read_plus_write": round(2 * W * H * 12 / (med["display_reinhard_srgb"] * 1e-3) / 1e9, 1)}
    res["meter_over_5_level_filter"] = round(med["meter_device"] / filter_ms, 4)
    result[content] = res
result["variance_guided_filter_median_ms"] = filter_ms
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
json.dump(result, open(OUT, "w"), indent=1)
print(json.dumps(result), flush=True)
