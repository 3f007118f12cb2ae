#!/usr/bin/env python3
"""Time of the temporal reprojection (mi355pt_temporal_accumulate_device, csrc/pt_kernels_temporal.hip) on one GPU beside the filter that
follows it and a plain copy, in one process: scene 3 at 1920x1080, frames of 4 spp (mis, ZSobol) with G-buffers at 16 spp.  Frame 0 (seed
0, the scene's camera) is accumulated as a first frame; frame 1 (seed 1) comes from the same camera (a STATIC view: every pixel lands on a
pixel centre) and from the camera moved by (0.3, 0.1, -0.2) and yawed 0.05 rad (a MOVED view), each with and without the half film.  After
WARMUP calls of each, RUNS calls of each, ALTERNATING with mi355pt_denoise_var_device (5 levels, on the accumulated pair with spp 2) and with
a device-to-device copy that moves the bytes the kernel MUST move (each input film read once, each output written once: 152 B per pixel
with a half film, 116 B without), each call bracketed by HIP events.  Writes one JSON object to profiles/temporal_rate.json (or the path
given): medians and spread.  The expectation to confirm or refute: one gather pass costs less than the 5-level filter that follows it.
Needs a GPU; reads nothing outside the repository.
usage: tools/temporal_rate.py [RUNS (default 30, at least 20)] [OUTPUT.json]"""
import importlib, json, os, statistics, sys, time
import torch  # first: see tests/conftest.py
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("toy-cpu-pathtracing_amd")
W, H, SPP, GUIDE_SPP, WARMUP = 1920, 1080, 4, 16, 5
MOVE, YAW = (0.3, 0.1, -0.2), 0.05
RUNS = max(20, int(sys.argv[1])) if len(sys.argv) > 1 else 30
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "temporal_rate.json")
prod = pkg.Product()


def load(move, yaw):
    import math
    sc = prod.new_scene()
    cam = pkg.scenes.load_scene(sc, 3, W, H, build=False)
    d65 = sc.add_lut470(pkg.scenes.presets()["cie_illum_d6500"])
    c, s = math.cos(yaw), math.sin(yaw)
    x, y, z = tuple(cam.direction)
    for i, v in enumerate((c * x + s * z, y, -s * x + c * z)):
        cam.direction[i] = v
        cam.position[i] += move[i]
    sc.build(cam)
    return sc, cam, d65


def render(handle, seed):
    sc, cam, d65 = handle
    f = {k: torch.zeros((H, W, 3), device="cuda") for k in ("film", "half", "albedo", "shading_normal", "position", "hit")}
    prod.render_gbuffer_accum_device(sc, cam, pkg.make_params(GUIDE_SPP, "mis", "sobol", seed=seed), d65, 0, GUIDE_SPP,
                                     {k: f[k].data_ptr() for k in ("albedo", "shading_normal", "position", "hit")})
    prm = pkg.make_params(SPP, "mis", "sobol", seed=seed)
    prod.render_accum_device(sc, cam, prm, 0, SPP // 2, f["half"].data_ptr())
    torch.cuda.synchronize()
    f["film"].copy_(f["half"])
    prod.render_accum_device(sc, cam, prm, SPP // 2, SPP, f["film"].data_ptr())
    torch.cuda.synchronize()
    return f


base, moved = load((0.0, 0.0, 0.0), 0.0), load(MOVE, YAW)
f0 = render(base, 0)
cur = {"static": render(base, 1), "moved": render(moved, 1)}
view = {"static": prod.temporal_view_from_cameras(base[1], base[1]), "moved": prod.temporal_view_from_cameras(moved[1], base[1])}
tp, vp = prod.temporal_params_default(), prod.denoise_var_params_default()
GEO = ("position", "shading_normal", "hit")
acc = {k: torch.zeros((H, W, 3), device="cuda") for k in ("film", "half", "film1")}
acc["length"], acc["length1"] = torch.zeros((H, W), device="cuda"), torch.zeros((H, W), device="cuda")
ptrs = lambda f, keys: {k: f[k].data_ptr() for k in keys}   # noqa: E731
# frame 0 as a first frame: the accumulated pair, and the accumulated film of the call without a half film
prod.temporal_accumulate_device(ptrs(f0, ("film", "half") + GEO), SPP, None, None, W, H, tp, acc["film"].data_ptr(), acc["half"].data_ptr(), acc["length"].data_ptr())
prod.temporal_accumulate_device(ptrs(f0, ("film",) + GEO), SPP, None, None, W, H, tp, acc["film1"].data_ptr(), None, acc["length1"].data_ptr())
torch.cuda.synchronize()
out = {k: torch.full((H, W, 3), float("nan"), device="cuda") for k in ("film", "half", "filtered")}
out["length"] = torch.full((H, W), float("nan"), device="cuda")
need = prod.denoise_var_scratch_bytes(W, H)
scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
BYTES = {"half": (5 * 12 + 4 * 12 + 4 + 12 + 2 * 12 + 4) * W * H, "nohalf": (4 * 12 + 3 * 12 + 4 + 12 + 12 + 4) * W * H}
copy_src = {k: torch.zeros(b // 2, dtype=torch.uint8, device="cuda") for k, b in BYTES.items()}
copy_dst = {k: torch.empty_like(v) for k, v in copy_src.items()}


def accumulate(which, half):
    prev = dict(ptrs(f0, GEO), film=(acc["film"] if half else acc["film1"]).data_ptr(), length=(acc["length"] if half else acc["length1"]).data_ptr())
    if half:
        prev["half"] = acc["half"].data_ptr()
    prod.temporal_accumulate_device(ptrs(cur[which], (("film", "half") if half else ("film",)) + GEO), SPP, prev, view[which], W, H, tp, out["film"].data_ptr(),
                                    out["half"].data_ptr() if half else None, out["length"].data_ptr())    # the null stream = torch's current stream here


def filter5():
    prod.denoise_var_device(acc["film"].data_ptr(), acc["half"].data_ptr(), 2, None, f0["albedo"].data_ptr(), GUIDE_SPP, f0["shading_normal"].data_ptr(), GUIDE_SPP,
                            W, H, vp, scratch.data_ptr(), need, out["filtered"].data_ptr(), None)


CALLS = [("temporal_static_half", lambda: accumulate("static", True)), ("temporal_moved_half", lambda: accumulate("moved", True)),
         ("temporal_static_nohalf", lambda: accumulate("static", False)), ("temporal_moved_nohalf", lambda: accumulate("moved", False)),
         ("denoise_var_5_levels", filter5), ("copy_bytes_half", lambda: copy_dst["half"].copy_(copy_src["half"])),
         ("copy_bytes_nohalf", lambda: copy_dst["nohalf"].copy_(copy_src["nohalf"]))]


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "spread": round((max(ms) - min(ms)) / statistics.median(ms), 4), "runs": len(ms)}


ms, host_ms = {n: [] for n, _ in CALLS}, {n: [] for n, _ in CALLS}
for i in range(WARMUP + RUNS):
    for name, fn in CALLS:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        e0.record(); fn(); e1.record(); e1.synchronize()
        t1 = time.perf_counter()
        if i >= WARMUP: ms[name].append(e0.elapsed_time(e1)); host_ms[name].append((t1 - t0) * 1e3)
assert bool(torch.isfinite(out["film"]).all()) and bool(torch.isfinite(out["length"]).all()) and bool(torch.isfinite(out["filtered"]).all())
res = {n: spread(v) for n, v in ms.items()}
med = {n: r["median_ms"] for n, r in res.items()}
result = {"config": f"scene3 {W}x{H}, frames of {SPP} spp mis zsobol, G-buffers {GUIDE_SPP} spp, default parameters; moved view = ({MOVE[0]}, {MOVE[1]}, {MOVE[2]}) and a yaw "
                    f"of {YAW} rad; {RUNS} timed calls of each, alternating, after {WARMUP} warm-up calls of each, HIP events around each call",
          "library": prod.version(), **res,
          "host_clock_median_ms": {k: round(statistics.median(x), 4) for k, x in host_ms.items()},
          "bytes_that_must_move": BYTES, "bytes_per_pixel": {k: b // (W * H) for k, b in BYTES.items()},
          "GB_s_over_required_bytes": {n: round(BYTES["half" if n.endswith("_half") else "nohalf"] / (med[n] * 1e-3) / 1e9, 1) for n in med if n.startswith("temporal")},
          "copy_GB_s": {k: round(BYTES[k] / (med["copy_bytes_" + k] * 1e-3) / 1e9, 1) for k in BYTES},
          "temporal_over_filter": {n: round(med[n] / med["denoise_var_5_levels"], 4) for n in med if n.startswith("temporal")},
          "temporal_over_copy": {n: round(med[n] / med["copy_bytes_" + ("half" if n.endswith("_half") else "nohalf")], 4) for n in med if n.startswith("temporal")}}
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
json.dump(result, open(OUT, "w"), indent=1)
print(json.dumps(result), flush=True)
