#!/usr/bin/env python3
"""Time of the rectified temporal accumulation (mi355pt_temporal_accumulate_rectified_device, csrc/pt_kernels_temporal_rectify.hip: the gather
launch and the LDS-stencil launch together) on one GPU, beside the unrectified accumulation, the filter that follows both and a plain copy,
in one process: scene 3 at 1920x1080, frames of 4 spp (mis, ZSobol) with G-buffers at 16 spp.  Frame 0 (seed 0, the scene's camera) is
accumulated as a first frame; frame 1 (seed 1) comes from the camera moved by (0.3, 0.1, -0.2) and yawed 0.05 rad.  After WARMUP calls of
each, RUNS calls of each, ALTERNATING: the rectified call with and without the half film at radius 1, 2 and 3 (gamma 2),
mi355pt_temporal_accumulate_device with and without the half film, mi355pt_denoise_var_device (5 levels, on the accumulated pair with spp 2)
and a device-to-device copy that moves the bytes the two launches MUST move, each call bracketed by HIP events.  Those bytes per pixel:
  gather    reads the current position, shading-normal and hit films (36), the previous film, (half,) position, shading-normal and hit films
            (60 / 48) and the previous length (4); writes the 32-byte record                                   132 with a half film, 120 without
  rectify   reads the current film (and half film) (24 / 12) and the record (32); writes the film, (the half film) and the length (28 / 16)
                                                                                                                84 with a half film,  60 without
Writes one JSON object to profiles/temporal_rectify_rate.json (or the path given): medians and spread.  The expectation to confirm or refute:
both launches together cost less than the 5-level filter that follows them.  Needs a GPU; reads nothing outside the repository.
usage: tools/temporal_rectify_rate.py [RUNS (default 30, at least 20)] [OUTPUT.json]"""
import importlib, json, math, os, statistics, sys, time
import torch  # first: see tests/conftest.py
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("toy-cpu-pathtracing_amd")
W, H, SPP, GUIDE_SPP, WARMUP = 1920, 1080, 4, 16, 5
MOVE, YAW = (0.3, 0.1, -0.2), 0.05
RUNS = max(20, int(sys.argv[1])) if len(sys.argv) > 1 else 30
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "temporal_rectify_rate.json")
prod = pkg.Product()


def load(move, yaw):
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
f0, cur = render(base, 0), render(moved, 1)
view = prod.temporal_view_from_cameras(moved[1], base[1])
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
rneed = prod.temporal_rectify_scratch_bytes(W, H)
rscratch = torch.empty(rneed, dtype=torch.uint8, device="cuda")
PER_PIXEL = {"half": {"gather": 36 + 60 + 4 + 32, "rectify": 24 + 32 + 28}, "nohalf": {"gather": 36 + 48 + 4 + 32, "rectify": 12 + 32 + 16}}
BYTES = {k: (v["gather"] + v["rectify"]) * W * H for k, v in PER_PIXEL.items()}
copy_src = {k: torch.zeros(b // 2, dtype=torch.uint8, device="cuda") for k, b in BYTES.items()}
copy_dst = {k: torch.empty_like(v) for k, v in copy_src.items()}


def previous(half):
    prev = dict(ptrs(f0, GEO), film=(acc["film"] if half else acc["film1"]).data_ptr(), length=(acc["length"] if half else acc["length1"]).data_ptr())
    if half:
        prev["half"] = acc["half"].data_ptr()
    return prev


def plain(half):
    prod.temporal_accumulate_device(ptrs(cur, (("film", "half") if half else ("film",)) + GEO), SPP, previous(half), view, W, H, tp, out["film"].data_ptr(),
                                    out["half"].data_ptr() if half else None, out["length"].data_ptr())    # the null stream = torch's current stream here


def rectified(half, radius):
    rp = prod.temporal_rectify_params_default()
    rp.radius = radius
    prod.temporal_accumulate_rectified_device(ptrs(cur, (("film", "half") if half else ("film",)) + GEO), SPP, previous(half), view, W, H, tp, rp,
                                              rscratch.data_ptr(), rneed, out["film"].data_ptr(), out["half"].data_ptr() if half else None,
                                              out["length"].data_ptr())


def filter5():
    prod.denoise_var_device(acc["film"].data_ptr(), acc["half"].data_ptr(), 2, None, f0["albedo"].data_ptr(), GUIDE_SPP, f0["shading_normal"].data_ptr(), GUIDE_SPP,
                            W, H, vp, scratch.data_ptr(), need, out["filtered"].data_ptr(), None)


CALLS = [(f"rectified_{'half' if h else 'nohalf'}_r{r}", (lambda h=h, r=r: rectified(h, r))) for h in (True, False) for r in (1, 2, 3)]
CALLS += [("unrectified_half", lambda: plain(True)), ("unrectified_nohalf", lambda: plain(False)), ("denoise_var_5_levels", filter5),
          ("copy_bytes_half", lambda: copy_dst["half"].copy_(copy_src["half"])), ("copy_bytes_nohalf", lambda: copy_dst["nohalf"].copy_(copy_src["nohalf"]))]


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
kind = lambda n: "nohalf" if "_nohalf" in n else "half"   # noqa: E731
rect = [n for n in med if n.startswith("rectified")]
result = {"config": f"scene3 {W}x{H}, frames of {SPP} spp mis zsobol, G-buffers {GUIDE_SPP} spp, default temporal parameters, gamma 2; moved view = ({MOVE[0]}, {MOVE[1]}, "
                    f"{MOVE[2]}) and a yaw of {YAW} rad; {RUNS} timed calls of each, alternating, after {WARMUP} warm-up calls of each, HIP events around each call "
                    "(a rectified call is two launches)",
          "library": prod.version(), **res,
          "host_clock_median_ms": {k: round(statistics.median(x), 4) for k, x in host_ms.items()},
          "bytes_that_must_move": BYTES, "bytes_per_pixel": PER_PIXEL,
          "GB_s_over_required_bytes": {n: round(BYTES[kind(n)] / (med[n] * 1e-3) / 1e9, 1) for n in rect},
          "copy_GB_s": {k: round(BYTES[k] / (med["copy_bytes_" + k] * 1e-3) / 1e9, 1) for k in BYTES},
          "rectified_over_filter": {n: round(med[n] / med["denoise_var_5_levels"], 4) for n in rect},
          "rectified_over_copy": {n: round(med[n] / med["copy_bytes_" + kind(n)], 4) for n in rect},
          "rectified_over_unrectified": {n: round(med[n] / med["unrectified_" + kind(n)], 4) for n in rect}}
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
json.dump(result, open(OUT, "w"), indent=1)
print(json.dumps(result), flush=True)
