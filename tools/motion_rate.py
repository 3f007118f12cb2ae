#!/usr/bin/env python3
"""Time of the object-motion pieces (include/mi355pt_motion.h) on one GPU, each beside its existing twin and a plain copy, in one process:
scene 17 at 1920x1080 with its hero marked dynamic, frames of 4 spp (mis, ZSobol) with G-buffers at 16 spp.  Frame 0 (seed 0) is
accumulated as a first frame; between the frames the hero takes a translation and a yaw on the device (mi355pt_scene_move_instances) and
the camera a small step; frame 1 (seed 1) is the current frame of every timed call.  After WARMUP calls of each, RUNS calls of each,
ALTERNATING, each call bracketed by HIP events:
  ids                      mi355pt_render_ids_device, beside a 1-spp mi355pt_render_gbuffer_accum_device launch (shading normal, position, hit)
                           and a copy of the 4 bytes per pixel it writes
  motion_{half,nohalf}     mi355pt_temporal_accumulate_motion_device with the previous ids, beside mi355pt_temporal_accumulate_device —
                           the kernel of the parent commit, byte for byte (profiles/motion_asm_identity.txt), in the same binary
  motion_noids_*           the same without the previous ids (one gather fewer per tap)
  rectified_motion_*       mi355pt_temporal_accumulate_rectified_motion_device (radius 2), beside mi355pt_temporal_accumulate_rectified_device
  copy_*                   a device-to-device copy that moves the bytes the plain accumulation MUST move.  Those bytes per pixel: the current
                           film (and half film), position, shading-normal and hit films (48 / 60 with a half film), the previous ones (48 / 60)
                           and the previous length (4); written: the film, (the half film,) the length (16 / 28): 116 without a half film, 152
                           with; the motion twin adds the pixel's id (4) and, with the previous ids, theirs (4; the taps' reuse is the cache's)
Writes one JSON object to profiles/motion_rate.json (or the path given): medians, spread, ratios.  Needs a GPU; reads nothing outside the
repository.
usage: tools/motion_rate.py [RUNS (default 30, at least 20)] [OUTPUT.json]"""
import importlib, json, math, os, statistics, sys
import numpy as np
import torch  # first: see tests/conftest.py
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("toy-cpu-pathtracing_amd")
W, H, SPP, GUIDE_SPP, WARMUP = 1920, 1080, 4, 16, 5
HERO, HERO_T, HERO_YAW, CAMERA_STEP = 0, (0.12, 0.0, 0.06), 0.05, (0.1, 0.02, -0.05)
RUNS = max(20, int(sys.argv[1])) if len(sys.argv) > 1 else 30
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "motion_rate.json")
prod = pkg.Product()

sc = prod.new_scene()
cam = pkg.scenes.load_scene(sc, 17, W, H, build=False)
d65 = sc.add_lut470(pkg.scenes.presets()["cie_illum_d6500"])
sc.set_instance_dynamic(HERO)
sc.build(cam)
GEO = ("position", "shading_normal", "hit")
ptrs = lambda f, keys: {k: f[k].data_ptr() for k in keys}   # noqa: E731


def render(seed):
    f = {k: torch.zeros((H, W, 3), device="cuda") for k in ("film", "half") + GEO}
    prod.render_gbuffer_accum_device(sc, cam, pkg.make_params(GUIDE_SPP, "mis", "sobol", seed=seed), d65, 0, GUIDE_SPP, ptrs(f, GEO))
    prm = pkg.make_params(SPP, "mis", "sobol", seed=seed)
    prod.render_accum_device(sc, cam, prm, 0, SPP // 2, f["half"].data_ptr())
    torch.cuda.synchronize()
    f["film"].copy_(f["half"])
    prod.render_accum_device(sc, cam, prm, SPP // 2, SPP, f["film"].data_ptr())
    f["ids"] = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    prod.render_ids_device(sc, cam, pkg.make_params(1), f["ids"].data_ptr())
    torch.cuda.synchronize()
    return f


f0 = render(0)
cam_prev = pkg.ffi.Camera.from_buffer_copy(cam)
m_prev = [m.copy() for _, _, m in sc.instances]
for i in range(3):
    cam.position[i] += CAMERA_STEP[i]
move_cam = sc.move_camera(cam)
c, s = math.cos(HERO_YAW), math.sin(HERO_YAW)
step = np.eye(4); step[:3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]; step[:3, 3] = HERO_T
m_cur = [m.copy() for m in m_prev]
m_cur[HERO] = (step @ m_prev[HERO].astype(np.float64)).astype(np.float32)
move_inst = sc.move_instances(cam, [HERO], [m_cur[HERO]])
cur = render(1)
view = prod.temporal_view_from_cameras(cam, cam_prev)
table = torch.from_numpy(prod.motion_table(cam, cam_prev, m_cur, m_prev)).cuda()
tp, rp = prod.temporal_params_default(), prod.temporal_rectify_params_default()
acc = {k: torch.zeros((H, W, 3), device="cuda") for k in ("film", "half", "film1")}
acc["length"], acc["length1"] = torch.zeros((H, W), device="cuda"), torch.zeros((H, W), device="cuda")
prod.temporal_accumulate_device(ptrs(f0, ("film", "half") + GEO), SPP, None, None, W, H, tp, acc["film"].data_ptr(), acc["half"].data_ptr(), acc["length"].data_ptr())
prod.temporal_accumulate_device(ptrs(f0, ("film",) + GEO), SPP, None, None, W, H, tp, acc["film1"].data_ptr(), None, acc["length1"].data_ptr())
torch.cuda.synchronize()
out = {k: torch.full((H, W, 3), float("nan"), device="cuda") for k in ("film", "half")}
out["length"] = torch.full((H, W), float("nan"), device="cuda")
out["ids"] = torch.zeros((H, W), dtype=torch.int32, device="cuda")
gb1 = {k: torch.zeros((H, W, 3), device="cuda") for k in GEO}
rneed = prod.temporal_rectify_scratch_bytes(W, H)
rscratch = torch.empty(rneed, dtype=torch.uint8, device="cuda")
PER_PIXEL = {"half": 60 + 60 + 4 + 28, "nohalf": 48 + 48 + 4 + 16, "ids": 4}
BYTES = {k: v * W * H for k, v in PER_PIXEL.items()}
copy_src = {k: torch.zeros(b // 2, dtype=torch.uint8, device="cuda") for k, b in BYTES.items()}
copy_dst = {k: torch.empty_like(v) for k, v in copy_src.items()}


def previous(half):
    prev = dict(ptrs(f0, GEO), film=(acc["film"] if half else acc["film1"]).data_ptr(), length=(acc["length"] if half else acc["length1"]).data_ptr())
    if half:
        prev["half"] = acc["half"].data_ptr()
    return prev


def frame(half):
    return ptrs(cur, (("film", "half") if half else ("film",)) + GEO)


def outs(half):
    return out["film"].data_ptr(), out["half"].data_ptr() if half else None, out["length"].data_ptr()


def existing(half, rectified):
    if rectified:
        prod.temporal_accumulate_rectified_device(frame(half), SPP, previous(half), view, W, H, tp, rp, rscratch.data_ptr(), rneed, *outs(half))
    else:
        prod.temporal_accumulate_device(frame(half), SPP, previous(half), view, W, H, tp, *outs(half))


def motion(half, rectified, prev_ids=True):
    kw = dict(rectify_params=rp, d_scratch_ptr=rscratch.data_ptr(), scratch_bytes=rneed) if rectified else {}
    prod.temporal_accumulate_motion_device(frame(half), SPP, previous(half), view, W, H, tp, cur["ids"].data_ptr(), f0["ids"].data_ptr() if prev_ids else None,
                                           table.data_ptr(), table.shape[0], *outs(half), **kw)


def gbuffer1():
    for t in gb1.values():
        t.zero_()
    prod.render_gbuffer_accum_device(sc, cam, pkg.make_params(1, "mis", "sobol"), d65, 0, 1, ptrs(gb1, GEO))


CALLS = [("ids", lambda: prod.render_ids_device(sc, cam, pkg.make_params(1), out["ids"].data_ptr())), ("gbuffer_1spp_with_clears", gbuffer1),
         ("gbuffer_clears", lambda: [t.zero_() for t in gb1.values()])]
for h in (True, False):
    k = "half" if h else "nohalf"
    CALLS += [(f"existing_{k}", lambda h=h: existing(h, False)), (f"motion_{k}", lambda h=h: motion(h, False)),
              (f"motion_noids_{k}", lambda h=h: motion(h, False, False)), (f"rectified_existing_{k}", lambda h=h: existing(h, True)),
              (f"rectified_motion_{k}", lambda h=h: motion(h, True)), (f"copy_{k}", lambda k=k: copy_dst[k].copy_(copy_src[k]))]
CALLS += [("copy_ids", lambda: copy_dst["ids"].copy_(copy_src["ids"]))]


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "spread": round((max(ms) - min(ms)) / statistics.median(ms), 4), "runs": len(ms)}


ms = {n: [] for n, _ in CALLS}
for i in range(WARMUP + RUNS):
    for name, fn in CALLS:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(); fn(); e1.record(); e1.synchronize()
        if i >= WARMUP: ms[name].append(e0.elapsed_time(e1))
assert bool(torch.isfinite(out["film"]).all()) and bool(torch.isfinite(out["length"]).all()) and int(out["ids"].max()) > 0
res = {n: spread(v) for n, v in ms.items()}
med = {n: r["median_ms"] for n, r in res.items()}
ratios = {f"{a}_over_{b}": round(med[a] / med[b], 4) for a, b in
          [(f"{p}motion_{k}", f"{p}existing_{k}") for p in ("", "rectified_") for k in ("half", "nohalf")] +
          [(f"motion_noids_{k}", f"existing_{k}") for k in ("half", "nohalf")] + [(f"motion_{k}", f"copy_{k}") for k in ("half", "nohalf")] +
          [(f"existing_{k}", f"copy_{k}") for k in ("half", "nohalf")] + [("ids", "copy_ids")]}
ratios["ids_over_gbuffer_1spp"] = round(med["ids"] / max(med["gbuffer_1spp_with_clears"] - med["gbuffer_clears"], 1e-6), 4)
ids_now = cur["ids"].cpu().numpy()
result = {"config": f"scene17 {W}x{H}, hero dynamic, frames of {SPP} spp mis zsobol, G-buffers {GUIDE_SPP} spp, default temporal parameters, rectify radius 2 gamma 2; between "
                    f"the frames the hero moves by {HERO_T} and yaws {HERO_YAW} rad, the camera steps {CAMERA_STEP}; {RUNS} timed calls of each, alternating, after "
                    f"{WARMUP} warm-up calls of each, HIP events around each call (a rectified call is two launches; the 1-spp G-buffer launch is timed with the "
                    "clears of its three films, which are timed alone too)",
          "library": prod.version(), "camera_move": move_cam, "instance_move": {k: (float(v) if isinstance(v, np.floating) else v) for k, v in move_inst.items()},
          "hero_pixels": int((ids_now == HERO + 1).sum()), "table_entries": int(table.shape[0]), **res,
          "bytes_that_must_move": BYTES, "bytes_per_pixel": PER_PIXEL, "ratios": ratios,
          "copy_GB_s": {k: round(BYTES[k] / (med["copy_" + k] * 1e-3) / 1e9, 1) for k in BYTES}}
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
json.dump(result, open(OUT, "w"), indent=1)
print(json.dumps(result), flush=True)
