#!/usr/bin/env python3
"""Time of the per-pixel motion pieces (include/mi355pt_flow.h) on one GPU, each beside what it stands beside, in one process: scene 17 at
1920x1080 with its hero marked dynamic, frames of 4 spp (mis, ZSobol) with G-buffers at 16 spp.  Frame 0 (seed 0) is accumulated as a
first frame; then the scene is marked, the hero takes a translation and a yaw on the device (mi355pt_scene_move_instances) and the camera a
small step; frame 1 (seed 1) is the current frame of every timed call.  The motion is rigid so that the motion-table twin can run on the
same frames.  After WARMUP calls of each, RUNS calls of each, ALTERNATING, each call bracketed by HIP events:
  flow, flow_with_ids      mi355pt_render_flow_device without and with d_ids, beside mi355pt_render_ids_device (ids) and a copy of the 32
                           (36) bytes per pixel it writes
  flow_{half,nohalf}       mi355pt_temporal_accumulate_flow_device with the previous ids, beside mi355pt_temporal_accumulate_motion_device
                           (motion_*, the per-instance table form) and mi355pt_temporal_accumulate_device (existing_*)
  flow_noids_*             the same without ids (no id loads at all)
  rectified_flow_*         mi355pt_temporal_accumulate_rectified_flow_device (radius 2), beside its _motion twin and the existing call
  copy_*                   a device-to-device copy that moves the bytes the flow form MUST move per pixel: what tools/motion_rate.py counts
                           for the plain accumulation (116 without a half film, 152 with) plus the pixel's record (32) and, with the previous
                           ids, the two ids (8)
  mark                     mi355pt_scene_flow_mark, beside a device-to-device copy of the same 48 bytes per triangle (copy_mark)
Writes one JSON object to profiles/flow_rate.json (or the path given): medians, spread, ratios.  Needs a GPU; reads nothing outside the
repository.
usage: tools/flow_rate.py [RUNS (default 30, at least 20)] [OUTPUT.json]"""
import importlib, json, math, os, statistics, sys
import numpy as np
import torch  # first: see tests/conftest.py
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("toy-cpu-pathtracing_amd")
W, H, SPP, GUIDE_SPP, WARMUP = 1920, 1080, 4, 16, 5
HERO, HERO_T, HERO_YAW, CAMERA_STEP = 0, (0.12, 0.0, 0.06), 0.05, (0.1, 0.02, -0.05)
RUNS = max(20, int(sys.argv[1])) if len(sys.argv) > 1 else 30
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "flow_rate.json")
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
prod.scene_flow_mark(sc)
for i in range(3):
    cam.position[i] += CAMERA_STEP[i]
move_cam = sc.move_camera(cam)
c, s = math.cos(HERO_YAW), math.sin(HERO_YAW)
step = np.eye(4); step[:3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]; step[:3, 3] = HERO_T
m_cur = [m.copy() for m in m_prev]
m_cur[HERO] = (step @ m_prev[HERO].astype(np.float64)).astype(np.float32)
move_inst = sc.move_instances(cam, [HERO], [m_cur[HERO]])
assert prod.scene_flow_marked(sc)
cur = render(1)
cur["flow"] = torch.zeros((H, W, 8), dtype=torch.int32, device="cuda")
prod.render_flow_device(sc, cam, pkg.make_params(1), cur["flow"].data_ptr())
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
out["flow"] = torch.zeros((H, W, 8), dtype=torch.int32, device="cuda")
rneed = prod.temporal_rectify_scratch_bytes(W, H)
rscratch = torch.empty(rneed, dtype=torch.uint8, device="cuda")
n_tris = prod.export_bvh(sc)[1].shape[0]
PER_PIXEL = {"half": 60 + 60 + 4 + 28 + 32 + 8, "nohalf": 48 + 48 + 4 + 16 + 32 + 8, "flow": 32, "flow_with_ids": 36, "ids": 4}
BYTES = {k: v * W * H for k, v in PER_PIXEL.items()}
BYTES["mark"] = 48 * n_tris
copy_src = {k: torch.zeros(max(b // 2, 1), dtype=torch.uint8, device="cuda") for k, b in BYTES.items()}      # a copy of b / 2 bytes reads and writes b bytes ...
copy_src["mark"] = torch.zeros(BYTES["mark"], dtype=torch.uint8, device="cuda")                             # ... the mark's copy is compared as what it is
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


def motion(half, rectified):
    kw = dict(rectify_params=rp, d_scratch_ptr=rscratch.data_ptr(), scratch_bytes=rneed) if rectified else {}
    prod.temporal_accumulate_motion_device(frame(half), SPP, previous(half), view, W, H, tp, cur["ids"].data_ptr(), f0["ids"].data_ptr(), table.data_ptr(),
                                           table.shape[0], *outs(half), **kw)


def flow(half, rectified, ids=True):
    kw = dict(rectify_params=rp, d_scratch_ptr=rscratch.data_ptr(), scratch_bytes=rneed) if rectified else {}
    prod.temporal_accumulate_flow_device(frame(half), SPP, previous(half), view, W, H, tp, cur["ids"].data_ptr() if ids else None,
                                         f0["ids"].data_ptr() if ids else None, cur["flow"].data_ptr(), *outs(half), **kw)


CALLS = [("ids", lambda: prod.render_ids_device(sc, cam, pkg.make_params(1), out["ids"].data_ptr())),
         ("flow", lambda: prod.render_flow_device(sc, cam, pkg.make_params(1), out["flow"].data_ptr())),
         ("flow_with_ids", lambda: prod.render_flow_device(sc, cam, pkg.make_params(1), out["flow"].data_ptr(), out["ids"].data_ptr())),
         ("mark", lambda: prod.scene_flow_mark(sc)), ("copy_mark", lambda: copy_dst["mark"].copy_(copy_src["mark"]))]
for h in (True, False):
    k = "half" if h else "nohalf"
    CALLS += [(f"existing_{k}", lambda h=h: existing(h, False)), (f"motion_{k}", lambda h=h: motion(h, False)), (f"flow_{k}", lambda h=h: flow(h, False)),
              (f"flow_noids_{k}", lambda h=h: flow(h, False, False)), (f"rectified_existing_{k}", lambda h=h: existing(h, True)),
              (f"rectified_motion_{k}", lambda h=h: motion(h, True)), (f"rectified_flow_{k}", lambda h=h: flow(h, True)),
              (f"copy_{k}", lambda k=k: copy_dst[k].copy_(copy_src[k]))]
CALLS += [(f"copy_{k}", lambda k=k: copy_dst[k].copy_(copy_src[k])) for k in ("flow", "flow_with_ids", "ids")]


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
# (the timed marks re-marked the moved scene: the records written by the timed flow passes after them are all zero, those in cur["flow"] are not)
assert bool(torch.isfinite(out["film"]).all()) and bool(torch.isfinite(out["length"]).all()) and int(out["ids"].max()) > 0 and bool((cur["flow"] != 0).any())
res = {n: spread(v) for n, v in ms.items()}
med = {n: r["median_ms"] for n, r in res.items()}
pairs = [("flow", "ids"), ("flow_with_ids", "ids"), ("flow", "copy_flow"), ("flow_with_ids", "copy_flow_with_ids"), ("ids", "copy_ids"), ("mark", "copy_mark")]
for k in ("half", "nohalf"):
    pairs += [(f"flow_{k}", f"motion_{k}"), (f"flow_{k}", f"existing_{k}"), (f"flow_noids_{k}", f"existing_{k}"), (f"flow_{k}", f"copy_{k}"),
              (f"rectified_flow_{k}", f"rectified_motion_{k}"), (f"rectified_flow_{k}", f"rectified_existing_{k}"), (f"motion_{k}", f"existing_{k}")]
ratios = {f"{a}_over_{b}": round(med[a] / med[b], 4) for a, b in pairs}
ids_now = cur["ids"].cpu().numpy()
result = {"config": f"scene17 {W}x{H}, hero dynamic, frames of {SPP} spp mis zsobol, G-buffers {GUIDE_SPP} spp, default temporal parameters, rectify radius 2 gamma 2; the "
                    f"scene is marked, then the hero moves by {HERO_T} and yaws {HERO_YAW} rad and the camera steps {CAMERA_STEP}; {RUNS} timed calls of each, alternating, "
                    f"after {WARMUP} warm-up calls of each, HIP events around each call (a rectified call is two launches; the flow and ID passes include the clear of "
                    "their work counter)",
          "library": prod.version(), "camera_move": move_cam, "instance_move": {k: (float(v) if isinstance(v, np.floating) else v) for k, v in move_inst.items()},
          "hero_pixels": int((ids_now == HERO + 1).sum()), "triangles": int(n_tris), **res,
          "bytes_that_must_move": BYTES, "bytes_per_pixel": PER_PIXEL, "ratios": ratios,
          "copy_GB_s": {k: round((BYTES[k] if k != "mark" else 2 * BYTES[k]) / (med["copy_" + k] * 1e-3) / 1e9, 1) for k in BYTES}}
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
json.dump(result, open(OUT, "w"), indent=1)
print(json.dumps(result), flush=True)
