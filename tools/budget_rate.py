#!/usr/bin/env python3
"""Time of the sample-budget pieces (include/mi355pt_budget.h) on one GPU, each beside what it stands beside, in one process: scene 17 at
1920x1080 with its hero marked dynamic, frames of 4 spp (mis, ZSobol) with G-buffers at 16 spp.  Frame 0 (seed 0) is accumulated as a first
frame; then the scene is marked, the hero takes a translation and a yaw on the device and the camera a small step; frame 1 (seed 1) is the
current frame of every timed call (tools/flow_rate.py's setup).  After WARMUP calls of each, RUNS calls of each, ALTERNATING, each call
bracketed by HIP events:
  probe_{static,table,table_ids,flow,flow_ids}   mi355pt_temporal_budget_device (with d_pred_length), beside the accumulation of the same carry
                           with the half film: accumulate_static (temporal_kernel, static carry), accumulate_table_ids, accumulate_flow_ids;
                           probe_first is the probe without a previous frame
  copy_probe               a device-to-device copy of the bytes the static probe MUST move per pixel: 36 of the current frame (position,
                           normal, hit), 4 x (8 + 4 + 12 + 12) = 144 of the four taps' hit.y, length, position and normal at most — neighbouring
                           lanes share taps, so 36 + 36 + 4 of P is the floor that is copied here (76 bytes per pixel)
  adaptive_step            mi355pt_adaptive_step_device at level 4 (launch_adaptive_step: adaptive_err_kernel + adaptive_compact_kernel) on the
                           plain frame's pair — the select + compact pass of the budget driver is not a call of its own; its kernels are timed
                           by a kernel trace of this script, merged with --merge-kernel-stats
  pair_normalize, length_credit, film_copy        the two streaming steps, beside a copy of one film
  frame_plain              the plain 4-spp frame: [0, 2) into H, F := H, [2, 4) into F, the table-form accumulation
  frame_budget             the budgeted frame on the same inputs: probe (table form, previous ids), driver (base 4, max 32, target 8), pair
                           normalise, the same accumulation with spp = 2, length credit; its total samples are recorded beside it
Writes one JSON object to profiles/budget_rate.json (or the path given): medians, spread, ratios.  Needs a GPU; reads nothing outside the
repository.
usage: tools/budget_rate.py [RUNS (default 30, at least 20)] [OUTPUT.json]
       tools/budget_rate.py --merge-kernel-stats KERNEL_STATS.csv OUTPUT.json     (no GPU: adds the per-kernel averages of a kernel trace)"""
import csv, importlib, json, math, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if len(sys.argv) > 1 and sys.argv[1] == "--merge-kernel-stats":
    want = ("budget_select_kernel", "adaptive_compact_kernel", "adaptive_err_kernel", "budget_probe_kernel", "temporal_kernel",
            "pair_normalize_tiles_kernel", "length_credit_kernel")
    rows = {}
    for r in csv.DictReader(open(sys.argv[2])):
        name = r.get("Name") or r.get("KernelName") or ""
        for w in want:
            if w in name:
                rows[name] = {"calls": int(r["Calls"]), "average_us": round(float(r["AverageNs"]) / 1e3, 2), "min_us": round(float(r["MinNs"]) / 1e3, 2),
                              "max_us": round(float(r["MaxNs"]) / 1e3, 2)}
    res = json.load(open(sys.argv[3]))
    res["kernel_trace"] = {"source": "rocprofv3 --kernel-trace --stats around this script in a run of its own (its event timings are not the ones above)", "kernels": rows}
    json.dump(res, open(sys.argv[3], "w"), indent=1)
    print(json.dumps(res["kernel_trace"]))
    sys.exit(0)
import numpy as np
import torch  # first: see tests/conftest.py
sys.path.insert(0, ROOT)
pkg = importlib.import_module("toy-cpu-pathtracing_amd")
W, H, SPP, GUIDE_SPP, WARMUP = 1920, 1080, 4, 16, 5
BASE, MAX, TARGET = 4, 32, 8.0
HERO, HERO_T, HERO_YAW, CAMERA_STEP = 0, (0.12, 0.0, 0.06), 0.05, (0.1, 0.02, -0.05)
RUNS = max(20, int(sys.argv[1])) if len(sys.argv) > 1 else 30
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "budget_rate.json")
prod = pkg.Product()

sc = prod.new_scene()
cam = pkg.scenes.load_scene(sc, 17, W, H, build=False)
d65 = sc.add_lut470(pkg.scenes.presets()["cie_illum_d6500"])
sc.set_instance_dynamic(HERO)
sc.build(cam)
GEO = ("position", "shading_normal", "hit")
ptrs = lambda f, keys: {k: f[k].data_ptr() for k in keys}   # noqa: E731


def render_pair(seed, film, half):
    prm = pkg.make_params(SPP, "mis", "sobol", seed=seed)
    film.zero_(); half.zero_()
    prod.render_accum_device(sc, cam, prm, 0, SPP // 2, half.data_ptr())
    film.copy_(half)
    prod.render_accum_device(sc, cam, prm, SPP // 2, SPP, film.data_ptr())


def render(seed):
    f = {k: torch.zeros((H, W, 3), device="cuda") for k in ("film", "half") + GEO}
    prod.render_gbuffer_accum_device(sc, cam, pkg.make_params(GUIDE_SPP, "mis", "sobol", seed=seed), d65, 0, GUIDE_SPP, ptrs(f, GEO))
    render_pair(seed, f["film"], f["half"])
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
sc.move_camera(cam)
c, s = math.cos(HERO_YAW), math.sin(HERO_YAW)
step = np.eye(4); step[:3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]; step[:3, 3] = HERO_T
m_cur = [m.copy() for m in m_prev]
m_cur[HERO] = (step @ m_prev[HERO].astype(np.float64)).astype(np.float32)
sc.move_instances(cam, [HERO], [m_cur[HERO]])
cur = render(1)
cur["flow"] = torch.zeros((H, W, 8), dtype=torch.int32, device="cuda")
prod.render_flow_device(sc, cam, pkg.make_params(1), cur["flow"].data_ptr())
view = prod.temporal_view_from_cameras(cam, cam_prev)
table = torch.from_numpy(prod.motion_table(cam, cam_prev, m_cur, m_prev)).cuda()
tp = prod.temporal_params_default()
bp = prod.budget_params(BASE, MAX, TARGET)
acc = {k: torch.zeros((H, W, 3), device="cuda") for k in ("film", "half")}
acc["length"] = torch.zeros((H, W), device="cuda")
prod.temporal_accumulate_device(ptrs(f0, ("film", "half") + GEO), SPP, None, None, W, H, tp, acc["film"].data_ptr(), acc["half"].data_ptr(), acc["length"].data_ptr())
torch.cuda.synchronize()
prev = dict(ptrs(f0, GEO), film=acc["film"].data_ptr(), half=acc["half"].data_ptr(), length=acc["length"].data_ptr())
out = {k: torch.full((H, W, 3), float("nan"), device="cuda") for k in ("film", "half")}
out["length"] = torch.full((H, W), float("nan"), device="cuda")
TY, TX = (H + 7) // 8, (W + 7) // 8
pred = torch.zeros((H, W), device="cuda")
tile_len = torch.zeros(TY * TX, device="cuda")
tile_spp = torch.zeros(TY * TX, dtype=torch.int32, device="cuda")
tile_err = torch.zeros(TY * TX, device="cuda")
step_spp = torch.zeros(TY * TX, dtype=torch.int32, device="cuda")
lst = torch.zeros(TY * TX, dtype=torch.int32, device="cuda")
count = torch.zeros(4, dtype=torch.int32, device="cuda")
nbytes = prod.adaptive_scratch_bytes(W, H)
scratch = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
work = {k: torch.zeros((H, W, 3), device="cuda") for k in ("film", "half")}
ap = pkg.ffi.AdaptiveParams(0.05, 1e-3, BASE)
MOTIONS = {"static": None, "table": prod.budget_motion(cur["ids"].data_ptr(), None, table.data_ptr(), table.shape[0]),
           "table_ids": prod.budget_motion(cur["ids"].data_ptr(), f0["ids"].data_ptr(), table.data_ptr(), table.shape[0]),
           "flow": prod.budget_motion(None, None, None, 0, cur["flow"].data_ptr()),
           "flow_ids": prod.budget_motion(cur["ids"].data_ptr(), f0["ids"].data_ptr(), None, 0, cur["flow"].data_ptr())}
frame = ptrs(cur, ("film", "half") + GEO)
outs = (out["film"].data_ptr(), out["half"].data_ptr(), out["length"].data_ptr())


def probe(kind, with_prev=True):
    prod.temporal_budget_device(ptrs(cur, GEO), prev if with_prev else None, view if with_prev else None, W, H, tp, MOTIONS[kind], bp, pred.data_ptr(),
                                tile_len.data_ptr(), tile_spp.data_ptr())


def accumulate(kind, spp=SPP, cur_frame=None):
    fr = cur_frame or frame
    if kind == "static":
        prod.temporal_accumulate_device(fr, spp, prev, view, W, H, tp, *outs)
    elif kind == "table_ids":
        prod.temporal_accumulate_motion_device(fr, spp, prev, view, W, H, tp, cur["ids"].data_ptr(), f0["ids"].data_ptr(), table.data_ptr(), table.shape[0], *outs)
    else:
        prod.temporal_accumulate_flow_device(fr, spp, prev, view, W, H, tp, cur["ids"].data_ptr(), f0["ids"].data_ptr(), cur["flow"].data_ptr(), *outs)


def adaptive_step():
    step_spp.fill_(BASE)
    prod.adaptive_step_device(cur["film"].data_ptr(), work["half"].data_ptr(), W, H, step_spp.data_ptr(), tile_err.data_ptr(), ap, BASE, MAX, scratch.data_ptr(), nbytes,
                              lst.data_ptr(), count.data_ptr())


work_frame = dict(ptrs(cur, GEO), film=work["film"].data_ptr(), half=work["half"].data_ptr())
totals = []


def frame_plain():
    render_pair(1, work["film"], work["half"])
    accumulate("table_ids", SPP, work_frame)


def frame_budget():
    probe("table_ids")
    res = prod.render_budget_device(sc, cam, pkg.make_params(MAX, "mis", "sobol", seed=1), bp, tile_spp.data_ptr(), work["film"].data_ptr(), work["half"].data_ptr(),
                                    lst.data_ptr(), scratch.data_ptr(), nbytes)
    totals.append((int(res.total_samples), int(res.passes), int(res.tiles_at_max)))
    prod.film_pair_normalize_tiles_device(work["film"].data_ptr(), work["half"].data_ptr(), tile_spp.data_ptr(), W, H, work["film"].data_ptr(), work["half"].data_ptr())
    accumulate("table_ids", 2, work_frame)
    prod.temporal_length_credit_device(out["length"].data_ptr(), tile_spp.data_ptr(), BASE, float(tp.max_history), W, H)


COPY_BYTES = {"probe": 76 * W * H, "film": 24 * W * H}
copy_src = {k: torch.zeros(b // 2, dtype=torch.uint8, device="cuda") for k, b in COPY_BYTES.items()}     # a copy of b / 2 bytes reads and writes b bytes
copy_dst = {k: torch.empty_like(v) for k, v in copy_src.items()}
CALLS = [(f"probe_{k}", lambda k=k: probe(k)) for k in MOTIONS] + [("probe_first", lambda: probe("static", False))]
CALLS += [(f"accumulate_{k}", lambda k=k: accumulate(k)) for k in ("static", "table_ids", "flow_ids")]
CALLS += [("copy_probe", lambda: copy_dst["probe"].copy_(copy_src["probe"])), ("film_copy", lambda: copy_dst["film"].copy_(copy_src["film"])),
          ("adaptive_step", adaptive_step),
          ("pair_normalize", lambda: prod.film_pair_normalize_tiles_device(cur["film"].data_ptr(), cur["half"].data_ptr(), tile_spp.data_ptr(), W, H,
                                                                           work["film"].data_ptr(), work["half"].data_ptr())),
          ("length_credit", lambda: prod.temporal_length_credit_device(out["length"].data_ptr(), tile_spp.data_ptr(), BASE, float(tp.max_history), W, H)),
          ("frame_plain", frame_plain), ("frame_budget", frame_budget)]


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "spread": round((max(ms) - min(ms)) / statistics.median(ms), 4), "runs": len(ms)}


probe("table_ids")        # (tile_spp holds a budget before the first timed pair normalise)
torch.cuda.synchronize()
ms = {n: [] for n, _ in CALLS}
for i in range(WARMUP + RUNS):
    for name, fn in CALLS:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(); fn(); e1.record(); e1.synchronize()
        if i >= WARMUP: ms[name].append(e0.elapsed_time(e1))
assert bool(torch.isfinite(out["film"]).all()) and bool(torch.isfinite(out["length"]).all()) and len(set(totals)) == 1
res = {n: spread(v) for n, v in ms.items()}
med = {n: r["median_ms"] for n, r in res.items()}
pairs = [("probe_static", "accumulate_static"), ("probe_table_ids", "accumulate_table_ids"), ("probe_flow_ids", "accumulate_flow_ids"), ("probe_static", "copy_probe"),
         ("probe_table", "probe_static"), ("probe_flow", "probe_static"), ("pair_normalize", "film_copy"), ("length_credit", "film_copy"), ("frame_budget", "frame_plain")]
spp_host = tile_spp.cpu().numpy()
total, passes, at_max = totals[0]
result = {"config": f"scene17 {W}x{H}, hero dynamic, frames of {SPP} spp mis zsobol, G-buffers {GUIDE_SPP} spp, default temporal parameters, budget base {BASE} max {MAX} "
                    f"target {TARGET}; the hero moves by {HERO_T} and yaws {HERO_YAW} rad and the camera steps {CAMERA_STEP}; {RUNS} timed calls of each, alternating, "
                    f"after {WARMUP} warm-up calls of each, HIP events around each call (frame_budget includes the driver's 4-byte read-backs and its read-back of "
                    "tile_spp for the result)",
          "library": prod.version(), **res, "ratios": {f"{a}_over_{b}": round(med[a] / med[b], 4) for a, b in pairs},
          "budget_frame": {"total_samples": total, "uniform_samples": SPP * W * H, "samples_over_uniform": round(total / (SPP * W * H), 4), "passes": passes,
                           "tiles_at_max": at_max, "tiles": int(spp_host.size), "tiles_by_spp": {str(int(v)): int((spp_host == v).sum()) for v in np.unique(spp_host)}},
          "copy_GB_s": {k: round(COPY_BYTES[k] / (med["copy_probe" if k == "probe" else "film_copy"] * 1e-3) / 1e9, 1) for k in COPY_BYTES}}
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
json.dump(result, open(OUT, "w"), indent=1)
print(json.dumps(result), flush=True)
