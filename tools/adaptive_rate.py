#!/usr/bin/env python3
"""Adaptive sampling against uniform sampling at equal time, on one GPU in one process: scenes 3 and 8 at 1920x1080, mis +
ZSobol.  Per scene: uniform renders at 64, 256 and 1024 spp and the reference at 4096 spp (mi355pt_render_accum_device), adaptive renders
(mi355pt_render_adaptive_device, maximum 1024, minimum 16) at three thresholds taken from the frame itself — 1/2, 1/4 and 1/8 of the median
tile error after the first 16 samples: an error falls with the square root of the samples, so each step asks about four times the
samples of the tiles above it.  Every render is ONE call timed by HIP events around the whole call (host round trips of the adaptive
passes included).  Recorded per render: the time, the mean spp, the RMSE of the resolved frame against the resolved 4096-spp frame; per
adaptive render also the tiles per count (the spp map as a histogram) and, from a replay of the same passes through the public pieces, the
device time of the whole-frame launches, the tile-list launches and the steps.  The step and the normalisation alone: median of 30 calls
after 5 warm-up calls.  Writes profiles/adaptive_rate.json (or the path given).  Needs a GPU; reads nothing outside the repository.
usage: tools/adaptive_rate.py [OUTPUT.json]"""
import importlib, json, os, statistics, sys
import numpy as np
import torch  # first: see tests/conftest.py
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("toy-cpu-pathtracing_amd")
W, H, MAX_SPP, MIN_SPP, REF_SPP, DARK_EPS, WARMUP, RUNS = 1920, 1080, 1024, 16, 4096, 1e-3, 5, 30
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "adaptive_rate.json")
TX, TY = (W + 7) // 8, (H + 7) // 8
NT = TX * TY
prod = pkg.Product()


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(); r = fn(); e1.record(); e1.synchronize()
    return e0.elapsed_time(e1), r


def median_ms(fn):
    ms = [timed(fn)[0] for _ in range(WARMUP + RUNS)][WARMUP:]
    return round(statistics.median(ms), 4)


def film():
    return torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")


def resolve(f, spp):
    out = torch.empty_like(f)
    prod.film_resolve_device(f.data_ptr(), H * W, spp, out.data_ptr(), None)
    torch.cuda.synchronize()
    return out.cpu().numpy().astype(np.float64)


def state():
    return dict(film=film(), half=film(), spp=torch.zeros(NT, dtype=torch.int32, device="cuda"), err=torch.zeros(NT, dtype=torch.float32, device="cuda"),
                lst=torch.zeros(NT, dtype=torch.int32, device="cuda"), cnt=torch.zeros(1, dtype=torch.int32, device="cuda"),
                scratch=torch.zeros(prod.adaptive_scratch_bytes(W, H), dtype=torch.uint8, device="cuda"))


def step(st, ap, level):
    prod.adaptive_step_device(st["film"].data_ptr(), st["half"].data_ptr(), W, H, st["spp"].data_ptr(), st["err"].data_ptr(), ap, level, MAX_SPP,
                              st["scratch"].data_ptr(), st["scratch"].numel(), st["lst"].data_ptr(), st["cnt"].data_ptr(), None)


def run_scene(scene_id):
    sc = prod.new_scene()
    cam = pkg.scenes.load_scene(sc, scene_id, W, H)
    out = {"uniform": [], "adaptive": []}
    ref_prm = pkg.make_params(REF_SPP, "mis", "sobol")
    f = film()
    prod.render_accum_device(sc, cam, ref_prm, 0, REF_SPP, f.data_ptr(), None)
    ref = resolve(f, REF_SPP)
    for spp in (64, 256, 1024):
        prm = pkg.make_params(spp, "mis", "sobol")
        f = film()
        ms, _ = timed(lambda: prod.render_accum_device(sc, cam, prm, 0, spp, f.data_ptr(), None))
        out["uniform"].append({"spp": spp, "ms": round(ms, 2), "rmse": round(float(np.sqrt(np.mean((resolve(f, spp) - ref) ** 2))), 6)})
    prm = pkg.make_params(MAX_SPP, "mis", "sobol")
    # the frame's own scale: the median tile error after the first MIN_SPP samples (a threshold nothing exceeds: the step only writes the errors)
    st = state()
    st["spp"].fill_(MIN_SPP)
    prod.render_accum_device(sc, cam, prm, 0, MIN_SPP // 2, st["half"].data_ptr(), None)
    st["film"].copy_(st["half"])
    prod.render_accum_device(sc, cam, prm, MIN_SPP // 2, MIN_SPP, st["film"].data_ptr(), None)
    step(st, pkg.ffi.AdaptiveParams(3e38, DARK_EPS, MIN_SPP), MIN_SPP)
    torch.cuda.synchronize()
    med = float(np.nanmedian(st["err"].cpu().numpy()))
    out["median_tile_err_at_min_spp"] = med
    in_frame = np.minimum(8, W - 8 * (np.arange(NT) % TX)) * np.minimum(8, H - 8 * (np.arange(NT) // TX))
    for div in (2, 2, 4, 8):                                     # (the first pass is the warm-up: it loads the tile-list kernels, and is not recorded)
        ap = pkg.ffi.AdaptiveParams(med / div, DARK_EPS, MIN_SPP)
        st = state()
        ms, res = timed(lambda: prod.render_adaptive_device(sc, cam, prm, ap, st["film"].data_ptr(), st["half"].data_ptr(), st["spp"].data_ptr(), st["err"].data_ptr(),
                                                            st["lst"].data_ptr(), st["scratch"].data_ptr(), st["scratch"].numel(), None))
        if div == 2 and not out.get("warm"):
            out["warm"] = True
            continue
        spp = st["spp"].cpu().numpy()
        mean = film()
        prod.film_normalize_tiles_device(st["film"].data_ptr(), st["spp"].data_ptr(), W, H, mean.data_ptr(), None)
        rmse = float(np.sqrt(np.mean((resolve(mean, 1) - ref) ** 2)))
        # the same passes again through the public pieces, each launch with its own device time
        rp = state()
        rp["spp"].fill_(MIN_SPP)
        t_frame = t_list = t_step = 0.0
        s0 = pkg.ffi.Stats(); prod.render_accum_device(sc, cam, prm, 0, MIN_SPP // 2, rp["half"].data_ptr(), None, stats=s0)
        rp["film"].copy_(rp["half"])
        s1 = pkg.ffi.Stats(); prod.render_accum_device(sc, cam, prm, MIN_SPP // 2, MIN_SPP, rp["film"].data_ptr(), None, stats=s1)
        t_frame = s0.kernel_ms + s1.kernel_ms
        level = MIN_SPP
        while level <= MAX_SPP:
            t, _ = timed(lambda: step(rp, ap, level))
            t_step += t
            n = int(rp["cnt"].cpu().numpy()[0])
            if n == 0:
                break
            for b in range(level, 2 * level, 4096):              # (one launch per call: stats keep a range in one piece)
                s = pkg.ffi.Stats()
                prod.render_accum_tiles_device(sc, cam, prm, rp["lst"].cpu().numpy()[:n].astype(np.uint32), b, min(b + 4096, 2 * level), rp["film"].data_ptr(), None, stats=s)
                t_list += s.kernel_ms
            level *= 2
        assert torch.equal(rp["film"], st["film"]) and torch.equal(rp["spp"], st["spp"])
        out["adaptive"].append({"threshold": ap.threshold, "threshold_over_median": 1.0 / div, "ms": round(ms, 2), "passes": res.passes,
                                "mean_spp": round(res.total_samples / (W * H), 2), "tiles_at_max": res.tiles_at_max, "rmse": round(rmse, 6),
                                "tiles_per_count": {int(n): int((spp == n).sum()) for n in sorted(set(spp.tolist()))},
                                "replay_ms": {"whole_frame_launches": round(t_frame, 3), "tile_list_launches": round(t_list, 3), "steps": round(t_step, 3)},
                                "share_not_in_path_kernels": round(max(0.0, 1.0 - (t_frame + t_list) / ms), 4)})
        assert int((spp.astype(np.int64) * in_frame).sum()) == res.total_samples
    del out["warm"]
    # the step (at the maximum: it activates nothing, so every call does the same work) and the normalisation alone, on the last state
    ap = pkg.ffi.AdaptiveParams(med, DARK_EPS, MIN_SPP)
    st["spp"].fill_(MAX_SPP)
    out["step_median_ms"] = median_ms(lambda: step(st, ap, MAX_SPP))
    mean = film()
    out["normalize_median_ms"] = median_ms(lambda: prod.film_normalize_tiles_device(st["film"].data_ptr(), st["spp"].data_ptr(), W, H, mean.data_ptr(), None))
    return out


result = {"config": f"{W}x{H}, mis zsobol, adaptive max {MAX_SPP} min {MIN_SPP} dark_eps {DARK_EPS}, reference {REF_SPP} spp; single timed calls (HIP events around the whole "
                    f"call) for the renders, median of {RUNS} after {WARMUP} warm-up calls for the step and the normalisation",
          "library": prod.version()}
for scene_id in (3, 8):
    result[f"scene{scene_id}"] = run_scene(scene_id)
    print(json.dumps({f"scene{scene_id}": result[f"scene{scene_id}"]}), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
json.dump(result, open(OUT, "w"), indent=1)
