#!/usr/bin/env python3
"""Quality of the robust film (include/mi355pt_robust.h) on the CPU: bucket films from the oracle, combined by the NumPy restatement
(tests/robust_reference.py).  No GPU.

Cases (160 x 120, ZSobol): two where the plain frame shows fireflies, and a control.
  scene 8 under pt    a smooth SF11 glass hero under the room's area light: without light sampling every caustic path is found by chance;
  scene 12 under nee  four BK7 glass heroes of roughness 0.05 .. 0.75: light sampling cannot connect through the glass, the rough lobes
                      give rare strong contributions;
  scene 3 under mis   the textured Lambert hero: the control, where nothing should be trimmed.
For each, at n = 64 and n = 256 samples: the frame as 32 bucket films of n / 32 consecutive sample indices (Oracle.render_accum(s_begin,
s_end), one call per bucket); the K = 16 and K = 8 films are sums of two and four neighbours (the same sample ranges; the float sum is
taken in another order than one call would).  MEAN (the plain film), MOM and GMON at K = 8 / 16 / 32 — and GMON with gini_scale 0.5 and 2
at K = 16 — against a reference of 4096 samples (16 x the larger count, another seed):
  rmse_resolved   RMSE after Sensor::to_rgb (mean, Reinhard, sRGB) of both;
  rel_mse         mean over pixels and channels of (x - r)^2 / (r^2 + 0.01) on the linear film;
  energy          sum of the linear film over the reference's: the bias (below 1: energy removed);
  trimmed         share of pixels with t > 0.
`fireflies` counts the pixels of the plain frame with a channel above 4 x the reference's + 0.5.
Writes profiles/robust_quality.json (or the path given).
usage: tools/robust_quality.py [OUTPUT.json] [WIDTH HEIGHT]"""
import importlib, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import robust_reference as rr  # noqa: E402
import ptoracle  # noqa: E402
pkg = importlib.import_module("toy-cpu-pathtracing_amd")
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "robust_quality.json")
W, H = (int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else (160, 120)
CASES = [(8, "pt", "smooth glass hero, no light sampling: caustic paths found by chance"),
         (12, "nee", "four rough-glass heroes: light sampling cannot connect through glass"),
         (3, "mis", "control: textured Lambert hero, nothing to trim")]
COUNTS, KS, REF_SPP, KMAX = (64, 256), (8, 16, 32), 4096, 32
THREADS = min(16, os.cpu_count() or 1)
orc = ptoracle.Oracle()


def metrics(theta, ref_mean, ref_rgb, trim):
    x = theta.astype(np.float64)
    rgb = orc.film_resolve(theta, 1).astype(np.float64)
    return {"rmse_resolved": round(float(np.sqrt(np.mean((rgb - ref_rgb) ** 2))), 5),
            "rel_mse": round(float(np.mean((x - ref_mean) ** 2 / (ref_mean ** 2 + 0.01))), 5),
            "energy": round(float(x.sum() / ref_mean.sum()), 4),
            "trimmed": round(float((trim[..., 0] != 0).mean()), 4)}


result = {"config": f"{W}x{H}, ZSobol, oracle films; reference {REF_SPP} spp with seed 1; buckets from {KMAX} calls of Oracle.render_accum per frame, "
                    f"K = 16 and 8 as sums of neighbours; combination: tests/robust_reference.py", "cases": []}
for scene_id, strategy, why in CASES:
    t0 = time.time()
    sc = orc.new_scene()
    cam = pkg.scenes.load_scene(sc, scene_id, W, H)
    orc.set_faithful(sc, False)
    ref, _ = orc.render_accum(sc, cam, pkg.make_params(REF_SPP, strategy, "sobol", seed=1), threads=THREADS)
    ref_mean = ref.astype(np.float64) / REF_SPP
    ref_rgb = orc.film_resolve(ref, REF_SPP).astype(np.float64)
    case = {"scene": scene_id, "strategy": strategy, "why": why, "frames": []}
    for n in COUNTS:
        prm = pkg.make_params(n, strategy, "sobol", seed=0)
        per = n // KMAX
        films = np.stack([orc.render_accum(sc, cam, prm, k * per, (k + 1) * per, threads=THREADS)[0] for k in range(KMAX)])
        plain = films.sum(0, dtype=np.float64) / n
        frame = {"spp": n, "fireflies": int(((plain > 4.0 * ref_mean + 0.5).any(axis=2)).sum()), "combos": {}}
        for k in KS:
            g = KMAX // k
            stack = films.reshape(k, g, H, W, 3).sum(1, dtype=np.float32) if g > 1 else films
            combos = [("mean", 1.0), ("mom", 1.0), ("gmon", 1.0)] + ([("gmon", 0.5), ("gmon", 2.0)] if k == 16 else [])
            for mode, scale in combos:
                theta, _, trim = rr.combine(stack, n // k, rr.MODES[mode], scale, False)
                frame["combos"][f"K{k}_{mode}" + ("" if scale == 1.0 else f"_scale{scale:g}")] = metrics(theta, ref_mean, ref_rgb, trim)
        case["frames"].append(frame)
        print(scene_id, strategy, n, json.dumps(frame), flush=True)
    case["seconds"] = round(time.time() - t0, 1)
    result["cases"].append(case)
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
json.dump(result, open(OUT, "w"), indent=1)
