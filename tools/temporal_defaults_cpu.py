#!/usr/bin/env python3
"""Does the SPECIFICATION of the temporal reprojection (include/mi355pt_temporal.h, restated by tests/temporal_reference.py) meet the bar
of tests/test_temporal_gpu.py::test_temporal_static_accumulation, and what would other validity parameters give?  No GPU: the oracle renders
the films, the CPU restatement of the G-buffer pass the G-buffers.  Scene 3 at 64x48, mis + ZSobol; 8 static frames of 4 spp (seeds 0 .. 7)
with G-buffers at 16 spp, accumulated with and without the half film; RMSE after the resolve against a 1024-spp frame (seed 1000), beside
plain 4-spp and 32-spp frames (seed 0).  The bar is E_acc <= sqrt(E_4 E_32).  Writes profiles/temporal_defaults_cpu.json (or the path given).
usage: tools/temporal_defaults_cpu.py [OUTPUT.json]"""
import importlib, json, os, sys
import numpy as np
import torch  # noqa: F401  first: see tests/conftest.py
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
pkg = importlib.import_module("toy-cpu-pathtracing_amd")
import gbuffer_reference, ptoracle, temporal_reference as tr  # noqa: E401,E402
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "temporal_defaults_cpu.json")
W, H, SPP, GUIDE_SPP, FRAMES = 64, 48, 4, 16, 8
orc, ref = ptoracle.Oracle(), gbuffer_reference.GbufferReference()
sc, cam, _ = tr.load_moved(orc, pkg, 3, W, H); orc.set_faithful(sc, False)
gsc, gcam, gd65 = tr.load_moved(ref, pkg, 3, W, H); ref.set_faithful(gsc, False)
rmse = lambda a, b: float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))   # noqa: E731
plain = lambda spp, seed: orc.film_resolve(orc.render_accum(sc, cam, pkg.make_params(spp, "mis", "sobol", seed=seed))[0], spp)   # noqa: E731
truth = plain(1024, 1000)
e4, e32 = rmse(plain(4, 0), truth), rmse(plain(32, 0), truth)
frames = []
for k in range(FRAMES):
    p = pkg.make_params(SPP, "mis", "sobol", seed=k)
    half = orc.render_accum(sc, cam, p, 0, SPP // 2)[0]
    film = orc.render_accum(sc, cam, p, SPP // 2, SPP, accum=half.copy())[0]
    gb = ref.render_gbuffer_accum(gsc, gcam, pkg.make_params(GUIDE_SPP, "mis", "sobol", seed=k), gd65, want=("shading_normal", "position", "hit"))
    frames.append((film, half, gb))
view = tr.view_from_cameras(cam, cam)
rows = []
for kw in ({}, {"normal_cos": 0.8}, {"normal_cos": 0.5, "pos_tol": 0.02}):
    for with_half in (True, False):
        prev = None
        for film, half, gb in frames:
            cur = dict(gb, film=film, half=half if with_half else None)
            of, oh, L = tr.accumulate(cur, SPP, prev, view if prev is not None else None, tr.params(**kw))
            prev = dict(gb, film=of, half=oh, length=L)
        hit = frames[-1][2]["hit"][..., 1] > 0
        eacc = rmse(orc.film_resolve(of, 2 if with_half else 1), truth)
        rows.append({"params": dict(tr.DEFAULTS, **kw), "half_film": with_half, "E_acc": round(eacc, 5), "E_acc_over_E_32": round(eacc / e32, 3),
                     "meets_bar": eacc <= (e4 * e32) ** 0.5, "share_of_hit_pixels_at_length_8": round(float((L[hit] == FRAMES).mean()), 4)})
out = {"config": f"scene3 {W}x{H} mis zsobol, {FRAMES} static frames of {SPP} spp (seeds 0..{FRAMES - 1}), G-buffers {GUIDE_SPP} spp, oracle films, "
                 "NumPy f32 restatement; RMSE of the resolved frame against 1024 spp (seed 1000)",
       "E_4": round(e4, 5), "E_32": round(e32, 5), "bar_sqrt_E4_E32": round((e4 * e32) ** 0.5, 5), "runs": rows}
json.dump(out, open(OUT, "w"), indent=1)
print(json.dumps(out))
