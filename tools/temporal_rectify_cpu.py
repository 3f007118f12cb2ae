#!/usr/bin/env python3
"""Does the SPECIFICATION of the rectified temporal accumulation (include/mi355pt_temporal_rectify.h, restated by
tests/temporal_rectify_reference.py) do what it is for?  No GPU: the oracle renders the films, the CPU restatement of the G-buffer pass the
G-buffers — the setup of tools/temporal_defaults_cpu.py.  Scene 3 at 64x48, mis + ZSobol, a static camera, frames of 4 spp with seeds 0 .. 11
(a half film each) and G-buffers at 16 spp; RMSE after the resolve against a 1024-spp frame (seed 1000), beside plain 4-spp and 32-spp frames
(seed 0).  Frames 0 .. 7 build the history, frames 8 .. 11 follow:
  static      every frame as rendered: the rectification must cost nothing.  Bar: E_rect after 8 frames <= sqrt(E_4 E_32).
  x0.25, x4,  the films of frames 0 .. 7 are scaled (the light was a quarter / four times as bright; split: a quarter on the left half of the
  split       image, four times on the right), frames 8 .. 11 are the true ones.  Bar after the 4 true frames:
              E_rect <= sqrt(E_unrectified E_32), the geometric midpoint between "did nothing" and "ideal".
Each case runs with the rectification (default parameters) and without.  Writes profiles/temporal_rectify_cpu.json (or the path given);
tests/test_temporal_rectify.py asserts the bars on the same figures (it imports `figures` from here).
usage: tools/temporal_rectify_cpu.py [OUTPUT.json]"""
import importlib, json, os, sys
import numpy as np
import torch  # noqa: F401  first: see tests/conftest.py
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)
W, H, SPP, GUIDE_SPP, HISTORY, AFTER = 64, 48, 4, 16, 8, 4
CASES = ("static", "x0.25", "x4", "split")


def scale_of(case):
    """the factor on the films of the history frames, (1, W, 1)"""
    s = np.ones((1, W, 1), np.float32)
    if case == "x0.25":
        s[:] = 0.25
    elif case == "x4":
        s[:] = 4.0
    elif case == "split":
        s[:, :W // 2], s[:, W // 2:] = 0.25, 4.0
    return s


def rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))


def chain(frames, view, case, rectified, resolve):
    """accumulates the HISTORY scaled frames and the AFTER true ones -> the resolved frames after frame HISTORY - 1, HISTORY and the last"""
    import temporal_reference as tr
    import temporal_rectify_reference as rr
    s, prev, out = scale_of(case), None, {}
    for k, (film, half, gb) in enumerate(frames):
        f = s if k < HISTORY else np.float32(1.0)
        cur = dict(gb, film=film * f, half=half * f)
        acc = (rr.accumulate if rectified else tr.accumulate)(cur, SPP, prev, view if prev is not None else None)
        prev = dict(gb, film=acc[0], half=acc[1], length=acc[2])
        if k in (HISTORY - 1, HISTORY, HISTORY + AFTER - 1):
            out[k] = resolve(acc[0])
    return out


def figures():
    """-> the dict this tool writes"""
    pkg = importlib.import_module("toy-cpu-pathtracing_amd")
    import gbuffer_reference, ptoracle, temporal_reference as tr  # noqa: E401
    orc, ref = ptoracle.Oracle(), gbuffer_reference.GbufferReference()
    sc, cam, _ = tr.load_moved(orc, pkg, 3, W, H); orc.set_faithful(sc, False)
    gsc, gcam, gd65 = tr.load_moved(ref, pkg, 3, W, H); ref.set_faithful(gsc, False)
    plain = lambda spp, seed: orc.film_resolve(orc.render_accum(sc, cam, pkg.make_params(spp, "mis", "sobol", seed=seed))[0], spp)   # noqa: E731
    truth = plain(1024, 1000)
    e4, e32 = rmse(plain(4, 0), truth), rmse(plain(32, 0), truth)
    frames = []
    for k in range(HISTORY + AFTER):
        p = pkg.make_params(SPP, "mis", "sobol", seed=k)
        half = orc.render_accum(sc, cam, p, 0, SPP // 2)[0]
        film = orc.render_accum(sc, cam, p, SPP // 2, SPP, accum=half.copy())[0]
        gb = ref.render_gbuffer_accum(gsc, gcam, pkg.make_params(GUIDE_SPP, "mis", "sobol", seed=k), gd65, want=("shading_normal", "position", "hit"))
        frames.append((film, half, gb))
    view = tr.view_from_cameras(cam, cam)
    resolve = lambda film: orc.film_resolve(film, 2)   # noqa: E731
    runs = {}
    for case in CASES:
        err = {}
        for name, rectified in (("rectified", True), ("unrectified", False)):
            got = chain(frames, view, case, rectified, resolve)
            err[name] = {"history": rmse(got[HISTORY - 1], truth), "after_1": rmse(got[HISTORY], truth), "after_4": rmse(got[HISTORY + AFTER - 1], truth)}
        if case == "static":
            e_r, e_u, bar = err["rectified"]["history"], err["unrectified"]["history"], (e4 * e32) ** 0.5
        else:
            e_r, e_u = err["rectified"]["after_4"], err["unrectified"]["after_4"]
            bar = (e_u * e32) ** 0.5
        runs[case] = {"E_rect": round(e_r, 5), "E_unrectified": round(e_u, 5), "bar": round(bar, 5), "meets_bar": bool(e_r <= bar),
                      "E_rect_over_E_unrectified": round(e_r / e_u, 4), "rmse": {n: {k: round(v, 5) for k, v in d.items()} for n, d in err.items()}}
    return {"config": f"scene3 {W}x{H} mis zsobol, static camera, frames of {SPP} spp with a half film (seeds 0..{HISTORY + AFTER - 1}), G-buffers {GUIDE_SPP} spp, "
                      f"oracle films, NumPy f32 restatement, default parameters (radius 2, gamma 2); {HISTORY} history frames (scaled per case), then {AFTER} true "
                      "frames; RMSE of the resolved frame against 1024 spp (seed 1000); static: E after the history frames, bar sqrt(E_4 E_32); the others: E "
                      "after the 4 true frames, bar sqrt(E_unrectified E_32)",
            "E_4": round(e4, 5), "E_32": round(e32, 5), "bar_static_sqrt_E4_E32": round((e4 * e32) ** 0.5, 5), "runs": runs}


if __name__ == "__main__":
    OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "temporal_rectify_cpu.json")
    out = figures()
    json.dump(out, open(OUT, "w"), indent=1)
    print(json.dumps(out))
