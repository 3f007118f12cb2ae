#!/usr/bin/env python3
"""What guided half-resolution rendering (include/mi355pt_upsample.h) buys, on one GPU: scenes 3 (the default 1024 x 1024 textures, as
bench.py) and 19 at 1920x1080, mis + ZSobol, n in {4, 16, 64}.  Per scene and n four kinds of frame are compared —
    full          the full-resolution frame at n spp
    half          the half-resolution frame at n spp, upsampled with the guides (a quarter of the path samples)
    half_equal    the half-resolution frame at 4n spp, upsampled with the guides (EQUAL path samples)
    replicated    the half-resolution frame at n spp, each pixel written to its four full pixels
— the guided ones with and without the albedo films, and every one but the replicated with and without the variance-guided filter behind
it (then with the half film).  Each entry records the tone-mapped RMSE against a 1024-spp full-resolution frame (seed 1000) and the wall
time of ALL launches of that pipeline — both G-buffers (16 spp), the beauty launches, the upsample, the filter, the resolve, and the clears of
the films they write — as the median of RUNS synchronised repetitions after one warm-up.  Writes one JSON object to profiles/upsample_quality.json (or the path given).
Needs a GPU; reads nothing outside the repository.
usage: tools/upsample_quality.py [OUTPUT.json]"""
import importlib, json, os, statistics, sys, time
import torch  # first: see tests/conftest.py
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("toy-cpu-pathtracing_amd")
W, H, GUIDE_SPP, REF_SPP, RUNS = 1920, 1080, 16, 1024, 3
w, h = W // 2, H // 2
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "upsample_quality.json")
prod = pkg.Product()
GUIDES = ("albedo", "shading_normal", "position", "hit")
GEO = ("shading_normal", "position", "hit")
up, vp = prod.upsample_params_default(), prod.denoise_var_params_default()
need = prod.denoise_var_scratch_bytes(W, H)
scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
z = lambda hh, ww: torch.zeros((hh, ww, 3), device="cuda")   # noqa: E731
ptrs = lambda d, keys: {k: d[k].data_ptr() for k in keys}   # noqa: E731


def beauty(sc, cam, hh, ww, n, with_half, seed=0):
    """-> (film, half or None): sums of n samples"""
    prm = pkg.make_params(n, "mis", "sobol", seed=seed)
    film = z(hh, ww)
    if not with_half:
        prod.render_accum_device(sc, cam, prm, 0, n, film.data_ptr())
        return film, None
    half = z(hh, ww)
    prod.render_accum_device(sc, cam, prm, 0, n // 2, half.data_ptr())
    film.copy_(half)                                        # (torch's current stream is the null stream the launches run on)
    prod.render_accum_device(sc, cam, prm, n // 2, n, film.data_ptr())
    return film, half


def gbuffer(sc, cam, d65, hh, ww, keys):
    g = {k: z(hh, ww) for k in keys}
    prod.render_gbuffer_accum_device(sc, cam, pkg.make_params(GUIDE_SPP, "mis", "sobol", seed=0), d65, 0, GUIDE_SPP, ptrs(g, keys))
    return g


def resolve(film, spp):
    rgb = torch.empty_like(film)
    prod.film_resolve_device(film.data_ptr(), film.shape[0] * film.shape[1], spp, rgb.data_ptr())
    return rgb


def filtered(film, half, spp, g):
    out = z(H, W)
    prod.denoise_var_device(film.data_ptr(), half.data_ptr(), spp, None, g["albedo"].data_ptr(), GUIDE_SPP, g["shading_normal"].data_ptr(), GUIDE_SPP, W, H, vp,
                            scratch.data_ptr(), need, out.data_ptr())
    return resolve(out, 1)


def full_frame(sc, cam, low_cam, d65, n, albedo, dv):
    film, half = beauty(sc, cam, H, W, n, dv)
    if not dv:
        return resolve(film, n)
    return filtered(film, half, n, gbuffer(sc, cam, d65, H, W, ("albedo", "shading_normal")))


def half_frame(sc, cam, low_cam, d65, n, albedo, dv):
    gf = gbuffer(sc, cam, d65, H, W, GUIDES if (albedo or dv) else GEO)
    gl = gbuffer(sc, low_cam, d65, h, w, GUIDES if albedo else GEO)
    film, half = beauty(sc, low_cam, h, w, n, dv)
    of, oh = z(H, W), (z(H, W) if dv else None)
    keys = GUIDES if albedo else GEO
    prod.upsample_device(film.data_ptr(), half.data_ptr() if dv else None, n, ptrs(gl, keys), GUIDE_SPP, ptrs(gf, keys), GUIDE_SPP, W, H, up, of.data_ptr(),
                         oh.data_ptr() if dv else None)
    return filtered(of, oh, 2, gf) if dv else resolve(of, 1)


def replicated_frame(sc, cam, low_cam, d65, n, albedo, dv):
    film, _ = beauty(sc, low_cam, h, w, n, False)
    return resolve(film, n).repeat_interleave(2, 0).repeat_interleave(2, 1)


def measure(fn, ref, *args):
    ms, img = [], None
    for i in range(RUNS + 1):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        img = fn(*args)
        torch.cuda.synchronize()
        if i > 0: ms.append((time.perf_counter() - t0) * 1e3)
    assert bool(torch.isfinite(img).all())
    return {"rmse": round(float(((img.double() - ref) ** 2).mean().sqrt()), 5), "wall_ms": round(statistics.median(ms), 3), "wall_ms_min": round(min(ms), 3)}


result = {"config": f"{W}x{H} from {w}x{h}, mis zsobol, G-buffers {GUIDE_SPP} spp at both sizes, default parameters, tone-mapped RMSE against {REF_SPP} spp (seed 1000); "
                    f"wall time of all launches of a pipeline, synchronised, median of {RUNS} after one warm-up",
          "library": prod.version(), "scenes": {}}
for scene_id in (3, 19):
    sc = prod.new_scene()
    cam = pkg.scenes.load_scene(sc, scene_id, W, H, build=False)
    d65 = sc.add_lut470(pkg.scenes.presets()["cie_illum_d6500"])
    sc.build(cam)
    low_cam = prod.upsample_low_camera(cam)
    rf, _ = beauty(sc, cam, H, W, REF_SPP, False, seed=1000)
    ref = resolve(rf, REF_SPP).double()
    torch.cuda.synchronize()
    per_scene = {}
    for n in (4, 16, 64):
        e = {}
        for dv in (False, True):
            tag = "_filtered" if dv else ""
            e["full" + tag] = measure(full_frame, ref, sc, cam, low_cam, d65, n, False, dv)
            for albedo in (False, True):
                atag = "_albedo" if albedo else ""
                e["half" + atag + tag] = measure(half_frame, ref, sc, cam, low_cam, d65, n, albedo, dv)
                e["half_equal" + atag + tag] = measure(half_frame, ref, sc, cam, low_cam, d65, 4 * n, albedo, dv)
        e["replicated"] = measure(replicated_frame, ref, sc, cam, low_cam, d65, n, False, False)
        per_scene[str(n)] = e
        print(scene_id, n, json.dumps(e), flush=True)
    result["scenes"][str(scene_id)] = per_scene
    del sc
# the CLI's default for --half-res-albedo follows this: on only if the albedo variant has the lower RMSE on BOTH scenes at every n, unfiltered
wins = {s: all(r[n]["half_albedo"]["rmse"] < r[n]["half"]["rmse"] for n in r) for s, r in result["scenes"].items()}
result["albedo_wins"] = wins
result["albedo_default"] = "on" if all(wins.values()) else "off"
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
json.dump(result, open(OUT, "w"), indent=1)
print(json.dumps({"albedo_wins": wins, "albedo_default": result["albedo_default"]}), flush=True)
