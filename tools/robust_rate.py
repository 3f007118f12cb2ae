#!/usr/bin/env python3
"""Time of the robust film (include/mi355pt_robust.h, csrc/pt_kernels_robust.hip) on one GPU, in one process.

1. The combination on a 1920x1080 frame for K = 8 / 16 / 32 buckets, single and pair output, beside two device-to-device copies: of the K films' bytes (as many bytes READ as the combination reads; the copy also writes them) and of half the
   bytes the combination moves (read + write: the same TOTAL traffic).  The stack is tests/robust_reference.py's generator at 240 x 135,
   tiled 8 x 8.  After WARMUP calls of each, RUNS calls of each, ALTERNATING, HIP events around each call; before every timed call a 512 MB
   buffer is overwritten, so that no call finds its input in the 256 MB last-level cache because the call before it read the same films.
   The K = 8 / single / GMON output of the timed calls is compared with the restatement on one tile.
2. What bucketing costs the renderer: a 64-spp frame of scene 3 (MIS + ZSobol, 1920x1080) as 16 buckets (mi355pt_render_buckets_device,
   its clearing of the 16 films included) against the same frame in ONE launch (mi355pt_render_accum_device over [0, 64) into a film
   cleared inside the timed window), interleaved, HIP events around each.

Writes one JSON object to profiles/robust_rate.json (or the path given).  Needs a GPU; reads nothing outside the repository.
usage: tools/robust_rate.py [RUNS (default 20, at least 10)] [OUTPUT.json]"""
import importlib, json, os, statistics, sys
import numpy as np
import torch  # first: see tests/conftest.py
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import robust_reference as rr  # noqa: E402
pkg = importlib.import_module("toy-cpu-pathtracing_amd")
W, H, WARMUP, SPP_BUCKET = 1920, 1080, 3, 4
RUNS = max(10, int(sys.argv[1])) if len(sys.argv) > 1 else 20
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "robust_rate.json")
prod = pkg.Product()
PIX = W * H
FILM = PIX * 12


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "spread": round((max(ms) - min(ms)) / statistics.median(ms), 4), "runs": len(ms)}


def timed(fn, before=None):
    if before:
        before()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(); fn(); e1.record(); e1.synchronize()
    return e0.elapsed_time(e1)


# ---- 1. the combination ----
tile = rr.make_stack(32, 135, 240, seed=2024, spp_bucket=SPP_BUCKET)
stack = torch.from_numpy(np.tile(tile, (1, 8, 8, 1))).cuda()
assert stack.shape == (32, H, W, 3)
out = torch.full((H, W, 3), float("nan"), device="cuda")
half = torch.full((H, W, 3), float("nan"), device="cuda")
trim = torch.zeros((H, W, 2), dtype=torch.uint8, device="cuda")
copy_src = stack.view(-1)
copy_dst = torch.empty_like(copy_src)
flush = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")
rp = prod.robust_params_default()


def evict():
    flush.fill_(1)


def combine(k, pair):
    return lambda: prod.robust_combine_device(stack.data_ptr(), k, SPP_BUCKET, W, H, rp, out.data_ptr(), half.data_ptr() if pair else None, trim.data_ptr())


def copy_floats(n):
    return lambda: copy_dst[:n].copy_(copy_src[:n])


variants = {}
for k in (8, 16, 32):
    read, write = k * FILM, FILM + 2 * PIX
    variants[f"K{k}_single"] = dict(fn=combine(k, False), read_bytes=read, write_bytes=write, k=k)
    variants[f"K{k}_pair"] = dict(fn=combine(k, True), read_bytes=read, write_bytes=write + FILM, k=k)
    variants[f"copy_of_K{k}_films"] = dict(fn=copy_floats(k * PIX * 3), read_bytes=read, write_bytes=read, k=k)
    variants[f"copy_same_traffic_K{k}"] = dict(fn=copy_floats((read + write) // 8), read_bytes=(read + write) // 8 * 4, write_bytes=(read + write) // 8 * 4, k=k)
ms = {n: [] for n in variants}
for i in range(WARMUP + RUNS):
    for name, v in variants.items():
        t = timed(v["fn"], evict)
        if i >= WARMUP:
            ms[name].append(t)
# what was timed is what the restatement gives (one tile of the K = 8 single output; the last call of the loop was another variant)
combine(8, False)()
torch.cuda.synchronize()
want = rr.combine(tile[:8], SPP_BUCKET, rr.GMON, 1.0, False)
assert np.array_equal(rr.bits(out[:135, :240].cpu().numpy()), rr.bits(want[0])) and np.array_equal(trim[:135, :240].cpu().numpy(), want[2])
result = {"config": f"{W}x{H}, buckets of {SPP_BUCKET} spp, GMON scale 1, trims written; {RUNS} timed calls of each, alternating, after {WARMUP} warm-up calls of each, "
                    f"HIP events around each call, a 512 MB buffer overwritten before each",
          "library": prod.version(), "film_bytes": FILM, "combine": {}}
med = {}
for name, v in variants.items():
    r = spread(ms[name])
    med[name] = r["median_ms"]
    r["read_bytes"], r["write_bytes"] = v["read_bytes"], v["write_bytes"]
    r["GB_s_read_plus_write"] = round((v["read_bytes"] + v["write_bytes"]) / (r["median_ms"] * 1e-3) / 1e9, 1)
    result["combine"][name] = r
for name, v in variants.items():
    if name.startswith("K"):
        k = v["k"]
        result["combine"][name]["over_copy_of_films"] = round(med[name] / med[f"copy_of_K{k}_films"], 4)
        result["combine"][name]["over_copy_same_traffic"] = round(med[name] / med[f"copy_same_traffic_K{k}"], 4)
# (a second shape of the N = 32 kernel, which read the buckets twice instead of holding 96 values, was measured by an earlier form of this tool
# in the same interleaved way and then removed from the library: DESIGN 4.15 has both times)
del stack, copy_src, copy_dst, flush
torch.cuda.empty_cache()

# ---- 2. what bucketing costs the renderer ----
SPP, K = 64, 16
sc = prod.new_scene()
cam = pkg.scenes.load_scene(sc, 3, W, H)
prm = pkg.make_params(SPP, "mis", "sobol", seed=0)
buckets = torch.empty((K, H, W, 3), device="cuda")
film = torch.empty((H, W, 3), device="cuda")


def one_launch():
    film.zero_()
    prod.render_accum_device(sc, cam, prm, 0, SPP, film.data_ptr())


def as_buckets():
    prod.render_buckets_device(sc, cam, prm, K, buckets.data_ptr())


rms = {"one_launch": [], "buckets": []}
R2 = max(5, RUNS // 2)
for i in range(2 + R2):
    for name, fn in (("one_launch", one_launch), ("buckets", as_buckets)):
        t = timed(fn)
        if i >= 2:
            rms[name].append(t)
torch.cuda.synchronize()
total = buckets.sum(0)
rel = float(((total - film).abs().sum() / film.abs().sum()).item())
combine_ms = timed(lambda: prod.robust_combine_device(buckets.data_ptr(), K, SPP // K, W, H, rp, out.data_ptr(), None, trim.data_ptr()))
result["render"] = {"config": f"scene 3, mis + ZSobol, {W}x{H}, {SPP} spp; {R2} timed calls of each, interleaved, after 2 warm-up calls of each, HIP events around each call",
                    "one_launch": spread(rms["one_launch"]), f"buckets_{K}": spread(rms["buckets"]),
                    "buckets_over_one_launch": round(statistics.median(rms["buckets"]) / statistics.median(rms["one_launch"]), 4),
                    "sum_of_buckets_vs_one_launch_relative_l1": rel, "combine_after_it_ms": round(combine_ms, 4),
                    "share_of_pixels_trimmed": round(float((trim[..., 0] != 0).float().mean().item()), 4)}
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
json.dump(result, open(OUT, "w"), indent=1)
print(json.dumps(result), flush=True)
assert rel < 1e-5, rel                                                       # the same samples: the sums differ by rounding only
