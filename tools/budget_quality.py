#!/usr/bin/env python3
"""What the sample budget (include/mi355pt_budget.h) buys at EQUAL samples, on the two moving-hero setups of profiles/motion_parity.jsonl and
profiles/flow_parity.jsonl (tests/test_motion_gpu.py, tests/test_flow_gpu.py): scene 17 at 64 x 48, 8 frames, (a) the hero translating and
yawing every frame, carried by the per-instance table with the previous ids, (b) the hero under a wave with an advancing phase, carried by
the per-pixel records with the previous ids.  Three runs per setup over the same poses and seeds, each frame a film pair:
  budget    probe, driver (base 4, target 8, max 32), pair normalise, accumulation with spp = 2, length credit;
  uniform   every frame at the smallest even spp whose samples per frame are not below the budget run's for that frame (frame 0 included:
            the budget spends max_spp everywhere on a first frame), the plain accumulation — so uniform never has FEWER samples;
  plain     every frame at 4 spp: the base, and the run whose out_length says where the history is short.
RMSE of the last accumulated frame (a linear mean) against a 256-spp frame of the last pose, over the whole frame and over the pixels where
the plain run's out_length of the last frame is <= 2.  Writes profiles/budget_quality.json (or the path given).  Needs a GPU.
usage: tools/budget_quality.py [OUTPUT.json]"""
import importlib, json, os, sys
import numpy as np
import torch  # first: see tests/conftest.py
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
pkg = importlib.import_module("toy-cpu-pathtracing_amd")
import test_flow_gpu as tf  # noqa: E402
import test_motion_gpu as tm  # noqa: E402
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "budget_quality.json")
W, H, FRAMES, BASE, MAX, TARGET, GUIDE_SPP, REF_SPP = 64, 48, 8, 4, 32, 8.0, 16, 256
F = np.float32
prod = pkg.Product()
GEO = ("position", "shading_normal", "hit")
TY, TX = (H + 7) // 8, (W + 7) // 8
tp = prod.temporal_params_default()
bp = prod.budget_params(BASE, MAX, TARGET)
nbytes = prod.adaptive_scratch_bytes(W, H)
ptrs = lambda d: {k: v.data_ptr() for k, v in d.items()} if d is not None else None   # noqa: E731


class Motion:
    """the hero stepping every frame (tests/test_motion_gpu.py HeroScene): table form"""
    name = "moving hero, per-instance table (profiles/motion_parity.jsonl)"

    def __init__(self):
        self.hs = tm.HeroScene(prod, pkg, W, H)
        self.sc, self.cam, self.d65, self.m_prev, self.m = self.hs.sc, self.hs.cam, self.hs.d65, None, None

    def advance(self, k):
        self.m_prev, self.m = self.m, self.hs.pose(k)

    def carry(self, k, ids):
        if k == 0:
            return None, None
        return torch.from_numpy(prod.motion_table(self.cam, self.cam, self.m, self.m_prev)).cuda(), None


class Flow:
    """the hero under a wave with an advancing phase (tests/test_flow_gpu.py): per-pixel records"""
    name = "waving hero, per-pixel records (profiles/flow_parity.jsonl)"

    def __init__(self):
        self.hs = tf.HeroScene(prod, pkg)
        self.sc, self.cam, self.d65 = self.hs.sc, self.hs.cam, self.hs.d65
        ext = float(np.ptp(self.hs.pos0[:, 0]))
        self.amp, self.lam, self.step = float(F(tf.WAVE[0] * ext)), float(F(tf.WAVE[1] * ext)), tf.WAVE[2]

    def advance(self, k):
        if k > 0:
            prod.scene_flow_mark(self.sc)
        pos = tf.waved(self.hs.pos0, self.amp, self.lam, k * float(F(self.step)))
        assert self.sc.deform_meshes(self.cam, {tf.HERO: (pos, tf.area_normals(pos, self.hs.idx, self.hs.nrm0), None)})["rebuilt"] == 0

    def carry(self, k, ids):
        if k == 0:
            return None, None
        fl = torch.zeros((H, W, 8), dtype=torch.int32, device="cuda")
        prod.render_flow_device(self.sc, self.cam, pkg.make_params(1), fl.data_ptr())
        return None, fl


def run(setup_cls, mode, uniform_spp=None):
    """-> (mean film (H, W, 3) f64, out_length of the last frame before any credit, samples per frame)"""
    s = setup_cls()
    sc, cam = s.sc, s.cam
    view = prod.temporal_view_from_cameras(cam, cam)
    scratch = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    lst = torch.zeros(TY * TX, dtype=torch.int32, device="cuda")
    tile_len = torch.zeros(TY * TX, device="cuda")
    tile_spp = torch.zeros(TY * TX, dtype=torch.int32, device="cuda")
    prev, prev_ids, samples, last_len = None, None, [], None
    for k in range(FRAMES):
        s.advance(k)
        f = {n: torch.zeros((H, W, 3), device="cuda") for n in ("film", "half") + GEO}
        prod.render_gbuffer_accum_device(sc, cam, pkg.make_params(GUIDE_SPP, "mis", "sobol", seed=k), s.d65, 0, GUIDE_SPP, {n: f[n].data_ptr() for n in GEO})
        ids = torch.zeros((H, W), dtype=torch.int32, device="cuda")
        prod.render_ids_device(sc, cam, pkg.make_params(1), ids.data_ptr())
        table, flow = s.carry(k, ids)
        has = prev is not None
        if mode == "budget":
            motion = prod.budget_motion(ids.data_ptr(), prev_ids.data_ptr(), table.data_ptr() if table is not None else None, table.shape[0] if table is not None else 0,
                                        flow.data_ptr() if flow is not None else None) if has else None
            prod.temporal_budget_device(ptrs({n: f[n] for n in GEO}), ptrs(prev), view if has else None, W, H, tp, motion, bp, None, tile_len.data_ptr(), tile_spp.data_ptr())
            res = prod.render_budget_device(sc, cam, pkg.make_params(MAX, "mis", "sobol", seed=k), bp, tile_spp.data_ptr(), f["film"].data_ptr(), f["half"].data_ptr(),
                                            lst.data_ptr(), scratch.data_ptr(), nbytes)
            samples.append(int(res.total_samples))
            prod.film_pair_normalize_tiles_device(f["film"].data_ptr(), f["half"].data_ptr(), tile_spp.data_ptr(), W, H, f["film"].data_ptr(), f["half"].data_ptr())
            spp = 2
        else:
            spp = BASE if mode == "plain" else uniform_spp[k]
            prm = pkg.make_params(spp, "mis", "sobol", seed=k)
            prod.render_accum_device(sc, cam, prm, 0, spp // 2, f["half"].data_ptr())
            torch.cuda.synchronize()
            f["film"].copy_(f["half"])
            prod.render_accum_device(sc, cam, prm, spp // 2, spp, f["film"].data_ptr())
            samples.append(spp * W * H)
        out = [torch.zeros((H, W, 3), device="cuda"), torch.zeros((H, W, 3), device="cuda"), torch.zeros((H, W), device="cuda")]
        o = [t.data_ptr() for t in out]
        if not has:
            prod.temporal_accumulate_device(ptrs(f), spp, None, None, W, H, tp, *o)
        elif table is not None:
            prod.temporal_accumulate_motion_device(ptrs(f), spp, ptrs(prev), view, W, H, tp, ids.data_ptr(), prev_ids.data_ptr(), table.data_ptr(), table.shape[0], *o)
        else:
            prod.temporal_accumulate_flow_device(ptrs(f), spp, ptrs(prev), view, W, H, tp, ids.data_ptr(), prev_ids.data_ptr(), flow.data_ptr(), *o)
        torch.cuda.synchronize()
        last_len = out[2].cpu().numpy()
        if mode == "budget":
            prod.temporal_length_credit_device(out[2].data_ptr(), tile_spp.data_ptr(), BASE, float(tp.max_history), W, H)
        prev = dict({n: f[n] for n in GEO}, film=out[0], half=out[1], length=out[2])
        prev_ids = ids
    torch.cuda.synchronize()
    ref = torch.zeros((H, W, 3), device="cuda")
    prod.render_accum_device(sc, cam, pkg.make_params(REF_SPP, "mis", "sobol", seed=1000), 0, REF_SPP, ref.data_ptr())
    torch.cuda.synchronize()
    return prev["film"].cpu().numpy().astype(np.float64) / 2.0, last_len, samples, ref.cpu().numpy().astype(np.float64) / REF_SPP, prev_ids.cpu().numpy().view(np.uint32)


result = {"config": f"scene17 {W}x{H}, {FRAMES} frames, mis zsobol, frame k with seed k, G-buffers {GUIDE_SPP} spp, default temporal parameters, previous ids as a tap test; "
                    f"budget base {BASE} target {TARGET} max {MAX}; reference {REF_SPP} spp of the last pose (seed 1000); RMSE of the last accumulated frame's linear mean",
          "library": prod.version(), "setups": {}}
for key, cls in (("motion", Motion), ("flow", Flow)):
    film_b, _, samples_b, ref, ids = run(cls, "budget")
    uniform_spp = [max(2, 2 * -(-n // (2 * W * H))) for n in samples_b]          # the smallest even spp with spp W H >= n
    film_u, _, samples_u, ref_u, _ = run(cls, "uniform", uniform_spp)
    film_p, len_p, samples_p, ref_p, _ = run(cls, "plain")
    assert np.array_equal(ref, ref_u) and np.array_equal(ref, ref_p)                # the three runs end in the same pose
    short = len_p <= 2.0
    rmse = lambda a, m=None: float(np.sqrt(np.mean(((a - ref)[m] if m is not None else (a - ref)) ** 2)))   # noqa: E731
    result["setups"][key] = {
        "setup": cls.name, "hero_pixels": int((ids == 1).sum()), "pixels_with_plain_out_length_le_2": int(short.sum()),
        "budget": {"samples_per_frame": samples_b, "total_samples": int(sum(samples_b)), "rmse": rmse(film_b), "rmse_short_history": rmse(film_b, short) if short.any() else None},
        "uniform": {"spp_per_frame": uniform_spp, "samples_per_frame": samples_u, "total_samples": int(sum(samples_u)), "rmse": rmse(film_u),
                    "rmse_short_history": rmse(film_u, short) if short.any() else None},
        "plain_base": {"samples_per_frame": samples_p, "total_samples": int(sum(samples_p)), "rmse": rmse(film_p), "rmse_short_history": rmse(film_p, short) if short.any() else None},
    }
    r = result["setups"][key]
    r["budget_over_uniform_rmse"] = round(r["budget"]["rmse"] / r["uniform"]["rmse"], 4)
    if short.any():
        r["budget_over_uniform_rmse_short_history"] = round(r["budget"]["rmse_short_history"] / r["uniform"]["rmse_short_history"], 4)
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
json.dump(result, open(OUT, "w"), indent=1)
print(json.dumps(result), flush=True)
