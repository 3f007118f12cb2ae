"""GPU tests of the sample budget by reprojected history (include/mi355pt_budget.h, csrc/pt_kernels_budget.hip): the probe against the
NumPy restatement of tests/budget_reference.py — BIT EQUALITY on P, tile_len and tile_spp — and against the out_length of the shipped
accumulation calls on the same inputs; the driver against a replay from the public calls; the pair normalise and the length credit against
the restatement; and three frames of a moving hero through the Python plumbing.  The outputs start as NaN or 0xff, so a value the kernels
leave out shows."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import budget_reference as br  # noqa: E402
import flow_reference as fr  # noqa: E402
import motion_reference as mr  # noqa: E402
import temporal_reference as tr  # noqa: E402
from test_flow_gpu import FlowDevice  # noqa: E402
from test_motion_gpu import GUIDE_SPP, HERO, HeroScene, MotionDevice  # noqa: E402
from test_temporal_rectify_gpu import bits, ffi_params, ffi_view  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
PROBE_SIZES = [(8, 8), (9, 9), (71, 13)]        # one full tile; one full and three ragged tiles; ragged in both axes, a block's last wave partly outside
G_FILMS = ("position", "shading_normal", "hit")
BUDGET = br.budget(4, 32, 8.0)
MIN_WEIGHT = 0.1                                  # between the footprint's weights 0.0625 and 0.1875 (a shift of a quarter pixel)


class BudgetDevice(FlowDevice, MotionDevice):
    """the Devices of the motion and flow tests plus the four calls of mi355pt_budget.h"""

    def probe(self, cur, prev, view, b, prm=None, ids_cur=None, ids_prev=None, table=None, flow=None, want_pred=True):
        """cur / prev: dicts of device tensors; ids, table, flow: device tensors -> (P or None, tile_len, tile_spp) on the host"""
        torch = self.torch
        H, W = cur["hit"].shape[:2]
        ty, tx = br.tiles_of(W, H)
        pred = torch.full((H, W), float("nan"), dtype=torch.float32, device="cuda") if want_pred else None
        tl = torch.full((ty, tx), float("nan"), dtype=torch.float32, device="cuda")
        ts = torch.full((ty, tx), -1, dtype=torch.int32, device="cuda")
        ptr = lambda d: {k: v.data_ptr() for k, v in d.items()} if d is not None else None   # noqa: E731
        dp = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
        motion = None
        if table is not None or flow is not None:
            motion = self.product.budget_motion(dp(ids_cur), dp(ids_prev), dp(table), table.shape[0] if table is not None else 0, dp(flow))
        self.product.temporal_budget_device(ptr(cur), ptr(prev), ffi_view(self.pkg, view), W, H, ffi_params(self.product, prm), motion,
                                            self.product.budget_params(b.base_spp, b.max_spp, float(b.target_history)), dp(pred), tl.data_ptr(), ts.data_ptr())
        torch.cuda.synchronize()
        return (pred.cpu().numpy() if want_pred else None), tl.cpu().numpy(), ts.cpu().numpy().view(np.uint32)

    def u32_up(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()

    def f32_up(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a, dtype=F)).cuda()


@pytest.fixture(scope="module")
def dev(product, pkg):
    return BudgetDevice(product, pkg)


# ---------------- 1. the probe ----------------
MODS = ("plane", "normal", "nohit", "nolength")


def probe_frames(W, H, without=None, seed=3):
    """Hand-made G-buffers on tests/temporal_reference.py's exact pixel grid (pixel (i, j) lands on (i + 0.25, j + 0.25): every tap weight
    is one of 0.5625, 0.1875, 0.1875, 0.0625, and the right and bottom edges gather taps outside the frame).  Current frame: (0, 0) has no
    hit, (1, 0) lies behind the previous camera, (2, 0) projects outside in x, (3, 0) outside in y.  Previous frame: (4, 4) lies off the
    current surface's plane, (5, 5) has another normal, (2, 5) has no hit, (6, 2) and three taps of pixel (1, 3)'s footprint have length 0
    (pixel (1, 3) keeps the tap of weight 0.0625 alone: Wt <= min_weight).  `without`: one of MODS left out of the previous frame.
    -> (cur, prev, view, params) with random positive films so that the accumulation calls take the same frames"""
    rng = np.random.default_rng([seed, W, H])
    cur, prev = tr.grid_frame(W, H), tr.grid_frame(W, H)
    view = tr.grid_view(W, H, 0.25, 0.25)
    for k in G_FILMS:
        cur[k][0, 0] = 0.0                                                   # h == 0
    cur["position"][0, 1, 2] = 1.0                                           # zc = -1
    cur["position"][0, 2, 0] = 1000.0                                        # gx >= W
    cur["position"][0, 3, 1] = 1000.0                                        # gy < -1
    # three samples through the same point: the sums are 3 x, the quotients exact
    cur = {k: (v * F(3)).astype(F) for k, v in cur.items()}
    length = rng.integers(1, 41, size=(H, W)).astype(F)
    if without != "plane":
        prev["position"][4, 4, 2] = -1.5
    if without != "normal":
        prev["shading_normal"][5, 5] = (1.0, 0.5, 0.5)
    if without != "nohit":
        for k in G_FILMS:
            prev[k][5, 2] = 0.0
    if without != "nolength":
        length[2, 6] = 0.0
    length[3, 1] = length[3, 2] = length[4, 1] = 0.0                         # pixel (1, 3): x0 = 1, y0 = 3; only the tap (2, 4) stays
    prev["length"] = length
    for f in (cur, prev):
        f["half"] = tr.hdr(rng, (H, W, 3))
        f["film"] = f["half"] + tr.hdr(rng, (H, W, 3))
    return cur, prev, view, tr.params(min_weight=MIN_WEIGHT)


def probe_carries(W, H, view):
    """the carries of a frame: name -> dict(ids_cur, ids_prev, table, flow) of host arrays"""
    ids_cur, ids_prev = mr.synthetic_ids(W, H)
    table = mr.static_table(view, 3)
    table[1] = mr.moved_entry(view, shift=(0.5, -0.25, 0.0), yaw=0.01)
    flow = fr.zero_records(W, H)
    flow["d"] = np.asarray(view.delta, F)
    flow["d"][:, W // 2:] += np.array([0.5, 0.0, 0.0], F)
    flow["dn"][:, W // 2:] = np.array([0.0, 0.01, 0.0], F)
    flow["id"] = ids_cur + 1
    return {"static": {}, "table": dict(ids_cur=ids_cur, table=table), "table_ids": dict(ids_cur=ids_cur, ids_prev=ids_prev, table=table),
            "flow": dict(flow=flow), "flow_ids": dict(ids_cur=ids_cur, ids_prev=ids_prev, flow=flow)}


def test_probe_frames_hold_every_case():
    """at 9 x 9 the hand-made frames make all of these occur: the four "no history" cases, taps out of the frame, taps failing the plane,
    the normal and the id test (and a tap without a hit, a tap without a length), a pixel with Wt <= min_weight"""
    W, H = 9, 9
    cur, prev, view, prm = probe_frames(W, H)
    info = tr.accumulate(cur, 2, prev, view, prm, detail=True)[3]
    with np.errstate(all="ignore"):
        X = cur["position"] / cur["hit"][..., 1:2]
        fx, fy, zc = tr.project(view, X, F)
    gx, gy = fx - F(0.5), fy - F(0.5)
    ok = info["ok"]
    assert cur["hit"][0, 0, 1] == 0 and not ok[0, 0]
    assert cur["hit"][0, 1, 1] > 0 and not zc[0, 1] > 0 and not ok[0, 1]
    assert zc[0, 2] > 0 and gx[0, 2] >= W and -1 <= gy[0, 2] < H and not ok[0, 2]
    assert zc[0, 3] > 0 and -1 <= gx[0, 3] < W and gy[0, 3] < -1 and not ok[0, 3]
    assert ok.sum() == W * H - 4
    assert (ok & (info["x0"] + 1 > W - 1)).any() and (ok & (info["y0"] + 1 > H - 1)).any()                 # taps out of the frame
    for mod in MODS:                                        # leaving the modification out makes a tap valid that is invalid with it
        _, prev2, _, _ = probe_frames(W, H, without=mod)
        info2 = tr.accumulate(cur, 2, prev2, view, prm, detail=True)[3]
        assert any((b & ~a).any() for a, b in zip(info["valid"], info2["valid"])), mod
    c = probe_carries(W, H, view)["table_ids"]
    with_ids = mr.accumulate_motion(cur, 2, prev, view, c["ids_cur"], c["ids_prev"], mr.static_table(view, 3), prm, detail=True)[3]
    assert any((a & ~b).any() for a, b in zip(info["valid"], with_ids["valid"]))                          # the id test fails a tap
    Wt = info["Wt"]
    assert ok[3, 1] and 0 < Wt[3, 1] <= prm.min_weight and not info["has"][3, 1] and Wt[3, 1] == F(0.0625)
    assert info["has"].sum() > 40


@pytest.mark.parametrize("carry", ["first", "static", "table", "table_ids", "flow", "flow_ids"])
@pytest.mark.parametrize("shape", PROBE_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_probe_bit_equal(dev, product, pkg, shape, carry):
    """P, tile_len and tile_spp bit-equal to the restatement, without a previous frame, static, table form and flow form with and without
    previous ids; out_length of the matching shipped accumulation call on the same inputs equals where(P > 0, min(P + 1, max_history), 1)
    bit for bit; without d_pred_length the tile outputs are the same; the host-buffer form equals the device form."""
    W, H = shape
    cur, prev, view, prm = probe_frames(W, H)
    kw = probe_carries(W, H, view)[carry] if carry != "first" else {}
    if carry == "first":
        prev, view = None, None
    want = br.probe(cur, prev, view, BUDGET, prm, **kw)
    dc, dp = dev.up(cur), dev.up(prev)
    dkw = {k: (dev.ids_up(v) if k.startswith("ids") else dev.table_up(v) if k == "table" else dev.flow_up(v)) for k, v in kw.items()}
    got = dev.probe(dc, dp, view, BUDGET, prm, **dkw)
    for name, g, w in zip(("P", "tile_len", "tile_spp"), got, want):
        assert g.shape == w.shape and np.array_equal(bits(g), bits(w)), (name, int((bits(g) != bits(w)).sum()), g, w)
    lean = dev.probe(dc, dp, view, BUDGET, prm, want_pred=False, **dkw)
    assert lean[0] is None and np.array_equal(bits(lean[1]), bits(want[1])) and np.array_equal(lean[2], want[2])
    host = product.temporal_budget(cur, prev, ffi_view(pkg, view), product.budget_params(BUDGET.base_spp, BUDGET.max_spp, float(BUDGET.target_history)),
                                   ffi_params(product, prm), **kw)
    for g, w in zip(host, want):
        assert np.array_equal(bits(g), bits(w))
    # the shipped accumulation on the same device buffers
    if carry in ("first", "static"):
        ol = dev.run_device(dc, 2, dp, view, prm, rectified=False)[2]
    elif carry.startswith("table"):
        ol = dev.run_motion_device(dc, 2, dp, view, dkw["ids_cur"], dkw.get("ids_prev"), dkw["table"], prm)[2]
    else:
        ol = dev.run_flow_device(dc, 2, dp, view, dkw.get("ids_cur"), dkw.get("ids_prev"), dkw["flow"], prm)[2]
    assert np.array_equal(bits(ol.cpu().numpy()), bits(br.expected_out_length(got[0], prm.max_history)))
    if carry == "first":
        assert not got[0].any() and not got[1].any() and (got[2] == 32).all()
    elif (W, H) == (9, 9):
        # (the four pixels without a history whatever the carry; pixel (1, 3) is carried elsewhere by the table's moved record)
        assert (got[0] > 0).sum() > 30 and (got[0][0, :4] == 0).all() and len(np.unique(got[2])) >= 2


@pytest.mark.parametrize("shape", PROBE_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_probe_static_carries_equal_the_static_probe(dev, shape):
    """with a table of static records and with records that hold the view's delta alone (zero flow beyond the camera's share; the flow form
    does not read view->delta), P is bit-equal to the static probe; so is the flow form at zero records against the static probe at delta = 0"""
    W, H = shape
    cur, prev, view, prm = probe_frames(W, H)
    dc, dp = dev.up(cur), dev.up(prev)
    ids_cur, _ = mr.synthetic_ids(W, H)
    base = dev.probe(dc, dp, view, BUDGET, prm)
    carried = fr.zero_records(W, H); carried["d"] = np.asarray(view.delta, F)
    for got in (dev.probe(dc, dp, view, BUDGET, prm, ids_cur=dev.ids_up(ids_cur), table=dev.table_up(mr.static_table(view, 3))),
                dev.probe(dc, dp, view, BUDGET, prm, flow=dev.flow_up(carried))):
        for a, b in zip(got, base):
            assert np.array_equal(bits(a), bits(b))
    v0 = fr.zero_delta(view)
    for a, b in zip(dev.probe(dc, dp, view, BUDGET, prm, flow=dev.flow_up(fr.zero_records(W, H))), dev.probe(dc, dp, v0, BUDGET, prm)):
        assert np.array_equal(bits(a), bits(b))


def test_probe_on_the_seeded_synthetic_frames(dev):
    """the seeded frames of the existing temporal tests (a camera move, the two-plane step, sample counts that differ per pixel) at a ragged
    size and the default parameters: bit-equal to the restatement, and a non-power-of-two target"""
    W, H = 70, 50
    b = br.budget(2, 64, 11.0)
    for view_name in ("move", "outside", "behind"):
        cur, prev, vw, _ = tr.synthetic(W, H, view_name, "step", True)
        want = br.probe(cur, prev, vw, b)
        got = dev.probe(dev.up(cur), dev.up(prev), vw, b)
        for g, w in zip(got, want):
            assert np.array_equal(bits(g), bits(w)), view_name
    assert len(np.unique(got[2])) >= 2


# ---------------- 2. the driver ----------------
TARGETS = {"mixed": [4, 8, 16, 4, 32, 8], "base": [4] * 6, "max": [32] * 6, "clamped": [0, 8, 1000, 4, 33, 2]}


@pytest.fixture(scope="module")
def scene3(product, pkg):
    cache = {}

    def get(W, H):
        if (W, H) not in cache:
            sc = product.new_scene()
            cam = pkg.scenes.load_scene(sc, 3, W, H, tex_size=16)
            cache[(W, H)] = (sc, cam)
        return cache[(W, H)]
    return get


def run_driver(dev, product, sc, cam, prm, b, tile_spp):
    torch = dev.torch
    W, H = cam.width, cam.height
    n_tiles = tile_spp.size
    film = torch.full((H, W, 3), float("nan"), dtype=torch.float32, device="cuda")
    half = torch.full((H, W, 3), float("nan"), dtype=torch.float32, device="cuda")
    lst = torch.full((n_tiles,), -1, dtype=torch.int32, device="cuda")
    nbytes = product.adaptive_scratch_bytes(W, H)
    scratch = torch.full((nbytes,), 0x5a, dtype=torch.uint8, device="cuda")
    d_spp = dev.u32_up(tile_spp)
    res = product.render_budget_device(sc, cam, prm, product.budget_params(b.base_spp, b.max_spp, float(b.target_history)), d_spp.data_ptr(), film.data_ptr(),
                                       half.data_ptr(), lst.data_ptr(), scratch.data_ptr(), nbytes)
    torch.cuda.synchronize()
    assert np.array_equal(d_spp.cpu().numpy().view(np.uint32), tile_spp)                    # tile_spp is an input
    return film.cpu().numpy(), half.cpu().numpy(), res


def replay(dev, product, sc, cam, prm, b, tile_spp):
    """the header's sequence from the public calls: mi355pt_render_accum_device, mi355pt_render_accum_tiles_device with the host list, NumPy
    copies for H := F"""
    torch = dev.torch
    W, H = cam.width, cam.height
    f = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    h = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    product.render_accum_device(sc, cam, prm, 0, b.base_spp // 2, h.data_ptr())
    torch.cuda.synchronize()
    f.copy_(h)
    product.render_accum_device(sc, cam, prm, b.base_spp // 2, b.base_spp, f.data_ptr())
    torch.cuda.synchronize()
    passes = 0
    for level, tiles in br.driver_levels(tile_spp, b):
        passes += 1
        if tiles.size == 0:
            break
        fh, hh = f.cpu().numpy(), h.cpu().numpy()
        listed = br.per_pixel(np.isin(np.arange(tile_spp.size), tiles).reshape(br.tiles_of(W, H)), W, H)
        hh[listed] = fh[listed]
        h = dev.f32_up(hh)
        product.render_accum_tiles_device(sc, cam, prm, tiles, level, 2 * level, f.data_ptr())
        torch.cuda.synchronize()
    return f.cpu().numpy(), h.cpu().numpy(), passes


@pytest.mark.parametrize("targets", list(TARGETS))
@pytest.mark.parametrize("shape", [(24, 16), (20, 12)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_driver_equals_the_replay(dev, product, pkg, scene3, shape, targets):
    """scene 3 at 24 x 16 (6 full tiles) and 20 x 12 (ragged), hand-set per-tile counts, all-base, all-max and counts outside the range
    (clamped on the device): F and H bit-equal to the replay from the public calls; all-base bit-equal to the plain two-range render; the
    result's figures are those of the clamped counts"""
    W, H = shape
    sc, cam = scene3(W, H)
    b = BUDGET
    prm = pkg.make_params(b.max_spp, "mis", "sobol", seed=5)
    tile_spp = np.array(TARGETS[targets], np.uint32)
    film, half, res = run_driver(dev, product, sc, cam, prm, b, tile_spp)
    want_f, want_h, passes = replay(dev, product, sc, cam, prm, b, tile_spp)
    assert not np.isnan(film).any() and not np.isnan(half).any()
    assert np.array_equal(bits(film), bits(want_f)), int((bits(film) != bits(want_f)).sum())
    assert np.array_equal(bits(half), bits(want_h)), int((bits(half) != bits(want_h)).sum())
    counts = br.rendered_count(tile_spp, b).reshape(br.tiles_of(W, H))
    tw = np.minimum(8, W - 8 * np.arange(counts.shape[1]))[None, :]
    th = np.minimum(8, H - 8 * np.arange(counts.shape[0]))[:, None]
    assert res.passes == passes and res.tiles_at_max == int((counts == b.max_spp).sum()) and res.total_samples == int((counts.astype(np.int64) * tw * th).sum())
    if targets == "base":
        torch = dev.torch
        plain = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
        first = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
        product.render_accum_device(sc, cam, prm, 0, 2, first.data_ptr())
        torch.cuda.synchronize()
        plain.copy_(first)
        product.render_accum_device(sc, cam, prm, 2, 4, plain.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(bits(film), bits(plain.cpu().numpy())) and np.array_equal(bits(half), bits(first.cpu().numpy())) and res.passes == 1
    if targets == "mixed":
        assert film.mean() > 0 and res.passes == 3 and res.tiles_at_max == 1


def test_driver_refusals_on_a_built_scene(dev, product, pkg, scene3):
    """what the driver refuses after the scene's own checks: the budget params, spp != max_spp, a null buffer, film == half, the scratch"""
    torch = dev.torch
    sc, cam = scene3(24, 16)
    lib, f = product.lib, pkg.ffi
    import ctypes
    ref = ctypes.byref
    film = torch.zeros((16, 24, 3), dtype=torch.float32, device="cuda")
    half = torch.zeros_like(film)
    spp = dev.u32_up(np.full(6, 4, np.uint32))
    lst = torch.zeros(6, dtype=torch.int32, device="cuda")
    nbytes = product.adaptive_scratch_bytes(24, 16)
    scratch = torch.zeros(nbytes + 4, dtype=torch.uint8, device="cuda")
    good = dict(p=pkg.make_params(32), bp=f.BudgetParams(4, 32, 8.0), spp=spp.data_ptr(), film=film.data_ptr(), half=half.data_ptr(), lst=lst.data_ptr(),
                sp=scratch.data_ptr(), nbytes=nbytes)

    def refused(text, **kw):
        a = dict(good); a.update(kw)
        rc = lib.mi355pt_render_budget_device(sc.h, ref(cam), ref(a["p"]), ref(a["bp"]) if a["bp"] is not None else None, a["spp"], a["film"], a["half"], a["lst"],
                                              a["sp"], a["nbytes"], None, None)
        assert rc == -1 and text in lib.mi355pt_last_error(), (text, lib.mi355pt_last_error())
    refused(b"null budget_params", bp=None)
    refused(b"base_spp must be a power of two >= 2", bp=f.BudgetParams())
    refused(b"max_spp must be a power of two >= base_spp", bp=f.BudgetParams(4, 24, 8.0))
    refused(b"target_history must be finite and >= 1", bp=f.BudgetParams(4, 32, 0.0))
    refused(b"spp must equal max_spp", p=pkg.make_params(16))
    for k in ("spp", "film", "half", "lst"):
        refused(b"budget: null buffer", **{k: None})
    refused(b"the same buffer", half=film.data_ptr())
    refused(b"scratch missing or smaller", sp=None)
    refused(b"scratch missing or smaller", nbytes=nbytes - 1)
    refused(b"not 4-byte aligned", sp=scratch.data_ptr() + 1)
    shards = pkg.make_params(32); shards.shard_count = 2
    refused(b"shard_count must be 0 or 1", p=shards)
    stats = pkg.make_params(32); stats.collect_stats = 1
    refused(b"collect_stats must be 0", p=stats)
    torch.cuda.synchronize()
    assert not film.any() and not half.any()


# ---------------- 3. the pair normalise and the length credit ----------------
@pytest.mark.parametrize("shape", [(9, 9), (71, 13)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_pair_normalize_and_length_credit(dev, product, shape):
    """bit-equal to the restatement, out of place, in place and through the host form; the credit leaves tiles at base_spp untouched byte
    for byte (NaN payloads included) and caps at max_history"""
    torch = dev.torch
    W, H = shape
    rng = np.random.default_rng([9, W, H])
    ty, tx = br.tiles_of(W, H)
    tile_spp = (4 << rng.integers(0, 4, size=(ty, tx))).astype(np.uint32)
    tile_spp[0, 0], tile_spp[-1, -1] = 4, 32
    film, half = tr.hdr(rng, (H, W, 3)) * F(7), tr.hdr(rng, (H, W, 3)) * F(3)
    film[0, 0], half[H - 1, W - 1] = (np.nan, np.inf, -1.0), (0.0, -0.0, 1e-40)
    want_f, want_h = br.pair_normalize(film, half, tile_spp)
    d_spp, df, dh = dev.u32_up(tile_spp), dev.f32_up(film), dev.f32_up(half)
    of, oh = torch.full((H, W, 3), float("nan"), dtype=torch.float32, device="cuda"), torch.full((H, W, 3), float("nan"), dtype=torch.float32, device="cuda")
    product.film_pair_normalize_tiles_device(df.data_ptr(), dh.data_ptr(), d_spp.data_ptr(), W, H, of.data_ptr(), oh.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(bits(of.cpu().numpy()), bits(want_f)) and np.array_equal(bits(oh.cpu().numpy()), bits(want_h))
    assert np.array_equal(bits(df.cpu().numpy()), bits(film)) and np.array_equal(bits(dh.cpu().numpy()), bits(half))      # the inputs are left alone
    product.film_pair_normalize_tiles_device(df.data_ptr(), dh.data_ptr(), d_spp.data_ptr(), W, H, df.data_ptr(), dh.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(bits(df.cpu().numpy()), bits(want_f)) and np.array_equal(bits(dh.cpu().numpy()), bits(want_h))
    hf, hh = product.film_pair_normalize_tiles(film, half, tile_spp)
    assert np.array_equal(bits(hf), bits(want_f)) and np.array_equal(bits(hh), bits(want_h))

    length = rng.integers(1, 33, size=(H, W)).astype(F)
    at_base = br.per_pixel(tile_spp, W, H) == 4
    length.view(np.uint32)[at_base & (rng.random((H, W)) < 0.3)] = 0x7fc12345               # a NaN with a payload: a rewrite would be seen
    length[~at_base & (rng.random((H, W)) < 0.1)] = 31.5
    want = br.length_credit(length, tile_spp, 4, 32.0)
    dl = dev.f32_up(length)
    product.temporal_length_credit_device(dl.data_ptr(), d_spp.data_ptr(), 4, 32.0, W, H)
    torch.cuda.synchronize()
    got = dl.cpu().numpy()
    assert np.array_equal(bits(got), bits(want))
    assert np.array_equal(bits(got)[at_base], bits(length)[at_base]) and (got[~at_base] <= 32).all() and (got[~at_base] > length[~at_base] - 1e-6).all()
    assert (got[~at_base] == 32).any() and (bits(got)[~at_base] != bits(length)[~at_base]).any()


# ---------------- 4. end to end: three frames of a moving hero through the Python plumbing ----------------
def host_view(v):
    return SimpleNamespace(delta=np.array(list(v.delta), F), rows=np.array(list(v.rows), F), sx=F(v.sx), sy=F(v.sy), cx=F(v.cx), cy=F(v.cy))


def test_three_frames_of_a_moving_hero(dev, product, pkg):
    """Scene 17 at 64 x 48, the hero stepping every frame (the CLI's --instance-step move): per frame G-buffer, ids, probe, driver, pair
    normalise, the unchanged mi355pt_temporal_accumulate_motion_device with spp = 2, length credit.  The probe's outputs, the accumulated
    pair and the credited length are bit-equal to the restatement chain (which carries its own previous outputs); the first frame is at
    min(max_spp, base 2^ceil(log2 target)) everywhere; a tile whose every pixel has P + 1 >= target is at base_spp."""
    torch = dev.torch
    W, H = 64, 48
    b = BUDGET
    hs = HeroScene(product, pkg, W, H)
    cam = hs.cam
    view = product.temporal_view_from_cameras(cam, cam)
    hview = host_view(view)
    tp = product.temporal_params_default()
    hprm = tr.params()
    bp = product.budget_params(b.base_spp, b.max_spp, float(b.target_history))
    nbytes = product.adaptive_scratch_bytes(W, H)
    scratch = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    ty, tx = br.tiles_of(W, H)
    lst = torch.zeros(ty * tx, dtype=torch.int32, device="cuda")
    d_prev, h_prev, d_ids_prev, h_ids_prev, m_prev = None, None, None, None, None
    boosted_later = 0
    for k in range(3):
        m = hs.pose(k)
        g = {n: torch.zeros((H, W, 3), dtype=torch.float32, device="cuda") for n in G_FILMS}
        product.render_gbuffer_accum_device(hs.sc, cam, pkg.make_params(GUIDE_SPP, "mis", "sobol", seed=k), hs.d65, 0, GUIDE_SPP, {n: g[n].data_ptr() for n in G_FILMS})
        h_ids, d_ids = dev.render_ids(hs.sc, cam, pkg.make_params(1))
        hg = {n: g[n].cpu().numpy() for n in G_FILMS}
        table = product.motion_table(cam, cam, m, m_prev) if k else None
        d_table = dev.table_up(table) if k else None
        # probe
        kw = dict(ids_cur=d_ids, ids_prev=d_ids_prev, table=d_table) if k else {}
        P, tile_len, tile_spp = dev.probe(g, d_prev, view if k else None, b, None, **kw)
        hkw = dict(ids_cur=h_ids, ids_prev=h_ids_prev, table=table) if k else {}
        wP, wlen, wspp = br.probe(hg, h_prev, hview if k else None, b, hprm, **hkw)
        assert np.array_equal(bits(P), bits(wP)) and np.array_equal(bits(tile_len), bits(wlen)) and np.array_equal(tile_spp, wspp), k
        if k == 0:
            assert (tile_spp == min(b.max_spp, b.base_spp * 8)).all()                      # 2^ceil(log2 8) = 8
        else:
            settled = br.tile_min(P) + F(1) >= b.target_history
            assert (tile_spp[settled] == b.base_spp).all() and (tile_spp[~settled] > b.base_spp).all()
            boosted_later += int((~settled).sum())
        # driver, pair normalise
        film = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
        half = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
        d_spp = dev.u32_up(tile_spp)
        prm = pkg.make_params(b.max_spp, "mis", "sobol", seed=k)
        res = product.render_budget_device(hs.sc, cam, prm, bp, d_spp.data_ptr(), film.data_ptr(), half.data_ptr(), lst.data_ptr(), scratch.data_ptr(), nbytes)
        torch.cuda.synchronize()
        assert res.total_samples == int(br.per_pixel(tile_spp, W, H).astype(np.int64).sum())
        hF, hH = film.cpu().numpy(), half.cpu().numpy()
        product.film_pair_normalize_tiles_device(film.data_ptr(), half.data_ptr(), d_spp.data_ptr(), W, H, film.data_ptr(), half.data_ptr())
        torch.cuda.synchronize()
        f2, h2 = br.pair_normalize(hF, hH, tile_spp)
        assert np.array_equal(bits(film.cpu().numpy()), bits(f2)) and np.array_equal(bits(half.cpu().numpy()), bits(h2))
        # the unchanged accumulation with spp = 2, then the credit
        d_cur = dict(g, film=film, half=half)
        h_cur = dict(hg, film=f2, half=h2)
        if k == 0:
            out = dev.run_device(d_cur, 2, None, None, rectified=False)
            want = tr.accumulate(h_cur, 2)
        else:
            out = dev.run_motion_device(d_cur, 2, d_prev, view, d_ids, d_ids_prev, d_table)
            want = mr.accumulate_motion(h_cur, 2, h_prev, hview, h_ids, h_ids_prev, table, hprm)
        product.temporal_length_credit_device(out[2].data_ptr(), d_spp.data_ptr(), b.base_spp, float(tp.max_history), W, H)
        torch.cuda.synchronize()
        want_len = br.length_credit(want[2], tile_spp, b.base_spp, float(hprm.max_history))
        for name, a, w in zip(("film", "half", "length"), out, (want[0], want[1], want_len)):
            assert np.array_equal(bits(a.cpu().numpy()), bits(w)), (k, name)
        if k == 0:
            assert (want_len == 8).all()                                                   # a first frame at 8 x base leaves with length 8
        d_prev = dict(g, film=out[0], half=out[1], length=out[2])
        h_prev = dict(hg, film=want[0], half=want[1], length=want_len)
        d_ids_prev, h_ids_prev, m_prev = d_ids, h_ids, m
    assert boosted_later > 0 and (h_ids_prev == HERO + 1).sum() > 100                      # the moving hero disoccludes something


# ---------------- 5. the CLI ----------------
from test_instance_move_gpu import cli, cli_matrix  # noqa: E402,F401  (the CLI fixture and host/main.cpp's matrix, shared)
from test_motion_gpu import CLI_STEPS, FRAME_SPP  # noqa: E402


def cli_replay(product, pkg, dev, frames, b):
    """the calls of `mi355pt --scene 3 --temporal-frames N --temporal-budget T --instance-step ...` through the ABI from the public pieces -> u8"""
    torch = dev.torch
    W, H = 64, 48
    sc = product.new_scene()
    cam = pkg.scenes.load_scene(sc, 3, W, H, build=False)
    d65 = sc.add_lut470(pkg.scenes.presets()["cie_illum_d6500"])
    for i in CLI_STEPS:
        sc.set_instance_dynamic(i)
    sc.build(cam)
    now = [m.copy() for _, _, m in sc.instances]
    bp = product.budget_params(b.base_spp, b.max_spp, float(b.target_history))
    tp = product.temporal_params_default()
    nbytes = product.adaptive_scratch_bytes(W, H)
    scratch = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    ty, tx = br.tiles_of(W, H)
    lst = torch.zeros(ty * tx, dtype=torch.int32, device="cuda")
    tl = torch.zeros(ty * tx, dtype=torch.float32, device="cuda")
    ts = torch.zeros(ty * tx, dtype=torch.int32, device="cuda")
    view = product.temporal_view_from_cameras(cam, cam)
    acc, g, prev_ids, totals = None, None, None, []
    for k in range(frames):
        prev_m = [m.copy() for m in now]
        if k > 0:
            for i, (t, ry) in CLI_STEPS.items():
                now[i] = cli_matrix(t, ry, (1.0, 1.0, 1.0), now[i])
            assert sc.move_instances(cam, sorted(CLI_STEPS), [now[i] for i in sorted(CLI_STEPS)])["rebuilt"] == 0
        f = {n: torch.zeros((H, W, 3), dtype=torch.float32, device="cuda") for n in ("film", "half") + G_FILMS}
        product.render_gbuffer_accum_device(sc, cam, pkg.make_params(GUIDE_SPP, "mis", "sobol", seed=k), d65, 0, GUIDE_SPP, {n: f[n].data_ptr() for n in G_FILMS})
        _, ids = dev.render_ids(sc, cam, pkg.make_params(GUIDE_SPP, "mis", "sobol", seed=k))
        table = dev.table_up(product.motion_table(cam, cam, now, prev_m))
        prev = dict({n: g[n] for n in G_FILMS}, film=acc[0], half=acc[1], length=acc[2]) if acc is not None else None
        ptr = lambda d: {n: v.data_ptr() for n, v in d.items()} if d is not None else None   # noqa: E731
        motion = product.budget_motion(ids.data_ptr(), prev_ids.data_ptr() if prev is not None else None, table.data_ptr(), table.shape[0])
        product.temporal_budget_device(ptr(f), ptr(prev), view if prev is not None else None, W, H, tp, motion, bp, None, tl.data_ptr(), ts.data_ptr())
        res = product.render_budget_device(sc, cam, pkg.make_params(b.max_spp, "mis", "sobol", seed=k), bp, ts.data_ptr(), f["film"].data_ptr(), f["half"].data_ptr(),
                                           lst.data_ptr(), scratch.data_ptr(), nbytes)
        totals.append(int(res.total_samples))
        product.film_pair_normalize_tiles_device(f["film"].data_ptr(), f["half"].data_ptr(), ts.data_ptr(), W, H, f["film"].data_ptr(), f["half"].data_ptr())
        acc = dev.run_motion_device(f, 2, prev, view if prev is not None else None, ids, prev_ids if prev is not None else None, table)
        product.temporal_length_credit_device(acc[2].data_ptr(), ts.data_ptr(), b.base_spp, float(tp.max_history), W, H)
        g, prev_ids = f, ids
    rgb = torch.empty_like(acc[0])
    product.film_resolve_device(acc[0].data_ptr(), W * H, 2, rgb.data_ptr())
    torch.cuda.synchronize()
    return product.quantize_u8(rgb.cpu().numpy()), totals


def test_budget_cli(product, pkg, dev, cli, tmp_path):
    """`--temporal-frames 3 --temporal-budget 8 --instance-step ...` at 64 x 48 writes the picture of the same calls replayed through the ABI,
    u8-equal, and says one line per frame with the driver's total on stderr; the picture differs from the one without the budget; it also runs
    with --flow, --temporal-rectify, --camera-step and --denoise-variance; every refusal exits 2 naming --temporal-budget, and
    --adaptive-threshold with --temporal-frames stays refused with its own message."""
    import subprocess
    from PIL import Image
    exe, env = cli
    base = [exe, "--scene", "3", "--renderer", "mis", "--sampler", "sobol", "--spp", str(FRAME_SPP), "--width", "64", "--height", "48",
            "--denoise-guide-spp", str(GUIDE_SPP)]
    steps = []
    for i, (t, ry) in sorted(CLI_STEPS.items()):
        steps += ["--instance-step", "%d:%g,%g,%g" % ((i,) + t) + (":%g" % ry if ry else "")]
    t3 = ["--temporal-frames", "3"]

    def picture(extra, name):
        path = str(tmp_path / name)
        r = subprocess.run(base + t3 + extra + ["-o", path], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        return np.asarray(Image.open(path).convert("RGB")), r.stderr
    plain, _ = picture(steps, "plain.png")
    got, err = picture(steps + ["--temporal-budget", "8"], "budget.png")
    want, totals = cli_replay(product, pkg, dev, 3, br.budget(FRAME_SPP, 8 * FRAME_SPP, 8.0))
    lines = [ln for ln in err.splitlines() if ln.startswith("temporal budget, frame ")]
    assert len(lines) == 3 and all("total_samples=%d " % t in ln for t, ln in zip(totals, lines)), (err, totals)
    assert totals[0] == 64 * 48 * 32 and totals[1] < totals[0] and totals[2] < totals[0]
    assert got.shape == want.shape and np.array_equal(got, want), int((got != want).sum())
    assert got.mean() > 10.0 and not np.array_equal(got, plain)
    for extra in (["--flow", "--camera-step", "0.05,0,0"] + steps, ["--temporal-rectify", "--denoise-variance", "--temporal-budget-max-spp", "16"]):
        pic, err = picture(extra + ["--temporal-budget", "6"], "more.png")
        assert pic.mean() > 10.0 and err.count("temporal budget, frame ") == 3, err
    for args in (["--temporal-budget", "8"],                                                   # without --temporal-frames
                 t3 + ["--temporal-budget-max-spp", "16"],                                      # without --temporal-budget
                 t3 + ["--temporal-budget", "8", "--half-res", "--denoise-variance"],
                 t3 + ["--temporal-budget", "0.5"], t3 + ["--temporal-budget", "nan"],
                 t3 + ["--temporal-budget", "8", "--temporal-budget-max-spp", "2"], t3 + ["--temporal-budget", "8", "--temporal-budget-max-spp", "24"],
                 ["--spp", "6"] + t3 + ["--temporal-budget", "8"]):
        r = subprocess.run(base + args, env=env, capture_output=True, text=True, timeout=120, cwd=tmp_path)
        assert r.returncode == 2 and "--temporal-budget" in r.stderr, (args, r.returncode, r.stderr)
    r = subprocess.run(base + ["--spp", "16"] + t3 + ["--adaptive-threshold", "0.05"], env=env, capture_output=True, text=True, timeout=120, cwd=tmp_path)
    assert r.returncode == 2 and "temporal accumulation takes one sample count per frame" in r.stderr
