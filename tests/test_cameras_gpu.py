"""Every kernel that shoots camera rays, under the cameras of tests/camera_cases.py: rolled (s.y != 0), along +z, +-x and +-y, 1 to 170 degrees
wide, portrait and one-pixel-wide frames, unnormalised inputs, `up` a degree from the direction, a world 2000 units from the origin, and
scenes 3 and 17 through a rolled and a 120-degree camera.  Every camera of every other GPU test has up = +y, looks into -z and is 45 (once 70)
degrees wide, so a term of the basis that is zero there (s.y) could be dropped from any of the statements of the camera (regen_path,
camera_ray_dir, cam_pyramid) without one of them noticing.

Every bar is the bar of the test that owns the comparison, imported: the ID pass is equal to its CPU restatement pixel for pixel (but on
the ties tests/test_cameras.py counts and caps), the G-buffer and the AOVs meet PER_SAMPLE_MIN / TIGHT_MIN / FRAME_BAR, the path kernels the
bars of test_other_scenes_radiance_parity and FRAME_BAR, the lowering modes those of test_lowering_paths_agree_with_the_oracle, lists against
traversal bit equality, the device bytes after a camera move the pinned host lowering's, the flow records and the temporal accumulation bit
equality with their NumPy restatements.  One line per (test, case) goes to the file MI355PT_FRAME_LOG names (profiles/camera_parity.jsonl)."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aov_reference  # noqa: E402
import camera_cases as cc  # noqa: E402
import flow_hits_reference  # noqa: E402
import flow_reference as fr  # noqa: E402
import gbuffer_reference  # noqa: E402
import ids_reference  # noqa: E402
import temporal_reference as tr  # noqa: E402
from test_aov_gpu import FRAME_BAR, PER_SAMPLE_MIN, TIGHT_MIN  # noqa: E402
from test_camera_candidates_gpu import bits  # noqa: E402
from test_cameras import (REPROJECTION_MEDIAN_BAR, SMALL_FRAMES, SPARSE_COUNT, SPARSE_SHARDS, SPARSE_SPP, TEMPORAL_CASES, TEMPORAL_PREVIOUS,  # noqa: E402
                          assert_lists_in_use, lists_in_use, turned_camera)
from test_flow_gpu import XC_REL_TOL, FlowDevice, raw  # noqa: E402
from test_gbuffer_gpu import FILMS, gpu_films  # noqa: E402
from test_temporal_gpu import FRAME_SPP, GUIDE_SPP, Device, assert_bit_equal, frame_of, host, render_frame  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
STRATEGIES = ("pt", "nee", "mis")
N_PROBED = 20000


def log_line(rec):
    print(json.dumps(rec))
    if os.environ.get("MI355PT_FRAME_LOG"):
        with open(os.environ["MI355PT_FRAME_LOG"], "a") as f:
            f.write(json.dumps(rec) + "\n")


@pytest.fixture(scope="module")
def dev(product, pkg):
    return FlowDevice(product, pkg)


@pytest.fixture(scope="module")
def temporal_dev(product, pkg):
    return Device(product, pkg)           # (tests/test_temporal_gpu.py's: the plain accumulation)


@pytest.fixture(scope="module")
def ids_ref():
    return ids_reference.IdsReference()


@pytest.fixture(scope="module")
def hits_ref():
    return flow_hits_reference.FlowHitsReference()


@pytest.fixture(scope="module")
def aov_ref():
    return aov_reference.AovReference()


@pytest.fixture(scope="module")
def gbuffer_ref():
    return gbuffer_reference.GbufferReference()


def cached(make):
    """a per-module cache of what make(name) builds: references are computed once, shared and left unchanged"""
    store = {}

    def get(*key):
        if key not in store:
            store[key] = make(*key)
        return store[key]
    return get


@pytest.fixture(scope="module")
def gpu_scene(product):
    """case -> (scene, camera, d65) on the product, default builder and lowering, built once"""
    return cached(lambda name: cc.build_scene(product, name))


@pytest.fixture(scope="module")
def cpu_scene(oracle, aov_ref, gbuffer_ref, ids_ref):
    """(backend name, case) -> (scene, camera, d65) on a CPU backend, in its fast mode (bit-equal to the faithful one for primary rays)"""
    backends = {"oracle": oracle, "aov": aov_ref, "gbuffer": gbuffer_ref, "ids": ids_ref}

    def make(backend, name):
        be = backends[backend]
        sc, cam, d65 = cc.build_scene(be, name)
        be.set_faithful(sc, False)
        return sc, cam, d65
    return cached(make)


@pytest.fixture(scope="module")
def census(pkg, ids_ref, cpu_scene):
    """case -> (ids of the CPU restatement, tie mask, options per pixel): the float64 census of tests/camera_cases.py; that it holds for the
    reference alone (ties within TIE_CAP, the restatement equal to the brute force outside them) is tests/test_cameras.py, without a GPU"""
    def make(name):
        sc, cam, _ = cpu_scene("ids", name)
        _, _, tie, options = cc.centre_census(sc, cam)
        want = ids_ref.render_ids(sc, cam, pkg.make_params(1))
        assert tie.mean() <= cc.TIE_CAP
        want.setflags(write=False); tie.setflags(write=False)
        return want, tie, options
    return cached(make)


def assert_ids(got, want, tie, options, tag):
    bad = (got != want) & ~tie
    assert not bad.any(), (tag, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    for y, x in np.argwhere(tie):
        assert int(got[y, x]) in options[y * got.shape[1] + x], (tag, int(x), int(y))
    return int(bad.sum())


# ---------------------------------------------------------------------------------------------------------------- a. the ID pass
@pytest.mark.parametrize("builder", ["host", "gpu"])
@pytest.mark.parametrize("name", cc.NAMES)
def test_ids_under_every_camera(dev, product, pkg, census, name, builder):
    sc, cam, _ = cc.build_scene(product, name, builder=builder)
    want, tie, options = census(name)
    got, _ = dev.render_ids(sc, cam, pkg.make_params(1))
    assert_ids(got, want, tie, options, (name, builder))
    log_line({"test": "ids", "case": name, "builder": builder, "pixels": int(want.size), "ties": int(tie.sum()), "instances_seen": int(np.unique(want[want > 0]).size),
              "mismatching_outside_ties": 0})
    other, _ = dev.render_ids(sc, cam, pkg.make_params(7, "nee", "random", seed=12345))
    assert np.array_equal(other, got)


@pytest.mark.parametrize("name", ["roll30", "fov170", "portrait_fov120_roll"])
def test_ids_shards_and_host_buffer(dev, product, pkg, census, gpu_scene, name):
    """as test_ids_match_the_cpu_restatement: one shard of three leaves the other pixels as they were, three shards into one buffer are the
    unsharded buffer, the host-buffer form gives the same"""
    import torch
    sc, cam, _ = gpu_scene(name)
    want, tie, options = census(name)
    W, H = cam.width, cam.height
    whole, _ = dev.render_ids(sc, cam, pkg.make_params(1))
    buf = torch.full((H, W), -1, dtype=torch.int32, device="cuda")
    product.render_ids_device(sc, cam, pkg.make_params(1, shard_index=1, shard_count=3), buf.data_ptr())
    torch.cuda.synchronize()
    one = buf.cpu().numpy().view(np.uint32)
    mine = ((np.arange(H)[:, None] // 8) * ((W + 7) // 8) + np.arange(W)[None, :] // 8) % 3 == 1
    assert np.array_equal(one[mine], whole[mine]) and (one[~mine] == 0xffffffff).all()
    for k in (0, 2):
        product.render_ids_device(sc, cam, pkg.make_params(1, shard_index=k, shard_count=3), buf.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy().view(np.uint32), whole)
    assert np.array_equal(product.render_ids(sc, cam, pkg.make_params(1)), whole)
    assert_ids(whole, want, tie, options, name)


# ---------------------------------------------------------------------------------------------------------------- b. G-buffer and AOVs
@pytest.mark.parametrize("name", cc.NAMES)
def test_gbuffer_under_every_camera(product, pkg, gbuffer_ref, gpu_scene, cpu_scene, name):
    """tests/test_gbuffer_gpu.py test_gbuffer_parity_with_the_cpu_restatement on the case's frame, one sample per pixel: shading_normal and
    hit.yz bit-equal where both sides hit the same class, position and hit.x at the two per-sample bars over all pixels; and the albedo
    film bit-equal to the albedo AOV's"""
    import torch
    gpu = gpu_scene(name)
    sc, cam, d65 = cpu_scene("gbuffer", name)
    W, H = cam.width, cam.height
    g = gpu_films(product, pkg, gpu, W, H, 1)
    c, cls = gbuffer_ref.render_gbuffer_accum(sc, cam, pkg.make_params(1, "mis", "sobol"), d65, want_classes=True)
    for k in FILMS:
        assert np.isfinite(g[k]).all() and np.isfinite(c[k]).all(), k
    g_class = np.where(g["hit"][..., 1] == 0, 2, np.where(g["hit"][..., 2] == 1, 1, 0))
    same = g_class == np.argmax(cls, axis=2)
    assert np.array_equal(g["shading_normal"][same].view(np.uint32), c["shading_normal"][same].view(np.uint32))
    assert np.array_equal(g["hit"][..., 1:][same].view(np.uint32), c["hit"][..., 1:][same].view(np.uint32))
    t = c["hit"][..., 0]
    line = {"test": "gbuffer", "case": name, "same_class": float(same.mean())}
    shares = {}
    for film, gv, cv in (("position", g["position"], c["position"]), ("hit_x", g["hit"][..., :1], c["hit"][..., :1])):
        d = np.abs(gv - cv)
        close = (np.all(d <= 1e-3 * np.abs(cv) + 1e-4, axis=2) & same).mean()
        tight = (np.all(d <= 1e-5 * np.maximum(1.0, t)[..., None], axis=2) & same).mean()
        shares[film] = (close, tight)
        line.update({f"{film}_close": round(float(close), 6), f"{film}_tight": round(float(tight), 6), f"{film}_max_dev": float(f"{d.max():.3e}")})
    d = np.abs(g["albedo"] - c["albedo"])
    shares["albedo"] = ((np.all(d <= 1e-3 * np.abs(c["albedo"]) + 1e-4, axis=2) & same).mean(), (np.all(d <= 1e-5, axis=2) & same).mean())
    line["albedo_max_dev"] = float(f"{d.max():.3e}")
    aov = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    product.render_aov_accum_device(gpu[0], gpu[1], pkg.make_params(1, "mis", "sobol"), pkg.ffi.AOV_ALBEDO, gpu[2], 0, 1, aov.data_ptr(), None)
    torch.cuda.synchronize()
    line["albedo_differs_from_aov"] = int((g["albedo"].view(np.uint32) != aov.cpu().numpy().view(np.uint32)).sum())
    log_line(line)
    assert line["albedo_differs_from_aov"] == 0
    for film, (close, tight) in shares.items():
        assert close >= PER_SAMPLE_MIN, (film, close)
        assert tight >= TIGHT_MIN, (film, tight)


@pytest.mark.parametrize("kind", ["normal", "albedo", "shading_normal"])
@pytest.mark.parametrize("name", cc.NAMES)
def test_aovs_under_every_camera(product, pkg, aov_ref, gpu_scene, cpu_scene, name, kind):
    """tests/test_aov_gpu.py: one sample per pixel at PER_SAMPLE_MIN / TIGHT_MIN, and the 64-spp frame at FRAME_BAR"""
    (sg, cam, dg), (sc, _, dc) = gpu_scene(name), cpu_scene("aov", name)
    k = pkg.ffi.AOV[kind]
    line = {"test": "aov", "case": name, "kind": kind}
    for spp in (1, 64):
        prm = pkg.make_params(spp, "mis", "sobol")
        g, c = product.render_aov(sg, cam, prm, k, dg), aov_ref.render_aov(sc, cam, prm, k, dc)
        assert np.isfinite(g).all() and np.isfinite(c).all()
        d = np.abs(g - c)
        if spp == 1:
            close, tight = np.all(d <= 1e-3 * np.abs(c) + 1e-4, axis=2).mean(), np.all(d <= 1e-5, axis=2).mean()
            line.update({"close": round(float(close), 6), "tight": round(float(tight), 6), "max_dev": float(f"{d.max():.3e}")})
        else:
            rmse, off = float(np.sqrt(np.mean((g - c) ** 2))), int((d.max(axis=2) > 0.01).sum())
            line.update({"frame_rmse": float(f"{rmse:.3e}"), "frame_off": off})
            assert c.mean() > 0.01
    log_line(line)
    assert line["close"] >= PER_SAMPLE_MIN and line["tight"] >= TIGHT_MIN, line
    assert line["frame_rmse"] <= FRAME_BAR[0] and line["frame_off"] <= FRAME_BAR[1], line


# ---------------------------------------------------------------------------------------------------------------- c. the path kernels
def radiance_parity(product, oracle, pkg, gpu, cpu, strategy, sampler, tag):
    """the bars of tests/test_parity_gpu.py test_other_scenes_radiance_parity on at most 20 000 probed samples, no NaN sample on either side
    (the scenes hold no glass), and the 64-spp frame at FRAME_BAR"""
    (sg, cam, _), (sc, _, _) = gpu, cpu
    rng = np.random.default_rng(3)
    n = min(N_PROBED, cam.width * cam.height * 64)
    xys = np.stack([rng.integers(0, cam.width, n), rng.integers(0, cam.height, n), rng.integers(0, 64, n)], 1).astype(np.uint32)
    prm = pkg.make_params(64, strategy, sampler)
    Lg, lg, pg = sg.probe_radiance(cam, prm, xys)
    Lc, lc, pc = sc.probe_radiance(cam, prm, xys)
    assert np.isfinite(Lc).all() and np.isfinite(Lg).all()
    assert np.array_equal(lg, lc)
    same_term = np.all(pg == pc, axis=1).mean()
    close = np.all(np.abs(Lg - Lc) <= 1e-3 * np.abs(Lc) + 1e-4, axis=1).mean()
    tight = np.all(np.abs(Lg - Lc) <= 1e-5 * np.abs(Lc) + 1e-12, axis=1).mean()
    g, c = product.render(sg, cam, prm), oracle.render(sc, cam, prm)
    assert np.isfinite(g).all() and np.isfinite(c).all()
    rmse, off = float(np.sqrt(np.mean((g - c) ** 2))), int((np.abs(g - c).max(axis=2) > 0.01).sum())
    log_line({"test": "radiance", **tag, "strategy": strategy, "sampler": sampler, "samples": n, "same_term": round(float(same_term), 6),
              "close": round(float(close), 6), "tight": round(float(tight), 6), "frame_rmse": float(f"{rmse:.3e}"), "frame_off": off, "mean": float(f"{c.mean():.4f}")})
    assert same_term >= 0.995, same_term
    assert close >= PER_SAMPLE_MIN, close
    assert tight >= 0.997, tight
    assert float(Lc.mean()) > 0.0 and c.mean() > 0.01
    assert rmse <= FRAME_BAR[0] and off <= FRAME_BAR[1], (rmse, off)


@pytest.mark.parametrize("strategy", STRATEGIES)
@pytest.mark.parametrize("name", cc.NAMES)
def test_path_kernels_under_every_camera(product, oracle, pkg, gpu_scene, cpu_scene, name, strategy):
    radiance_parity(product, oracle, pkg, gpu_scene(name), cpu_scene("oracle", name), strategy, "sobol", {"case": name})


@pytest.mark.parametrize("name", cc.ONE_PER_FAMILY)
def test_path_kernels_with_the_random_sampler(product, oracle, pkg, gpu_scene, cpu_scene, name):
    radiance_parity(product, oracle, pkg, gpu_scene(name), cpu_scene("oracle", name), "mis", "random", {"case": name})


# ---------------------------------------------------------------------------------------------------------------- d. lowering modes
@pytest.mark.parametrize("strategy", ["mis", "nee"])
@pytest.mark.parametrize("name", ["roll30", "fov120", "look_pz"])
def test_lowering_modes_under_a_camera_from_the_table(product, oracle, pkg, cpu_scene, name, strategy):
    """tests/test_parity_gpu.py test_lowering_paths_agree_with_the_oracle with the room: its default lowering is the general one (two
    instances are rotated and scaled), the all-translations variant takes the local-triangle path.  identity == general bit for bit, every
    mode within that test's bars of the oracle, the default and the local path within FRAME_BAR."""
    so, cam, _ = cpu_scene("oracle", name)
    prm = pkg.make_params(64, strategy, "sobol")
    c = oracle.render(so, cam, prm)
    frames = {}
    for mode, lowering, variant in (("auto", "auto", "room"), ("identity", "no_local_tris", "room"), ("general", "general", "room"),
                                    ("local", "auto", "room_translated")):
        sc, cam_g, _ = cc.build_scene(product, name, lowering=lowering, scene=variant)
        assert ("tri_space=local" in product.scene_info(sc)) == (mode == "local")
        frames[mode] = product.render(sc, cam_g, prm)
    assert np.array_equal(frames["identity"], frames["general"])
    # the translated variant is the same world up to the float32 rounding of its baked vertices: its own oracle scene
    st, cam_t, _ = cc.build_scene(oracle, name, scene="room_translated")
    oracle.set_faithful(st, False)
    want = {"auto": c, "identity": c, "general": c, "local": oracle.render(st, cam_t, prm)}
    line = {"test": "lowering", "case": name, "strategy": strategy}
    for mode, g in frames.items():
        rmse, off = float(np.sqrt(np.mean((g - want[mode]) ** 2))), int((np.abs(g - want[mode]).max(axis=2) > 0.01).sum())
        line[mode] = [float(f"{rmse:.3e}"), off]
        assert rmse <= 5e-4 and off <= 2, (mode, rmse, off)
        if mode in ("auto", "local"):
            assert rmse <= FRAME_BAR[0] and off <= FRAME_BAR[1], (mode, rmse, off)
    log_line(line)


# ---------------------------------------------------------------------------------------------------------------- e. lists against traversal
LIST_CASES = [(n, (1920, 1080), SPARSE_SHARDS[n], SPARSE_COUNT, SPARSE_SPP) for n in SPARSE_SHARDS] + [(n, None, 0, 1, 64) for n in SMALL_FRAMES]


@pytest.mark.parametrize("name,size,shard_index,shard_count,spp", LIST_CASES, ids=[c[0] for c in LIST_CASES])
def test_lists_and_traversal_agree_under_a_camera_from_the_table(product, pkg, monkeypatch, name, size, shard_index, shard_count, spp):
    """tests/test_camera_candidates_gpu.py: MI355PT_NO_CAMERA_LISTS on and off, per-sample log and film bit-equal, on a sparse shard of the
    1920 x 1080 frame (2 x 2-pixel work items, lists really in use: tests/test_cameras.py checks that on the host walk) and on the three
    smallest frames whole (one work item sees the whole room: lists and the fallback side by side)"""
    sc, cam, _ = cc.build_scene(product, name, size=size)
    share, counts, over = lists_in_use(sc, cam, name, shard_index, shard_count, spp)
    if size is not None:
        assert_lists_in_use(name, share, counts, over)
    prm = pkg.make_params(spp, "mis", "sobol", shard_index=shard_index, shard_count=shard_count)
    monkeypatch.setenv("MI355PT_NO_CAMERA_LISTS", "1")
    ref = product.render_sample_log(sc, cam, prm, 0, spp, want_accum=True)
    monkeypatch.delenv("MI355PT_NO_CAMERA_LISTS")
    got = product.render_sample_log(sc, cam, prm, 0, spp, want_accum=True)
    assert float(np.nansum(ref[3])) > 0.0 and not np.isnan(ref[0]).any()
    differ = {what: int((bits(a) != bits(b)).sum()) for what, a, b in zip(("L", "lambda", "pdf", "film"), ref, got)}
    log_line({"test": "lists_vs_traversal", "case": name, "items": int(counts.size), "within_cap": round(share, 4), "overflowing": int(over.sum()),
              "longest": int(counts[~over].max(initial=0)), "values_differing": differ})
    assert not any(differ.values()), differ


# ---------------------------------------------------------------------------------------------------------------- f. camera moves and flow
MOVE_STEP = (0.31, -0.17, 0.23)


@pytest.mark.parametrize("builder", ["host", "gpu"])
@pytest.mark.parametrize("name", ["roll30", "look_px"])
def test_camera_move_and_flow_under_a_camera_from_the_table(dev, product, pkg, hits_ref, name, builder):
    """mark, move the camera by a general step: the device bytes are the pinned host lowering's (tests/test_rebase_gpu.py's bar: bytes), the
    flow records are bit-equal to tests/flow_reference.py fed the kernel's own hits, and those hits are the oracle's at the new position
    (tests/test_flow_gpu.py check_records): the instance on every pixel that is not a tie, the triangle on every pixel where no second
    triangle is within the census' 1e-6, and the interpolated position Xc within XC_REL_TOL x max|P| of the oracle's hit position"""
    sc, cam, _ = cc.build_scene(product, name, builder=builder)
    fresh = sc.debug_device_digest()
    assert fresh == sc.debug_pinned_digest(cam)
    product.scene_flow_mark(sc)
    marked = product.export_bvh(sc)[1]
    for i in range(3):
        cam.position[i] = float(F(cam.position[i]) + F(MOVE_STEP[i]))
    res = sc.move_camera(cam)
    assert res["rebuilt"] == 0 and res["reason"] == "rebased"
    got, want = sc.debug_device_digest(), sc.debug_pinned_digest(cam)
    differ = [n for n in want[0] if got[0][n] != want[0][n]]
    assert not differ and got[1] == want[1] and got[0]["tris_render"] != fresh[0]["tris_render"]
    flow, ids, hits = product.render_flow_debug(sc, cam, pkg.make_params(1))
    tris_cur, tris_prev = product.export_bvh(sc)[1], product.scene_export_flow_mark(sc)
    assert np.array_equal(raw(tris_prev), raw(marked))
    records = fr.records_from_hits(hits, ids, tris_cur, tris_prev)
    bad = int((raw(flow) != raw(records)).sum())
    plain, plain_ids, _ = dev.render_flow(sc, cam, pkg.make_params(1))
    assert np.array_equal(raw(plain), raw(flow)) and np.array_equal(plain_ids, ids)
    # the reference at the new position: the same scene described to the oracle, the camera moved with it
    so, cam_o, _ = cc.build_scene(hits_ref, name, build=False)
    for i in range(3):
        cam_o.position[i] = cam.position[i]
    so.build(cam_o)
    _, _, tie, options, want_pair, tri_tie = cc.centre_census(so, cam_o, want_triangles=True)
    assert tri_tie.mean() <= cc.TIE_CAP
    o_ids, o_tri, o_pos = hits_ref.render_flow_hits(so, cam_o, pkg.make_params(1))
    assert_ids(ids, o_ids, tie, options, (name, builder))
    hit = ids != 0
    sure = hit & ~tri_tie
    pair = product.scene_export_triangle_ids(sc)[hits["tri"]].astype(np.int64)
    wrong = int(((pair[..., 0] + 1 != o_ids) & sure).sum() + ((pair[..., 1] != o_tri) & sure).sum())
    wrong_f64 = int((pair[sure] != want_pair[sure]).any(axis=-1).sum())          # ... and the float64 brute force's, directly
    Pc = fr.positions(tris_cur)
    xc = fr.interpolate(hits["b"], Pc[hits["tri"]])
    scale = float(np.abs(Pc).max())
    xc_rel = float(np.abs(xc.astype(np.float64) - o_pos.astype(np.float64))[sure].max() / scale)
    moved = int((np.abs(flow["d"]).max(axis=-1) > 0).sum())
    log_line({"test": "move_and_flow", "case": name, "builder": builder, "arrays": len(want[0]), "arrays_differing": differ, "flow_words_differing": bad,
              "moved_pixels": moved, "ties": int(tie.sum()), "triangle_ties": int(tri_tie.sum()), "hits_differing_from_oracle": wrong,
              "hits_differing_from_float64": wrong_f64, "xc_rel_max": xc_rel, "xc_scale": scale})
    assert bad == 0 and moved > 0.9 * ids.size
    assert wrong == 0 and wrong_f64 == 0, (wrong, wrong_f64)
    assert xc_rel <= XC_REL_TOL, xc_rel


# ---------------------------------------------------------------------------------------------------------------- g. temporal accumulation
@pytest.mark.parametrize("name", TEMPORAL_CASES)
def test_temporal_accumulation_across_a_roll_and_a_yaw(temporal_dev, product, pkg, name):
    """tests/test_temporal_gpu.py test_temporal_rendered_parity_and_geometry with a previous camera rolled by 10 degrees, yawed by 5 and
    standing elsewhere: both accumulations bit-equal to tests/temporal_reference.py on the same buffers, the reprojection geometry at that
    test's bars and the median at REPROJECTION_MEDIAN_BAR"""
    dev = temporal_dev
    cur = cc.build_scene(product, name)
    W, H = cur[1].width, cur[1].height
    assert (W, H) == (64, 48)                                                  # (render_frame's size)
    sp, cam_p, d65_p = cc.build_scene(product, name, build=False)
    cam_p = turned_camera(pkg, cam_p, *TEMPORAL_PREVIOUS)
    sp.build(cam_p)
    f0, f1 = render_frame(product, pkg, (sp, cam_p, d65_p), 0), render_frame(product, pkg, cur, 1)
    cam_c = cur[1]
    view = product.temporal_view_from_cameras(cam_c, cam_p)
    h0, h1 = host(f0), host(f1)
    a0 = dev.run_device(frame_of(f0), FRAME_SPP, None, None, None)
    assert_bit_equal([x.cpu().numpy() for x in a0], tr.accumulate(frame_of(h0), FRAME_SPP), f"camera_temporal_{name}_frame0")
    prev = dict(frame_of(f0, ("position", "shading_normal", "hit")), film=a0[0], half=a0[1], length=a0[2])
    a1 = dev.run_device(frame_of(f1), FRAME_SPP, prev, view, None)
    want = tr.accumulate(frame_of(h1), FRAME_SPP, host(prev), view, detail=True)
    assert_bit_equal([x.cpu().numpy() for x in a1], want[:3], f"camera_temporal_{name}_frame1")
    info = want[3]
    hit = h1["hit"][..., 1] > 0
    assert info["has"][hit].mean() > 0.5 and (~info["has"]).any()
    gb = ("position", "shading_normal", "hit")
    cur_g, prev_g, prm = tr.geometry_frames(frame_of(h1, gb), frame_of(h0, gb), cam_c, cam_p, GUIDE_SPP)
    got = dev.run(cur_g, GUIDE_SPP, prev_g, view, prm)
    assert_bit_equal(got, tr.accumulate(cur_g, GUIDE_SPP, prev_g, view, prm), f"camera_temporal_{name}_geometry")
    fig = tr.geometry_figures(got[0], cur_g, prev_g, view, prm, cam_c, GUIDE_SPP)
    log_line({"test": "temporal", "case": name, **{k: round(v, 4) if isinstance(v, float) else v for k, v in fig.items()}})
    bars = tr.GEOMETRY_BARS
    assert fig["interior_share"] >= bars["interior_share"] and fig["share_under_quarter"] >= bars["share_under_quarter"], fig
    assert fig["median"] <= min(bars["median"], REPROJECTION_MEDIAN_BAR), fig
