"""Moving the camera of a built scene on the MI355X (include/mi355pt_rebase.h): after mi355pt_scene_move_camera EVERY device array has
the bytes of the host lowering for the new camera over the built tree (mi355pt_scene_debug_device_digest against
mi355pt_scene_debug_move_digest, which tests/test_rebase.py ties to the recorded digests and to the stress families' own vertices); the
moved scene traces what a scene freshly built at the new position traces; the fallbacks rebuild; the CLI's --camera-move rebase writes
the frame of the same calls through the ABI.  One line per comparison goes to the file MI355PT_FRAME_LOG names (profiles/rebase_parity.jsonl)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geometry_stress as gs  # noqa: E402
from conftest import linear_rmse_u8  # noqa: E402
from test_rebase import check_exported_tree, moved, sliver_scene  # noqa: E402
from test_scene_lowering import _describe  # noqa: E402
from test_temporal_gpu import FRAME_SPP, GUIDE_SPP, H3, W3, cli, dev, frame_of  # noqa: E402,F401  (the CLI fixture and the temporal replay's device helper)

pytestmark = pytest.mark.gpu
F = np.float32
W, H = 64, 48
SCENES = ["1", "3", "3:no_local_tris", "3:general", "17", "19", "21", "24", "29", "31"]      # tests/test_scene_lowering.py's set
FAMILIES = ["instanced", "slivers64", "soup1025"]
# both builders where the GPU builder accepts the scene: it refuses fewer than 8 triangles (scene 24: a root that is a leaf)
CASES = [(c, b) for c in SCENES + FAMILIES for b in ("host", "gpu") if not (c == "24" and b == "gpu")]
STEP = (0.3, -0.2, 0.45)


def log_line(line):
    if os.environ.get("MI355PT_FRAME_LOG"):
        with open(os.environ["MI355PT_FRAME_LOG"], "a") as f:
            f.write(json.dumps(line) + "\n")


def describe(pkg, product, case, builder):
    """(scene, camera, D65 LUT id or None), described and not built"""
    if case in FAMILIES:
        sc, cam, d65 = gs.build_scene(product, case, builder=builder, env_light=True, width=W, height=H, build=False)
        return sc, cam, d65
    sc, cam = _describe(pkg, product, case)
    sc.set_bvh_builder(builder)
    return sc, cam, None


def heights_of(nodes, root):
    """the number of node heights of an exported BVH2 (height 1: both children are leaves)"""
    links = nodes[:, 12:14].view(np.int32)
    used = nodes[:, [0, 1]].view(F) < np.finfo(F).max                          # the wrapped single leaf's second child is the empty point box
    h = {}
    stack = [(int(root), False)]
    while stack:
        v, done = stack.pop()
        kids = [int(links[v, s]) for s in (0, 1) if used[v, s] and links[v, s] >= 0]
        if done:
            h[v] = 1 + max([h[k] for k in kids], default=0)
        else:
            stack.append((v, True)); stack.extend((k, False) for k in kids)
    return h[int(root)]


@pytest.mark.parametrize("case,builder", CASES)
def test_device_bytes_after_a_move(product, pkg, case, builder):
    """the main test: build at cam, move to cam2 — every device array has the digest of the pinned host lowering, camera-free arrays
    thereby undisturbed; the exported tree keeps its links and has exact boxes; a render with the old position is refused as after a
    build and an unchanged position is a no-op; moving back restores the bytes of the fresh build"""
    sc, cam, _ = describe(pkg, product, case, builder)
    sc.build(cam)
    assert f"builder={builder}" in product.scene_info(sc)
    fresh, fresh_info = sc.debug_device_digest()
    if builder == "host":
        assert (fresh, fresh_info) == sc.debug_lowering_digest(cam)             # the read-back itself: what was lowered is what the device holds
    nodes0, tris0, root0 = product.export_bvh(sc)
    cam2 = moved(pkg, cam, STEP)
    res = sc.move_camera(cam2)
    assert res["rebuilt"] == 0 and res["reason"] == "rebased"
    assert res["launches"] == heights_of(nodes0, root0) + 2 and res["launches"] <= 22 + 1 + 2
    got, got_info = sc.debug_device_digest()
    want, want_info, reason = sc.debug_move_digest(cam, cam2)
    assert reason == "rebased" and list(got) == list(want) == list(fresh)
    differ = [n for n in want if got[n] != want[n]]
    log_line({"test": "device_bytes", "case": case, "builder": builder, "arrays": len(want), "differ": differ, "launches": res["launches"],
              "host_ms": round(res["host_ms"], 3), "device_ms": round(res["device_ms"], 3)})
    assert not differ and got_info == want_info
    assert got["tris_render"] != fresh["tris_render"] and got["nodes"] != fresh["nodes"] and got["rgb2spec"] == fresh["rgb2spec"] and got["shade"] == fresh["shade"]
    nodes1, tris1, root1 = product.export_bvh(sc)
    assert root1 == root0 and np.array_equal(nodes1[:, 12:16], nodes0[:, 12:16]) and np.array_equal(tris1[:, 9:], tris0[:, 9:])
    check_exported_tree(nodes1, tris1, root1)
    prm = pkg.make_params(1, "mis", "sobol")
    with pytest.raises(RuntimeError, match="camera position differs"):
        product.render(sc, cam, prm)
    assert np.isfinite(product.render(sc, cam2, prm)).all()
    again = sc.move_camera(cam2)
    assert again["reason"] == "same_position" and again["rebuilt"] == 0 and again["launches"] == 0
    assert sc.debug_device_digest()[0] == got
    back = sc.move_camera(cam)
    assert back["rebuilt"] == 0 and back["reason"] == "rebased"
    home = sc.debug_device_digest()[0]
    differ = [n for n in home if home[n] != fresh[n]]
    log_line({"test": "round_trip", "case": case, "builder": builder, "differ": differ})
    assert not differ


@pytest.mark.parametrize("case,builder", [("3", "host"), ("17", "gpu"), ("instanced", "host")])
def test_a_chain_of_moves_is_one_move(product, pkg, case, builder):
    """three moves of (0.1, 0, -0.2) leave the bytes of one move to the end position, and the far excursion of tests/test_rebase.py comes
    home to the fresh build's bytes: nothing is incremental"""
    sc, cam, _ = describe(pkg, product, case, builder)
    sc.build(cam)
    fresh = sc.debug_device_digest()[0]
    for k in (1, 2, 3):
        assert sc.move_camera(moved(pkg, cam, (0.1, 0.0, -0.2), k))["rebuilt"] == 0
    chained = sc.debug_device_digest()[0]
    end = moved(pkg, cam, (0.1, 0.0, -0.2), 3)
    sc2, _, _ = describe(pkg, product, case, builder)
    sc2.build(cam)
    assert sc2.move_camera(end)["rebuilt"] == 0
    assert sc2.debug_device_digest()[0] == chained == sc.debug_move_digest(cam, end)[0]
    assert sc.move_camera(moved(pkg, cam, (2000.0, -3.0, 0.125)))["rebuilt"] == 0
    assert sc.move_camera(cam)["rebuilt"] == 0
    assert sc.debug_device_digest()[0] == fresh
    log_line({"test": "chain", "case": case, "builder": builder, "equal": True})


def rays_for(tris, n=3000, seed=5):
    """render-space rays: from the camera into its field of view, and from random points of the geometry's bounds in random directions"""
    o_cam, d_cam = gs.camera_like_rays(n, seed)
    rng = np.random.default_rng(seed)
    v = gs.tri_vertices(tris).reshape(-1, 3).astype(np.float64)
    lo, hi = v.min(axis=0), v.max(axis=0)
    o = rng.uniform(lo, hi, (n, 3))
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([o_cam, o.astype(F)]), np.concatenate([d_cam, d.astype(F)])


@pytest.mark.parametrize("case,builder", CASES)
def test_moved_scene_against_a_fresh_build(product, pkg, case, builder):
    """a scene moved to cam2 against a scene BUILT at cam2 (another tree over the same triangles): the same hit / miss pattern and bit-equal
    t on every probe ray, equal any-hit answers, the G-buffer's hit.x bit-equal on >= 0.9999 of the pixels (the bar of
    test_cooperative_traversal_does_not_depend_on_the_builder); the MIS film at 16 spp bit-equal where the two scenes' device digests are
    equal, else within linear_rmse_u8 2e-3 (tests/test_bvh_gpu.py's bar between two trees)"""
    import torch
    sa, cam, d65 = describe(pkg, product, case, builder)
    sa.build(cam)
    cam2 = moved(pkg, cam, STEP)
    assert sa.move_camera(cam2)["rebuilt"] == 0
    sb, _, _ = describe(pkg, product, case, builder)
    sb.build(cam2)
    _, tris, _ = product.export_bvh(sb)
    o, d = rays_for(tris)
    ta, ia, _, _ = sa.probe_intersect(o, d)
    tb, ib, _, _ = sb.probe_intersect(o, d)
    hits = float((tb >= 0).mean())
    assert np.array_equal(ta >= 0, tb >= 0) and np.array_equal(ta.view(np.uint32), tb.view(np.uint32))
    assert (tb >= 0).sum() >= 32 and (tb < 0).any()        # both answers occur (slivers64: triangles 2e-3 wide, 1 % of the rays hit)
    tm = np.where(tb >= 0, tb * F(1.5), F(10.0)).astype(F) * np.random.default_rng(9).uniform(0.3, 1.2, tb.shape).astype(F)
    oa, ob = sa.probe_occluded(o, d, tm), sb.probe_occluded(o, d, tm)
    assert np.array_equal(oa, ob)
    if d65 is None:
        d65 = 0                                                                 # (the position / hit films do not read the illuminant)
    share = []
    for sc in (sa, sb):
        buf = torch.zeros((2, H, W, 3), dtype=torch.float32, device="cuda")
        product.render_gbuffer_accum_device(sc, cam2, pkg.make_params(1, "mis", "sobol"), d65, 0, 1, {"position": buf[0].data_ptr(), "hit": buf[1].data_ptr()})
        torch.cuda.synchronize()
        share.append(buf[1].cpu().numpy()[..., 0].view(np.uint32))
    hit_share = float((share[0] == share[1]).mean())
    assert hit_share >= 0.9999, hit_share
    same_bytes = sa.debug_device_digest()[0] == sb.debug_device_digest()[0]
    prm = pkg.make_params(16, "mis", "sobol")
    img_a, img_b = product.render(sa, cam2, prm), product.render(sb, cam2, prm)
    rmse = linear_rmse_u8(product.quantize_u8(img_a), product.quantize_u8(img_b))
    log_line({"test": "moved_vs_fresh", "case": case, "builder": builder, "rays": int(o.shape[0]), "hit_share": round(hits, 4), "t_bit_equal": True,
              "occluded_equal": True, "gbuffer_hit_x_bit_equal": round(hit_share, 6), "device_digests_equal": bool(same_bytes),
              "film_bit_equal": bool(np.array_equal(img_a, img_b)), "linear_rmse_u8": rmse})
    if same_bytes:
        assert np.array_equal(img_a, img_b)
    else:
        assert rmse <= 2e-3, rmse


def test_fallback_rebuilds_when_the_degenerate_set_changes(product, pkg):
    """the sliver scene of tests/test_rebase.py: 4000 units away the sliver's vertices round to one point, the move builds again and the
    device holds a fresh build's bytes; on the way back the left-out triangle returns, which the host notices before any launch"""
    sc, cam, far = sliver_scene(pkg, product, build=True)
    res = sc.move_camera(far)
    assert res["rebuilt"] == 1 and res["reason"] == "degenerate_set_changed" and res["launches"] == 0
    got = sc.debug_device_digest()
    sf, _, _ = sliver_scene(pkg, product)
    sf.build(far)
    assert got == sf.debug_device_digest() and got == sc.debug_lowering_digest(far) and "degenerate=1" in got[1]
    assert np.isfinite(product.render(sc, far, pkg.make_params(1, "mis", "sobol"))).all()
    res = sc.move_camera(cam)
    assert res["rebuilt"] == 1 and res["reason"] == "degenerate_set_changed"
    assert sc.debug_device_digest() == sc.debug_lowering_digest(cam)
    near = sc.move_camera(moved(pkg, cam, (0.5, 0.0, 0.25)))
    assert near["rebuilt"] == 0
    log_line({"test": "fallback", "there": "degenerate_set_changed", "back": "degenerate_set_changed", "digests_equal_fresh_build": True})


def test_refusals(product, pkg):
    """an unbuilt scene and a scene built over several devices are refused (the latter with a message that says why)"""
    sc, cam = _describe(pkg, product, "1")
    with pytest.raises(RuntimeError, match="code -3.*scene not built"):
        sc.move_camera(cam)
    product.build_multi(sc, cam, [0, 0])
    with pytest.raises(RuntimeError, match="code -1.*mi355pt_scene_build_multi"):
        sc.move_camera(moved(pkg, cam, STEP))
    assert np.isfinite(product.render(sc, cam, pkg.make_params(1, "mis", "sobol"))).all()      # the refusal left the scene as it was


def replay_rebase(product, pkg, dev, frames, step, spp, guide_spp):
    """the calls of `mi355pt --temporal-frames N --camera-step .. --camera-move rebase` through the ABI -> the u8 picture, and the moves' results"""
    import torch
    sc = product.new_scene()
    cam = pkg.scenes.load_scene(sc, 3, W3, H3, build=False)
    d65 = sc.add_lut470(pkg.scenes.presets()["cie_illum_d6500"])
    base = np.array(list(cam.position), F)
    acc, g, prev_cam, moves = None, None, None, []
    for k in range(frames):
        pos = base + F(k) * np.asarray(step, F)
        for i in range(3):
            cam.position[i] = pos[i]
        if k == 0:
            sc.build(cam)
        else:
            moves.append(sc.move_camera(cam))
        f = {n: torch.zeros((H3, W3, 3), dtype=torch.float32, device="cuda") for n in ("film", "position", "shading_normal", "hit")}
        gb = {n: f[n].data_ptr() for n in ("shading_normal", "position", "hit")}
        product.render_gbuffer_accum_device(sc, cam, pkg.make_params(guide_spp, "mis", "sobol", seed=k), d65, 0, guide_spp, gb)
        product.render_accum_device(sc, cam, pkg.make_params(spp, "mis", "sobol", seed=k), 0, spp, f["film"].data_ptr())
        torch.cuda.synchronize()
        prev, view = None, None
        if acc is not None:
            prev = dict(frame_of(g, ("position", "shading_normal", "hit")), film=acc[0], length=acc[2])
            view = product.temporal_view_from_cameras(cam, prev_cam)
        acc = dev.run_device(frame_of(f), spp, prev, view, None)
        g, prev_cam = f, pkg.ffi.Camera.from_buffer_copy(cam)
    rgb = torch.empty_like(acc[0])
    product.film_resolve_device(acc[0].data_ptr(), W3 * H3, 1, rgb.data_ptr())
    torch.cuda.synchronize()
    return product.quantize_u8(rgb.cpu().numpy()), moves


def test_cli_camera_move_rebase(product, pkg, dev, cli, tmp_path):  # noqa: F811
    """`--temporal-frames 3 --camera-step 0.05,0,-0.1 --camera-move rebase` writes the frame of the same calls replayed through the ABI,
    says one line per moved frame on stderr, and leaves the default (rebuild) as it was; misuse exits 2"""
    from PIL import Image
    exe, env = cli
    base = [exe, "--scene", "3", "--renderer", "mis", "--sampler", "sobol", "--spp", str(FRAME_SPP), "--width", str(W3), "--height", str(H3),
            "--denoise-guide-spp", str(GUIDE_SPP), "--temporal-frames", "3", "--camera-step", "0.05,0,-0.1"]
    want, moves = replay_rebase(product, pkg, dev, 3, (0.05, 0.0, -0.1), FRAME_SPP, GUIDE_SPP)
    assert [m["rebuilt"] for m in moves] == [0, 0]
    pictures = {}
    for mode in ("rebase", "rebuild"):
        path = str(tmp_path / f"{mode}.png")
        r = subprocess.run(base + ["--camera-move", mode, "-o", path], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        lines = [ln for ln in r.stderr.splitlines() if ln.startswith("camera move, frame ")]
        assert len(lines) == (2 if mode == "rebase" else 0) and all("rebuilt=0 host_ms=" in ln and " device_ms=" in ln for ln in lines)
        pictures[mode] = np.asarray(Image.open(path).convert("RGB"))
    assert pictures["rebase"].shape == want.shape and np.array_equal(pictures["rebase"], want) and want.mean() > 10.0
    rmse = linear_rmse_u8(pictures["rebase"], pictures["rebuild"])                # another tree per frame: ties only
    log_line({"test": "cli", "rebase_equals_replay": True, "rebase_vs_rebuild_linear_rmse_u8": rmse})
    assert rmse <= 2e-3
    for args in (["--camera-move", "rebase"], ["--temporal-frames", "2", "--camera-move", "sideways"]):
        r = subprocess.run([exe, "--scene", "3", "--renderer", "mis", *args], env=env, capture_output=True, text=True, timeout=60, cwd=tmp_path)
        assert r.returncode == 2 and "--camera-move" in r.stderr, (args, r.returncode, r.stderr)
