"""Moving instances of a built scene on the MI355X (include/mi355pt_instances.h): after mi355pt_scene_move_instances EVERY device array
has the bytes of the host lowering of the updated description over the built tree (mi355pt_scene_debug_device_digest against
mi355pt_scene_debug_pinned_digest, which tests/test_instance_move.py ties to the recorded digests and the tree validator); sah_built and
sah_after are bit-equal to the host's fixed-order sum; the moved scene traces what a scene freshly built from the new matrices traces; the
fallbacks rebuild; the refusals leave the scene as it was.  One line per comparison goes to the file MI355PT_FRAME_LOG names
(profiles/instance_move_parity.jsonl)."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import linear_rmse_u8  # noqa: E402
from test_instance_move import DEGRADING_STEP, EMITTER, ORDINARY, applied, describe, trs  # noqa: E402
from test_rebase import check_exported_tree, moved, sliver_scene  # noqa: E402
from test_rebase_gpu import heights_of, rays_for  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
W, H = 64, 48
# (case, moved instance): one marked dynamic that carries ordinary geometry per scene and family, and the two emitters
MOVES = [(c, ORDINARY[c.partition(":")[0]]) for c in ("3:general", "17", "19", "21", "29", "31", "instanced")] + [(c, EMITTER[c]) for c in ("3", "31")]
CASES = [(c, i, b) for c, i in MOVES for b in ("host", "gpu")]
MOVE_LAUNCHES = 5             # positions, shading records, the 4-wide tree, two for the SAH cost; + one per node height (the header states it)
CAMERA_STEP = (0.3, -0.2, 0.45)


def log_line(line):
    if os.environ.get("MI355PT_FRAME_LOG"):
        with open(os.environ["MI355PT_FRAME_LOG"], "a") as f:
            f.write(json.dumps(line) + "\n")


def is_emitter(case, inst):
    return EMITTER.get(case.partition(":")[0]) == inst


class Redescribed:
    """a backend whose new scenes take other local_to_world matrices for some instance ids while they are described: the way to a scene
    DESCRIBED with a moved transform from the start, through the package's own scene descriptions"""

    def __init__(self, backend, matrices):
        self._backend, self._matrices = backend, matrices

    def __getattr__(self, name):
        return getattr(self._backend, name)

    def new_scene(self):
        sc = self._backend.new_scene()
        add, matrices = sc.add_instance, self._matrices

        def add_instance(geom, mat, local_to_world=None):
            return add(geom, mat, matrices.get(len(sc.instances), local_to_world))
        sc.add_instance = add_instance
        return sc


def describe_with(pkg, product, case, builder, matrices):
    return describe(pkg, Redescribed(product, matrices), case, builder=builder)


def built(pkg, product, case, inst, builder, l2w=None):
    """(scene, camera) with `inst` marked dynamic, built; l2w: described with this matrix for `inst` from the start"""
    sc, cam = describe(pkg, product, case, builder=builder) if l2w is None else describe_with(pkg, product, case, builder, {inst: l2w})
    sc.set_instance_dynamic(inst)
    sc.build(cam)
    return sc, cam


def host_sah(product, sc, cam):
    """the host's fixed-order SAH sum over the tree the DEVICE holds (its exported nodes; the entries follow from the links)"""
    nodes, _, root = product.export_bvh(sc)
    return product.debug_sah_cost(nodes, root, sc.debug_pinned_export(cam)[3])


@pytest.mark.parametrize("case,inst,builder", CASES)
def test_device_bytes_after_a_move(product, pkg, case, inst, builder):
    """the main test: build, give one instance T R S on the left — every device array has the digest of the pinned host lowering; exactly
    the arrays a move can reach differ from the fresh build's; both SAH costs are the host's, bit for bit; the launch count is the
    header's; the same matrices again do nothing; the way back restores the fresh build's bytes and its cost"""
    sc, cam = built(pkg, product, case, inst, builder)
    assert f"builder={builder}" in product.scene_info(sc) and "tri_space=render" in product.scene_info(sc)
    fresh, fresh_info = sc.debug_device_digest()
    assert (fresh, fresh_info) == sc.debug_pinned_digest(cam)                    # the read-back and the kept topology, either builder
    nodes0, tris0, root0 = product.export_bvh(sc)
    sah0 = host_sah(product, sc, cam)
    old = sc.instances[inst][2]
    new = applied(trs(), old)
    res = sc.move_instances(cam, [inst], [new])
    assert res["rebuilt"] == 0 and res["reason"] == "rebased"
    assert res["launches"] == heights_of(nodes0, root0) + MOVE_LAUNCHES
    got, got_info = sc.debug_device_digest()
    want, want_info = sc.debug_pinned_digest(cam)
    differ = [n for n in want if got[n] != want[n]]
    sah1 = host_sah(product, sc, cam)
    log_line({"test": "device_bytes", "case": case, "instance": inst, "builder": builder, "arrays": len(want), "differ": differ, "launches": res["launches"],
              "sah_built": float(res["sah_built"]), "sah_after": float(res["sah_after"]), "sah_bit_equal_host": bool(res["sah_built"] == sah0 and res["sah_after"] == sah1),
              "host_ms": round(res["host_ms"], 3), "device_ms": round(res["device_ms"], 3)})
    assert not differ and got_info == want_info and list(got) == list(fresh)
    changed = {n for n in got if got[n] != fresh[n]}
    must = {"shade", "tris_render", "nodes", "nodes4", "instances"} | ({"lights", "light_tris"} if is_emitter(case, inst) else set())
    # (lights may change without an emitter: a directional light's area follows the scene bounds, scene 21)
    assert must <= changed <= must | {"lights", "light_tris"}, changed
    assert np.float32(res["sah_built"]).tobytes() == np.float32(sah0).tobytes() and np.float32(res["sah_after"]).tobytes() == np.float32(sah1).tobytes()
    assert sah0 > 1.0 and sah1 > 1.0
    nodes1, tris1, root1 = product.export_bvh(sc)
    assert root1 == root0 and np.array_equal(nodes1[:, 12:16], nodes0[:, 12:16]) and np.array_equal(tris1[:, 9:], tris0[:, 9:])
    check_exported_tree(nodes1, tris1, root1)
    assert np.isfinite(product.render(sc, cam, pkg.make_params(1, "mis", "sobol"))).all()
    again = sc.move_instances(cam, [inst], [new])
    assert again["reason"] == "same_transforms" and again["rebuilt"] == 0 and again["launches"] == 0
    assert sc.debug_device_digest()[0] == got
    back = sc.move_instances(cam, [inst], [old])
    assert back["rebuilt"] == 0 and back["reason"] == "rebased"
    home = sc.debug_device_digest()[0]
    differ = [n for n in home if home[n] != fresh[n]]
    log_line({"test": "round_trip", "case": case, "instance": inst, "builder": builder, "differ": differ,
              "sah_restored": bool(back["sah_after"] == back["sah_built"] == res["sah_built"])})
    assert not differ
    assert np.float32(back["sah_after"]).tobytes() == np.float32(back["sah_built"]).tobytes() == np.float32(res["sah_built"]).tobytes()


@pytest.mark.parametrize("case,inst,builder", [("3:general", 1, "host"), ("17", 0, "gpu"), ("31", 7, "host")])
def test_partial_moves_are_one_move(product, pkg, case, inst, builder):
    """three partial moves leave the bytes of one move to the end pose: nothing is incremental"""
    sc, cam = built(pkg, product, case, inst, builder)
    old = sc.instances[inst][2]
    end = applied(trs(), old)
    for k in (1, 2):
        part = applied(trs((0.1 * k, -0.07 * k, 0.15 * k), 0.13 * k, (1.0 + 0.03 * k, 1.0 - 0.03 * k, 1.0)), old)
        assert sc.move_instances(cam, [inst], [part])["rebuilt"] == 0
    last = sc.move_instances(cam, [inst], [end])
    chained = sc.debug_device_digest()[0]
    sc2, _ = built(pkg, product, case, inst, builder)
    once = sc2.move_instances(cam, [inst], [end])
    assert once["rebuilt"] == 0 and sc2.debug_device_digest()[0] == chained == sc.debug_pinned_digest(cam)[0]
    assert np.float32(last["sah_after"]).tobytes() == np.float32(once["sah_after"]).tobytes()
    log_line({"test": "partial_moves", "case": case, "instance": inst, "builder": builder, "equal": True})


@pytest.mark.parametrize("case,inst,builder", [("3", 7, "host"), ("31", 7, "gpu"), ("17", 0, "host"), ("instanced", 2, "gpu")])
def test_camera_move_after_an_instance_move(product, pkg, case, inst, builder):
    """an instance move followed by mi355pt_scene_move_camera gives the pinned lowering for the new camera — for the emitters this holds
    the light caches the camera move starts from to the moved areas —, and the other order gives the same bytes"""
    sc, cam = built(pkg, product, case, inst, builder)
    new = applied(trs(), sc.instances[inst][2])
    assert sc.move_instances(cam, [inst], [new])["rebuilt"] == 0
    cam2 = moved(pkg, cam, CAMERA_STEP)
    res = sc.move_camera(cam2)
    assert res["rebuilt"] == 0 and res["reason"] == "rebased"
    got = sc.debug_device_digest()
    want = sc.debug_pinned_digest(cam2)
    differ = [n for n in want[0] if got[0][n] != want[0][n]]
    log_line({"test": "instance_then_camera", "case": case, "instance": inst, "builder": builder, "differ": differ})
    assert not differ and got[1] == want[1]
    with pytest.raises(RuntimeError, match="code -1.*camera position differs"):
        sc.move_instances(cam, [inst], [new])                                    # the scene is at cam2 now
    sc2, _ = built(pkg, product, case, inst, builder)
    assert sc2.move_camera(cam2)["rebuilt"] == 0 and sc2.move_instances(cam2, [inst], [new])["rebuilt"] == 0
    assert sc2.debug_device_digest() == got
    assert np.isfinite(product.render(sc, cam2, pkg.make_params(1, "mis", "sobol"))).all()


@pytest.mark.parametrize("case,inst,builder", CASES)
def test_moved_scene_against_a_fresh_build(product, pkg, case, inst, builder):
    """a moved scene against a scene DESCRIBED with the new matrix (same dynamic mark) and built — another tree over the same triangles:
    the same hit / miss pattern and bit-equal t on every probe ray, equal any-hit answers, the G-buffer's hit.x bit-equal on >= 0.9999 of
    the pixels, the film at 16 spp bit-equal where the two scenes' device digests are equal, else within linear_rmse_u8 2e-3 (the bars of
    tests/test_rebase_gpu.py and tests/test_bvh_gpu.py between two trees); all three strategies where an emitter moved"""
    import torch
    sa, cam = built(pkg, product, case, inst, builder)
    new = applied(trs(), sa.instances[inst][2])
    assert sa.move_instances(cam, [inst], [new])["rebuilt"] == 0
    sb, _ = built(pkg, product, case, inst, builder, l2w=new)
    da, db = sa.debug_device_digest()[0], sb.debug_device_digest()[0]
    for name in ("instances", "lights", "light_tris", "materials", "texels", "rgb2spec"):          # tree-order-free arrays: the same description
        assert da[name] == db[name], name
    _, tris, _ = product.export_bvh(sb)
    o, d = rays_for(tris)
    ta, _, _, _ = sa.probe_intersect(o, d)
    tb, _, _, _ = sb.probe_intersect(o, d)
    assert np.array_equal(ta >= 0, tb >= 0) and np.array_equal(ta.view(np.uint32), tb.view(np.uint32))
    assert (tb >= 0).sum() >= 32 and (tb < 0).any()
    tm = np.where(tb >= 0, tb * F(1.5), F(10.0)).astype(F) * np.random.default_rng(9).uniform(0.3, 1.2, tb.shape).astype(F)
    assert np.array_equal(sa.probe_occluded(o, d, tm), sb.probe_occluded(o, d, tm))
    share = []
    for sc in (sa, sb):
        buf = torch.zeros((2, H, W, 3), dtype=torch.float32, device="cuda")
        product.render_gbuffer_accum_device(sc, cam, pkg.make_params(1, "mis", "sobol"), 0, 0, 1, {"position": buf[0].data_ptr(), "hit": buf[1].data_ptr()})
        torch.cuda.synchronize()
        share.append(buf[1].cpu().numpy()[..., 0].view(np.uint32))
    hit_share = float((share[0] == share[1]).mean())
    assert hit_share >= 0.9999, hit_share
    same_bytes = da == db
    for strategy in (("mis", "nee", "pt") if is_emitter(case, inst) else ("mis",)):
        prm = pkg.make_params(16, strategy, "sobol")
        img_a, img_b = product.render(sa, cam, prm), product.render(sb, cam, prm)
        rmse = linear_rmse_u8(product.quantize_u8(img_a), product.quantize_u8(img_b))
        log_line({"test": "moved_vs_fresh", "case": case, "instance": inst, "builder": builder, "strategy": strategy, "rays": int(o.shape[0]),
                  "t_bit_equal": True, "occluded_equal": True, "gbuffer_hit_x_bit_equal": round(hit_share, 6), "device_digests_equal": bool(same_bytes),
                  "film_bit_equal": bool(np.array_equal(img_a, img_b)), "linear_rmse_u8": rmse})
        assert img_a.mean() > 0.0
        if same_bytes:
            assert np.array_equal(img_a, img_b)
        else:
            assert rmse <= 2e-3, (strategy, rmse)


@pytest.mark.parametrize("inst", [1, 7])
def test_translation_of_a_pure_translation_instance(product, pkg, inst):
    """3:no_local_tris: a translation given to an instance that is NOT marked dynamic keeps its class, so the move is in place — the box
    and the emitter (whose world-space areas change in float32 under a translation, and with them cdf and light_pdf_area)"""
    sc, cam = describe(pkg, product, "3:no_local_tris", builder="host")
    sc.build(cam)
    fresh = sc.debug_device_digest()[0]
    old = sc.instances[inst][2]
    new = applied(trs((0.3, -0.2, 0.45), 0.0, (1.0, 1.0, 1.0)), old)
    res = sc.move_instances(cam, [inst], [new])
    assert res["rebuilt"] == 0 and res["reason"] == "rebased"
    got, want = sc.debug_device_digest(), sc.debug_pinned_digest(cam)
    assert got == want and got[0]["tris_render"] != fresh["tris_render"] and got[0]["instances"] != fresh["instances"]
    if inst == 7:
        assert got[0]["light_tris"] != fresh["light_tris"]
    assert sc.move_instances(cam, [inst], [old])["rebuilt"] == 0 and sc.debug_device_digest()[0] == fresh
    log_line({"test": "pure_translation", "instance": inst, "equal": True})


def test_fallbacks(product, pkg):
    """each fallback ends with the device digest equal to debug_lowering_digest(cam) of the updated description: a rotation on a pure-
    translation instance that is not dynamic; any move in plain scene 3 (local-triangle mode); a scale that collapses the sliver; and
    rebuild_above = 1.0 with the hero of scene 17 carried to the pose tests/test_instance_move.py found to cost more than the build"""
    def check(sc, cam, inst, new, reason, **kw):
        res = sc.move_instances(cam, [inst], [new], **kw)
        assert res["rebuilt"] == 1 and res["reason"] == reason and res["launches"] == 0 and res["sah_after"] == 0.0, res
        got = sc.debug_device_digest()
        twin = sc.debug_pinned_digest(cam)                                       # the rebuilt scene's own tree, unchanged transforms
        assert got == twin
        log_line({"test": "fallback", "reason": reason, "digests_equal_fresh_lowering": True})
        return got

    sc, cam = describe(pkg, product, "3:no_local_tris", builder="host"); sc.build(cam)
    new = applied(trs(), sc.instances[1][2])
    got = check(sc, cam, 1, new, "instance_class_changed")
    s2, _ = describe_with(pkg, product, "3:no_local_tris", "host", {1: new})
    assert got == s2.debug_lowering_digest(cam)

    sc, cam = describe(pkg, product, "3", builder="host"); sc.build(cam)
    new = applied(trs((0.1, 0.0, 0.0), 0.0, (1.0, 1.0, 1.0)), sc.instances[1][2])
    got = check(sc, cam, 1, new, "instance_class_changed")
    s2, _ = describe_with(pkg, product, "3", "host", {1: new})
    assert got == s2.debug_lowering_digest(cam) and "tri_space=render" in got[1]

    sc, cam, _ = sliver_scene(pkg, product)
    sc.set_instance_dynamic(0); sc.build(cam)
    assert "degenerate=0" in product.scene_info(sc)
    # x and y scaled by 1e-19: the sliver's 1e-5 edges lie in that plane and the square of their product underflows to zero, while the
    # matrix still has a float32 inverse (determinant 1e-38) — the host finds nothing (no triangle was left out), the device counts
    collapse = np.diag([1e-19, 1e-19, 1.0, 1.0]).astype(F)
    res = sc.move_instances(cam, [0], [collapse])
    assert res["rebuilt"] == 1 and res["reason"] == "degenerate_set_changed" and res["launches"] == 0
    assert "degenerate=" in product.scene_info(sc) and "degenerate=0" not in product.scene_info(sc)
    s2, _, _ = sliver_scene(pkg, Redescribed(product, {0: collapse})); s2.set_instance_dynamic(0)
    assert sc.debug_device_digest() == sc.debug_pinned_digest(cam) == s2.debug_lowering_digest(cam)
    log_line({"test": "fallback", "reason": "degenerate_set_changed", "digests_equal_fresh_lowering": True})

    sc, cam = built(pkg, product, "17", 0, "host")
    new = applied(trs(DEGRADING_STEP, 0.0, (1.0, 1.0, 1.0)), sc.instances[0][2])
    got = check(sc, cam, 0, new, "sah_degraded", rebuild_above=1.0)
    s2, _ = describe_with(pkg, product, "17", "host", {0: new}); s2.set_instance_dynamic(0)
    assert got == s2.debug_lowering_digest(cam)
    sc, cam = built(pkg, product, "17", 0, "host")                               # the same pose without the threshold stays in place
    res = sc.move_instances(cam, [0], [new])
    assert res["rebuilt"] == 0 and res["sah_after"] > res["sah_built"]


def test_refusals(product, pkg):
    """a wrong camera position, ids out of range or out of order, a singular or non-finite matrix, the mark on a built scene, a scene built
    over several devices: refused with MI355PT_E_INVALID, the scene rendering as before"""
    sc, cam = built(pkg, product, "3:general", 1, "host")
    prm = pkg.make_params(1, "mis", "sobol")
    before = product.render(sc, cam, prm)
    digest = sc.debug_device_digest()
    old = sc.instances[1][2]
    ok = applied(trs(), old)
    singular = ok.copy(); singular[:3, 1] = 0.0
    nan = ok.copy(); nan[0, 3] = np.nan
    for ids, ms, cam_x, msg in (([1], [ok], moved(pkg, cam, CAMERA_STEP), "camera position differs"), ([99], [ok], cam, "bad instance id"),
                                ([2, 1], [ok, ok], cam, "strictly ascending"), ([1, 1], [ok, ok], cam, "strictly ascending"),
                                ([1], [singular], cam, "singular"), ([1], [nan], cam, "singular")):
        with pytest.raises(RuntimeError, match="code -1.*" + msg):
            sc.move_instances(cam_x, ids, ms)
    with pytest.raises(RuntimeError, match="code -1.*before mi355pt_scene_build"):
        sc.set_instance_dynamic(2)
    assert sc.debug_device_digest() == digest and np.array_equal(product.render(sc, cam, prm), before)
    s2, cam2 = describe(pkg, product, "1")
    product.build_multi(s2, cam2, [0, 0])
    with pytest.raises(RuntimeError, match="code -1.*mi355pt_scene_build_multi"):
        s2.move_instances(cam2, [0], [np.eye(4, dtype=F)])
    assert np.isfinite(product.render(s2, cam2, prm)).all()
    log_line({"test": "refusals", "scene_unchanged": True})


# ---------------- the CLI ----------------
@pytest.fixture(scope="module")
def cli(pkg, tmp_path_factory):
    import subprocess
    root = pkg.ffi.ROOT
    exe = os.path.join(root, "toy-cpu-pathtracing_amd", "host", "mi355pt")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.dirname(exe)])
    assets_dir = str(tmp_path_factory.mktemp("assets"))
    subprocess.check_call([sys.executable, os.path.join(root, "tools", "export_assets.py"), assets_dir])
    return exe, dict(os.environ, MI355PT_ASSETS=assets_dir, MI355PT_DATA=os.path.join(root, "toy-cpu-pathtracing_amd", "data"))


def cli_matrix(t, ry_deg, s, l2w):
    """host/main.cpp instance_transform_matrix: T R_y S composed in double (libm's cos / sin) and rounded to float32, times local_to_world"""
    import math
    a = ry_deg * (math.pi / 180.0)
    c, sn = math.cos(a), math.sin(a)
    x = np.eye(4)
    x[:3, :3] = np.array([[c, 0.0, sn], [0.0, 1.0, 0.0], [-sn, 0.0, c]]) * np.asarray(s, np.float64)[None, :]
    x[:3, 3] = np.asarray(t, F)
    return applied(x.astype(F), l2w)


def test_cli_instance_transform(product, pkg, cli, tmp_path):
    """`--instance-transform` (twice: the box with T R S, the emitter with a translation) writes the picture of the same calls replayed
    through the ABI, u8-equal, within linear_rmse_u8 2e-3 of a scene DESCRIBED with the moved transforms from the start, and says one line
    on stderr; an AOV renderer takes the flag too; misuse exits 2 with the flag's name, and so does the combination with --temporal-frames"""
    import subprocess
    from PIL import Image
    exe, env = cli
    spp = 16
    base = [exe, "--scene", "3", "--sampler", "sobol", "--spp", str(spp), "--width", str(W), "--height", str(H)]
    moves = ["--instance-transform", "7:0.125,0,-0.25", "--instance-transform", "1:0.25,-0.125,0.5:25:1.25,0.75,1"]      # (given out of order: the CLI sorts)
    path = str(tmp_path / "moved.png")
    r = subprocess.run(base + ["--renderer", "mis"] + moves + ["-o", path], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = [ln for ln in r.stderr.splitlines() if ln.startswith("instance move: ")]
    assert len(lines) == 1 and "rebuilt=0 reason=0 launches=" in lines[0] and " sah=" in lines[0] and "→" in lines[0] and " host_ms=" in lines[0] and " device_ms=" in lines[0]
    got = np.asarray(Image.open(path).convert("RGB"))

    def scene(backend):
        sc = backend.new_scene()
        cam = pkg.scenes.load_scene(sc, 3, W, H, build=False)
        sc.set_instance_dynamic(1); sc.set_instance_dynamic(7)
        return sc, cam
    sc, cam = scene(product)
    m1 = cli_matrix((0.25, -0.125, 0.5), 25.0, (1.25, 0.75, 1.0), sc.instances[1][2])
    m7 = cli_matrix((0.125, 0.0, -0.25), 0.0, (1.0, 1.0, 1.0), sc.instances[7][2])
    sc.build(cam)
    res = sc.move_instances(cam, [1, 7], [m1, m7])
    assert res["rebuilt"] == 0
    prm = pkg.make_params(spp, "mis", "sobol")
    want = product.quantize_u8(product.render(sc, cam, prm))
    assert got.shape == want.shape and np.array_equal(got, want) and want.mean() > 10.0
    s2, _ = scene(Redescribed(product, {1: m1, 7: m7}))
    s2.build(cam)
    rmse = linear_rmse_u8(got, product.quantize_u8(product.render(s2, cam, prm)))
    plain = subprocess.run(base + ["--renderer", "mis", "-o", str(tmp_path / "plain.png")], env=env, capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0 and "instance move" not in plain.stderr
    moved_by = linear_rmse_u8(got, np.asarray(Image.open(str(tmp_path / "plain.png")).convert("RGB")))
    log_line({"test": "cli", "equals_replay": True, "vs_described_moved_linear_rmse_u8": rmse, "vs_unmoved_linear_rmse_u8": moved_by})
    assert rmse <= 2e-3 and moved_by > 10 * 2e-3                                  # ... and the move is visible in the picture
    r = subprocess.run(base + ["--renderer", "normal"] + moves + ["-o", str(tmp_path / "n.png")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "instance move: rebuilt=0" in r.stderr, r.stderr
    for args, flag in ((["--instance-transform", "1:0.1,0"], "--instance-transform"), (["--instance-transform", "x:0,0,0"], "--instance-transform"),
                       (["--instance-transform", "1:0,0,0:30:1,2"], "--instance-transform"), (["--instance-transform", "99:0,0,0"], "--instance-transform"),
                       (["--instance-transform", "1:0,0,0", "--instance-transform", "1:1,0,0"], "--instance-transform"),
                       (["--instance-rebuild-above", "1.5"], "--instance-rebuild-above"), (["--instance-transform", "1:0,0,0", "--instance-rebuild-above", "-1"], "--instance-rebuild-above"),
                       (["--instance-transform", "1:0,0,0", "--temporal-frames", "2", "--denoise-guide-spp", "4"], "--temporal-frames")):
        r = subprocess.run(base + ["--renderer", "mis", *args], env=env, capture_output=True, text=True, timeout=120, cwd=tmp_path)
        assert r.returncode == 2 and flag in r.stderr, (args, r.returncode, r.stderr)
