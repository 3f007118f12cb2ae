"""Deforming meshes of a built scene on the MI355X (include/mi355pt_deform.h): after mi355pt_scene_deform_meshes EVERY device array has
the bytes of the host lowering of the updated description over the built tree (mi355pt_scene_debug_device_digest against
mi355pt_scene_debug_pinned_digest, which tests/test_deform.py ties to the tree validator and to a fresh lowering of the deformed
description); sah_built and sah_after are bit-equal to the host's fixed-order sum; deformations compose with each other, with camera moves
and with instance moves; the deformed scene traces what a scene freshly built from the deformed mesh traces; the fallbacks rebuild; the
refusals leave the scene as it was.  One line per comparison goes to the file MI355PT_FRAME_LOG names (profiles/deform_parity.jsonl)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geometry_stress as gs  # noqa: E402
from conftest import linear_rmse_u8  # noqa: E402
from test_deform import EMITTER3, EMITTER31, HERO17, SHARED, WALL, Remeshed, arrays_of, deformed  # noqa: E402
from test_instance_move import applied, describe, trs  # noqa: E402
from test_rebase import check_exported_tree, moved  # noqa: E402
from test_rebase_gpu import heights_of, rays_for  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
W, H = 64, 48
# (case, deformed mesh): a wall and the emitter of scene 3 in its default lowering (the local-triangle mode), the box in the general lowering,
# the 20 k-triangle hero, the textured emitter, the mesh five instances share, and one soup on each side of the GPU builder's 1024-triangle
# workgroup
DEFORMS = [WALL, EMITTER3, ("3:general", 1), HERO17, EMITTER31, SHARED, ("soup1023", 0), ("soup1025", 0)]
CASES = [(c, g, b) for c, g in DEFORMS for b in ("host", "gpu")]
DEFORM_LAUNCHES = 6           # local records, positions, shading records, the 4-wide tree, two for the SAH cost; + one per node height (the header states it)
CAMERA_STEP = (0.3, -0.2, 0.45)


def log_line(line):
    if os.environ.get("MI355PT_FRAME_LOG"):
        with open(os.environ["MI355PT_FRAME_LOG"], "a") as f:
            f.write(json.dumps(line) + "\n")


def is_emitter(case, geom):
    return (case.partition(":")[0], geom) in (EMITTER3, EMITTER31)


def built(pkg, product, case, builder, replace=None, dynamic=()):
    """(scene, camera) built; replace: described with these vertex arrays for some meshes from the start; sc.meshes holds what was given"""
    sc, cam = describe(pkg, Remeshed(product, replace), case, dynamic=dynamic, builder=builder)
    sc.build(cam)
    return sc, cam


def host_sah(product, sc, cam):
    """the host's fixed-order SAH sum over the tree the DEVICE holds (its exported nodes; the entries follow from the links)"""
    nodes, _, root = product.export_bvh(sc)
    return product.debug_sah_cost(nodes, root, sc.debug_pinned_export(cam)[3])


def bits(x):
    return np.float32(x).tobytes()


@pytest.mark.parametrize("case,geom,builder", CASES)
def test_device_bytes_after_a_deformation(product, pkg, case, geom, builder):
    """the main test: build, give one mesh a smooth displacement of positions, normals and (with uv) tangents — every device array has the
    digest of the pinned host lowering; exactly the arrays a deformation can reach differ from the fresh build's; both SAH costs are the
    host's, bit for bit; the launch count is the header's; the same arrays again do nothing; the old arrays restore the fresh build's bytes
    and its cost"""
    sc, cam = built(pkg, product, case, builder)
    info = product.scene_info(sc)
    assert f"builder={builder}" in info and ("tri_space=local" in info) == (case in ("3", "31", "soup1023", "soup1025"))
    fresh, fresh_info = sc.debug_device_digest()
    assert (fresh, fresh_info) == sc.debug_pinned_digest(cam)                    # the read-back and the kept topology, either builder
    nodes0, tris0, root0 = product.export_bvh(sc)
    sah0 = host_sah(product, sc, cam)
    new = deformed(sc.meshes[geom])
    assert (new[2] is not None) == (sc.meshes[geom].get("uv") is not None)
    res = sc.deform_meshes(cam, {geom: new})
    assert res["rebuilt"] == 0 and res["reason"] == "rebased"
    assert res["launches"] == heights_of(nodes0, root0) + DEFORM_LAUNCHES
    got, got_info = sc.debug_device_digest()
    want, want_info = sc.debug_pinned_digest(cam)
    differ = [n for n in want if got[n] != want[n]]
    sah1 = host_sah(product, sc, cam)
    log_line({"test": "device_bytes", "case": case, "geom": geom, "builder": builder, "arrays": len(want), "differ": differ, "launches": res["launches"],
              "sah_built": float(res["sah_built"]), "sah_after": float(res["sah_after"]), "sah_bit_equal_host": bool(res["sah_built"] == sah0 and res["sah_after"] == sah1),
              "host_ms": round(res["host_ms"], 3), "device_ms": round(res["device_ms"], 3)})
    assert not differ and got_info == want_info and list(got) == list(fresh)
    changed = {n for n in got if got[n] != fresh[n]}
    # the reachable set: the local and the render triangle arrays, the shading records, both trees; the light records where an emitter
    # deformed (lights may change without one where a directional light's area follows the scene bounds: none of these scenes has one)
    must = {"tris_local", "tris_render", "shade", "nodes", "nodes4"} | ({"lights", "light_tris"} if is_emitter(case, geom) else set())
    assert must <= changed <= must | {"lights", "light_tris"}, changed
    assert bits(res["sah_built"]) == bits(sah0) and bits(res["sah_after"]) == bits(sah1)
    assert sah0 > 1.0 and sah1 > 1.0
    nodes1, tris1, root1 = product.export_bvh(sc)
    assert root1 == root0 and np.array_equal(nodes1[:, 12:16], nodes0[:, 12:16]) and np.array_equal(tris1[:, 9:], tris0[:, 9:])
    check_exported_tree(nodes1, tris1, root1)
    assert np.isfinite(product.render(sc, cam, pkg.make_params(1, "mis", "sobol"))).all()
    again = sc.deform_meshes(cam, {geom: new})
    assert again["reason"] == "same_vertices" and again["rebuilt"] == 0 and again["launches"] == 0
    assert sc.debug_device_digest()[0] == got
    back = sc.deform_meshes(cam, {geom: arrays_of(sc.meshes[geom])})
    assert back["rebuilt"] == 0 and back["reason"] == "rebased"
    home = sc.debug_device_digest()[0]
    differ = [n for n in home if home[n] != fresh[n]]
    log_line({"test": "round_trip", "case": case, "geom": geom, "builder": builder, "differ": differ,
              "sah_restored": bool(back["sah_after"] == back["sah_built"] == res["sah_built"])})
    assert not differ
    assert bits(back["sah_after"]) == bits(back["sah_built"]) == bits(res["sah_built"])


@pytest.mark.parametrize("case,geom,builder", [("3", 2, "host"), ("17", 0, "gpu"), ("31", 7, "host")])
def test_partial_deformations_are_one_deformation(product, pkg, case, geom, builder):
    """two partial deformations followed by the final one leave the bytes of the final one alone, and a call that names two meshes leaves
    the bytes of two calls: nothing is incremental"""
    sc, cam = built(pkg, product, case, builder)
    end = deformed(sc.meshes[geom])
    for k in (1, 2):
        assert sc.deform_meshes(cam, {geom: deformed(sc.meshes[geom], seed=10 + k, amp=0.01 * k)})["rebuilt"] == 0
    last = sc.deform_meshes(cam, {geom: end})
    chained = sc.debug_device_digest()[0]
    sc2, _ = built(pkg, product, case, builder)
    once = sc2.deform_meshes(cam, {geom: end})
    assert once["rebuilt"] == 0 and sc2.debug_device_digest()[0] == chained == sc.debug_pinned_digest(cam)[0]
    assert bits(last["sah_after"]) == bits(once["sah_after"])
    other = 1 if geom != 1 else 2
    both = {geom: end, other: deformed(sc.meshes[other], seed=5)}
    assert sc.deform_meshes(cam, {other: both[other]})["rebuilt"] == 0
    sc3, _ = built(pkg, product, case, builder)
    assert sc3.deform_meshes(cam, both)["rebuilt"] == 0
    assert sc3.debug_device_digest()[0] == sc.debug_device_digest()[0] == sc.debug_pinned_digest(cam)[0]
    log_line({"test": "partial_deformations", "case": case, "geom": geom, "builder": builder, "equal": True})


@pytest.mark.parametrize("case,geom,builder", [("3", 7, "host"), ("31", 7, "gpu"), ("17", 0, "host"), ("instanced", 0, "gpu")])
def test_camera_move_and_deformation_commute(product, pkg, case, geom, builder):
    """a deformation followed by mi355pt_scene_move_camera gives the pinned lowering for the new camera — for the emitters this holds the
    light caches the camera move starts from to the deformed areas —, and the other order gives the same bytes"""
    sc, cam = built(pkg, product, case, builder)
    new = deformed(sc.meshes[geom])
    assert sc.deform_meshes(cam, {geom: new})["rebuilt"] == 0
    cam2 = moved(pkg, cam, CAMERA_STEP)
    res = sc.move_camera(cam2)
    assert res["rebuilt"] == 0 and res["reason"] == "rebased"
    got = sc.debug_device_digest()
    want = sc.debug_pinned_digest(cam2)
    differ = [n for n in want[0] if got[0][n] != want[0][n]]
    log_line({"test": "deform_then_camera", "case": case, "geom": geom, "builder": builder, "differ": differ})
    assert not differ and got[1] == want[1]
    with pytest.raises(RuntimeError, match="code -1.*camera position differs"):
        sc.deform_meshes(cam, {geom: arrays_of(sc.meshes[geom])})                # the scene is at cam2 now
    sc2, _ = built(pkg, product, case, builder)
    assert sc2.move_camera(cam2)["rebuilt"] == 0 and sc2.deform_meshes(cam2, {geom: new})["rebuilt"] == 0
    assert sc2.debug_device_digest() == got
    assert np.isfinite(product.render(sc, cam2, pkg.make_params(1, "mis", "sobol"))).all()


@pytest.mark.parametrize("case,geom,inst,builder", [("3", 1, 1, "host"), ("31", 7, 7, "gpu"), ("17", 0, 0, "gpu"), ("instanced", 0, 2, "host")])
def test_instance_move_and_deformation_commute(product, pkg, case, geom, inst, builder):
    """a deformation followed by mi355pt_scene_move_instances of an instance of that mesh (marked dynamic before the build) gives the
    pinned lowering of the description that holds both, and the other order gives the same bytes"""
    sc, cam = built(pkg, product, case, builder, dynamic=[inst])
    assert sc.instances[inst][0] == geom
    new = deformed(sc.meshes[geom])
    l2w = applied(trs(), sc.instances[inst][2])
    assert sc.deform_meshes(cam, {geom: new})["rebuilt"] == 0
    res = sc.move_instances(cam, [inst], [l2w])
    assert res["rebuilt"] == 0 and res["reason"] == "rebased"
    got = sc.debug_device_digest()
    want = sc.debug_pinned_digest(cam)
    differ = [n for n in want[0] if got[0][n] != want[0][n]]
    log_line({"test": "deform_then_instance", "case": case, "geom": geom, "instance": inst, "builder": builder, "differ": differ})
    assert not differ and got[1] == want[1]
    sc2, _ = built(pkg, product, case, builder, dynamic=[inst])
    assert sc2.move_instances(cam, [inst], [l2w])["rebuilt"] == 0 and sc2.deform_meshes(cam, {geom: new})["rebuilt"] == 0
    assert sc2.debug_device_digest() == got
    assert np.isfinite(product.render(sc, cam, pkg.make_params(1, "mis", "sobol"))).all()


@pytest.mark.parametrize("case,geom,builder", CASES)
def test_deformed_scene_against_a_fresh_build(product, pkg, case, geom, builder):
    """a deformed scene against a scene DESCRIBED with the deformed mesh and built — another tree over the same triangles: the same hit /
    miss pattern and bit-equal t on every probe ray, equal any-hit answers, the G-buffer's hit.x bit-equal on >= 0.9999 of the pixels, the
    film at 16 spp bit-equal where the two scenes' device digests are equal, else within linear_rmse_u8 2e-3 (the bars of
    tests/test_instance_move_gpu.py between two trees); all three strategies where the emitter deformed"""
    import torch
    sa, cam = built(pkg, product, case, builder)
    new = deformed(sa.meshes[geom])
    assert sa.deform_meshes(cam, {geom: new})["rebuilt"] == 0
    sb, _ = built(pkg, product, case, builder, replace={geom: new})
    da, db = sa.debug_device_digest()[0], sb.debug_device_digest()[0]
    for name in ("instances", "lights", "light_tris", "light_uvs", "materials", "texels", "rgb2spec"):     # tree-order-free arrays: the same description
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
    for strategy in (("mis", "nee", "pt") if is_emitter(case, geom) else ("mis",)):
        prm = pkg.make_params(16, strategy, "sobol")
        img_a, img_b = product.render(sa, cam, prm), product.render(sb, cam, prm)
        rmse = linear_rmse_u8(product.quantize_u8(img_a), product.quantize_u8(img_b))
        log_line({"test": "deformed_vs_fresh", "case": case, "geom": geom, "builder": builder, "strategy": strategy, "rays": int(o.shape[0]),
                  "t_bit_equal": True, "occluded_equal": True, "gbuffer_hit_x_bit_equal": round(hit_share, 6), "device_digests_equal": bool(same_bytes),
                  "film_bit_equal": bool(np.array_equal(img_a, img_b)), "linear_rmse_u8": rmse})
        assert img_a.mean() > 0.0
        if same_bytes:
            assert np.array_equal(img_a, img_b)
        else:
            assert rmse <= 2e-3, (strategy, rmse)


def collapsed(mesh, tri=0):
    """the mesh with the three corners of one triangle at one point (the soups have unshared vertices: no other triangle changes)"""
    pos, nrm, tan = arrays_of(mesh)
    pos = pos.copy()
    idx = np.asarray(mesh["idx"], np.uint32).reshape(-1, 3)[tri]
    pos[idx[1]] = pos[idx[0]]; pos[idx[2]] = pos[idx[0]]
    return pos, nrm, tan


@pytest.mark.parametrize("lowering", ["auto", "general"])
def test_fallback_when_the_degenerate_set_changes(product, pkg, lowering):
    """one triangle collapsed to a point rebuilds — found by the host on the local vertices in local-triangle mode, by the device's counter
    on the render-space vertices otherwise —, and so does the way back, where a triangle the tree left out stops being degenerate; after
    either the device holds a fresh build of the updated description"""
    def scene(replace=None):
        sc, cam = describe(pkg, Remeshed(product, replace), "soup1025", builder="host")
        sc.debug_set_lowering(lowering)
        return sc, cam
    sc, cam = scene()
    sc.build(cam)
    assert "degenerate=0" in product.scene_info(sc) and ("tri_space=local" in product.scene_info(sc)) == (lowering == "auto")
    flat = collapsed(sc.meshes[0], tri=17)
    res = sc.deform_meshes(cam, {0: flat})
    assert res["rebuilt"] == 1 and res["reason"] == "degenerate_set_changed" and res["launches"] == 0 and res["sah_after"] == 0.0, res
    assert "degenerate=1" in product.scene_info(sc)
    s2, _ = scene({0: flat})
    assert sc.debug_device_digest() == sc.debug_pinned_digest(cam) == s2.debug_lowering_digest(cam)
    res = sc.deform_meshes(cam, {0: arrays_of(sc.meshes[0])})
    assert res["rebuilt"] == 1 and res["reason"] == "degenerate_set_changed" and "degenerate=0" in product.scene_info(sc)
    s3, _ = scene()
    assert sc.debug_device_digest() == s3.debug_lowering_digest(cam)
    log_line({"test": "fallback", "reason": "degenerate_set_changed", "lowering": lowering, "digests_equal_fresh_lowering": True})


def test_fallback_when_the_tree_degrades(product, pkg):
    """the hero of scene 17 scattered — every vertex displaced by noise of 30 % of the mesh's extent, so that neighbouring triangles no
    longer lie together and the boxes of the built tree overlap —: without a threshold the refit stays and reports a cost above the
    built tree's; with rebuild_above just under that measured ratio the call builds again, and the device then holds a fresh build"""
    sc, cam = built(pkg, product, "17", "host")
    pos, nrm, tan = arrays_of(sc.meshes[0])
    ext = float((pos.max(axis=0) - pos.min(axis=0)).max())
    noise = np.random.default_rng(3).uniform(-0.3 * ext, 0.3 * ext, pos.shape)
    scattered = ((pos + noise).astype(F), nrm, tan)
    res = sc.deform_meshes(cam, {0: scattered})
    assert res["rebuilt"] == 0 and res["reason"] == "rebased" and res["sah_after"] > res["sah_built"] > 1.0
    ratio = float(res["sah_after"]) / float(res["sah_built"])
    assert sc.debug_device_digest() == sc.debug_pinned_digest(cam)
    sc2, _ = built(pkg, product, "17", "host")
    again = sc2.deform_meshes(cam, {0: scattered}, rebuild_above=ratio * 1.001)                  # just above the ratio: stays
    assert again["rebuilt"] == 0 and bits(again["sah_after"]) == bits(res["sah_after"])
    sc3, _ = built(pkg, product, "17", "host")
    res3 = sc3.deform_meshes(cam, {0: scattered}, rebuild_above=ratio * 0.999)                   # just under it: builds again
    assert res3["rebuilt"] == 1 and res3["reason"] == "sah_degraded" and res3["launches"] == 0 and res3["sah_after"] == 0.0, res3
    s4, _ = describe(pkg, Remeshed(product, {0: scattered}), "17", builder="host")
    assert sc3.debug_device_digest() == sc3.debug_pinned_digest(cam) == s4.debug_lowering_digest(cam)
    log_line({"test": "fallback", "reason": "sah_degraded", "ratio": ratio, "digests_equal_fresh_lowering": True})


def test_refusals(product, pkg):
    """a wrong camera position, bad ids, a tangent without uv, a non-finite position, a scene built over several devices, another current
    device: refused, the scene and its description as they were"""
    import torch
    sc, cam = built(pkg, product, "3", "host")
    prm = pkg.make_params(1, "mis", "sobol")
    before = product.render(sc, cam, prm)
    digest = sc.debug_device_digest()
    new = deformed(sc.meshes[1])
    bad = new[0].copy(); bad[3, 0] = np.inf
    for cam_x, meshes, msg in ((moved(pkg, cam, CAMERA_STEP), {1: new}, "camera position differs"), (cam, {99: new}, "bad geom id"),
                               (cam, {1: (new[0], None, np.zeros((12, 3), F))}, "without uv"), (cam, {1: (bad, None, None)}, "non-finite vertex position")):
        with pytest.raises(RuntimeError, match="code -1.*" + msg):
            sc.deform_meshes(cam_x, meshes)
    if torch.cuda.device_count() >= 2:
        with torch.cuda.device(1):
            with pytest.raises(RuntimeError, match="code -2.*current HIP device"):
                sc.deform_meshes(cam, {1: new})
    assert sc.debug_device_digest() == digest == sc.debug_pinned_digest(cam) and np.array_equal(product.render(sc, cam, prm), before)
    s2, cam2 = describe(pkg, Remeshed(product), "1")
    product.build_multi(s2, cam2, [0, 0])
    with pytest.raises(RuntimeError, match="code -1.*mi355pt_scene_build_multi"):
        s2.deform_meshes(cam2, {0: deformed(s2.meshes[0])})
    assert np.isfinite(product.render(s2, cam2, prm)).all()
    log_line({"test": "refusals", "scene_unchanged": True})


# ---------------- the CLI ----------------
@pytest.fixture(scope="module")
def cli(pkg, tmp_path_factory):
    root = pkg.ffi.ROOT
    exe = os.path.join(root, "toy-cpu-pathtracing_amd", "host", "mi355pt")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.dirname(exe)])
    assets_dir = str(tmp_path_factory.mktemp("assets"))
    subprocess.check_call([sys.executable, os.path.join(root, "tools", "export_assets.py"), assets_dir])
    return exe, dict(os.environ, MI355PT_ASSETS=assets_dir, MI355PT_DATA=os.path.join(root, "toy-cpu-pathtracing_amd", "data"))


def test_cli_mesh_wave(product, pkg, cli, tmp_path):
    """`--mesh-wave` (twice: the hero and the floor of scene 3) writes a frame that differs from the undeformed one and says one line on
    stderr; with --instance-rebuild-above 1e-6 the call builds again and the frame is within linear_rmse_u8 2e-3 of the refit run's (the
    bar between two trees); an AOV renderer takes the flag too; misuse exits 2 with the flag's name, and so does --temporal-frames"""
    from PIL import Image
    exe, env = cli
    base = [exe, "--scene", "3", "--sampler", "sobol", "--spp", "16", "--width", str(W), "--height", str(H), "--renderer", "mis"]
    waves = ["--mesh-wave", "4:0.15,1.5", "--mesh-wave", "0:0.05,0.7,1.25"]                      # (given out of order: the CLI sorts)

    def run(extra, name):
        path = str(tmp_path / name)
        r = subprocess.run(base + extra + ["-o", path], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        return np.asarray(Image.open(path).convert("RGB")), [ln for ln in r.stderr.splitlines() if ln.startswith("mesh deform: ")]
    refit, lines = run(waves, "refit.png")
    assert len(lines) == 1 and "rebuilt=0 reason=0 launches=" in lines[0] and " sah=" in lines[0] and "→" in lines[0] and " device_ms=" in lines[0]
    plain, none = run([], "plain.png")
    assert not none
    rebuilt, lines = run(waves + ["--instance-rebuild-above", "1e-6"], "rebuilt.png")
    assert len(lines) == 1 and "rebuilt=1 reason=6 launches=0" in lines[0]
    rmse, moved_by = linear_rmse_u8(refit, rebuilt), linear_rmse_u8(refit, plain)
    log_line({"test": "cli", "refit_vs_rebuilt_linear_rmse_u8": rmse, "vs_undeformed_linear_rmse_u8": moved_by})
    assert rmse <= 2e-3 and moved_by > 10 * 2e-3 and refit.mean() > 10.0                         # ... and the wave is visible in the picture
    r = subprocess.run(base[:-1] + ["normal"] + waves + ["-o", str(tmp_path / "n.png")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "mesh deform: rebuilt=0" in r.stderr, r.stderr
    for args, flag in ((["--mesh-wave", "1:0.1"], "--mesh-wave"), (["--mesh-wave", "x:0.1,1"], "--mesh-wave"), (["--mesh-wave", "1:0.1,0"], "--mesh-wave"),
                       (["--mesh-wave", "99:0.1,1"], "--mesh-wave"), (["--mesh-wave", "1:0.1,1", "--mesh-wave", "1:0.2,1"], "--mesh-wave"),
                       (["--mesh-wave", "1:0.1,1", "--instance-rebuild-above", "-1"], "--instance-rebuild-above"),
                       (["--mesh-wave", "1:0.1,1", "--temporal-frames", "2", "--denoise-guide-spp", "4"], "--temporal-frames")):
        r = subprocess.run(base + args, env=env, capture_output=True, text=True, timeout=120, cwd=tmp_path)
        assert r.returncode == 2 and flag in r.stderr, (args, r.returncode, r.stderr)
