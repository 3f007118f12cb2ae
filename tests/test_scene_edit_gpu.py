"""Editing lights and materials of a built scene on the MI355X (include/mi355pt_edit.h): after mi355pt_scene_edit EVERY device array has the
bytes of the host lowering of the edited description over the built tree (mi355pt_scene_debug_device_digest against
mi355pt_scene_debug_pinned_digest, which tests/test_scene_edit.py ties to a fresh lowering of a scene described with the edited records);
the one kernel at its edges; the edited scene renders, bit for bit, the film of a scene freshly built from the edited description, and
what the oracle renders for it; edits compose with the three other updates; a real change of light drives the rectified accumulation;
the fallbacks rebuild; the refusals leave the scene as it was.  One line per comparison goes to the file MI355PT_FRAME_LOG names
(profiles/scene_edit_parity.jsonl)."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geometry_stress as gs  # noqa: E402
import scene_edit_cases as sec  # noqa: E402
import scene_edit_refusal_cases as refusals  # noqa: E402
from test_deform import arrays_of, deformed  # noqa: E402
from test_instance_move import applied, trs  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
W, H, SPP = 64, 48, 16
BUILDERS = ("host", "gpu")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "scene_edit_refusals.json")


def log_line(line):
    print(json.dumps(line))
    if os.environ.get("MI355PT_FRAME_LOG"):
        with open(os.environ["MI355PT_FRAME_LOG"], "a") as f:
            f.write(json.dumps(line) + "\n")


def linear_film(product, pkg, sc, cam, strategy, spp=SPP, seed=0):
    """the linear film sums of [0, spp) as the device holds them"""
    import torch
    film = torch.zeros((cam.height, cam.width, 3), dtype=torch.float32, device="cuda")
    product.render_accum_device(sc, cam, pkg.make_params(spp, strategy, "sobol", seed=seed), 0, spp, film.data_ptr())
    torch.cuda.synchronize()
    return film.cpu().numpy()


# ---------------- 4. bytes ----------------
@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("name", list(sec.CASES))
def test_device_bytes_after_an_edit(product, pkg, name, builder):
    """build, edit: every device array has the digest of the pinned host lowering of the edited description; exactly the arrays the edit can
    reach differ from the fresh build's; one launch when a class changed, none otherwise; the same edit again uploads nothing; the original
    records restore the fresh build's bytes"""
    sc, cam, edits = sec.described(pkg, product, name, builder=builder)
    sc.build(cam)
    assert f"builder={builder}" in product.scene_info(sc)
    fresh, fresh_info = sc.debug_device_digest()
    assert (fresh, fresh_info) == sc.debug_pinned_digest(cam)
    res = sc.edit(cam, **edits)
    got, got_info = sc.debug_device_digest()
    want, want_info = sc.debug_pinned_digest(cam)
    differ = [n for n in want if got[n] != want[n]]
    log_line({"test": "device_bytes", "case": name, "builder": builder, "arrays": len(want), "differ": differ, "launches": res["launches"],
              "features": [res["features_before"], res["features_after"]], "host_ms": round(res["host_ms"], 3), "device_ms": round(res["device_ms"], 3)})
    assert res["rebuilt"] == 0 and res["reason"] == "rebased"
    assert not differ and got_info == want_info and list(got) == list(fresh)
    assert {n for n in got if got[n] != fresh[n]} == sec.DIFFER[name]
    assert res["launches"] == sec.LAUNCHES[name]
    assert (res["features_before"] != res["features_after"]) == ("scalars" in sec.DIFFER[name])
    assert f"features={res['features_after']}" in product.scene_info(sc)
    assert np.isfinite(product.render(sc, cam, pkg.make_params(1, "mis", "sobol"))).all()
    again = sc.edit(cam, **edits)
    assert again["reason"] == "same_records" and again["rebuilt"] == 0 and again["launches"] == 0 and again["device_ms"] == 0.0
    assert sc.debug_device_digest() == (got, got_info)
    back = sc.edit(cam, **sec.original_edits(sc, edits))
    assert back["rebuilt"] == 0 and back["reason"] == "rebased" and back["launches"] == sec.LAUNCHES[name]
    home = sc.debug_device_digest()
    assert home == (fresh, fresh_info), [n for n in fresh if home[0][n] != fresh[n]]


# ---------------- 5. the kernel at its edges ----------------
def soup_scene(pkg, product, n, builder, central):
    """the n-triangle soup of tests/geometry_stress.py as up to three meshes of one triangle set each — even triangles (material 0), odd
    triangles (material 1), and the triangle `central` alone (material 2; none for n = 1) — under a constant environment light"""
    f = pkg.ffi
    tris = gs.family("soup%d" % n).meshes[0]
    sc = product.new_scene()
    sc.set_rgb2spec(pkg.scenes.srgb_table())
    sc.set_bvh_builder(builder)
    mats = []
    for k in range(3):
        d = f.MaterialDesc(); d.type = f.MAT_LAMBERT; d.color = f.Spectrum.constant(0.3 + 0.2 * k); d.normal_tex = f.NONE
        mats.append(sc.add_material(d))
    ids = np.arange(len(tris))
    sets = [ids[(ids % 2 == 0) & (ids != central)], ids[(ids % 2 == 1) & (ids != central)], ids[ids == central] if n > 1 else ids[:0]]
    owner = []                                             # per instance: its material
    for k, s in enumerate(sets):
        if len(s):
            sc.add_instance(sc.add_mesh(gs._mesh_dict(tris[s])), mats[k], gs.IDENTITY)
            owner.append(k)
    sc.add_environment_light(1.0, np.ones((8, 16, 3), dtype=F), sc.add_lut470(pkg.scenes.presets()["cie_illum_d6500"]))
    cam = gs.camera("soup%d" % n, W, H)
    sc.build(cam)
    return sc, cam, mats, np.asarray(owner)


def glass(pkg):
    f = pkg.ffi
    d = f.MaterialDesc(); d.type = f.MAT_GLASS; d.eta = f.Spectrum.constant(1.5); d.color = f.Spectrum.constant(1.0)
    d.normal_tex = f.NONE; d.thin = 0; d.roughness = 0.0
    return d


@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("owns", ["first", "last", "neither"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_reclass_kernel_at_its_edges(product, pkg, n, owns, builder):
    """one material of a small soup becomes glass: the material that owns the first leaf-order triangle, the last one, or neither (for one
    triangle: a material no triangle has).  One launch; the device bytes are the pinned lowering's; the triangles of the edited material
    carry the new class in their last word and nothing else changed, the triangles of the other materials are byte-identical to before"""
    if builder == "gpu" and n < 8:
        builder = "host"                                   # (the GPU builder takes 8 triangles and more: the case runs on the host's tree twice)
    for central in ((n // 2, n // 3, n // 5) if n > 1 else (-1,)):               # the lone triangle must own neither end of the leaf order: at most three tries
        sc, cam, mats, owner = soup_scene(pkg, product, n, builder, central)
        nodes0, tris0, root0 = product.export_bvh(sc)
        leaf_owner = owner[tris0[:, 9]]
        if n == 1 or 2 not in (leaf_owner[0], leaf_owner[-1]):
            break
    assert n == 1 or 2 not in (leaf_owner[0], leaf_owner[-1])
    target = {"first": int(leaf_owner[0]), "last": int(leaf_owner[-1]), "neither": 2}[owns]
    assert len(tris0) == n
    res = sc.edit(cam, materials={mats[target]: glass(pkg)})
    assert res["rebuilt"] == 0 and res["reason"] == "rebased" and res["launches"] == 1
    got, want = sc.debug_device_digest(), sc.debug_pinned_digest(cam)
    assert got == want, [k for k in want[0] if got[0][k] != want[0][k]]
    nodes1, tris1, root1 = product.export_bvh(sc)
    mine = leaf_owner == target
    assert np.array_equal(nodes1, nodes0) and root1 == root0
    assert np.array_equal(tris1[~mine], tris0[~mine])                                   # the other materials' triangles: byte-identical
    assert np.array_equal(tris1[mine][:, :11], tris0[mine][:, :11]) and (tris1[mine][:, 11] == 2).all() and (tris0[:, 11] == 0).all()
    assert (mine.sum() == 0) == (n == 1 and owns == "neither")
    assert (res["features_before"] != res["features_after"]) == bool(mine.any())          # a material no instance has adds no feature
    log_line({"test": "reclass_edges", "n": n, "owns": owns, "builder": builder, "rewritten": int(mine.sum()), "device_ms": round(res["device_ms"], 4)})


# ---------------- 6. frames ----------------
FRAME_CASES = ["3:look_and_glass", "2:point_to_spot", "19:env_turn", "17:coat_roughness"]


@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("name", FRAME_CASES)
def test_frames_after_an_edit_are_a_fresh_builds(product, pkg, name, builder):
    """64 x 48 x 16 spp under pt, nee and mis: the linear film after an in-place edit is, value for value, the film of a fresh build of the
    edited description (equal device bytes, deterministic kernels); where the feature set changed another kernel was selected"""
    sc, cam, edits = sec.described(pkg, product, name, builder=builder)
    sc.build(cam)
    before = {s: linear_film(product, pkg, sc, cam, s) for s in ("pt", "nee", "mis")}      # (the launch context has seen the old feature set)
    res = sc.edit(cam, **edits)
    assert res["rebuilt"] == 0 and res["reason"] == "rebased"
    fresh, _, _ = sec.described(pkg, product, name, edited=True, builder=builder)
    fresh.build(cam)
    assert sc.debug_device_digest() == fresh.debug_device_digest()
    if name == "3:look_and_glass":
        assert res["features_before"] != res["features_after"] and res["features_after"] & 2 and not res["features_before"] & 2      # FEAT_DIEL: the dielectric kernels
    for strategy in ("pt", "nee", "mis"):
        a, b = linear_film(product, pkg, sc, cam, strategy), linear_film(product, pkg, fresh, cam, strategy)
        log_line({"test": "frames", "case": name, "builder": builder, "strategy": strategy, "equal": bool(np.array_equal(a, b)), "mean": float(a.mean())})
        assert np.array_equal(a, b)
        assert np.isfinite(a).all()
        assert not np.array_equal(a, before[strategy]) or not before[strategy].any()      # (plain path tracing never reaches scene 2's delta light: black twice)


@pytest.mark.parametrize("edit_first", [True, False])
def test_edits_compose_with_the_other_updates(product, pkg, edit_first):
    """an edit before or after a camera move, an instance move and a deformation: the device bytes are the pinned lowering's after every
    step, both orders end in the same bytes and the same film, and the flow mark survives the edit"""
    from test_deform import Remeshed
    name = "3:look_and_glass"
    ends = []
    for first in (edit_first, not edit_first):
        case, maps, make = sec.CASES[name]
        from test_scene_lowering import _describe
        sc, cam = _describe(pkg, Remeshed(sec.Edited(product)), case)
        sc.set_bvh_builder("host")
        sc.set_instance_dynamic(1)
        edits = make(pkg, sc)
        sc.build(cam)
        product.scene_flow_mark(sc)
        cam2 = pkg.make_camera(tuple(float(v) for v in np.array(cam.position[:], F) + np.asarray((0.3, -0.2, 0.45), F)), tuple(cam.direction[:]), tuple(cam.up[:]), W, H, cam.fov_deg)

        def others(c):
            assert sc.move_camera(cam2)["rebuilt"] == 0
            assert sc.move_instances(cam2, [1], [applied(trs(), sc.instances[1][2])])["rebuilt"] == 0
            assert sc.deform_meshes(cam2, {2: deformed(sc.meshes[2])})["rebuilt"] == 0
        if first:
            assert sc.edit(cam, **edits)["rebuilt"] == 0
            assert product.scene_flow_marked(sc)
            assert sc.debug_device_digest() == sc.debug_pinned_digest(cam)
            others(cam2)
        else:
            others(cam2)
            assert sc.edit(cam2, **edits)["rebuilt"] == 0
        assert sc.debug_device_digest() == sc.debug_pinned_digest(cam2)
        ends.append((sc.debug_device_digest(), linear_film(product, pkg, sc, cam2, "mis")))
    assert ends[0][0] == ends[1][0] and np.array_equal(ends[0][1], ends[1][1])


@pytest.mark.parametrize("builder", BUILDERS)
def test_a_light_that_follows_the_camera(product, pkg, builder):
    """build at A, move the camera by d, then move the point light by the same d: its render-space position is then bytewise what the
    BUILD held, and must still be uploaded over what the camera move left on the device.  The device bytes are the pinned lowering's after
    each step, the edit is no "same records", and the film is a fresh build's"""
    sc, cam, _ = sec.described(pkg, product, "2:point_moved", builder=builder)
    sc.build(cam)
    d = np.asarray((0.25, -0.125, 0.5), F)                                          # (exact in binary: p + d - (A + d) rounds back to p - A)
    cam2 = pkg.make_camera(tuple(float(v) for v in np.array(cam.position[:], F) + d), tuple(cam.direction[:]), tuple(cam.up[:]), W, H, cam.fov_deg)
    built_lights = sc.debug_device_digest()[0]["lights"]
    assert sc.move_camera(cam2)["rebuilt"] == 0
    assert sc.debug_device_digest() == sc.debug_pinned_digest(cam2)
    assert sc.debug_device_digest()[0]["lights"] != built_lights
    light = sec.copy_of(sc.light_descs[0])
    sec.set_matrix(light, sec.translate(*[float(v) for v in d]) @ sec.matrix_of(light))
    res = sc.edit(cam2, lights={0: light})
    got, want = sc.debug_device_digest(), sc.debug_pinned_digest(cam2)
    log_line({"test": "light_follows_camera", "builder": builder, "reason": res["reason"], "differ": [n for n in want[0] if got[0][n] != want[0][n]],
              "lights_as_built": bool(got[0]["lights"] == built_lights)})
    assert res["rebuilt"] == 0 and res["reason"] == "rebased"
    assert got == want
    assert got[0]["lights"] == built_lights                                          # the case: the new record equals the one the cache held before the move
    fresh, _ = __import__("test_scene_lowering")._describe(pkg, sec.Edited(product, lights={0: light}), "2")
    fresh.set_bvh_builder(builder)
    fresh.build(cam2)
    for strategy in ("nee", "mis"):
        a = linear_film(product, pkg, sc, cam2, strategy)
        assert a.any() and np.array_equal(a, linear_film(product, pkg, fresh, cam2, strategy))
    # ... and the cache the next edit compares with is what this one uploaded
    assert sc.edit(cam2, lights={0: light})["reason"] == "same_records"


# ---------------- 9. the CLI ----------------
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


CLI_EDITS = [("3", ["--emitter-gain", "7:0.7"]), ("2", ["--light-step", "0:0.2,-0.1,0.1:1.3", "--camera-step", "0.2,-0.1,0.1", "--camera-move", "rebase"]),
             ("19", ["--env-yaw-step", "30"])]


@pytest.mark.parametrize("scene,flags", CLI_EDITS, ids=[c[0] for c in CLI_EDITS])
def test_cli_inplace_equals_rebuild(cli, tmp_path, scene, flags):
    """`mi355pt --temporal-frames 4 <edit flags> --scene-edit inplace` writes the PNG of `--scene-edit rebuild`, byte for byte, and another
    one than without the flags; every frame's edit ran in place; without --temporal-rectify one line on stderr says what the plain
    accumulation does with the change; the misuse cases exit 2"""
    import subprocess
    exe, env = cli
    base = [exe, "--scene", scene, "--renderer", "mis", "--sampler", "sobol", "--spp", "4", "--width", str(W), "--height", str(H), "--denoise-guide-spp", "16",
            "--temporal-frames", "4"]

    def picture(extra, name):
        path = str(tmp_path / name)
        r = subprocess.run(base + extra + ["-o", path], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        return open(path, "rb").read(), r.stderr
    inplace, err_in = picture(flags + ["--scene-edit", "inplace"], "inplace.png")
    rebuild, err_re = picture(flags + ["--scene-edit", "rebuild"], "rebuild.png")
    default, _ = picture(flags, "default.png")
    moves = [f for f in flags if f.startswith("--camera")] and flags[flags.index("--camera-step"):]
    plain, err_plain = picture(list(moves), "plain.png")
    assert inplace == rebuild == default and inplace != plain
    edits = [ln for ln in err_in.splitlines() if ln.startswith("scene edit, frame")]
    assert len(edits) == 3 and all("rebuilt=0 reason=0" in ln for ln in edits), err_in
    note = "the plain accumulation averages the change of light over its history"
    assert note in err_in and note in err_re and note not in err_plain
    rectified, err_rect = picture(flags + ["--scene-edit", "inplace", "--temporal-rectify"], "rectified.png")
    assert note not in err_rect and rectified != inplace
    for bad in (["--scene-edit", "sideways"] + flags, ["--scene-edit", "inplace"], ["--emitter-gain", "0:2"], ["--light-step", "9:0,0,0"], ["--light-step", "0:1,2"]):
        r = subprocess.run(base + bad + ["-o", str(tmp_path / "bad.png")], env=env, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "error:" in r.stderr, (bad, r.returncode, r.stderr)
    r = subprocess.run([exe, "--scene", scene, "--renderer", "mis", "--spp", "4", "--width", str(W), "--height", str(H)] + flags[:2] + ["-o", str(tmp_path / "bad.png")],
                       env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--temporal-frames" in r.stderr


# ---------------- 7. against the oracle ----------------
@pytest.mark.parametrize("name", ["3:emitter_look", "19:env_turn"])
def test_edited_scene_matches_the_oracle(product, oracle, pkg, name):
    """the scene edited in place against the oracle's render of a scene DESCRIBED with the edited records (not an edited oracle), at the
    frame bar tests/test_parity_gpu.py holds these scenes to"""
    from test_parity_gpu import FRAME_BAR
    case, maps, make = sec.CASES[name]
    sc = product.new_scene()
    cam = pkg.scenes.load_scene(sc, int(case), W, H, tex_size=128, build=False)
    edits = make(pkg, sc)
    sc.build(cam)
    assert sc.edit(cam, **edits)["rebuilt"] == 0
    osc = sec.Edited(oracle, **edits).new_scene()
    ocam = pkg.scenes.load_scene(osc, int(case), W, H, tex_size=128)
    oracle.set_faithful(osc, False)
    prm = pkg.make_params(64, "mis", "sobol")
    g, c = product.render(sc, cam, prm), oracle.render(osc, ocam, prm)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(np.isnan(g), np.isnan(c))
        d = np.nan_to_num(g - c)
    rmse, off = float(np.sqrt(np.mean(d ** 2))), int((np.abs(d).max(axis=2) > 0.01).sum())
    log_line({"test": "oracle", "case": name, "rmse": rmse, "off": off})
    assert rmse <= FRAME_BAR[0] and off <= FRAME_BAR[1], (rmse, off)


# ---------------- 8. a real change of light for the rectified accumulation ----------------
def test_temporal_rectify_follows_an_emitter_edit(product, pkg):
    """tests/test_temporal_rectify_gpu.py's x4 protocol with a REAL change of light: scene 3 at 64 x 48, a static camera, frames of 4 spp;
    frames 0 .. 7 are rendered with the emitter edited in place to four times its intensity, frames 8 .. 11 after the edit back.  RMSE after
    the resolve against the product's 1024-spp frame of the final scene: E_rect <= sqrt(E_unrectified E_32), that test's own bar"""
    import temporal_reference as tr
    from test_temporal_rectify_gpu import AFTER, FRAME_SPP, H3, HISTORY, W3, Device, render_frame, resolved
    dev = Device(product, pkg)
    sc = sec.Edited(product).new_scene()
    cam = pkg.scenes.load_scene(sc, 3, W3, H3, tex_size=128, build=False)
    d65 = sc.add_lut470(pkg.scenes.presets()["cie_illum_d6500"])
    sc.build(cam)
    handle = (sc, cam, d65)
    bright = sec.emitter_gain(4.0)(pkg, sc)
    res = sc.edit(cam, **bright)
    assert res["rebuilt"] == 0 and res["launches"] == 0
    frames = [render_frame(product, pkg, handle, k) for k in range(HISTORY)]
    res = sc.edit(cam, **sec.original_edits(sc, bright))
    assert res["rebuilt"] == 0 and res["reason"] == "rebased"
    frames += [render_frame(product, pkg, handle, k) for k in range(HISTORY, HISTORY + AFTER)]
    view = product.temporal_view_from_cameras(cam, cam)
    geo = ("position", "shading_normal", "hit")
    acc = {}
    for kind, rectified in (("rectified", True), ("unrectified", False)):
        prev = None
        for f in frames:
            cur = dict({g: f[g] for g in geo}, film=f["film"], half=f["half"])
            out = dev.run_device(cur, FRAME_SPP, prev, view if prev is not None else None, rectified=rectified)
            prev = dict({g: f[g] for g in geo}, film=out[0], half=out[1], length=out[2])
        acc[kind] = out
    rmse = lambda a, b: float(np.sqrt(np.mean((a - b) ** 2)))   # noqa: E731
    ref = product.render(sc, cam, pkg.make_params(1024, "mis", "sobol", seed=1000)).astype(np.float64)
    e32 = rmse(product.render(sc, cam, pkg.make_params(32, "mis", "sobol", seed=0)).astype(np.float64), ref)
    e_r, e_u = rmse(resolved(product, acc["rectified"][0], 2), ref), rmse(resolved(product, acc["unrectified"][0], 2), ref)
    log_line({"test": "temporal_rectify_emitter_edit", "E_32": round(e32, 5), "E_rect": round(e_r, 5), "E_unrectified": round(e_u, 5), "bar": round((e_u * e32) ** 0.5, 5)})
    assert e_u > e32
    assert e_r <= (e_u * e32) ** 0.5, (e_r, e_u, e32)


# ---------------- the fallbacks and the refusals of a built scene ----------------
def built_scene_records(pkg, product=None):
    """part 2 of tests/golden/scene_edit_refusals.json: what only a built scene can refuse, as (code, last_error), and every reason an edit
    falls back for, as (0, "reason=<name> rebuilt=<n>")"""
    f = pkg.ffi
    product = product or pkg.Product()
    caller = refusals.Caller(pkg, product, build=lambda sc, cam: sc.build(cam))
    out = []

    def refusal(name, sc, cam, **edits):
        se, keep = sc._scene_edits(**edits)
        import ctypes as C
        code, text = caller.raw("mi355pt_scene_edit", sc.h.value, C.byref(cam), C.byref(se))
        out.append({"part": 2, "entry": "mi355pt_scene_edit", "case": name, "code": code, "error": text})

    def fallback(name, sc, cam, **edits):
        want = sec.Edited(product, **edits)
        res = sc.edit(cam, **edits)
        out.append({"part": 2, "entry": "mi355pt_scene_edit", "case": name, "code": 0, "error": "reason=%s rebuilt=%d" % (res["reason"], res["rebuilt"])})
        return want
    sc, cam = caller.scene("21")
    valid = refusals._valid(pkg, sc, "21")
    off = pkg.make_camera(tuple(float(v) for v in np.array(cam.position[:], F) + np.asarray((0.3, -0.2, 0.45), F)), tuple(cam.direction[:]), tuple(cam.up[:]), W, H, cam.fov_deg)
    before = sc.debug_device_digest()
    refusal("cam.wrong_position", sc, off, **valid)
    late, late_cam = caller.scene("21")      # (a scene of its own: the read-back digest sizes its reads by the description, which these cases extend)
    for name in ("later_table.texture", "later_table.lut", "finite.light_matrix", "ids.material_equal"):
        code, text = caller.call("mi355pt_scene_edit", name, *((late, late_cam) if name.startswith("later_table") else (sc, cam)))
        out.append({"part": 2, "entry": "mi355pt_scene_edit", "case": name, "code": code, "error": text})
    code, text = caller.call("mi355pt_scene_debug_apply_edits", "valid.scene_21", sc, cam)
    out.append({"part": 2, "entry": "mi355pt_scene_debug_apply_edits", "case": "built.scene", "code": code, "error": text})
    assert sc.debug_device_digest() == before                                          # nothing reached the device or the description
    assert sc.debug_pinned_digest(cam) == before
    from test_scene_lowering import _describe
    multi, mcam = _describe(pkg, sec.Edited(product), "21")
    product.build_multi(multi, mcam, [0, 0])
    refusal("multi.scene", multi, mcam, **refusals._valid(pkg, multi, "21"))
    wall = sec._first(sc, f.MAT_LAMBERT, skip=2)
    fallback("fallback.same_records", sc, cam, materials={wall: sec.copy_of(sc.material_descs[wall])})
    em = sec.copy_of(sc.material_descs[sec._first(sc, f.MAT_EMISSIVE)])
    em.color = f.Spectrum.constant(1.0)         # (the fresh scene below describes the wall before the emitter's LUT exists)
    fallback("fallback.emitter_set_changed", sc, cam, materials={wall: em})
    coat = f.MaterialDesc(); coat.type = f.MAT_SIMPLE_PBR; coat.color = f.Spectrum.constant(0.5); coat.normal_tex = f.NONE
    coat.metallic = 0.2; coat.roughness = 0.5; coat.ior = 1.5
    fallback("fallback.table_shape_changed", sc, cam, materials={wall + 1: coat})
    # after the two rebuilds the device holds a fresh build of the description with both edits
    fresh, fcam = _describe(pkg, sec.Edited(product, materials={wall: em, wall + 1: coat}), "21")
    fresh.set_bvh_builder("host")
    fresh.build(fcam)
    assert sc.debug_device_digest() == fresh.debug_device_digest()
    return out


def test_fallbacks_and_refusals_of_a_built_scene(product, pkg):
    """a wrong camera position, a texture or LUT added after the build, a scene built over several devices and the debug twin on a built
    scene are refused, the device bytes as they were; an edit with the built records does nothing; a material that enters the emitters and a
    new clearcoat material build again, and the device then holds a fresh build of the edited description — replayed from the golden file"""
    golden = [r for r in json.load(open(GOLDEN))["records"] if r["part"] == 2]
    got = built_scene_records(pkg, product)
    assert got == golden, [(g, w) for g, w in zip(got, golden) if g != w]
    by = {r["case"]: r for r in got}
    assert by["fallback.same_records"]["error"] == "reason=same_records rebuilt=0"
    assert by["fallback.emitter_set_changed"]["error"] == "reason=emitter_set_changed rebuilt=1"
    assert by["fallback.table_shape_changed"]["error"] == "reason=table_shape_changed rebuilt=1"
    assert all(by[c]["code"] == -1 for c in ("cam.wrong_position", "later_table.texture", "later_table.lut", "multi.scene", "built.scene"))
