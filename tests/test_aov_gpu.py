"""GPU tests of the AOV renderers (mi355pt_render_aov & co., csrc/pt_kernels_aov.hip) against the CPU reference of tests/aov_reference.cpp:
the reference's NormalRenderer / AlbedoRenderer semantics sample for sample, and the shading-normal extension."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aov_reference  # noqa: E402

pytestmark = pytest.mark.gpu

# every material type (Lambert 0, metal 7, glass 8, plastic 10, clearcoat 15 / 17 / 19, SimplePbr 22), a texture (3, 15), a transformed
# instance (17), the environment (19), an emitter in view (0, 3, ...) and a textured emitter (30)
SCENES = [0, 3, 7, 8, 10, 15, 17, 19, 22, 30]
KINDS = ["normal", "albedo", "shading_normal"]
# the project's bars (tests/test_parity_gpu.py): frames, and per-sample values
FRAME_BAR = (1.5e-4, 0)          # RMSE, pixels off by more than 0.01
PER_SAMPLE_MIN = 0.9995          # share within 1e-3 |c| + 1e-4: what is left out are exact-t ties / silhouette edges (profiles/r03_exact_t_ties.jsonl)
TIGHT_MIN = 0.997                # share within 1e-5: what sits between the bars is the arithmetic of the hit point and the hardware exp2 / rcp


@pytest.fixture(scope="module")
def ref():
    return aov_reference.AovReference()


@pytest.fixture(scope="module")
def scenes(product, ref, pkg):
    """scene id -> {"gpu": (scene, camera, d65), "cpu": ...}, built once (the build depends on the camera's position only)"""
    cache = {}

    def get(scene_id):
        if scene_id not in cache:
            pair = {"gpu": aov_reference.load(product, scene_id, 64, 48), "cpu": aov_reference.load(ref, scene_id, 64, 48)}
            ref.set_faithful(pair["cpu"][0], False)       # (faithful == fast for the AOVs, bit for bit: tests/test_aov.py)
            cache[scene_id] = pair
        return cache[scene_id]
    return get


def sized(cam, w, h, pkg):
    c = pkg.ffi.Camera.from_buffer_copy(cam)
    c.width, c.height = w, h
    return c


def both(product, ref, pkg, pair, kind, w, h, spp, sampler="sobol", want_classes=False):
    k = pkg.ffi.AOV[kind]
    prm = pkg.make_params(spp, "mis", sampler)
    (sg, cg, dg), (sc, cc, dc) = pair["gpu"], pair["cpu"]
    g = product.render_aov(sg, sized(cg, w, h, pkg), prm, k, dg)
    c = ref.render_aov(sc, sized(cc, w, h, pkg), prm, k, dc, want_classes=want_classes)
    return (g,) + c if want_classes else (g, c)


def log_line(text):
    if os.environ.get("MI355PT_FRAME_LOG"):
        with open(os.environ["MI355PT_FRAME_LOG"], "a") as f:
            f.write(text + "\n")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("scene_id", SCENES)
def test_aov_per_sample_parity(product, ref, pkg, scenes, scene_id, kind):
    """One pixel = one sample (256x192 at 1 spp, Sobol): the resolved value of every pixel against the CPU reference, per channel, with the
    two bars the project puts on per-sample radiance.  Both are caps on what may be left out (the reference's faithful and fast modes
    leave out 0 pixels against each other); the measured shares and the largest deviation go to MI355PT_FRAME_LOG
    (profiles/aov_parity.jsonl)."""
    g, c = both(product, ref, pkg, scenes(scene_id), kind, 256, 192, 1)
    assert np.array_equal(np.isnan(g), np.isnan(c))
    d = np.abs(g - c)
    close = np.all(d <= 1e-3 * np.abs(c) + 1e-4, axis=2)
    tight = np.all(d <= 1e-5, axis=2)
    log_line(f'{{"test": "per_sample", "scene": {scene_id}, "kind": "{kind}", "close": {close.mean():.6f}, "tight": {tight.mean():.6f}, '
             f'"bit_equal": {np.all(g == c, axis=2).mean():.6f}, "max_dev": {d.max():.3e}}}')
    print(scene_id, kind, "close", close.mean(), "tight", tight.mean(), "max", d.max())
    assert close.mean() >= PER_SAMPLE_MIN, close.mean()
    assert tight.mean() >= TIGHT_MIN, tight.mean()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("scene_id", SCENES)
def test_aov_frame_parity(product, ref, pkg, scenes, scene_id, kind):
    """64x48 at 64 spp, Sobol: FRAME_BAR as it stands for the path renderers' frames."""
    g, c = both(product, ref, pkg, scenes(scene_id), kind, 64, 48, 64)
    assert np.array_equal(np.isnan(g), np.isnan(c))
    rmse = float(np.sqrt(np.mean((g - c) ** 2)))
    off = int((np.abs(g - c).max(axis=2) > 0.01).sum())
    log_line(f'{{"test": "frame", "scene": {scene_id}, "kind": "{kind}", "rmse": {rmse:.3e}, "off": {off}, "max_dev": {np.abs(g - c).max():.3e}}}')
    print(scene_id, kind, "rmse", rmse, "off", off)
    assert c.mean() > 0.01
    assert rmse <= FRAME_BAR[0] and off <= FRAME_BAR[1], (rmse, off)


@pytest.mark.parametrize("kind", ["normal", "shading_normal"])
@pytest.mark.parametrize("scene_id", [3, 19])
def test_aov_random_sampler_parity(product, ref, pkg, scenes, scene_id, kind):
    """The random sampler (the reference's ThreadRng ignores the seed: statistical parity only there) — but both of OUR sides draw from the
    same counter hash, so the frames meet FRAME_BAR like the Sobol ones."""
    g, c = both(product, ref, pkg, scenes(scene_id), kind, 64, 48, 64, sampler="random")
    rmse = float(np.sqrt(np.mean((g - c) ** 2)))
    off = int((np.abs(g - c).max(axis=2) > 0.01).sum())
    log_line(f'{{"test": "random", "scene": {scene_id}, "kind": "{kind}", "rmse": {rmse:.3e}, "off": {off}}}')
    assert rmse <= FRAME_BAR[0] and off <= FRAME_BAR[1], (rmse, off)


def test_aov_sampler_order(product, ref, pkg, scenes):
    """The draws: get_2d_pixel() alone (pattern "2", Sobol dimensions 0-1) for the normal kinds, get_1d() then get_2d_pixel() ("12") for the
    albedo — the Sobol words of the product's probe equal the oracle's.  And the GPU against itself: `normal` and `shading_normal` of the
    same call are bit-equal on every pixel whose samples all hit emitters or miss, and `normal` is (0.5, 0.5, 1.0) within 1e-6 where the
    CPU reference says that all samples hit BSDF surfaces."""
    rng = np.random.default_rng(5)
    n = 4096
    xys = np.stack([rng.integers(0, 64, n), rng.integers(0, 48, n), rng.integers(0, 64, n)], 1).astype(np.uint32)
    for pattern in ("2", "12"):
        assert np.array_equal(product.probe_sobol(64, 48, 64, 0, xys, pattern), ref.probe_sobol(64, 48, 64, 0, xys, pattern))
    for scene_id in (3, 19, 30):
        pair = scenes(scene_id)
        g_n, _, cls = both(product, ref, pkg, pair, "normal", 64, 48, 64, want_classes=True)
        g_s, _ = both(product, ref, pkg, pair, "shading_normal", 64, 48, 64)
        no_bsdf = cls[..., 0] == 0
        only_bsdf = (cls[..., 1] == 0) & (cls[..., 2] == 0)
        assert only_bsdf.sum() > 1000 and (no_bsdf.sum() > 0 or scene_id == 30)
        assert np.array_equal(g_n[no_bsdf], g_s[no_bsdf])
        assert np.abs(g_n[only_bsdf] - np.array([0.5, 0.5, 1.0], np.float32)).max() <= 1e-6
        assert np.abs(g_s[only_bsdf] - np.array([0.5, 0.5, 1.0], np.float32)).max() > 0.1      # (the extension shows the surfaces)


@pytest.mark.parametrize("kind", KINDS)
def test_aov_device_resident_path(product, pkg, scenes, kind):
    """render_aov_accum_device over [0, 32) then [32, 64) into one buffer + aov_resolve_device = render_aov at 64 spp, bit for bit; three
    shards into one zeroed buffer = the whole frame, bit for bit; a second identical call reproduces the first bit for bit; the stats
    block counts the samples and primary rays."""
    import torch
    W, H, spp = 64, 48, 64
    sc, cam, d65 = scenes(3)["gpu"]
    cam = sized(cam, W, H, pkg)
    k = pkg.ffi.AOV[kind]
    prm = pkg.make_params(spp, "mis", "sobol")
    whole, st = product.render_aov(sc, cam, prm, k, d65, want_stats=True)
    assert st.samples == st.closest_rays == W * H * spp and 0 < st.closest_hits <= st.samples and st.launches == 1 and st.kernel_ms > 0.0
    assert st.shadow_rays == 0 and st.bounces == 0
    assert np.array_equal(product.render_aov(sc, cam, prm, k, d65), whole)

    def resolved(acc):
        out = torch.empty_like(acc)
        product.aov_resolve_device(k, acc.data_ptr(), W * H, spp, out.data_ptr(), None)
        torch.cuda.synchronize()
        return out.cpu().numpy()
    a = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    product.render_aov_accum_device(sc, cam, prm, k, d65, 0, 32, a.data_ptr(), None)
    product.render_aov_accum_device(sc, cam, prm, k, d65, 32, 64, a.data_ptr(), None)
    assert np.array_equal(resolved(a), whole)
    b = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    for shard in range(3):
        product.render_aov_accum_device(sc, cam, pkg.make_params(spp, "mis", "sobol", shard_index=shard, shard_count=3), k, d65, 0, spp, b.data_ptr(), None)
    assert np.array_equal(resolved(b), whole)
    # one shard alone leaves the other tiles untouched
    c = torch.full((H, W, 3), -1.0, dtype=torch.float32, device="cuda")
    product.render_aov_accum_device(sc, cam, pkg.make_params(spp, "mis", "sobol", shard_index=1, shard_count=3), k, d65, 0, spp, c.data_ptr(), None)
    torch.cuda.synchronize()
    ys, xs = np.mgrid[0:H, 0:W]
    other = ((ys // 8) * ((W + 7) // 8) + xs // 8) % 3 != 1
    assert np.all(c.cpu().numpy()[other] == -1.0)


def test_aov_errors_on_device(product, pkg, scenes):
    """The documented codes on a built scene, and the next valid call still succeeds."""
    f = pkg.ffi
    sc, cam, d65 = scenes(0)["gpu"]
    cam = sized(cam, 64, 48, pkg)
    prm = pkg.make_params(4, "mis", "sobol")
    out = np.zeros((48, 64, 3), np.float32)
    lib = product.lib

    def call(cam_, prm_, kind, lut):
        return lib.mi355pt_render_aov(sc.h, ctypes.byref(cam_), ctypes.byref(prm_), kind, lut, out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), None)
    assert call(cam, prm, f.AOV_ALBEDO, 12345) == -1                       # MI355PT_E_INVALID: not a LUT of this scene
    assert b"illuminant" in lib.mi355pt_last_error()
    assert call(cam, prm, f.AOV_NORMAL, 12345) == 0                        # ignored for the normal kinds
    assert call(cam, pkg.make_params(4, "mis", "sobol", collect_stats=1), f.AOV_NORMAL, d65) == -1
    assert call(cam, prm, 3, d65) == -1 and call(cam, prm, -1, d65) == -1  # unknown kind
    moved = f.Camera.from_buffer_copy(cam)
    moved.position[0] += 1.0
    assert call(moved, prm, f.AOV_NORMAL, d65) == -1                       # the camera position is baked into the build
    bad = pkg.make_params(4, "mis", "sobol"); bad.strategy = 77; bad.max_depth = 100000   # ignored by the AOV renderers
    assert call(cam, bad, f.AOV_SHADING_NORMAL, d65) == 0
    bad.sampler = 9
    assert call(cam, bad, f.AOV_SHADING_NORMAL, d65) == -1
    fresh = product.new_scene()
    assert lib.mi355pt_render_aov(fresh.h, ctypes.byref(cam), ctypes.byref(prm), 0, 0, out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), None) == -3   # NOT_BUILT
    img = product.render_aov(sc, cam, prm, f.AOV_ALBEDO, d65)              # and the next valid call succeeds
    assert np.isfinite(img).all() and img.mean() > 0.05


def test_aov_cli(product, pkg, tmp_path):
    """mi355pt without --renderer runs the reference's default, `normal` (main.rs:38-40), and its PNG is quantize_u8 of render_aov(NORMAL);
    the same for --renderer albedo and the shading-normal extension; an unknown renderer still exits with status 2."""
    from PIL import Image
    root = pkg.ffi.ROOT
    exe = os.path.join(root, "toy-cpu-pathtracing_amd", "host", "mi355pt")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.dirname(exe)])
    assets_dir = str(tmp_path / "assets")
    subprocess.check_call([sys.executable, os.path.join(root, "tools", "export_assets.py"), assets_dir])
    env = dict(os.environ, MI355PT_ASSETS=assets_dir, MI355PT_DATA=os.path.join(root, "toy-cpu-pathtracing_amd", "data"))
    sc = product.new_scene()
    cam = pkg.scenes.load_scene(sc, 3, 96, 64, build=False)
    d65 = sc.add_lut470(pkg.scenes.presets()["cie_illum_d6500"])
    sc.build(cam)
    base = [exe, "--scene", "3", "--sampler", "sobol", "--spp", "8", "--width", "96", "--height", "64"]
    for flag, kind in ((None, "normal"), ("albedo", "albedo"), ("shading-normal", "shading_normal")):
        out = str(tmp_path / f"aov_{kind}.png")
        r = subprocess.run(base + (["--renderer", flag] if flag else []) + ["--output", out], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        assert "Finish rendering" in r.stdout
        cli = np.asarray(Image.open(out).convert("RGB"))
        want = product.quantize_u8(product.render_aov(sc, cam, pkg.make_params(8, "mis", "sobol"), pkg.ffi.AOV[kind], d65))
        assert cli.shape == want.shape
        print(kind, "pixels differing", int((cli != want).any(axis=2).sum()))
        assert np.array_equal(cli, want), int((cli != want).any(axis=2).sum())
    r = subprocess.run(base + ["--renderer", "nonsense"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 2
    r = subprocess.run(base + ["--renderer", "albedo", "--gpus", "2"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "one GPU" in r.stderr
