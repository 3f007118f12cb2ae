"""GPU tests of the denoiser (mi355pt_denoise_device / mi355pt_denoise, csrc/pt_kernels_denoise.hip) against the NumPy restatement of
tests/denoise_reference.py.  The measure is max |x - ref64| / (|ref64| + 1e-3) over EVERY value of the frame; the bar of a case is 8 times
what the f32 restatement itself shows on that case (e32): the factor covers the hardware exp2 and reciprocal and another summation order
over 25 taps x levels, while a wrong tap or a missing term shows at 1e-3 and more."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import denoise_reference as dr  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (3, 2), (7, 5), (64, 1), (1, 64), (67, 35), (130, 70)]    # (W, H): below a wave, ragged edges, one row, one column, > 1 block
LEVELS = [1, 5, 6, 8]
GUIDES = {"both": (True, True), "normal": (False, True), "albedo": (True, False), "none": (False, False)}
SPPS = [(4, 64, 64), (1, 1, 1)]
FACTOR = 8.0


def log_line(text):
    print(text)
    if os.environ.get("MI355PT_FRAME_LOG"):
        with open(os.environ["MI355PT_FRAME_LOG"], "a") as f:
            f.write(text + "\n")


class Device:
    """films on the device + one call of mi355pt_denoise_device; the output starts as NaN, so a pixel the kernels leave out shows"""

    def __init__(self, product):
        import torch
        self.torch, self.product = torch, product

    def up(self, x):
        return None if x is None else self.torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()

    def run(self, b, sb, a, sa, n, sn, params, out=None):
        torch = self.torch
        H, W, _ = b.shape
        need = self.product.denoise_scratch_bytes(W, H)
        scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
        out = torch.full((H, W, 3), float("nan"), dtype=torch.float32, device="cuda") if out is None else out
        self.product.denoise_device(b.data_ptr(), sb, a.data_ptr() if a is not None else None, sa, n.data_ptr() if n is not None else None, sn,
                                    W, H, params, scratch.data_ptr(), need, out.data_ptr(), None)
        torch.cuda.synchronize()
        return out


@pytest.fixture(scope="module")
def dev(product):
    return Device(product)


def make_params(product, **kw):
    p = product.denoise_params_default()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def check_against_reference(dev, product, films, spps, guides, levels, tag):
    b, a, n = films
    use_a, use_n = GUIDES[guides]
    a, n = (a if use_a else None), (n if use_n else None)
    ref64 = dr.denoise(b, spps[0], a, spps[1], n, spps[2], levels=levels, dtype=np.float64)
    ref32 = dr.denoise(b, spps[0], a, spps[1], n, spps[2], levels=levels, dtype=np.float32)
    e32 = dr.rel_err(ref32, ref64)
    got = dev.run(dev.up(b), spps[0], dev.up(a), spps[1], dev.up(n), spps[2], make_params(product, levels=levels)).cpu().numpy()
    assert np.isfinite(got).all(), f"{tag}: {int((~np.isfinite(got)).sum())} values not written or not finite"
    egpu = dr.rel_err(got, ref64)
    log_line(f'{{"test": "{tag}", "guides": "{guides}", "levels": {levels}, "spp": {list(spps)}, "e32": {e32:.3e}, "gpu": {egpu:.3e}, '
             f'"ratio": {egpu / e32 if e32 > 0 else 0.0:.2f}}}')
    assert egpu <= FACTOR * e32, (tag, guides, levels, spps, egpu, e32)
    if n is not None:                                                       # background pixels: c, bit for bit
        bg = dr.background(n)
        c = dr.prepass(b, spps[0], dtype=np.float32)[0]
        assert np.array_equal(got[bg].view(np.uint32), c[bg].view(np.uint32)), tag
    return got


@pytest.mark.parametrize("guides", list(GUIDES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_denoise_synthetic_parity(dev, product, shape, guides):
    """Seeded synthetic films (piecewise-planar guides, HDR noise up to about 100, a background region, NaN / inf / negative values) at
    every shape, level count, guide set and spp triple: the GPU within 8 e32 of the f64 restatement on every value, nothing left out."""
    W, H = shape
    for spps in SPPS:
        films = dr.synthetic(W, H, *spps)
        for levels in LEVELS:
            check_against_reference(dev, product, films, spps, guides, levels, f"synthetic_{W}x{H}")


# ---------------------------------------------------------------- rendered films
RW, RH, SPP, GUIDE_SPP, REF_SPP = 160, 120, 4, 64, 256


@pytest.fixture(scope="module")
def rendered(product, pkg):
    """scene id -> dict of device films (linear sums): beauty at 4 spp, albedo and shading normal at 64 spp, beauty at 256 spp; mis + Sobol"""
    import torch
    cache = {}

    def get(scene_id):
        if scene_id not in cache:
            sc = product.new_scene()
            cam = pkg.scenes.load_scene(sc, scene_id, RW, RH, build=False)
            d65 = sc.add_lut470(pkg.scenes.presets()["cie_illum_d6500"])
            sc.build(cam)
            films = {k: torch.zeros((RH, RW, 3), dtype=torch.float32, device="cuda") for k in ("beauty", "albedo", "normal", "ref")}
            product.render_accum_device(sc, cam, pkg.make_params(SPP, "mis", "sobol"), 0, SPP, films["beauty"].data_ptr(), None)
            product.render_accum_device(sc, cam, pkg.make_params(REF_SPP, "mis", "sobol"), 0, REF_SPP, films["ref"].data_ptr(), None)
            g = pkg.make_params(GUIDE_SPP, "mis", "sobol")
            product.render_aov_accum_device(sc, cam, g, pkg.ffi.AOV_ALBEDO, d65, 0, GUIDE_SPP, films["albedo"].data_ptr(), None)
            product.render_aov_accum_device(sc, cam, g, pkg.ffi.AOV_SHADING_NORMAL, d65, 0, GUIDE_SPP, films["normal"].data_ptr(), None)
            torch.cuda.synchronize()
            cache[scene_id] = films
        return cache[scene_id]
    return get


def resolve(product, film, spp):
    import torch
    out = torch.empty_like(film)
    product.film_resolve_device(film.data_ptr(), film.shape[0] * film.shape[1], spp, out.data_ptr(), None)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("scene_id", [3, 8, 19])
def test_denoise_rendered_parity(dev, product, rendered, scene_id):
    """Scenes 3, 8 and 19 at 160 x 120, GPU beauty at 4 spp and GPU guides at 64 spp, default parameters: the same bar, and background
    pixels bit-equal to c (check_against_reference)."""
    f = rendered(scene_id)
    films = tuple(f[k].cpu().numpy() for k in ("beauty", "albedo", "normal"))
    assert np.isfinite(films[1]).all() and np.isfinite(films[2]).all()
    check_against_reference(dev, product, films, (SPP, GUIDE_SPP, GUIDE_SPP), "both", 5, f"rendered_scene{scene_id}")


def test_denoise_is_deterministic_and_host_form_matches(dev, product, rendered):
    """Two calls are bit-equal; mi355pt_denoise on host buffers is bit-equal to mi355pt_denoise_device; the resolved output (a film with
    spp 1) is finite and in [0, 1]."""
    f = rendered(3)
    p = product.denoise_params_default()
    one = dev.run(f["beauty"], SPP, f["albedo"], GUIDE_SPP, f["normal"], GUIDE_SPP, p)
    two = dev.run(f["beauty"], SPP, f["albedo"], GUIDE_SPP, f["normal"], GUIDE_SPP, p)
    assert np.array_equal(one.cpu().numpy().view(np.uint32), two.cpu().numpy().view(np.uint32))
    host = product.denoise(f["beauty"].cpu().numpy(), SPP, f["albedo"].cpu().numpy(), GUIDE_SPP, f["normal"].cpu().numpy(), GUIDE_SPP, p)
    assert np.array_equal(host.view(np.uint32), one.cpu().numpy().view(np.uint32))
    img = resolve(product, one, 1)
    assert np.isfinite(img).all() and img.min() >= 0.0 and img.max() <= 1.0


@pytest.mark.parametrize("scene_id,bar", [(3, 0.5), (19, 0.75)])
def test_denoise_is_useful(dev, product, rendered, scene_id, bar):
    """RMSE against the GPU's own 256-spp frame, after the resolve (Reinhard + OETF), of the 4-spp film: denoised / noisy <= 0.5 on scene 3
    and <= 0.75 on scene 19 (the NumPy filter on CPU-oracle films gave 0.34 and 0.61)."""
    f = rendered(scene_id)
    den = dev.run(f["beauty"], SPP, f["albedo"], GUIDE_SPP, f["normal"], GUIDE_SPP, product.denoise_params_default())
    ref = resolve(product, f["ref"], REF_SPP).astype(np.float64)
    noisy = float(np.sqrt(np.mean((resolve(product, f["beauty"], SPP) - ref) ** 2)))
    clean = float(np.sqrt(np.mean((resolve(product, den, 1) - ref) ** 2)))
    log_line(f'{{"test": "usefulness", "scene": {scene_id}, "noisy_rmse": {noisy:.4f}, "denoised_rmse": {clean:.4f}, "ratio": {clean / noisy:.3f}}}')
    assert clean / noisy <= bar, (noisy, clean)


def test_denoise_cli(pkg, tmp_path):
    """mi355pt --denoise exits 0 and writes another picture than the run without the flag; with an AOV renderer or --gpus 2 it exits 2."""
    root = pkg.ffi.ROOT
    exe = os.path.join(root, "toy-cpu-pathtracing_amd", "host", "mi355pt")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.dirname(exe)])
    assets_dir = str(tmp_path / "assets")
    subprocess.check_call([sys.executable, os.path.join(root, "tools", "export_assets.py"), assets_dir])
    env = dict(os.environ, MI355PT_ASSETS=assets_dir, MI355PT_DATA=os.path.join(root, "toy-cpu-pathtracing_amd", "data"))
    base = [exe, "--scene", "3", "--renderer", "mis", "--sampler", "sobol", "--spp", "4", "--width", "64", "--height", "48"]
    plain, den = str(tmp_path / "plain.png"), str(tmp_path / "x.png")
    r = subprocess.run(base + ["-o", plain], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run(base + ["--denoise", "-o", den], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "Finish rendering" in r.stdout
    a, b = open(plain, "rb").read(), open(den, "rb").read()
    assert len(b) > 100 and a != b
    r = subprocess.run([exe, "--scene", "3", "--renderer", "normal", "--denoise"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--denoise" in r.stderr
    r = subprocess.run(base + ["--denoise", "--gpus", "2"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "one GPU" in r.stderr
