"""GPU tests of the variance-guided denoiser (mi355pt_denoise_var_device / mi355pt_denoise_var, csrc/pt_kernels_denoise_var.hip) against the
NumPy restatement of tests/denoise_var_reference.py.  The measure is the shipped denoiser's: max |x - ref64| / (|ref64| + 1e-3) over EVERY
value of the frame; the bar of a case is 8 times what the f32 restatement itself shows on that case (e32): the factor covers the hardware
exp2, another summation order over 25 taps x levels and the luminance difference taken on the sums, while a wrong tap or a missing term
shows at 1e-3 and more."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import denoise_reference as dr  # noqa: E402
import denoise_var_reference as dv  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (3, 2), (7, 5), (64, 1), (1, 64), (67, 35), (130, 70)]    # (W, H): below a wave, ragged edges, one row, one column, > 1 block
LEVELS = [1, 5, 8]
GUIDES = {"both": (True, True), "normal": (False, True), "albedo": (True, False), "none": (False, False)}
SPPS = (4, 64, 64)
FACTOR = 8.0


def log_line(text):
    print(text)
    if os.environ.get("MI355PT_FRAME_LOG"):
        with open(os.environ["MI355PT_FRAME_LOG"], "a") as f:
            f.write(text + "\n")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class Device:
    """films on the device + one call of mi355pt_denoise_var_device; the output starts as NaN, so a pixel the kernels leave out shows"""

    def __init__(self, product):
        import torch
        self.torch, self.product = torch, product

    def up(self, x):
        if x is None:
            return None
        x = np.ascontiguousarray(x)
        return self.torch.from_numpy(x.view(np.int32) if x.dtype == np.uint32 else x.astype(np.float32)).cuda()

    def run(self, b, h, sb, t, a, sa, n, sn, params):
        torch = self.torch
        H, W, _ = b.shape
        need = self.product.denoise_var_scratch_bytes(W, H)
        scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
        out = torch.full((H, W, 3), float("nan"), dtype=torch.float32, device="cuda")
        ptr = lambda x: x.data_ptr() if x is not None else None   # noqa: E731
        self.product.denoise_var_device(b.data_ptr(), h.data_ptr(), sb, ptr(t), ptr(a), sa, ptr(n), sn, W, H, params, scratch.data_ptr(), need,
                                        out.data_ptr(), None)
        torch.cuda.synchronize()
        return out


@pytest.fixture(scope="module")
def dev(product):
    return Device(product)


def make_params(product, **kw):
    p = product.denoise_var_params_default()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def check_against_reference(dev, product, films, spp_b, tiles, spp_g, guides, levels, tag):
    b, h, a, n = films
    use_a, use_n = GUIDES[guides]
    a, n = (a if use_a else None), (n if use_n else None)
    ref64 = dv.denoise(b, h, spp_b, tiles, a, spp_g, n, spp_g, levels=levels, dtype=np.float64)
    ref32 = dv.denoise(b, h, spp_b, tiles, a, spp_g, n, spp_g, levels=levels, dtype=np.float32)
    e32 = dv.rel_err(ref32, ref64)
    got = dev.run(dev.up(b), dev.up(h), spp_b, dev.up(tiles), dev.up(a), spp_g, dev.up(n), spp_g, make_params(product, levels=levels)).cpu().numpy()
    assert np.isfinite(got).all(), f"{tag}: {int((~np.isfinite(got)).sum())} values not written or not finite"
    egpu = dv.rel_err(got, ref64)
    log_line(f'{{"test": "{tag}", "guides": "{guides}", "levels": {levels}, "e32": {e32:.3e}, "gpu": {egpu:.3e}, '
             f'"ratio": {egpu / e32 if e32 > 0 else 0.0:.2f}}}')
    assert egpu <= FACTOR * e32, (tag, guides, levels, egpu, e32)
    if n is not None:                                                       # background pixels: c, bit for bit
        bg = dv.background(n)
        c = dv.prepass(b, h, spp_b, tiles, dtype=np.float32)[0]
        assert np.array_equal(bits(got[bg]), bits(c[bg])), tag
    return got


@pytest.mark.parametrize("guides", list(GUIDES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_denoise_var_synthetic_parity(dev, product, shape, guides):
    """Seeded synthetic films (piecewise-planar guides, HDR noise up to about 100, a background region, NaN / inf / negative values in the
    film and in the half film) at every shape, level count and guide set: the GPU within 8 e32 of the f64 restatement on every value,
    nothing left out."""
    W, H = shape
    films = dv.synthetic(W, H, *SPPS)
    for levels in LEVELS:
        check_against_reference(dev, product, films, SPPS[0], None, SPPS[1], guides, levels, f"var_synthetic_{W}x{H}")


@pytest.mark.parametrize("guides", list(GUIDES))
def test_denoise_var_tile_counts_parity(dev, product, guides):
    """19 x 13 = 3 x 2 tiles, partial on both edges, with tile counts drawn from {2, 4, 8}: the same bar; and uniform counts are bit-equal
    to the same spp_beauty without counts."""
    W, H = 19, 13
    b, h, t, a, n = dv.synthetic_tiles(W, H, SPPS[1], SPPS[2])
    assert set(t.reshape(-1).tolist()) == {2, 4, 8}
    for levels in LEVELS:
        check_against_reference(dev, product, (b, h, a, n), 0, t, SPPS[1], guides, levels, f"var_tiles_{W}x{H}")
    use_a, use_n = GUIDES[guides]
    fb, fh, fa, fn = dv.synthetic(W, H, *SPPS)
    args = (dev.up(fa) if use_a else None, SPPS[1], dev.up(fn) if use_n else None, SPPS[2], make_params(product))
    one = dev.run(dev.up(fb), dev.up(fh), 4, None, *args).cpu().numpy()
    two = dev.run(dev.up(fb), dev.up(fh), 0, dev.up(np.full((2, 3), 4, np.uint32)), *args).cpu().numpy()
    assert np.array_equal(bits(one), bits(two))


def test_denoise_var_is_deterministic_and_host_form_matches(dev, product):
    """Two calls are bit-equal; mi355pt_denoise_var on host buffers is bit-equal to mi355pt_denoise_var_device, with and without tile
    counts and guides; every value is written (the output starts as NaN)."""
    W, H = 67, 35
    b, h, a, n = dv.synthetic(W, H, *SPPS)
    p = product.denoise_var_params_default()
    one = dev.run(dev.up(b), dev.up(h), 4, None, dev.up(a), 64, dev.up(n), 64, p).cpu().numpy()
    two = dev.run(dev.up(b), dev.up(h), 4, None, dev.up(a), 64, dev.up(n), 64, p).cpu().numpy()
    assert np.isfinite(one).all() and np.array_equal(bits(one), bits(two))
    assert np.array_equal(bits(product.denoise_var(b, h, 4, None, a, 64, n, 64, p)), bits(one))
    bare = dev.run(dev.up(b), dev.up(h), 4, None, None, 0, None, 0, p).cpu().numpy()
    assert np.isfinite(bare).all() and np.array_equal(bits(product.denoise_var(b, h, 4, params=p)), bits(bare))
    tb, th, t, ta, tn = dv.synthetic_tiles(19, 13, 64, 64)
    tiled = dev.run(dev.up(tb), dev.up(th), 0, dev.up(t), dev.up(ta), 64, dev.up(tn), 64, p).cpu().numpy()
    assert np.isfinite(tiled).all() and np.array_equal(bits(product.denoise_var(tb, th, 0, t, ta, 64, tn, 64, p)), bits(tiled))


# ---------------------------------------------------------------- rendered films
RW, RH, GUIDE_SPP, REF_SPP = 160, 120, 64, 1024


class Rendered:
    """one scene on the device (mis + ZSobol): guides at 64 spp and the 1024-spp frame once, and per spp the pair the filter takes —
    H = [0, spp / 2), F = H + [spp / 2, spp) with the sequence of that spp"""

    def __init__(self, product, pkg, scene_id, w=RW, h=RH, want_ref=True):
        import torch
        self.torch, self.product, self.pkg, self.w, self.h = torch, product, pkg, w, h
        self.sc = product.new_scene()
        self.cam = pkg.scenes.load_scene(self.sc, scene_id, w, h, build=False)
        self.d65 = self.sc.add_lut470(pkg.scenes.presets()["cie_illum_d6500"])
        self.sc.build(self.cam)
        self.albedo, self.normal = self.zeros(), self.zeros()
        g = pkg.make_params(GUIDE_SPP, "mis", "sobol")
        product.render_aov_accum_device(self.sc, self.cam, g, pkg.ffi.AOV_ALBEDO, self.d65, 0, GUIDE_SPP, self.albedo.data_ptr(), None)
        product.render_aov_accum_device(self.sc, self.cam, g, pkg.ffi.AOV_SHADING_NORMAL, self.d65, 0, GUIDE_SPP, self.normal.data_ptr(), None)
        self.ref = None
        if want_ref:
            ref = self.zeros()
            product.render_accum_device(self.sc, self.cam, pkg.make_params(REF_SPP, "mis", "sobol"), 0, REF_SPP, ref.data_ptr(), None)
            self.ref = self.resolve(ref, REF_SPP).astype(np.float64)
        self._pairs = {}

    def zeros(self):
        return self.torch.zeros((self.h, self.w, 3), dtype=self.torch.float32, device="cuda")

    def pair(self, spp):
        if spp not in self._pairs:
            prm = self.pkg.make_params(spp, "mis", "sobol")
            half = self.zeros()
            self.product.render_accum_device(self.sc, self.cam, prm, 0, spp // 2, half.data_ptr(), None)
            film = half.clone()
            self.product.render_accum_device(self.sc, self.cam, prm, spp // 2, spp, film.data_ptr(), None)
            self.torch.cuda.synchronize()
            self._pairs[spp] = (film, half)
        return self._pairs[spp]

    def resolve(self, film, spp):
        out = self.torch.empty_like(film)
        self.product.film_resolve_device(film.data_ptr(), film.shape[0] * film.shape[1], spp, out.data_ptr(), None)
        self.torch.cuda.synchronize()
        return out.cpu().numpy()


@pytest.fixture(scope="module")
def rendered(product, pkg):
    cache = {}

    def get(scene_id):
        if scene_id not in cache:
            cache[scene_id] = Rendered(product, pkg, scene_id)
        return cache[scene_id]
    return get


def shipped_filter(product, r, film, spp):
    torch = r.torch
    need = product.denoise_scratch_bytes(r.w, r.h)
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    out = torch.full((r.h, r.w, 3), float("nan"), dtype=torch.float32, device="cuda")
    product.denoise_device(film.data_ptr(), spp, r.albedo.data_ptr(), GUIDE_SPP, r.normal.data_ptr(), GUIDE_SPP, r.w, r.h, product.denoise_params_default(),
                           scratch.data_ptr(), need, out.data_ptr(), None)
    torch.cuda.synchronize()
    return out


QUALITY_BARS = {4: 0.97, 16: 0.90, 64: 0.80}
# 256 spp has no bar of its own in the filter's specification: the ratio falls as the frame converges (CPU oracle films: 0.57 / 0.30 at
# 256 spp against 0.68 / 0.39 at 64 spp), so the case keeps the 64-spp bar and logs its three figures
QUALITY_SPPS = sorted(QUALITY_BARS) + [256]


@pytest.mark.parametrize("spp", QUALITY_SPPS)
@pytest.mark.parametrize("scene_id", [3, 19])
def test_denoise_var_beats_the_shipped_filter(dev, product, rendered, scene_id, spp):
    """Scenes 3 and 19 at 160 x 120, mis + ZSobol, guides at 64 spp, RMSE after the resolve (Reinhard + OETF) against the GPU's own 1024-spp
    frame, both filters on the same film with their default parameters: variance-guided / shipped below 0.97 at 4 spp, 0.90 at 16 spp and
    0.80 at 64 spp and at 256 spp, and from 64 spp on the variance-guided filter also below the unfiltered frame (the NumPy filters on
    CPU-oracle films gave 0.89 / 0.81 / 0.68 / 0.57 on scene 3 and 0.93 / 0.55 / 0.39 / 0.30 on scene 19)."""
    r = rendered(scene_id)
    film, half = r.pair(spp)
    new = dev.run(film, half, spp, None, r.albedo, GUIDE_SPP, r.normal, GUIDE_SPP, product.denoise_var_params_default())
    old = shipped_filter(product, r, film, spp)

    def rmse(img):
        return float(np.sqrt(np.mean((img - r.ref) ** 2)))
    e_raw, e_old, e_new = rmse(r.resolve(film, spp)), rmse(r.resolve(old, 1)), rmse(r.resolve(new, 1))
    log_line(f'{{"test": "var_quality", "scene": {scene_id}, "spp": {spp}, "unfiltered_rmse": {e_raw:.4f}, "shipped_rmse": {e_old:.4f}, '
             f'"variance_guided_rmse": {e_new:.4f}, "ratio_to_shipped": {e_new / e_old:.3f}}}')
    assert e_new / e_old < QUALITY_BARS[min(spp, 64)], (e_raw, e_old, e_new)
    if spp >= 64:
        assert e_new < e_raw, (e_raw, e_new)


@pytest.mark.parametrize("scene_id", [3, 19])
def test_denoise_var_rendered_parity(dev, product, rendered, scene_id):
    """The 16-spp pair of the quality test with default parameters against the restatement: the same bar as the synthetic films, and
    background pixels bit-equal to c."""
    r = rendered(scene_id)
    film, half = r.pair(16)
    films = (film.cpu().numpy(), half.cpu().numpy(), r.albedo.cpu().numpy(), r.normal.cpu().numpy())
    assert np.isfinite(films[2]).all() and np.isfinite(films[3]).all()
    check_against_reference(dev, product, films, 16, None, GUIDE_SPP, "both", 5, f"var_rendered_scene{scene_id}")


def adaptive_state(product, pkg, r, threshold, min_spp, max_spp):
    """mi355pt_render_adaptive_device on r's scene -> film, half, tile_spp, tile_err (device tensors)"""
    torch = r.torch
    nt = ((r.w + 7) // 8) * ((r.h + 7) // 8)
    film, half = r.zeros(), r.zeros()
    spp, lst = torch.zeros(nt, dtype=torch.int32, device="cuda"), torch.zeros(nt, dtype=torch.int32, device="cuda")
    err = torch.zeros(nt, dtype=torch.float32, device="cuda")
    scratch = torch.zeros(product.adaptive_scratch_bytes(r.w, r.h), dtype=torch.uint8, device="cuda")
    product.render_adaptive_device(r.sc, r.cam, pkg.make_params(max_spp, "mis", "sobol"), pkg.ffi.AdaptiveParams(threshold, 1e-3, min_spp), film.data_ptr(),
                                   half.data_ptr(), spp.data_ptr(), err.data_ptr(), lst.data_ptr(), scratch.data_ptr(), scratch.numel(), None)
    torch.cuda.synchronize()
    return film, half, spp, err


def test_denoise_var_composes_with_the_adaptive_driver(dev, product, pkg):
    """mi355pt_render_adaptive_device on scene 3 at 64 x 48 (min 4, max 64, the threshold the median
    tile error at 4 spp, so that about half of the tiles sample on), then mi355pt_denoise_var_device on its F, H and tile_spp as they
    are — no normalise step —: within the bar of the restatement on the same buffers read back, with more than one count in the frame."""
    r = Rendered(product, pkg, 3, 64, 48, want_ref=False)
    _, _, _, err = adaptive_state(product, pkg, r, 3e38, 4, 64)           # a threshold nothing exceeds: the errors at min_spp, nothing sampled on
    threshold = float(np.median(err.cpu().numpy()))
    assert np.isfinite(threshold) and threshold > 0
    film, half, spp, _ = adaptive_state(product, pkg, r, threshold, 4, 64)
    t = spp.cpu().numpy().view(np.uint32).reshape(6, 8)
    counts = sorted(set(t.reshape(-1).tolist()))
    log_line(f'{{"test": "var_composition_counts", "tiles_per_count": {json.dumps({str(n): int((t == n).sum()) for n in counts})}}}')
    assert len(counts) > 1 and all(n in (4, 8, 16, 32, 64) for n in counts)
    films = (film.cpu().numpy(), half.cpu().numpy(), r.albedo.cpu().numpy(), r.normal.cpu().numpy())
    got = check_against_reference(dev, product, films, 0, t, GUIDE_SPP, "both", 5, "var_composition_scene3")
    img = r.resolve(r.torch.from_numpy(got).cuda(), 1)
    assert np.isfinite(img).all() and img.min() >= 0.0 and img.max() <= 1.0


def test_denoise_var_cli(dev, product, pkg, tmp_path):
    """mi355pt --denoise-variance alone and with --adaptive-threshold: the PNG is quantize_u8 of the same calls made through the ABI; with
    --denoise, an AOV renderer, an odd --spp or --gpus 2 it exits 2."""
    from PIL import Image
    root = pkg.ffi.ROOT
    exe = os.path.join(root, "toy-cpu-pathtracing_amd", "host", "mi355pt")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.dirname(exe)])
    assets_dir = str(tmp_path / "assets")
    subprocess.check_call([sys.executable, os.path.join(root, "tools", "export_assets.py"), assets_dir])
    env = dict(os.environ, MI355PT_ASSETS=assets_dir, MI355PT_DATA=os.path.join(root, "toy-cpu-pathtracing_amd", "data"))
    W, H, SPP = 64, 48, 32
    base = [exe, "--scene", "3", "--renderer", "mis", "--sampler", "sobol", "--spp", str(SPP), "--width", str(W), "--height", str(H)]
    r = Rendered(product, pkg, 3, W, H, want_ref=False)

    def compare(png, linear_mean, tag):
        cli = np.asarray(Image.open(png).convert("RGB"))
        ref = product.quantize_u8(r.resolve(linear_mean, 1))
        diff = int((cli != ref).sum())
        log_line(f'{{"test": "var_cli", "case": "{tag}", "values": {ref.size}, "different": {diff}, "max_abs": {int(np.abs(cli.astype(int) - ref.astype(int)).max())}}}')
        assert cli.shape == ref.shape and diff == 0, tag
    plain, adaptive = str(tmp_path / "v.png"), str(tmp_path / "va.png")
    run = subprocess.run(base + ["--denoise-variance", "--denoise-sigma-lum", "3", "-o", plain], env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    assert "Finish rendering" in run.stdout
    film, half = r.pair(SPP)
    compare(plain, dev.run(film, half, SPP, None, r.albedo, GUIDE_SPP, r.normal, GUIDE_SPP, make_params(product, sigma_lum=3.0)), "plain")
    run = subprocess.run(base + ["--denoise-variance", "--adaptive-threshold", "0.05", "--adaptive-min-spp", "4", "-o", adaptive], env=env, capture_output=True,
                         text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    assert "adaptive:" in run.stdout
    film, half, spp, _ = adaptive_state(product, pkg, r, 0.05, 4, SPP)
    compare(adaptive, dev.run(film, half, 0, spp, r.albedo, GUIDE_SPP, r.normal, GUIDE_SPP, product.denoise_var_params_default()), "adaptive")
    assert open(plain, "rb").read() != open(adaptive, "rb").read()
    for extra, word in ((["--denoise-variance", "--denoise"], "--denoise"), (["--denoise-variance", "--gpus", "2"], "one GPU"),
                        (["--denoise-variance", "--spp", "7"], "even"), (["--denoise-sigma-lum", "3"], "--denoise-variance")):
        run = subprocess.run(base + extra, env=env, capture_output=True, text=True, timeout=300)
        assert run.returncode == 2 and word in run.stderr, (extra, run.stderr)
    run = subprocess.run([exe, "--scene", "3", "--renderer", "normal", "--denoise-variance"], env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 2 and "--denoise-variance" in run.stderr


def test_denoise_var_error_codes_on_a_built_scene(dev, product, pkg):
    """The documented refusals with real device buffers around a built scene's films: -1 (MI355PT_E_INVALID) with a message, the output
    untouched; the next valid call still succeeds and is bit-equal to the call before."""
    import ctypes
    r = Rendered(product, pkg, 3, 64, 48, want_ref=False)
    torch = r.torch
    film, half = r.pair(4)
    p = product.denoise_var_params_default()
    before = dev.run(film, half, 4, None, r.albedo, GUIDE_SPP, r.normal, GUIDE_SPP, p).cpu().numpy()
    need = product.denoise_var_scratch_bytes(r.w, r.h)
    scratch = torch.empty(need + 16, dtype=torch.uint8, device="cuda")
    out = torch.full((r.h, r.w, 3), 7.0, dtype=torch.float32, device="cuda")
    tiles = torch.full((48,), 4, dtype=torch.int32, device="cuda")
    lib = product.lib

    def call(b=film.data_ptr(), h=half.data_ptr(), sb=4, t=0, sa=GUIDE_SPP, sn=GUIDE_SPP, w=r.w, hh=r.h, prm=p, s=scratch.data_ptr(), sbytes=need, o=out.data_ptr()):
        return lib.mi355pt_denoise_var_device(ctypes.c_void_p(b), ctypes.c_void_p(h), sb, ctypes.c_void_p(t), ctypes.c_void_p(r.albedo.data_ptr()), sa,
                                              ctypes.c_void_p(r.normal.data_ptr()), sn, w, hh, ctypes.byref(prm), ctypes.c_void_p(s), sbytes, ctypes.c_void_p(o), None)
    bad = {"null half": dict(h=0), "odd spp": dict(sb=3), "zero spp": dict(sb=0), "spp with tile counts": dict(t=tiles.data_ptr()), "levels 9": dict(prm=make_params(product, levels=9)),
           "zeroed params": dict(prm=pkg.ffi.DenoiseVarParams()), "lum_eps 0": dict(prm=make_params(product, lum_eps=0.0)), "guide spp 0": dict(sa=0),
           "out = half": dict(o=half.data_ptr()), "out = beauty": dict(o=film.data_ptr()), "scratch too small": dict(sbytes=need - 1),
           "scratch misaligned": dict(s=scratch.data_ptr() + 4), "width 0": dict(w=0)}
    for name, kw in bad.items():
        assert call(**kw) == -1, name
        assert b"denoise_var" in lib.mi355pt_last_error(), name
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert np.array_equal(bits(out.cpu().numpy()), bits(before))
