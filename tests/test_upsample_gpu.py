"""GPU tests of guided half-resolution rendering (mi355pt_upsample_device / mi355pt_upsample, csrc/pt_kernels_upsample.hip) against the NumPy
restatement of tests/upsample_reference.py.  Every operation of the kernel is a single binary32 operation in the order the header states, so
the bar is BIT EQUALITY on every output value; the outputs start as NaN, so a value the kernel leaves out shows."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import denoise_var_reference as dv  # noqa: E402
import temporal_reference as tr  # noqa: E402
import upsample_reference as ur  # noqa: E402

pytestmark = pytest.mark.gpu

# (W, H) of the FULL frame: one low pixel, both edge clamps, one low row, one low column, ragged blocks, more than one block
SHAPES = [(2, 2), (4, 2), (2, 4), (6, 4), (128, 2), (2, 128), (66, 34), (130, 70)]
W3, H3 = 64, 48                  # the rendered tests: scene 3, low 32 x 24
GUIDE_SPP, FRAME_SPP = 16, 64


def log_line(text):
    print(text)
    if os.environ.get("MI355PT_FRAME_LOG"):
        with open(os.environ["MI355PT_FRAME_LOG"], "a") as f:
            f.write(text + "\n")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def ffi_params(product, prm):
    p = product.upsample_params_default()
    if prm is not None:
        for k in ur.DEFAULTS:
            setattr(p, k, float(getattr(prm, k)))
    return p


class Device:
    """films on the device + one call of mi355pt_upsample_device; the outputs start as NaN"""

    def __init__(self, product, pkg):
        import torch
        self.torch, self.product, self.pkg = torch, product, pkg

    def up(self, a):
        if a is None:
            return None
        if isinstance(a, dict):
            return {k: self.up(v) for k, v in a.items() if v is not None and k in ur.GUIDES}
        return self.torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()

    def outputs(self, W, H, half):
        nan = lambda *s: self.torch.full(s, float("nan"), dtype=self.torch.float32, device="cuda")   # noqa: E731
        return nan(H, W, 3), (nan(H, W, 3) if half else None)

    def run_device(self, film, half, spp, low, spp_al, full, spp_af, prm=None, outs=None):
        """device tensors in (low / full: dicts of tensors) -> the two output tensors (half None without a half film)"""
        H, W = full["hit"].shape[:2]
        of, oh = outs if outs is not None else self.outputs(W, H, half is not None)
        ptr = lambda d: {k: v.data_ptr() for k, v in d.items()}   # noqa: E731
        self.product.upsample_device(film.data_ptr(), half.data_ptr() if half is not None else None, spp, ptr(low), spp_al, ptr(full), spp_af, W, H,
                                     ffi_params(self.product, prm), of.data_ptr(), oh.data_ptr() if oh is not None else None)
        self.torch.cuda.synchronize()
        return of, oh

    def run(self, film, half, spp, low, spp_al, full, spp_af, prm=None):
        """host arrays in, host arrays out"""
        of, oh = self.run_device(self.up(film), self.up(half), spp, self.up(low), spp_al, self.up(full), spp_af, prm)
        return of.cpu().numpy(), (oh.cpu().numpy() if oh is not None else None)


@pytest.fixture(scope="module")
def dev(product, pkg):
    return Device(product, pkg)


def assert_bit_equal(got, want, tag):
    """every output value bit-equal to the f32 restatement, nothing left unwritten"""
    bad = {}
    for n, g, w in zip(("film", "half"), got, want):
        assert (g is None) == (w is None), (tag, n)
        if g is None:
            continue
        assert not np.isnan(g).any(), f"{tag}: {int(np.isnan(g).sum())} values of out_{n} not written"
        bad[n] = int((bits(g) != bits(w)).sum())
    log_line('{"test": "%s", "values": %d, "mismatching": %d}' % (tag, sum(g.size for g in got if g is not None), sum(bad.values())))
    assert not any(bad.values()), (tag, bad)


def variant(low, full, albedo):
    return (low, full) if albedo else (dict(low, albedo=None), dict(full, albedo=None))


@pytest.mark.parametrize("albedo", [True, False], ids=["albedo", "noalbedo"])
@pytest.mark.parametrize("half", [True, False], ids=["half", "nohalf"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_upsample_synthetic_parity(dev, shape, half, albedo):
    """Seeded synthetic frames (the two-plane step and the plane, HDR noise with NaN / inf / negative film values, a background band, an
    emitter patch, zero-albedo pixels) at every shape, with and without the half film and the albedo films: every output value is bit-equal
    to the f32 restatement, nothing is left unwritten."""
    W, H = shape
    for scene in ("step", "plane"):
        film, hf, spp, low, full, spp_g = ur.synthetic(W, H, scene, half, albedo)
        want = ur.upsample(film, hf, spp, low, spp_g, full, spp_g)
        got = dev.run(film, hf, spp, low, spp_g, full, spp_g)
        assert_bit_equal(got, want, f"upsample_synthetic_{W}x{H}_{'half' if half else 'nohalf'}_{'albedo' if albedo else 'noalbedo'}_{scene}")


def test_upsample_synthetic_parity_other_parameters(dev):
    """the same at one shape with EVERY parameter away from its default (and differing albedo sample counts), with and without the half film"""
    W, H = 66, 34
    prm = ur.params(**ur.OTHER)
    assert all(float(getattr(prm, k)) != float(np.float32(v)) for k, v in ur.DEFAULTS.items())
    for half in (True, False):
        film, hf, spp, low, full, spp_g = ur.synthetic(W, H, "step", half, True, spp=6)
        want = ur.upsample(film, hf, spp, low, spp_g, full, 2 * spp_g, prm, detail=True)
        assert want[2]["fallback"].any() and not want[2]["fallback"].all()
        assert_bit_equal(dev.run(film, hf, spp, low, spp_g, full, 2 * spp_g, prm), want[:2], f"upsample_synthetic_params_{'half' if half else 'nohalf'}")


# ---------------- rendered frames: scene 3 at 64 x 48 from 32 x 24 ----------------
@pytest.fixture(scope="module")
def handle(product, pkg):
    """scene 3 built ONCE, for its 64 x 48 camera; the camera of the low frame from mi355pt_upsample_low_camera"""
    sc, cam, d65 = tr.load_moved(product, pkg, 3, W3, H3)
    return sc, cam, d65, product.upsample_low_camera(cam)


def render_frame(product, pkg, handle, seed, spp=FRAME_SPP, guide_spp=GUIDE_SPP):
    """one frame's device films: the G-buffer sums of both resolutions at guide_spp, the low half film [0, spp / 2) and the low film [0, spp)"""
    import torch
    sc, cam, d65, low_cam = handle
    z = lambda h, w: torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")   # noqa: E731
    full = {k: z(H3, W3) for k in ur.GUIDES}
    low = {k: z(H3 // 2, W3 // 2) for k in ur.GUIDES}
    gp = pkg.make_params(guide_spp, "mis", "sobol", seed=seed)
    product.render_gbuffer_accum_device(sc, cam, gp, d65, 0, guide_spp, {k: v.data_ptr() for k, v in full.items()})
    product.render_gbuffer_accum_device(sc, low_cam, gp, d65, 0, guide_spp, {k: v.data_ptr() for k, v in low.items()})
    film, half = z(H3 // 2, W3 // 2), z(H3 // 2, W3 // 2)
    prm = pkg.make_params(spp, "mis", "sobol", seed=seed)
    product.render_accum_device(sc, low_cam, prm, 0, spp // 2, half.data_ptr())
    torch.cuda.synchronize()
    film.copy_(half)
    product.render_accum_device(sc, low_cam, prm, spp // 2, spp, film.data_ptr())
    torch.cuda.synchronize()
    return dict(film=film, half=half, low=low, full=full)


def host(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def no_albedo(g):
    return {k: v for k, v in g.items() if k != "albedo"}


@pytest.fixture(scope="module")
def frame0(product, pkg, handle):
    return render_frame(product, pkg, handle, 0)


def resolved(product, film_tensor, spp):
    import torch
    rgb = torch.empty_like(film_tensor)
    product.film_resolve_device(film_tensor.data_ptr(), film_tensor.shape[0] * film_tensor.shape[1], spp, rgb.data_ptr())
    torch.cuda.synchronize()
    return rgb.cpu().numpy().astype(np.float64)


def test_upsample_rendered_parity_and_quality(dev, product, pkg, handle, frame0):
    """Scene 3 rendered at 32 x 24 with the low camera on the scene built for 64 x 48 (guides 16 spp, beauty 64 spp with its half film).  The
    device form and the host form are bit-equal to the restatement on the buffers read back, with and without albedo; with the low film set
    to a_q + albedo_eps every surface pixel with a valid tap comes out as a_p + albedo_eps bit for bit; and the guided frame without albedo
    is nearer the GPU's own 1024-spp full-resolution frame than the pixel-replicated low frame (tone-mapped RMSE)."""
    f = frame0
    film, half, low, full = f["film"].cpu().numpy(), f["half"].cpu().numpy(), host(f["low"]), host(f["full"])
    assert np.isfinite(np.concatenate([v.ravel() for v in list(low.values()) + list(full.values())])).all()
    got = {}
    for alb in (False, True):
        lo, fu = (f["low"], f["full"]) if alb else (no_albedo(f["low"]), no_albedo(f["full"]))
        hlo, hfu = variant(low, full, alb)
        want = ur.upsample(film, half, FRAME_SPP, hlo, GUIDE_SPP, hfu, GUIDE_SPP, detail=True)
        of, oh = dev.run_device(f["film"], f["half"], FRAME_SPP, lo, GUIDE_SPP, fu, GUIDE_SPP)
        assert_bit_equal((of.cpu().numpy(), oh.cpu().numpy()), want[:2], f"upsample_rendered_device_{'albedo' if alb else 'noalbedo'}")
        assert_bit_equal(product.upsample(film, half, FRAME_SPP, hlo, GUIDE_SPP, hfu, GUIDE_SPP), want[:2], f"upsample_rendered_host_{'albedo' if alb else 'noalbedo'}")
        got[alb] = (of, want[2])
    # the constant-irradiance property on the rendered guides
    prm = ur.params()
    a_low = (ur.clip0(low["albedo"] / np.float32(GUIDE_SPP)) + prm.albedo_eps).astype(np.float32)
    of, _ = dev.run(a_low, None, 1, low, GUIDE_SPP, full, GUIDE_SPP)
    info = got[True][1]
    sel = info["surface"] & ~info["fallback"]
    want_a = (ur.clip0(full["albedo"] / np.float32(GUIDE_SPP)) + prm.albedo_eps).astype(np.float32)
    assert sel.sum() > 0.5 * W3 * H3 and np.array_equal(bits(of[sel]), bits(want_a[sel]))
    # guided against replicated, both against the GPU's own 1024-spp frame
    sc, cam, _, _ = handle
    ref = product.render(sc, cam, pkg.make_params(1024, "mis", "sobol", seed=1000)).astype(np.float64)
    e_g = ur.tonemapped_rmse(resolved(product, got[False][0], 2), ref)
    e_a = ur.tonemapped_rmse(resolved(product, got[True][0], 2), ref)
    e_r = ur.tonemapped_rmse(ur.replicate(resolved(product, f["film"], FRAME_SPP)), ref)
    info = got[False][1]
    surface = info["surface"]
    fb = int((info["fallback"] & surface).sum())
    log_line('{"test": "upsample_rendered_64x48", "rmse_guided": %.4f, "rmse_replicated": %.4f, "rmse_guided_albedo": %.4f, "fallback": %d, "surface": %d, "pixels": %d}'
             % (e_g, e_r, e_a, fb, int(surface.sum()), surface.size))
    assert fb < 0.5 * surface.sum(), (fb, int(surface.sum()))
    assert e_g < e_r, (e_g, e_r)


def test_upsample_chain_with_the_variance_denoiser(dev, product, frame0):
    """mi355pt_denoise_var_device(out_film, out_half, 2, ...) on the upsampled pair with the full guides meets that filter's own bar — 8 x e32
    of tests/denoise_var_reference.py — and its result resolves to finite values in [0, 1]."""
    import torch
    f = frame0
    of, oh = dev.run_device(f["film"], f["half"], FRAME_SPP, no_albedo(f["low"]), 0, no_albedo(f["full"]), 0)
    need = product.denoise_var_scratch_bytes(W3, H3)
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    out = torch.full((H3, W3, 3), float("nan"), dtype=torch.float32, device="cuda")
    product.denoise_var_device(of.data_ptr(), oh.data_ptr(), 2, None, f["full"]["albedo"].data_ptr(), GUIDE_SPP, f["full"]["shading_normal"].data_ptr(), GUIDE_SPP,
                               W3, H3, product.denoise_var_params_default(), scratch.data_ptr(), need, out.data_ptr())
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    film, half, a, n = of.cpu().numpy(), oh.cpu().numpy(), f["full"]["albedo"].cpu().numpy(), f["full"]["shading_normal"].cpu().numpy()
    ref64 = dv.denoise(film, half, 2, None, a, GUIDE_SPP, n, GUIDE_SPP, dtype=np.float64)
    e32 = dv.rel_err(dv.denoise(film, half, 2, None, a, GUIDE_SPP, n, GUIDE_SPP, dtype=np.float32), ref64)
    egpu = dv.rel_err(got, ref64)
    log_line('{"test": "upsample_chain_denoise_var", "e32": %.3e, "gpu": %.3e, "ratio": %.2f}' % (e32, egpu, egpu / e32 if e32 > 0 else 0.0))
    assert np.isfinite(got).all() and egpu <= 8.0 * e32, (egpu, e32)
    rgb = resolved(product, out, 1)
    assert np.isfinite(rgb).all() and rgb.min() >= 0.0 and rgb.max() <= 1.0


def test_upsample_chain_with_the_temporal_accumulation(dev, product, pkg, handle, frame0):
    """The upsampled pair as the CURRENT frame (spp 2) of mi355pt_temporal_accumulate_device, first frame and second frame of a static camera:
    bit-equal to temporal_reference.accumulate on the buffers read back."""
    import torch
    sc, cam, _, _ = handle
    frames = [frame0, render_frame(product, pkg, handle, 1)]
    view = product.temporal_view_from_cameras(cam, cam)
    prev_dev, prev_host = None, None
    for k, f in enumerate(frames):
        of, oh = dev.run_device(f["film"], f["half"], FRAME_SPP, no_albedo(f["low"]), 0, no_albedo(f["full"]), 0)
        cur = dict(film=of, half=oh, position=f["full"]["position"], shading_normal=f["full"]["shading_normal"], hit=f["full"]["hit"])
        nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device="cuda")   # noqa: E731
        af, ah, al = nan(H3, W3, 3), nan(H3, W3, 3), nan(H3, W3)
        ptr = lambda d: {n: v.data_ptr() for n, v in d.items()} if d is not None else None   # noqa: E731
        product.temporal_accumulate_device(ptr(cur), 2, ptr(prev_dev), view if prev_dev is not None else None, W3, H3, product.temporal_params_default(),
                                           af.data_ptr(), ah.data_ptr(), al.data_ptr())
        torch.cuda.synchronize()
        want = tr.accumulate(host(cur), 2, prev_host, view if prev_host is not None else None)
        got = (af.cpu().numpy(), ah.cpu().numpy(), al.cpu().numpy())
        assert not any(np.isnan(g).any() for g in got)
        bad = sum(int((bits(g) != bits(w)).sum()) for g, w in zip(got, want))
        log_line('{"test": "upsample_chain_temporal_frame%d", "values": %d, "mismatching": %d}' % (k, sum(g.size for g in got), bad))
        assert bad == 0
        prev_dev = dict(film=af, half=ah, length=al, position=cur["position"], shading_normal=cur["shading_normal"], hit=cur["hit"])
        prev_host = host(prev_dev)
    assert (got[2] == 2).mean() > 0.5                                              # most pixels found their history


def test_upsample_is_deterministic_and_host_form_matches(dev, product):
    """Two calls are bit-equal; mi355pt_upsample on host buffers is bit-equal to the device form, with and without the half film and albedo."""
    W, H = 66, 34
    for half in (True, False):
        for alb in (True, False):
            film, hf, spp, low, full, spp_g = ur.synthetic(W, H, "step", half, alb)
            one, two = dev.run(film, hf, spp, low, spp_g, full, spp_g), dev.run(film, hf, spp, low, spp_g, full, spp_g)
            hostf = product.upsample(film, hf, spp, low, spp_g, full, spp_g)
            for a, b, c in zip(one, two, hostf):
                assert (a is None) == (b is None) == (c is None)
                if a is not None:
                    assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a), bits(c))


def test_upsample_refusals_with_real_buffers(dev, product, pkg):
    """The refusals with device buffers return MI355PT_E_INVALID, the outputs stay untouched (all NaN), and the next valid call is
    bit-equal to the one before."""
    f = pkg.ffi
    W, H = 66, 34
    film, hf, spp, low, full, spp_g = ur.synthetic(W, H, "step", True, True)
    dfilm, dhalf, dl, dfu = dev.up(film), dev.up(hf), dev.up(low), dev.up(full)
    before = [x.cpu().numpy() for x in dev.run_device(dfilm, dhalf, spp, dl, spp_g, dfu, spp_g)]
    outs = dev.outputs(W, H, True)
    good = product.upsample_params_default()
    guides = lambda d, **kw: f.UpsampleGuides(*[dict({k: v.data_ptr() for k, v in d.items()}, **kw).get(k) for k in f.UPSAMPLE_GUIDES])   # noqa: E731
    o = [x.data_ptr() for x in outs]
    ref = lambda x: ctypes.byref(x) if x is not None else None   # noqa: E731
    b, h = dfilm.data_ptr(), dhalf.data_ptr()

    def refused(lf, lh, s, gl, sl, gf, sf, w, hh, p, of, oh):
        rc = product.lib.mi355pt_upsample_device(lf, lh, s, ref(gl), sl, ref(gf), sf, w, hh, ref(p), of, oh, None)
        assert rc == -1 and b"upsample" in product.lib.mi355pt_last_error(), rc
    gl, gf = guides(dl), guides(dfu)
    refused(None, h, spp, gl, spp_g, gf, spp_g, W, H, good, *o)
    refused(b, h, spp, None, spp_g, gf, spp_g, W, H, good, *o)
    refused(b, h, spp, guides(dl, hit=None), spp_g, gf, spp_g, W, H, good, *o)
    refused(b, h, spp, gl, spp_g, guides(dfu, position=None), spp_g, W, H, good, *o)
    refused(b, h, spp, guides(dl, albedo=None), spp_g, gf, spp_g, W, H, good, *o)
    refused(b, h, spp, gl, 0, gf, spp_g, W, H, good, *o)
    refused(b, None, spp, gl, spp_g, gf, spp_g, W, H, good, *o)
    refused(b, h, spp, gl, spp_g, gf, spp_g, W, H, good, o[0], None)
    refused(b, h, 0, gl, spp_g, gf, spp_g, W, H, good, *o)
    refused(b, h, 3, gl, spp_g, gf, spp_g, W, H, good, *o)
    refused(b, h, spp, gl, spp_g, gf, spp_g, 0, H, good, *o)
    refused(b, h, spp, gl, spp_g, gf, spp_g, W - 1, H, good, *o)
    refused(b, h, spp, gl, spp_g, gf, spp_g, W, H - 1, good, *o)
    refused(b, h, spp, gl, spp_g, gf, spp_g, W, H, f.UpsampleParams(), *o)
    refused(b, h, spp, gl, spp_g, gf, spp_g, W, H, None, *o)
    for k, v in (("pos_tol", 0.0), ("min_weight", float("nan")), ("albedo_eps", 0.0), ("emitter_tol", -0.5), ("normal_cos", 1.5)):
        p = product.upsample_params_default(); setattr(p, k, v)
        refused(b, h, spp, gl, spp_g, gf, spp_g, W, H, p, *o)
    refused(b, h, spp, gl, spp_g, gf, spp_g, W, H, good, b, o[1])
    refused(b, h, spp, gl, spp_g, gf, spp_g, W, H, good, o[0], dfu["hit"].data_ptr())
    refused(b, h, spp, gl, spp_g, gf, spp_g, W, H, good, dl["albedo"].data_ptr(), o[1])
    refused(b, h, spp, gl, spp_g, gf, spp_g, W, H, good, o[0], o[0])
    dev.torch.cuda.synchronize()
    assert all(np.isnan(x.cpu().numpy()).all() for x in outs)
    after = [x.cpu().numpy() for x in dev.run_device(dfilm, dhalf, spp, dl, spp_g, dfu, spp_g, None, outs)]
    assert all(np.array_equal(bits(a), bits(c)) for a, c in zip(before, after))


# ---------------- the CLI ----------------
CLI_SPP = 4


@pytest.fixture(scope="module")
def cli(pkg, tmp_path_factory):
    root = pkg.ffi.ROOT
    exe = os.path.join(root, "toy-cpu-pathtracing_amd", "host", "mi355pt")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.dirname(exe)])
    assets_dir = str(tmp_path_factory.mktemp("assets"))
    subprocess.check_call([sys.executable, os.path.join(root, "tools", "export_assets.py"), assets_dir])
    return exe, dict(os.environ, MI355PT_ASSETS=assets_dir, MI355PT_DATA=os.path.join(root, "toy-cpu-pathtracing_amd", "data"))


def replay(product, pkg, dev, frames, spp, guide_spp, variance, temporal):
    """the calls of `mi355pt --half-res` through the ABI -> the u8 picture"""
    import torch
    sc = product.new_scene()
    cam = pkg.scenes.load_scene(sc, 3, W3, H3, build=False)
    d65 = sc.add_lut470(pkg.scenes.presets()["cie_illum_d6500"])
    sc.build(cam)
    low_cam = product.upsample_low_camera(cam)
    view = product.temporal_view_from_cameras(cam, cam)
    z = lambda h, w, c=3: torch.zeros((h, w, c) if c else (h, w), dtype=torch.float32, device="cuda")   # noqa: E731
    acc, g = None, None
    for k in range(frames):
        names = ("shading_normal", "position", "hit")
        full = {n: z(H3, W3) for n in names + (("albedo",) if variance else ())}
        low = {n: z(H3 // 2, W3 // 2) for n in names}
        gp = pkg.make_params(guide_spp, "mis", "sobol", seed=k)
        product.render_gbuffer_accum_device(sc, cam, gp, d65, 0, guide_spp, {n: v.data_ptr() for n, v in full.items()})
        product.render_gbuffer_accum_device(sc, low_cam, gp, d65, 0, guide_spp, {n: v.data_ptr() for n, v in low.items()})
        prm = pkg.make_params(spp, "mis", "sobol", seed=k)
        film, half = z(H3 // 2, W3 // 2), None
        if variance:
            half = z(H3 // 2, W3 // 2)
            product.render_accum_device(sc, low_cam, prm, 0, spp // 2, half.data_ptr())
            torch.cuda.synchronize()
            film.copy_(half)
            product.render_accum_device(sc, low_cam, prm, spp // 2, spp, film.data_ptr())
        else:
            product.render_accum_device(sc, low_cam, prm, 0, spp, film.data_ptr())
        torch.cuda.synchronize()
        pair = dev.run_device(film, half, spp, low, guide_spp, no_albedo(full), guide_spp)
        if temporal:
            cur = dict(film=pair[0], position=full["position"], shading_normal=full["shading_normal"], hit=full["hit"])
            if variance:
                cur["half"] = pair[1]
            prev = None
            if acc is not None:
                prev = dict(film=acc[0], length=acc[2], position=g["position"], shading_normal=g["shading_normal"], hit=g["hit"])
                if variance:
                    prev["half"] = acc[1]
            out = (z(H3, W3), z(H3, W3) if variance else None, z(H3, W3, 0))
            ptr = lambda d: {n: v.data_ptr() for n, v in d.items()} if d is not None else None   # noqa: E731
            product.temporal_accumulate_device(ptr(cur), 2 if variance else 1, ptr(prev), view if prev is not None else None, W3, H3,
                                               product.temporal_params_default(), out[0].data_ptr(), out[1].data_ptr() if variance else None, out[2].data_ptr())
            torch.cuda.synchronize()
            acc, pair = out, (out[0], out[1])
        g = full
    film = pair[0]
    if variance:
        need = product.denoise_var_scratch_bytes(W3, H3)
        scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
        film = z(H3, W3)
        product.denoise_var_device(pair[0].data_ptr(), pair[1].data_ptr(), 2, None, g["albedo"].data_ptr(), guide_spp, g["shading_normal"].data_ptr(), guide_spp,
                                   W3, H3, product.denoise_var_params_default(), scratch.data_ptr(), need, film.data_ptr())
    rgb = torch.empty_like(film)
    product.film_resolve_device(film.data_ptr(), W3 * H3, 1, rgb.data_ptr())
    torch.cuda.synchronize()
    return product.quantize_u8(rgb.cpu().numpy())


@pytest.mark.parametrize("mode", ["alone", "denoise_variance", "temporal"])
def test_upsample_cli(product, pkg, dev, cli, tmp_path, mode):
    """`--half-res` at 64 x 48 alone, with --denoise-variance and with --temporal-frames 2: the PNG equals quantize_u8 of the same calls
    replayed through the ABI; the documented misuse cases exit 2 with a message naming --half-res."""
    from PIL import Image
    exe, env = cli
    variance, temporal = mode == "denoise_variance", mode == "temporal"
    args = [exe, "--scene", "3", "--renderer", "mis", "--sampler", "sobol", "--spp", str(CLI_SPP), "--width", str(W3), "--height", str(H3),
            "--denoise-guide-spp", str(GUIDE_SPP), "--half-res"] + (["--denoise-variance"] if variance else []) + (["--temporal-frames", "2"] if temporal else [])
    path = str(tmp_path / "h.png")
    r = subprocess.run(args + ["-o", path], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = np.asarray(Image.open(path).convert("RGB"))
    want = replay(product, pkg, dev, 2 if temporal else 1, CLI_SPP, GUIDE_SPP, variance, temporal)
    assert got.shape == want.shape == (H3, W3, 3) and np.array_equal(got, want), int((got != want).sum())
    assert got.mean() > 10.0
    if mode == "alone":
        for bad in ur.CLI_MISUSE:
            r = subprocess.run([exe, *bad], env=env, capture_output=True, text=True, timeout=60, cwd=tmp_path)
            assert r.returncode == 2 and "--half-res" in r.stderr, (bad, r.returncode, r.stderr)
