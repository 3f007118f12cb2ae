"""GPU tests of the display stage (mi355pt_display_meter_device / mi355pt_display_device and their host twins, csrc/pt_kernels_display.hip)
against the NumPy restatement of tests/display_reference.py.  Every float step of the kernels is a single binary32 operation in the order the
header states and every count an integer, so the bar is BIT EQUALITY on the meter's record and histogram and on every ENCODE_LINEAR value;
the sRGB encoding, whose powf is the device's, is held to the float64 OETF of the device's own linear output.  Outputs start as a sentinel or
NaN, so a value a kernel leaves out shows; a guard band behind every output must stay as written; the inputs must come back unchanged."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import display_reference as dr  # noqa: E402

pytestmark = pytest.mark.gpu

# smallest frames; the wave edge; the edge of the display's 256-thread block; the edge of the meter's 1024-thread block; ragged multi-block;
# and LARGE, where every block of the meter's first launch makes more than one trip through its grid-stride loop
# (test_large_frame_takes_more_than_one_trip asserts that from the plan)
SMALL = [(1, 1), (1, 3), (63, 1), (64, 1), (65, 1), (255, 1), (256, 1), (257, 1), (1023, 1), (1024, 1), (1025, 1), (66, 34), (130, 70)]
LARGE = (1920, 1080)
SIZES = SMALL + [LARGE]
SIZE_IDS = [f"{w}x{h}" for w, h in SIZES]
W3, H3, SPP3 = 64, 48, 16                      # the rendered tests: scene 3
GUARD = 16                                     # words behind every output
SENTINEL = 0xDEADBEEF
GUARD_VALUE = 12345.0
F32 = np.float32


def log_line(text):
    print(text)
    if os.environ.get("MI355PT_FRAME_LOG"):
        with open(os.environ["MI355PT_FRAME_LOG"], "a") as f:
            f.write(text + "\n")


def ffi_params(product, prm):
    p = product.display_params_default()
    for k in dr.DEFAULTS:
        setattr(p, k, (float if k in dr.FLOAT_FIELDS else int)(getattr(prm, k)))
    return p


def compare(tag, got, want):
    """bit equality of two arrays (f32 or u32) -> logs values compared, values mismatching and the worst distance in ulps (f32 only)"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, want.shape, got.dtype, want.dtype)
    gb, wb = got.view(np.uint32), want.view(np.uint32)
    bad = gb != wb
    worst = 0.0
    if bad.any() and got.dtype == np.float32:
        with np.errstate(all="ignore"):
            d = dr.ulp_distance(got[bad], want[bad].astype(np.float64))
        worst = float(np.nanmax(d)) if np.isfinite(d).any() else float("inf")
    log_line('{"test": "%s", "values": %d, "mismatching": %d, "worst_ulp": %.3f}' % (tag, got.size, int(bad.sum()), worst))
    assert not bad.any(), (tag, int(bad.sum()), np.flatnonzero(bad.ravel())[:8].tolist(), gb.ravel()[bad.ravel()][:8].tolist(), wb.ravel()[bad.ravel()][:8].tolist())


class Device:
    """films on the device + one call of an entry point; outputs start as a sentinel / NaN, guard bands and inputs are checked after the call"""

    def __init__(self, product):
        import torch
        self.torch, self.product = torch, product

    def words(self, n):
        t = self.torch
        return t.full((n + GUARD,), SENTINEL - (1 << 32), dtype=t.int32, device="cuda")

    def host_words(self, tensor):
        return tensor.cpu().numpy().view(np.uint32)

    def up(self, film):
        return self.torch.from_numpy(np.array(film, dtype=np.float32, copy=True)).cuda()

    def meter(self, film, spp, prm, prev=None, alias=False, want_hist=True, d_film=None):
        """-> (record: 8 uint32, hist: 258 uint32 or None)"""
        t = self.torch
        H, W = film.shape[:2]
        d_film = d_film if d_film is not None else self.up(film)
        need = self.product.display_scratch_bytes(W, H)
        assert need > 0 and need % (dr.HIST_WORDS * 4) == 0
        scratch, rec, hist = self.words(need // 4), self.words(dr.RECORD_WORDS), self.words(dr.HIST_WORDS)
        prev_ptr, d_prev = None, None
        if prev is not None:
            p = t.from_numpy(np.ascontiguousarray(prev, dtype=np.uint32).view(np.int32).copy()).cuda()
            if alias:
                rec[:dr.RECORD_WORDS] = p
                prev_ptr = rec.data_ptr()
            else:
                d_prev, prev_ptr = p, p.data_ptr()
        self.product.display_meter_device(d_film.data_ptr(), W, H, spp, ffi_params(self.product, prm), prev_ptr, scratch.data_ptr(), need, rec.data_ptr(),
                                          hist.data_ptr() if want_hist else None)
        t.cuda.synchronize()
        r, h, s = self.host_words(rec), self.host_words(hist), self.host_words(scratch)
        assert (r[dr.RECORD_WORDS:] == SENTINEL).all() and (h[dr.HIST_WORDS:] == SENTINEL).all() and (s[need // 4:] == SENTINEL).all(), "guard band overwritten"
        assert not (s[:need // 4] == SENTINEL).all()
        if not want_hist:
            assert (h == SENTINEL).all()
        assert np.array_equal(dr.bits(d_film.cpu().numpy()), dr.bits(film)), "the film was changed"
        if d_prev is not None:
            assert np.array_equal(self.host_words(d_prev), np.asarray(prev, dtype=np.uint32)), "the previous record was changed"
        return r[:dr.RECORD_WORDS].copy(), (h[:dr.HIST_WORDS].copy() if want_hist else None)

    def display(self, film, spp, prm, record=None, d_film=None):
        """-> (H, W, 3) f32"""
        t = self.torch
        H, W = film.shape[:2]
        n = H * W * 3
        d_film = d_film if d_film is not None else self.up(film)
        out = t.full((n + GUARD,), float("nan"), dtype=t.float32, device="cuda")
        out[n:] = GUARD_VALUE
        d_rec = None
        if record is not None:
            d_rec = t.from_numpy(np.ascontiguousarray(record, dtype=np.uint32).view(np.int32).copy()).cuda()
        self.product.display_device(d_film.data_ptr(), W, H, spp, ffi_params(self.product, prm), d_rec.data_ptr() if d_rec is not None else None, out.data_ptr())
        t.cuda.synchronize()
        o = out.cpu().numpy()
        assert (o[n:] == GUARD_VALUE).all(), "guard band overwritten"
        assert np.array_equal(dr.bits(d_film.cpu().numpy()), dr.bits(film)), "the film was changed"
        if d_rec is not None:
            assert np.array_equal(self.host_words(d_rec), np.asarray(record, dtype=np.uint32)), "the record was changed"
        return o[:n].reshape(H, W, 3).copy()


@pytest.fixture(scope="module")
def dev(product):
    return Device(product)


_FRAMES = {}


def frame(W, H, kind, prm=None, **kw):
    """the seeded frames, made once and shared (nobody writes to them: the harness checks that)"""
    key = (W, H, kind, prm.log2_lum_min if prm is not None else None, tuple(sorted(kw.items())))
    if key not in _FRAMES:
        film, spp = dr.frame(W, H, kind, prm=prm, **kw)
        film.setflags(write=False)
        _FRAMES[key] = (film, spp)
    return _FRAMES[key]


PREV = np.array([dr.bits(np.array([3.25], np.float32))[0], 1, 2, 3, 4, 5, 6, 7], np.uint32)      # a previous record: E = 3.25


def check_meter(dev, tag, film, spp, prm, prev=None, alias=False):
    want_rec, want_hist, info = dr.meter(film, spp, prm, prev)
    rec, hist = dev.meter(film, spp, prm, prev, alias)
    assert not (rec == SENTINEL).any() and not (hist == SENTINEL).any(), f"{tag}: words not written"
    compare(tag + "_hist", hist, want_hist)
    compare(tag + "_record", rec, want_rec)
    return rec, info


# ---------------- the meter ----------------
def test_large_frame_takes_more_than_one_trip(product):
    """LARGE qualifies: from the plan (rows = scratch bytes / (258 x 4), chunks of 1024 pixels), every block has at least two chunks; the
    small frames have one chunk per block, 130 x 70 nine blocks"""
    W, H = LARGE
    rows = product.display_scratch_bytes(W, H) // (dr.HIST_WORDS * 4)
    chunks = -(-W * H // 1024)
    assert rows == 256 and chunks >= 2 * rows
    for w, h in SMALL:
        assert product.display_scratch_bytes(w, h) // (dr.HIST_WORDS * 4) == -(-w * h // 1024)
    assert product.display_scratch_bytes(130, 70) // (dr.HIST_WORDS * 4) == 9


@pytest.mark.parametrize("shape", SIZES, ids=SIZE_IDS)
def test_meter_parity(dev, shape):
    """Record and histogram bit-equal to the restatement at every size, with the defaults and with every parameter off its default, on: a
    log-uniform frame over 2^-24 .. 2^24 with zeros, negatives, NaN, +-inf and subnormals in all three channels; a frame of luminances
    exactly on every bin edge and both range ends and one ulp to either side; a constant frame; frames entirely out of range."""
    W, H = shape
    for pname, prm in (("default", dr.params()), ("other", dr.params(**dr.OTHER))):
        for kind in ("loguniform", "edges", "constant") + (("above", "black") if shape != LARGE else ()):      # (LARGE: the three that differ by size)
            film, spp = frame(W, H, kind, prm if kind == "edges" else None)
            _, info = check_meter(dev, f"display_meter_{W}x{H}_{pname}_{kind}", film, spp, prm)
            if kind in ("above", "black"):
                assert info["Np"] == 0
    film, spp = frame(W, H, "below")
    check_meter(dev, f"display_meter_{W}x{H}_below_prev", film, spp, dr.params(adapt=0.25), PREV)


@pytest.mark.parametrize("alias", [False, True], ids=["apart", "in_place"])
@pytest.mark.parametrize("adapt", [0.0, 0.25, 1.0])
def test_meter_previous_record(dev, adapt, alias):
    """With a previous record — in a buffer of its own, and as the output record itself — and adapt 0, 0.25 and 1: bit-equal to the
    restatement; adapt 1 gives E = E_t in bits, adapt 0 the previous E."""
    W, H = 130, 70
    prm = dr.params(adapt=adapt)
    for kind in ("loguniform", "constant", "above"):
        film, spp = frame(W, H, kind)
        rec, info = check_meter(dev, f"display_meter_prev_{kind}_adapt{adapt}_{'in_place' if alias else 'apart'}", film, spp, prm, PREV, alias)
        if adapt == 1.0 or kind == "above":
            assert rec[0] == rec[1]
        if adapt == 0.0 or kind == "above":
            assert rec[0] == PREV[0]
        assert (info["Np"] == 0) == (kind == "above")


def test_meter_is_deterministic_and_host_form_matches(dev, product):
    """Two runs are bit-equal; mi355pt_display_meter on host buffers is bit-equal to the device form, with and without a previous record and
    a histogram."""
    for (W, H) in ((66, 34), (257, 1)):
        film, spp = frame(W, H, "loguniform")
        for prm, prev in ((dr.params(), None), (dr.params(**dr.OTHER), PREV)):
            one, two = dev.meter(film, spp, prm, prev), dev.meter(film, spp, prm, prev)
            host = product.display_meter(film, spp, ffi_params(product, prm), prev)
            assert np.array_equal(one[0], two[0]) and np.array_equal(one[1], two[1])
            compare(f"display_meter_host_{W}x{H}_{'prev' if prev is not None else 'first'}_record", host[0], one[0])
            compare(f"display_meter_host_{W}x{H}_{'prev' if prev is not None else 'first'}_hist", host[1], one[1])
            rec, none = dev.meter(film, spp, prm, prev, want_hist=False)
            assert none is None and np.array_equal(rec, one[0])
            rec, none = product.display_meter(film, spp, ffi_params(product, prm), prev, want_hist=False)
            assert none is None and np.array_equal(rec, one[0])


def test_meter_sequence_adapts_monotonically(dev):
    """A 4-frame sequence whose film is multiplied by 4 after frame 2, adapt 0.5, one record metered in place: every record follows the
    restatement bit for bit, and after the step E moves monotonically towards the new target without passing it."""
    W, H = 130, 70
    films, spp = dr.sequence(W, H)
    prm = dr.params(adapt=0.5)
    want = dr.run_sequence(films, spp, prm)
    prev, got = None, []
    for k, f in enumerate(films):
        prev, _ = dev.meter(f, spp, prm, prev, alias=prev is not None)
        compare(f"display_sequence_frame{k}_record", prev, want[k])
        got.append(dr.from_bits(prev[:3]).astype(np.float64))
    E, Et = [g[0] for g in got], [g[1] for g in got]
    assert Et[2] < 0.3 * Et[1] and Et[3] < 0.3 * Et[1]                               # four times the light: a quarter of the exposure, roughly
    assert E[1] > E[2] > E[3] > Et[3] and E[2] > Et[2]
    assert abs(E[3] - Et[3]) < abs(E[2] - Et[2]) < abs(E[1] - Et[2])


# ---------------- the display ----------------
def display_cases(W, H):
    """(tag, film, spp, params without tone, record): the constant exposure and an exposure from a record, default and other parameters"""
    film, spp = frame(W, H, "loguniform")
    rec = np.zeros(8, np.uint32); rec[0] = dr.bits(np.array([0.8125], np.float32))[0]
    rec_big = rec.copy(); rec_big[0] = dr.bits(np.array([2.0 ** 9], np.float32))[0]
    return [("const", film, spp, {}, None), ("record", film, spp, {}, rec), ("other_const", film, spp, dict(exposure=dr.OTHER["exposure"], white=dr.OTHER["white"]), None),
            ("other_record", film, spp, dict(white=dr.OTHER["white"]), rec_big)]


@pytest.mark.parametrize("shape", SIZES, ids=SIZE_IDS)
@pytest.mark.parametrize("name", list(dr.TONES))
def test_display_linear_parity(dev, name, shape):
    """ENCODE_LINEAR: every value bit-equal to the restatement, for each operator at every size, on the log-uniform film with the special
    values, with the constant exposure and with E from a record, nothing left unwritten."""
    W, H = shape
    for tag, film, spp, kw, rec in display_cases(W, H):
        prm = dr.params(tone=dr.TONES[name], encode=dr.ENCODE_LINEAR, **kw)
        got = dev.display(film, spp, prm, rec)
        assert not np.isnan(got).any(), f"{int(np.isnan(got).sum())} values not written"
        compare(f"display_linear_{name}_{W}x{H}_{tag}", got, dr.display(film, spp, prm, rec))


@pytest.mark.parametrize("name", list(dr.TONES))
def test_display_srgb_against_float64_oetf(dev, name):
    """ENCODE_SRGB against the float64 OETF of the device's own ENCODE_LINEAR output: within E_host + 4 ulp, E_host being the deviation of
    the f32 restatement of the OETF from float64 over the same inputs (measured here) and 4 the allowance tests/test_film_log_gpu.py grants
    the device's powf; NaN in the same places (there are none); the worst case is logged."""
    worst, e_host, count = 0.0, 0.0, 0
    for (W, H) in ((257, 1), (130, 70)):
        for tag, film, spp, kw, rec in display_cases(W, H):
            lin = dev.display(film, spp, dr.params(tone=dr.TONES[name], encode=dr.ENCODE_LINEAR, **kw), rec)
            got = dev.display(film, spp, dr.params(tone=dr.TONES[name], encode=dr.ENCODE_SRGB, **kw), rec)
            want = dr.srgb_oetf64(lin)
            assert np.array_equal(np.isnan(got), np.isnan(want)) and not np.isnan(got).any()
            e_host = max(e_host, float(dr.ulp_distance(dr.srgb_oetf32(lin), want).max()))
            worst = max(worst, float(dr.ulp_distance(got, want).max()))
            count += got.size
    log_line('{"test": "display_srgb_%s", "values": %d, "worst_ulp": %.3f, "host_ulp_E": %.3f, "tolerance_ulp": %.3f}' % (name, count, worst, e_host, e_host + 4.0))
    assert worst <= e_host + 4.0, (name, worst, e_host)


def test_display_is_deterministic_and_host_form_matches(dev, product):
    """Two runs are bit-equal; mi355pt_display on host buffers is bit-equal to the device form (sRGB included), with and without a record."""
    W, H = 66, 34
    for tag, film, spp, kw, rec in display_cases(W, H):
        for name in dr.TONES:
            prm = dr.params(tone=dr.TONES[name], **kw)
            one, two = dev.display(film, spp, prm, rec), dev.display(film, spp, prm, rec)
            assert np.array_equal(dr.bits(one), dr.bits(two))
            compare(f"display_host_{name}_{tag}", product.display(film, spp, ffi_params(product, prm), rec), one)


def resolve_device(dev, product, film, spp):
    t = dev.torch
    d_film = dev.up(film)
    rgb = t.full(film.shape, float("nan"), dtype=t.float32, device="cuda")
    product.film_resolve_device(d_film.data_ptr(), film.shape[0] * film.shape[1], spp, rgb.data_ptr())
    t.cuda.synchronize()
    return rgb.cpu().numpy()


@pytest.fixture(scope="module")
def scene3(product, pkg):
    sc = product.new_scene()
    cam = pkg.scenes.load_scene(sc, 3, W3, H3)
    return sc, cam


def render_film(dev, product, pkg, scene3, exposure=1.0, spp=SPP3):
    t = dev.torch
    sc, cam = scene3
    film = t.zeros((H3, W3, 3), dtype=t.float32, device="cuda")
    product.render_accum_device(sc, cam, pkg.make_params(spp, "mis", "sobol", exposure=exposure), 0, spp, film.data_ptr())
    t.cuda.synchronize()
    return film.cpu().numpy()


def test_display_reinhard_srgb_is_the_film_resolve(dev, product, pkg, scene3):
    """REINHARD + ENCODE_SRGB + no record + exposure 1 is bit-equal to mi355pt_film_resolve_device on a non-negative finite synthetic film and
    on a rendered scene-3 film (64 x 48, 16 spp)."""
    film, spp = frame(130, 70, "loguniform", specials=False)
    assert np.isfinite(film).all() and (film >= 0).all() and not np.signbit(film).any()
    rendered = render_film(dev, product, pkg, scene3)
    assert np.isfinite(rendered).all() and rendered.mean() > 0.05      # (out-of-gamut negatives occur: both sides clip them to +0)
    for tag, f, s in (("synthetic", film, spp), ("synthetic_spp3", film, 3), ("rendered", rendered, SPP3)):
        compare(f"display_vs_film_resolve_{tag}", dev.display(f, s, dr.params()), resolve_device(dev, product, f, s))


def test_rendered_exposure_scales_out(dev, product, pkg, scene3):
    """Scene 3 at 64 x 48 x 16 spp with params.exposure 1/16, 1 and 16, same seed: the three films are exact power-of-two multiples of one
    another (asserted first); the three auto-exposed ENCODE_LINEAR pictures are then bit-equal, for every operator; the three fixed-exposure
    Reinhard pictures are not."""
    films = {e: render_film(dev, product, pkg, scene3, e) for e in (1.0 / 16, 1.0, 16.0)}
    for e in (1.0 / 16, 16.0):
        assert np.array_equal(dr.bits(films[e]), dr.bits((films[1.0] * F32(e)).astype(np.float32))), f"the film at exposure {e} is not {e} times the film at 1"
    # "while nothing leaves the range": the scene's positive luminances span some 23 octaves at one exposure and 31 over the three, so the
    # 32 octaves are placed where all three films fit — the first edge at the power of two under the darkest positive luminance of the darkest
    # film — and that they do fit is asserted: the same counts in, below (the black pixels) and above the range for all three
    lum = {e: dr.luminance(dr.clean(f, SPP3)) for e, f in films.items()}
    darkest = lum[1.0 / 16][lum[1.0 / 16] > 0].min()
    prm = dr.params(log2_lum_min=int(np.floor(np.log2(float(darkest)))))
    assert lum[16.0].max() < 2.0 ** (prm.log2_lum_min + 32), (float(darkest), float(lum[16.0].max()))
    recs = {e: dev.meter(f, SPP3, prm)[0] for e, f in films.items()}
    assert recs[1.0][5] == 0 and recs[1.0][4] == int((lum[1.0] == 0).sum()) and recs[1.0][3] + recs[1.0][4] == W3 * H3
    for e in (1.0 / 16, 16.0):
        j = int(np.log2(e))
        assert np.array_equal(recs[e][3:], recs[1.0][3:])
        assert int(recs[e][2]) == int(recs[1.0][2]) + (j << 23) and int(recs[e][0]) == int(recs[1.0][0]) - (j << 23)
        assert float(prm.e_min) < dr.from_bits(recs[e][:1])[0] < float(prm.e_max)
    for name in dr.TONES:
        q = dr.params(tone=dr.TONES[name], encode=dr.ENCODE_LINEAR)
        pics = {e: dev.display(f, SPP3, q, recs[e]) for e, f in films.items()}
        compare(f"display_rendered_auto_{name}_restatement", pics[1.0], dr.display(films[1.0], SPP3, q, recs[1.0]))
        for e in (1.0 / 16, 16.0):
            compare(f"display_rendered_auto_{name}_exposure_{e:g}", pics[e], pics[1.0])
    fixed = {e: dev.display(f, SPP3, dr.params(encode=dr.ENCODE_LINEAR)) for e, f in films.items()}
    assert not np.array_equal(fixed[1.0 / 16], fixed[1.0]) and not np.array_equal(fixed[16.0], fixed[1.0])


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


def run_cli(cli, tmp_path, extra):
    from PIL import Image
    exe, env = cli
    path = str(tmp_path / "d.png")
    r = subprocess.run([exe, "--scene", "3", "--renderer", "mis", "--sampler", "sobol", "--spp", str(CLI_SPP), "--width", str(W3), "--height", str(H3), *extra, "-o", path],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return np.asarray(Image.open(path).convert("RGB")), r.stdout


def test_display_cli(dev, product, pkg, cli, tmp_path):
    """`--auto-exposure --tone-map aces` on scene 3 writes the PNG that the public calls give — mi355pt_render_accum_device, the meter, the
    display, mi355pt_quantize_u8 —, and a run without the new flags still writes mi355pt_render + mi355pt_quantize_u8, byte for byte."""
    t = dev.torch
    sc = product.new_scene()
    cam = pkg.scenes.load_scene(sc, 3, W3, H3, build=False)
    sc.add_lut470(pkg.scenes.presets()["cie_illum_d6500"])
    sc.build(cam)
    prm = pkg.make_params(CLI_SPP, "mis", "sobol", seed=0)
    got, _ = run_cli(cli, tmp_path, [])
    want = product.quantize_u8(product.render(sc, cam, prm))
    assert got.shape == want.shape == (H3, W3, 3) and np.array_equal(got, want), int((got != want).sum())
    film = t.zeros((H3, W3, 3), dtype=t.float32, device="cuda")
    product.render_accum_device(sc, cam, prm, 0, CLI_SPP, film.data_ptr())
    t.cuda.synchronize()
    f = film.cpu().numpy()
    rec, _ = dev.meter(f, CLI_SPP, dr.params())
    pic = dev.display(f, CLI_SPP, dr.params(tone=dr.TONE_ACES), rec)
    got, out = run_cli(cli, tmp_path, ["--auto-exposure", "--tone-map", "aces"])
    want_auto = product.quantize_u8(pic)
    assert np.array_equal(got, want_auto), int((got != want_auto).sum())
    assert "auto-exposure" in out and not np.array_equal(want_auto, want) and got.mean() > 10.0


@pytest.mark.parametrize("extra, meter_extra", [(["--denoise"], []), (["--denoise-variance"], []), (["--adaptive-threshold", "0.05", "--spp", "16"], []), (["--half-res"], []),
                                                (["--temporal-frames", "3"], ["--exposure-adapt", "0.5"]), (["--half-res", "--temporal-frames", "2", "--denoise-variance"], [])],
                         ids=["denoise", "denoise_variance", "adaptive", "half_res", "temporal", "half_res_temporal_variance"])
def test_display_cli_composes(cli, tmp_path, extra, meter_extra):
    """The display flags behind every device path of the CLI — the two filters, adaptive sampling, half resolution, temporal accumulation
    (every frame metered against the previous record) and their combination: the run succeeds, reports its exposure, and writes a picture
    that differs from the same path's picture without the flags."""
    plain, _ = run_cli(cli, tmp_path, ["--denoise-guide-spp", "16", *extra])
    got, out = run_cli(cli, tmp_path, ["--denoise-guide-spp", "16", *extra, "--auto-exposure", *meter_extra, "--tone-map", "hable", "--white", "6"])
    assert "auto-exposure: E" in out and got.shape == plain.shape == (H3, W3, 3)
    assert got.mean() > 10.0 and got.max() > 100 and not np.array_equal(got, plain)
