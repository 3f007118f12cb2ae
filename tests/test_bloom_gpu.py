"""GPU tests of the bloom stage (mi355pt_bloom_device / mi355pt_bloom, csrc/pt_kernels_bloom.hip) against the NumPy restatement of
tests/bloom_reference.py.  Every float step of the kernels is a single binary32 operation in the order the header states, so the bar is BIT
EQUALITY: on the output, on every level D_l of the down pass (read from the scratch buffer of a call with levels = l, as the header's layout
allows) and on the whole scratch buffer of the full call, pad words included.  Outputs and the scratch buffer start as a sentinel, so a word
a kernel leaves out shows; a guard band behind each must stay as written; the film must come back unchanged."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bloom_reference as br  # noqa: E402
import display_reference as dr  # noqa: E402

pytestmark = pytest.mark.gpu

# the shapes of the issue; one below, at and one above twice the reduction's 32 x 8 tile (tests/test_bloom.py pins the tile that
# csrc/bloom_plan.hpp chose), where a workgroup's staged texels end exactly at, before and behind the frame's edge; and one frame of many tiles
TILE_EDGES = [(63, 15), (64, 16), (65, 17)]
SHAPES = br.SHAPES + TILE_EDGES + [(256, 64)]
SHAPE_IDS = [f"{w}x{h}" for w, h in SHAPES]
W3, H3, SPP3 = 64, 48, 16                      # the rendered tests: scene 3
GUARD = 16                                     # words behind every output
SENTINEL = 0xDEADBEEF
NAN_BITS = 0xFFFFFFFF
F32 = np.float32


def levels_for(w, h):
    return 6 if (w, h) == (256, 64) else 8


def log_line(text):
    print(text)
    if os.environ.get("MI355PT_FRAME_LOG"):
        with open(os.environ["MI355PT_FRAME_LOG"], "a") as f:
            f.write(text + "\n")


def ffi_params(product, prm):
    p = product.bloom_params_default()
    for k in br.FIELDS:
        setattr(p, k, (float if k in br.FLOAT_FIELDS else int)(getattr(prm, k)))
    return p


def compare(tag, got, want):
    """bit equality of two f32 arrays -> logs the values compared and the values mismatching"""
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    gb, wb = got.view(np.uint32), want.view(np.uint32)
    bad = gb != wb
    log_line('{"test": "%s", "values": %d, "mismatching": %d}' % (tag, got.size, int(bad.sum())))
    assert not bad.any(), (tag, int(bad.sum()), np.flatnonzero(bad.ravel())[:8].tolist(), got.ravel()[bad.ravel()][:8].tolist(), want.ravel()[bad.ravel()][:8].tolist())


class Device:
    """a film on the device + one call of mi355pt_bloom_device; the output and the scratch buffer start as a pattern, their guard bands and the
    film are checked after the call"""

    def __init__(self, product):
        import torch
        self.torch, self.product = torch, product

    def words(self, n, fill=SENTINEL):
        t = self.torch
        return t.full((n + GUARD,), fill - (1 << 32), dtype=t.int32, device="cuda")

    def bloom(self, film, spp, prm, record=None, in_place=False, fill=SENTINEL):
        """-> (out (H, W, 3) f32, scratch (records, 4) f32)"""
        t = self.torch
        H, W = film.shape[:2]
        n = H * W * 3
        need = self.product.bloom_scratch_bytes(W, H, prm.levels)
        assert need == br.scratch_bytes(W, H, prm.levels) > 0
        d_film = self.words(n)
        d_film[:n] = t.from_numpy(br.bits(film).view(np.int32).reshape(-1).copy()).cuda()
        scratch = self.words(need // 4, fill)
        out = d_film if in_place else self.words(n)
        d_rec = t.from_numpy(np.ascontiguousarray(record, dtype=np.uint32).view(np.int32).copy()).cuda() if record is not None else None
        assert scratch.data_ptr() % 16 == 0
        self.product.bloom_device(d_film.data_ptr(), W, H, spp, ffi_params(self.product, prm), d_rec.data_ptr() if d_rec is not None else None, scratch.data_ptr(), need,
                                  out.data_ptr())
        t.cuda.synchronize()
        o, s, f = (x.cpu().numpy().view(np.uint32) for x in (out, scratch, d_film))
        assert (o[n:] == SENTINEL).all() and (s[need // 4:] == fill).all() and (f[n:] == SENTINEL).all(), "guard band overwritten"
        if not in_place:
            assert np.array_equal(f[:n], br.bits(film).reshape(-1)), "the film was changed"
        if d_rec is not None:
            assert np.array_equal(d_rec.cpu().numpy().view(np.uint32), np.asarray(record, np.uint32)), "the record was changed"
        return o[:n].view(np.float32).reshape(H, W, 3).copy(), s[:need // 4].view(np.float32).reshape(-1, 4).copy()


@pytest.fixture(scope="module")
def dev(product):
    return Device(product)


def level_of(scratch, w, h, levels, l):
    """level l of a scratch buffer of `levels` levels -> (H_l, W_l, 4)"""
    offs, _ = br.level_offsets(w, h, levels)
    lw, lh = br.level_sizes(w, h, levels)[l]
    return scratch[offs[l]:offs[l] + lw * lh].reshape(lh, lw, 4)


# ---------------- parity with the restatement ----------------
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_bloom_parity(dev, shape):
    """Per shape, under every parameter set of bloom_reference.VARIANTS (the weights on and off, no threshold and one with knee 0 and 0.5, a
    record and params.exposure, scatter 0, 0.7 and 1) on a film strewn with NaN, infinities, negatives and subnormals, and under the defaults
    on a clean HDR film: the output and the whole scratch buffer of the full call, and every D_l from a call with levels = l."""
    w, h = shape
    L = levels_for(w, h)
    runs = [(name, kw, rec, "specials") for name, kw, rec in br.VARIANTS] + [("defaults", {}, False, "hdr")]
    for name, kw, rec, kind in runs:
        film, spp = br.film(w, h, kind)
        prm = br.params(levels=L, **kw)
        record = br.record() if rec else None
        ref = br.bloom(film, spp, prm, record)
        out, scratch = dev.bloom(film, spp, prm, record)
        tag = f"bloom_{w}x{h}_{name}_{kind}"
        compare(tag + "_out", out, ref.out)
        compare(tag + "_scratch", scratch, ref.scratch)
        for l in range(1, L + 1):
            _, s = dev.bloom(film, spp, br.params(levels=l, **kw), record)
            got = level_of(s, w, h, l, l)
            compare(f"{tag}_D{l}", got[..., :3], ref.D[l])
            assert not br.bits(got[..., 3]).any(), (tag, l)


@pytest.mark.parametrize("shape", [(7, 5), (67, 19), (65, 17), (256, 64)], ids=["7x5", "67x19", "65x17", "256x64"])
def test_bloom_in_place(dev, shape):
    """d_out == d_film gives what the call with a buffer of its own gives, bit for bit (and that is the restatement's output)."""
    w, h = shape
    film, spp = br.film(w, h, "specials", seed=1)
    for kw, rec in ((dict(), False), (dict(threshold=1.5, knee=0.5, firefly=0, base=1.0, intensity=0.5), True)):
        prm = br.params(levels=levels_for(w, h), **kw)
        record = br.record() if rec else None
        apart, s0 = dev.bloom(film, spp, prm, record)
        same, s1 = dev.bloom(film, spp, prm, record, in_place=True)
        compare(f"bloom_in_place_{w}x{h}_out", same, apart)
        compare(f"bloom_in_place_{w}x{h}_scratch", s1, s0)
        compare(f"bloom_in_place_{w}x{h}_restatement", same, br.bloom(film, spp, prm, record).out)


def test_bloom_repeats_host_form_and_dirty_scratch(dev, product):
    """Two runs are bit-equal; the host form gives what the device form gives, with and without a record; a scratch buffer that starts as
    NaN patterns gives the same output and the same buffer — every word that is read was written by the call."""
    for (w, h), L in (((130, 10), 8), ((256, 64), 6), ((1, 1), 3)):
        film, spp = br.film(w, h, "specials", seed=2)
        for kw, rec in ((dict(), False), (dict(threshold=1.5, knee=0.5), True)):
            prm = br.params(levels=L, **kw)
            record = br.record() if rec else None
            a, sa = dev.bloom(film, spp, prm, record)
            b, sb = dev.bloom(film, spp, prm, record)
            compare(f"bloom_repeat_{w}x{h}_out", b, a)
            compare(f"bloom_repeat_{w}x{h}_scratch", sb, sa)
            c, sc = dev.bloom(film, spp, prm, record, fill=NAN_BITS)
            compare(f"bloom_nan_scratch_{w}x{h}_out", c, a)
            compare(f"bloom_nan_scratch_{w}x{h}_scratch", sc, sa)
            before = film.copy()
            host = product.bloom(film, spp, ffi_params(product, prm), record)
            compare(f"bloom_host_form_{w}x{h}", host, a)
            assert np.array_equal(br.bits(film), br.bits(before))


# ---------------- a rendered frame ----------------
@pytest.fixture(scope="module")
def rendered(dev, product, pkg):
    t = dev.torch
    sc = product.new_scene()
    cam = pkg.scenes.load_scene(sc, 3, W3, H3)
    film = t.zeros((H3, W3, 3), dtype=t.float32, device="cuda")
    product.render_accum_device(sc, cam, pkg.make_params(SPP3, "mis", "sobol"), 0, SPP3, film.data_ptr())
    t.cuda.synchronize()
    f = film.cpu().numpy()
    assert np.isfinite(f).all() and f.mean() > 0.05
    return f


def test_bloom_of_a_rendered_frame(dev, product, rendered):
    """Scene 3 at 64 x 48 x 16 spp: base 1 and intensity 0 return clean(F / spp) bit for bit; the default bloom is the restatement's, changes
    the frame while keeping its mean (out >= 0.96 c; the weighted glare adds at most about what the frame lost), and goes through
    mi355pt_display_device to a finite picture."""
    t = dev.torch
    out, _ = dev.bloom(rendered, SPP3, br.params(base=1.0, intensity=0.0))
    compare("bloom_rendered_identity", out, br.clean(rendered, SPP3))
    prm = br.params()
    out, _ = dev.bloom(rendered, SPP3, prm)
    compare("bloom_rendered_defaults", out, br.bloom(rendered, SPP3, prm).out)
    c = br.clean(rendered, SPP3)
    assert not np.array_equal(out, c) and 0.95 < float(out.mean()) / float(c.mean()) < 1.05
    d_out = t.from_numpy(out).cuda()
    pic = t.full(out.shape, float("nan"), dtype=t.float32, device="cuda")
    product.display_device(d_out.data_ptr(), W3, H3, 1, product.display_params_default(), None, pic.data_ptr())
    t.cuda.synchronize()
    p = pic.cpu().numpy()
    assert np.isfinite(p).all() and (p >= 0).all() and (p <= 1).all() and p.mean() > 0.05


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
    path = str(tmp_path / "b.png")
    r = subprocess.run([exe, "--scene", "3", "--renderer", "mis", "--sampler", "sobol", "--spp", str(CLI_SPP), "--width", str(W3), "--height", str(H3), *extra, "-o", path],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return np.asarray(Image.open(path).convert("RGB")), r.stdout


def test_bloom_cli_is_the_public_calls(dev, product, pkg, cli, tmp_path):
    """`--bloom` on a plain render of scene 3 writes the PNG that the public calls give — mi355pt_render_accum_device, mi355pt_bloom_device,
    mi355pt_film_resolve_device at spp 1, mi355pt_quantize_u8 —, byte for byte; `--auto-exposure --tone-map aces --bloom --bloom-additive
    --bloom-threshold 2 --bloom-intensity 0.5 --bloom-levels 4 --bloom-no-firefly` the one of the meter on the UN-bloomed film, the bloom with
    that record, and the display with it; and a run without the flag still writes mi355pt_render + mi355pt_quantize_u8."""
    t = dev.torch
    sc = product.new_scene()
    cam = pkg.scenes.load_scene(sc, 3, W3, H3, build=False)
    sc.add_lut470(pkg.scenes.presets()["cie_illum_d6500"])
    sc.build(cam)
    prm = pkg.make_params(CLI_SPP, "mis", "sobol", seed=0)
    got_plain, _ = run_cli(cli, tmp_path, [])
    want_plain = product.quantize_u8(product.render(sc, cam, prm))
    assert got_plain.shape == want_plain.shape == (H3, W3, 3) and np.array_equal(got_plain, want_plain), int((got_plain != want_plain).sum())
    film = t.zeros((H3, W3, 3), dtype=t.float32, device="cuda")
    product.render_accum_device(sc, cam, prm, 0, CLI_SPP, film.data_ptr())
    t.cuda.synchronize()
    f = film.cpu().numpy()
    # --bloom alone: the defaults, no record, then the resolve
    bloomed, _ = dev.bloom(f, CLI_SPP, br.params())
    d_b = t.from_numpy(bloomed).cuda()
    rgb = t.full(f.shape, float("nan"), dtype=t.float32, device="cuda")
    product.film_resolve_device(d_b.data_ptr(), W3 * H3, 1, rgb.data_ptr())
    t.cuda.synchronize()
    want = product.quantize_u8(rgb.cpu().numpy())
    got, _ = run_cli(cli, tmp_path, ["--bloom"])
    assert np.array_equal(got, want), int((got != want).sum())
    assert not np.array_equal(got, got_plain)
    # ... and between the meter and the tone curve
    need = product.display_scratch_bytes(W3, H3)
    scratch, rec = dev.words(need // 4), dev.words(dr.RECORD_WORDS)
    dp = product.display_params_default()
    dp.tone = dr.TONE_ACES
    product.display_meter_device(film.data_ptr(), W3, H3, CLI_SPP, dp, None, scratch.data_ptr(), need, rec.data_ptr())
    t.cuda.synchronize()
    record = rec.cpu().numpy().view(np.uint32)[:dr.RECORD_WORDS].copy()
    bp = br.params(levels=4, firefly=0, threshold=2.0, base=1.0, intensity=0.5)
    bloomed, _ = dev.bloom(f, CLI_SPP, bp, record)
    compare("bloom_cli_metered_restatement", bloomed, br.bloom(f, CLI_SPP, bp, record).out)
    d_b = t.from_numpy(bloomed).cuda()
    product.display_device(d_b.data_ptr(), W3, H3, 1, dp, rec.data_ptr(), rgb.data_ptr())
    t.cuda.synchronize()
    want = product.quantize_u8(rgb.cpu().numpy())
    flags = ["--auto-exposure", "--tone-map", "aces"]
    got, out = run_cli(cli, tmp_path, [*flags, "--bloom", "--bloom-additive", "--bloom-threshold", "2", "--bloom-intensity", "0.5", "--bloom-levels", "4", "--bloom-no-firefly"])
    assert np.array_equal(got, want), int((got != want).sum())
    unbloomed, out0 = run_cli(cli, tmp_path, flags)
    line = [ln for ln in out.splitlines() if "auto-exposure: E" in ln]
    assert line and line == [ln for ln in out0.splitlines() if "auto-exposure: E" in ln]      # the glare did not feed the exposure
    assert not np.array_equal(got, unbloomed)


@pytest.mark.parametrize("extra", [["--denoise"], ["--denoise-variance"], ["--adaptive-threshold", "0.05", "--spp", "16"], ["--half-res"], ["--robust-buckets", "4"],
                                   ["--temporal-frames", "3"]],
                         ids=["denoise", "denoise_variance", "adaptive", "half_res", "robust", "temporal"])
def test_bloom_cli_composes(cli, tmp_path, extra):
    """--bloom behind every device path of the CLI.  The picture differs from the path's own ONLY by the stage: with --bloom-intensity 0 the
    stage returns the cleaned film (base 1, B times 0), and the PNG is the path's PNG byte for byte — so everything before the stage, the
    accumulated history of --temporal-frames with it, is what it was; with the glare on, the picture changes and stays a picture."""
    path = ["--denoise-guide-spp", "16", *extra]
    plain, _ = run_cli(cli, tmp_path, path)
    neutral, _ = run_cli(cli, tmp_path, [*path, "--bloom", "--bloom-intensity", "0"])
    assert np.array_equal(neutral, plain), int((neutral != plain).sum())
    got, _ = run_cli(cli, tmp_path, [*path, "--bloom", "--bloom-intensity", "0.5"])
    assert got.shape == plain.shape == (H3, W3, 3) and not np.array_equal(got, plain) and got.mean() > 10.0 and got.max() > 100
