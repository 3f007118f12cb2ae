"""GPU tests of the robust film (include/mi355pt_robust.h; csrc/pt_kernels_robust.hip, csrc/api_robust.cpp) against the NumPy restatement of
tests/robust_reference.py.  Every float step of the kernel is a single binary32 operation in the order the header states, so the bar is BIT
EQUALITY on every output value — theta, theta_even, theta_even + theta_odd and both trim bytes.  Outputs start as NaN / a sentinel, so a
value the kernel leaves out shows; a guard band behind every output must stay as written; the bucket films must come back unchanged."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import robust_reference as rr  # noqa: E402

pytestmark = pytest.mark.gpu

# one pixel; less than a wave; one lane past a wave, three rows; tall and narrow; more than one 256-thread block both ways with ragged
# edges.  The launcher never splits: a frame has fewer than 2^32 pixels, so at most 2^24 blocks, one launch
FRAMES = [(1, 1), (63, 1), (65, 3), (8, 130), (200, 37)]
FRAME_IDS = [f"{w}x{h}" for w, h in FRAMES]
SCALES = (0.5, 1.0, 2.0)
SPP_BUCKET = 4
W3, H3, SPP3, K3 = 64, 48, 64, 16              # the rendered tests
GUARD = 16
GUARD_VALUE = 12345.0
TRIM_SENTINEL = 0xA5
F32 = np.float32


def log_line(text):
    print(text)
    if os.environ.get("MI355PT_FRAME_LOG"):
        with open(os.environ["MI355PT_FRAME_LOG"], "a") as f:
            f.write(text + "\n")


def compare(tag, got, want):
    """bit equality of two arrays (f32 or u8) -> logs the values compared and the values mismatching"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, want.shape, got.dtype, want.dtype)
    gb, wb = (got.view(np.uint32), want.view(np.uint32)) if got.dtype == np.float32 else (got, want)
    bad = gb != wb
    log_line('{"test": "%s", "values": %d, "mismatching": %d}' % (tag, got.size, int(bad.sum())))
    assert not bad.any(), (tag, int(bad.sum()), np.flatnonzero(bad.ravel())[:8].tolist(), gb.ravel()[bad.ravel()][:8].tolist(), wb.ravel()[bad.ravel()][:8].tolist())


class Device:
    """a bucket stack on the device + one call of mi355pt_robust_combine_device; outputs start as NaN / a sentinel, guard bands and the
    stack are checked after the call"""

    def __init__(self, product):
        import torch
        self.torch, self.product = torch, product

    def up(self, a):
        return self.torch.from_numpy(np.array(a, copy=True)).cuda()

    def combine(self, d_stack, stack, spp_bucket, params, pair, want_trim=True):
        """-> (out, half or None, trim or None) as host arrays"""
        t = self.torch
        k, h, w = stack.shape[:3]
        n = h * w * 3
        out = t.full((n + GUARD,), float("nan"), dtype=t.float32, device="cuda"); out[n:] = GUARD_VALUE
        half = t.full((n + GUARD,), float("nan"), dtype=t.float32, device="cuda"); half[n:] = GUARD_VALUE
        trim = t.full((h * w * 2 + GUARD,), TRIM_SENTINEL, dtype=t.uint8, device="cuda")
        self.product.robust_combine_device(d_stack.data_ptr(), k, spp_bucket, w, h, params, out.data_ptr(), half.data_ptr() if pair else None,
                                           trim.data_ptr() if want_trim else None)
        t.cuda.synchronize()
        o, hf, tr = out.cpu().numpy(), half.cpu().numpy(), trim.cpu().numpy()
        assert (o[n:] == GUARD_VALUE).all() and (hf[n:] == GUARD_VALUE).all() and (tr[h * w * 2:] == TRIM_SENTINEL).all(), "guard band overwritten"
        if not pair:
            assert np.isnan(hf[:n]).all(), "the half film was written in single-output mode"
        if not want_trim:
            assert (tr == TRIM_SENTINEL).all()
        assert np.array_equal(rr.bits(d_stack.cpu().numpy()), rr.bits(stack)), "the bucket films were changed"
        return (o[:n].reshape(h, w, 3).copy(), hf[:n].reshape(h, w, 3).copy() if pair else None,
                tr[:h * w * 2].reshape(h, w, 2).copy() if want_trim else None)


@pytest.fixture(scope="module")
def dev(product):
    return Device(product)


@pytest.mark.parametrize("frame", FRAMES, ids=FRAME_IDS)
@pytest.mark.parametrize("k", rr.BUCKET_COUNTS)
def test_combine_parity(dev, product, k, frame):
    """K x the three modes x single and pair output x gini_scale 0.5 / 1 / 2 on the seeded stack of rr.make_stack: every value of every
    output is bit-equal to the restatement, none is left out (the outputs start as NaN / 0xA5: a NaN or a sentinel left behind differs)"""
    w, h = frame
    stack = rr.make_stack(k, h, w, seed=1000 + 37 * k + w, spp_bucket=SPP_BUCKET)
    d_stack = dev.up(stack)
    for mode_name, mode in rr.MODES.items():
        for pair in (False, True):
            for scale in SCALES:
                tag = f"robust_combine_K{k}_{w}x{h}_{mode_name}_{'pair' if pair else 'single'}_scale{scale:g}"
                want_out, want_half, want_trim = rr.combine(stack, SPP_BUCKET, mode, scale, pair)
                assert not np.isnan(want_out).any()
                got_out, got_half, got_trim = dev.combine(d_stack, stack, SPP_BUCKET, product.robust_params(mode_name, scale), pair)
                compare(tag + "_out", got_out, want_out)
                if pair:
                    compare(tag + "_half", got_half, want_half)
                compare(tag + "_trim", got_trim, want_trim)


def test_combine_parity_odd_spp(dev, product):
    """a sample count that is no power of two: step 1 is an IEEE division there, not a product with the exact reciprocal"""
    stack = rr.make_stack(32, 37, 200, seed=77, spp_bucket=3)
    want = rr.combine(stack, 3, rr.GMON, 1.0, False)
    got = dev.combine(dev.up(stack), stack, 3, product.robust_params("gmon", 1.0), False)
    compare("robust_combine_K32_spp3_out", got[0], want[0])
    compare("robust_combine_K32_spp3_trim", got[2], want[2])
    for k in (4, 16):
        s = rr.make_stack(k, 3, 65, seed=78, spp_bucket=3)
        got = dev.combine(dev.up(s), s, 3, product.robust_params("gmon", 1.0), True)
        for name, g, wv in zip(("out", "half", "trim"), got, rr.combine(s, 3, rr.GMON, 1.0, True)):
            compare(f"robust_combine_K{k}_spp3_pair_{name}", g, wv)


@pytest.mark.parametrize("spp", [4, 3], ids=["spp4_reciprocal", "spp3_division"])
def test_combine_parity_at_the_ends_of_the_range(dev, product, spp):
    """the generator's stack scaled by 2^-140 — every mean, luminance and sum is SUBNORMAL — and by 2^100, for a power-of-two sample count
    (the kernel multiplies by the exact reciprocal: the same real number rounded once, so the same bits as the division of the definition)
    and for one that is not (IEEE division): bit-equal to the restatement, trims included"""
    for k, pair in ((8, False), (32, False), (32, True), (4, True)):
        base = rr.make_stack(k, 3, 65, seed=300 + k, spp_bucket=spp)
        for e in (-140, 100):
            with np.errstate(all="ignore"):
                stack = (base * F32(2.0) ** F32(e)).astype(F32)
            want = rr.combine(stack, spp, rr.GMON, 1.0, pair)
            if e < 0:
                assert 0 < np.abs(want[0][want[0] != 0]).max() < np.finfo(F32).tiny
                assert (k == 4 and pair) or len(set(want[2][..., 0].ravel().tolist())) > 1      # (sets of 2 have one trim count)
            got = dev.combine(dev.up(stack), stack, spp, product.robust_params("gmon", 1.0), pair)
            for name, g, wv in zip(("out", "half", "trim"), got, want):
                if wv is not None:
                    compare(f"robust_combine_K{k}_{'pair' if pair else 'single'}_spp{spp}_scaled_2^{e}_{name}", g, wv)


def test_combine_is_deterministic_and_forms_agree(dev, product):
    """two runs are bit-equal; the host form equals the device form; with d_out_trim == NULL the other outputs are unchanged"""
    for k, pair in ((8, False), (32, False), (16, True)):
        stack = rr.make_stack(k, 37, 200, seed=5 + k)
        d_stack = dev.up(stack)
        rp = product.robust_params("gmon", 1.0)
        a = dev.combine(d_stack, stack, SPP_BUCKET, rp, pair)
        b = dev.combine(d_stack, stack, SPP_BUCKET, rp, pair)
        c = dev.combine(d_stack, stack, SPP_BUCKET, rp, pair, want_trim=False)
        hst = product.robust_combine(stack, SPP_BUCKET, rp, pair=pair)
        hst_no_trim = product.robust_combine(stack, SPP_BUCKET, rp, pair=pair, want_trim=False)
        for i, name in enumerate(("out", "half", "trim")):
            if a[i] is None:
                assert b[i] is None and hst[i] is None
                continue
            compare(f"robust_rerun_K{k}_{name}", b[i], a[i])
            compare(f"robust_host_form_K{k}_{name}", hst[i], a[i])
            if name != "trim":
                compare(f"robust_no_trim_K{k}_{name}", c[i], a[i])
                compare(f"robust_host_no_trim_K{k}_{name}", hst_no_trim[i], a[i])
        assert c[2] is None and hst_no_trim[2] is None


# ---------------- rendered buckets ----------------

@pytest.fixture(scope="module")
def scenes(product, pkg):
    out = {}
    for n in (3, 8):
        sc = product.new_scene()
        out[n] = (sc, pkg.scenes.load_scene(sc, n, W3, H3))
    return out


def render_buckets(dev, product, sc, cam, prm, k, prefill=None):
    t = dev.torch
    d = t.full((k, H3, W3, 3), float("nan") if prefill is None else prefill, dtype=t.float32, device="cuda")      # the entry point clears the films itself
    product.render_buckets_device(sc, cam, prm, k, d.data_ptr())
    t.cuda.synchronize()
    return d


@pytest.mark.parametrize("scene", [3, 8])
def test_buckets_are_the_sample_ranges(dev, product, pkg, scenes, scene):
    """scenes 3 and 8 at 64 x 48, MIS + Sobol, 64 spp, K = 16: bucket k of mi355pt_render_buckets_device is bit-equal to
    mi355pt_render_accum_device over [4k, 4k + 4) into a zeroed film — the entry point every earlier test holds to the oracle —, whatever
    the films held before; the summed kernel_ms and launches come back; with shard 1 of 2 every pixel of the other shard is 0 in every
    bucket and in theta"""
    t = dev.torch
    sc, cam = scenes[scene]
    prm = pkg.make_params(SPP3, "mis", "sobol")
    d = render_buckets(dev, product, sc, cam, prm, K3)
    got = d.cpu().numpy()
    assert np.isfinite(got).all() and got.mean() > 0.0
    per = SPP3 // K3
    for k in range(K3):
        film = t.zeros((H3, W3, 3), dtype=t.float32, device="cuda")
        product.render_accum_device(sc, cam, prm, k * per, (k + 1) * per, film.data_ptr())
        t.cuda.synchronize()
        compare(f"robust_bucket_scene{scene}_k{k}", got[k], film.cpu().numpy())
    st = pkg.ffi.Stats()
    d2 = t.full((K3, H3, W3, 3), 7.0, dtype=t.float32, device="cuda")
    product.render_buckets_device(sc, cam, prm, K3, d2.data_ptr(), stats=st)
    compare(f"robust_buckets_scene{scene}_with_stats", d2.cpu().numpy(), got)
    assert st.launches >= K3 and st.kernel_ms > 0.0 and st.samples == 0
    # shard 1 of 2: the 8 x 8 tiles with an odd index
    sh = pkg.make_params(SPP3, "mis", "sobol", shard_index=1, shard_count=2)
    ds = render_buckets(dev, product, sc, cam, sh, K3)
    shard = ds.cpu().numpy()
    ty, tx = np.mgrid[0:H3, 0:W3] // 8
    other = ((ty * ((W3 + 7) // 8) + tx) % 2) == 0
    assert other.any() and (~other).any()
    assert (rr.bits(shard[:, other]) == 0).all(), "a pixel of the other shard was written"
    for k in range(K3):      # (a shard may split its ranges otherwise than the whole frame: the yardstick is the same call with the same shard)
        film = t.zeros((H3, W3, 3), dtype=t.float32, device="cuda")
        product.render_accum_device(sc, cam, sh, k * per, (k + 1) * per, film.data_ptr())
        t.cuda.synchronize()
        compare(f"robust_bucket_scene{scene}_shard1of2_k{k}", shard[k], film.cpu().numpy())
    assert shard[:, ~other].mean() > 0.0
    theta = dev.combine(ds, shard, per, product.robust_params_default(), False)[0]
    assert (rr.bits(theta[other]) == 0).all() and theta[~other].mean() > 0.0


def test_render_robust_is_its_public_pieces(dev, product, pkg, scenes):
    """mi355pt_render_robust = mi355pt_render_buckets_device + the single-output combination + mi355pt_film_resolve_device(spp 1), bit
    for bit, for the three modes; and MOM over K copies of ONE rendered film returns that film's cleaned mean, bit for bit"""
    t = dev.torch
    sc, cam = scenes[8]
    prm = pkg.make_params(SPP3, "mis", "sobol")
    d = render_buckets(dev, product, sc, cam, prm, K3)
    stack = d.cpu().numpy()
    pics = {}
    for mode in rr.MODES:
        rp = product.robust_params(mode, 1.0)
        theta = t.full((H3, W3, 3), float("nan"), dtype=t.float32, device="cuda")
        rgb = t.full((H3, W3, 3), float("nan"), dtype=t.float32, device="cuda")
        product.robust_combine_device(d.data_ptr(), K3, SPP3 // K3, W3, H3, rp, theta.data_ptr())
        product.film_resolve_device(theta.data_ptr(), W3 * H3, 1, rgb.data_ptr())
        t.cuda.synchronize()
        compare(f"robust_theta_scene8_{mode}", theta.cpu().numpy(), rr.combine(stack, SPP3 // K3, rr.MODES[mode])[0])
        pics[mode] = product.render_robust(sc, cam, prm, K3, rp)
        compare(f"robust_render_robust_scene8_{mode}", pics[mode], rgb.cpu().numpy())
    assert not np.array_equal(pics["gmon"], pics["mean"]) and not np.array_equal(pics["mom"], pics["mean"])
    film = t.zeros((H3, W3, 3), dtype=t.float32, device="cuda")
    product.render_accum_device(sc, cam, prm, 0, SPP3, film.data_ptr())
    t.cuda.synchronize()
    one = film.cpu().numpy()
    for k in rr.BUCKET_COUNTS:
        copies = np.repeat(one[None], k, axis=0)
        got = dev.combine(dev.up(copies), copies, SPP3, product.robust_params("mom", 1.0), False)
        compare(f"robust_mom_of_{k}_copies", got[0], rr.clean_means(one, SPP3))
        assert (got[2][..., 0] == k // 2 - 1).all() and (got[2][..., 1] == 0).all()


# ---------------- the CLI ----------------
CLI_SPP = 64


@pytest.fixture(scope="module")
def cli(pkg, tmp_path_factory):
    root = pkg.ffi.ROOT
    exe = os.path.join(root, "toy-cpu-pathtracing_amd", "host", "mi355pt")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.dirname(exe)])
    assets_dir = str(tmp_path_factory.mktemp("assets"))
    subprocess.check_call([sys.executable, os.path.join(root, "tools", "export_assets.py"), assets_dir])
    return exe, dict(os.environ, MI355PT_ASSETS=assets_dir, MI355PT_DATA=os.path.join(root, "toy-cpu-pathtracing_amd", "data"))


def run_cli(cli, tmp_path, extra, scene=3):
    from PIL import Image
    exe, env = cli
    path = str(tmp_path / "r.png")
    r = subprocess.run([exe, "--scene", str(scene), "--renderer", "mis", "--sampler", "sobol", "--spp", str(CLI_SPP), "--width", str(W3), "--height", str(H3), *extra, "-o", path],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return np.asarray(Image.open(path).convert("RGB")), r.stdout


def test_robust_cli(product, pkg, cli, tmp_path):
    """`--robust-buckets 16` writes the PNG of mi355pt_render_robust + mi355pt_quantize_u8, byte for byte, reports its trims, and a run
    without the flag still writes mi355pt_render's picture"""
    sc = product.new_scene()
    cam = pkg.scenes.load_scene(sc, 3, W3, H3, build=False)
    sc.add_lut470(pkg.scenes.presets()["cie_illum_d6500"])
    sc.build(cam)
    prm = pkg.make_params(CLI_SPP, "mis", "sobol", seed=0)
    plain, _ = run_cli(cli, tmp_path, [])
    want_plain = product.quantize_u8(product.render(sc, cam, prm))
    assert np.array_equal(plain, want_plain), int((plain != want_plain).sum())
    for extra, rp in ((["--robust-buckets", "16"], product.robust_params_default()),
                      (["--robust-buckets", "8", "--robust-mode", "mom"], product.robust_params("mom", 1.0)),
                      (["--robust-buckets", "16", "--robust-mode", "gmon", "--robust-scale", "2"], product.robust_params("gmon", 2.0))):
        got, out = run_cli(cli, tmp_path, extra)
        want = product.quantize_u8(product.render_robust(sc, cam, prm, int(extra[1]), rp))
        assert got.shape == want.shape == (H3, W3, 3) and np.array_equal(got, want), (extra, int((got != want).sum()))
        assert "robust film" in out and "pixels trimmed" in out and not np.array_equal(got, plain)


@pytest.mark.parametrize("extra", [["--denoise"], ["--denoise-variance"], ["--denoise", "--fused-guides"], ["--denoise-variance", "--fused-guides"],
                                   ["--tone-map", "aces"], ["--auto-exposure"], ["--denoise-variance", "--auto-exposure", "--tone-map", "hable", "--white", "6"]],
                         ids=["denoise", "denoise_variance", "denoise_fused", "denoise_variance_fused", "tone_map", "auto_exposure", "variance_display"])
def test_robust_cli_composes(cli, tmp_path, extra):
    """the robust film in front of the two filters (single output as beauty with spp 1; pair output as beauty and half with spp 2), with
    the fused guides and with the display stage: the run succeeds, reports its trims and writes a picture that differs from the plain robust
    picture and from the same path's picture without --robust-buckets"""
    robust, _ = run_cli(cli, tmp_path, ["--robust-buckets", "16"])
    without, _ = run_cli(cli, tmp_path, ["--denoise-guide-spp", "16", *extra])
    got, out = run_cli(cli, tmp_path, ["--denoise-guide-spp", "16", "--robust-buckets", "16", *extra])
    assert "robust film" in out and got.shape == robust.shape == (H3, W3, 3)
    assert ("even and odd sets" in out) == ("--denoise-variance" in extra)
    assert got.mean() > 10.0 and not np.array_equal(got, robust) and not np.array_equal(got, without)
