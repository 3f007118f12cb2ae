"""GPU tests of the temporal reprojection (mi355pt_temporal_accumulate_device / mi355pt_temporal_accumulate, csrc/pt_kernels_temporal.hip)
against the NumPy restatement of tests/temporal_reference.py.  Every operation of the kernel is a single binary32 operation in the order
the header states, so the bar is BIT EQUALITY on every output value; the outputs start as NaN, so a value the kernel leaves out shows."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import denoise_var_reference as dv  # noqa: E402
import temporal_reference as tr  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (3, 2), (7, 5), (64, 1), (1, 64), (67, 35), (130, 70)]    # (W, H): below a wave, ragged edges, one row, one column, > 1 block
W3, H3 = 64, 48                  # the rendered tests: scene 3
GUIDE_SPP, FRAME_SPP = 16, 4


def log_line(text):
    print(text)
    if os.environ.get("MI355PT_FRAME_LOG"):
        with open(os.environ["MI355PT_FRAME_LOG"], "a") as f:
            f.write(text + "\n")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def ffi_view(pkg, v):
    if isinstance(v, pkg.ffi.TemporalView) or v is None:
        return v
    return pkg.ffi.TemporalView((ctypes.c_float * 3)(*v.delta), (ctypes.c_float * 9)(*v.rows), v.sx, v.sy, v.cx, v.cy)


def ffi_params(product, prm):
    p = product.temporal_params_default()
    if prm is not None:
        for k in tr.DEFAULTS:
            setattr(p, k, float(getattr(prm, k)))
    return p


class Device:
    """frames on the device + one call of mi355pt_temporal_accumulate_device; the outputs start as NaN"""

    def __init__(self, product, pkg):
        import torch
        self.torch, self.product, self.pkg = torch, product, pkg

    def up(self, frame):
        if frame is None:
            return None
        return {k: self.torch.from_numpy(np.ascontiguousarray(frame[k], dtype=np.float32)).cuda() for k in tr.FILMS if frame.get(k) is not None}

    def outputs(self, W, H, half):
        nan = lambda *s: self.torch.full(s, float("nan"), dtype=self.torch.float32, device="cuda")   # noqa: E731
        return nan(H, W, 3), (nan(H, W, 3) if half else None), nan(H, W)

    def run_device(self, cur, spp, prev, view, prm, outs=None):
        """cur / prev: dicts of device tensors -> the three output tensors (half None without a half film)"""
        H, W = cur["film"].shape[:2]
        of, oh, ol = outs if outs is not None else self.outputs(W, H, "half" in cur)
        ptr = lambda d: {k: v.data_ptr() for k, v in d.items()} if d is not None else None   # noqa: E731
        self.product.temporal_accumulate_device(ptr(cur), spp, ptr(prev), ffi_view(self.pkg, view), W, H, ffi_params(self.product, prm), of.data_ptr(),
                                                oh.data_ptr() if oh is not None else None, ol.data_ptr())
        self.torch.cuda.synchronize()
        return of, oh, ol

    def run(self, cur, spp, prev=None, view=None, prm=None):
        """host frames in, host arrays out"""
        of, oh, ol = self.run_device(self.up(cur), spp, self.up(prev), view, prm)
        return of.cpu().numpy(), (oh.cpu().numpy() if oh is not None else None), ol.cpu().numpy()


@pytest.fixture(scope="module")
def dev(product, pkg):
    return Device(product, pkg)


def assert_bit_equal(got, want, tag):
    """every output value bit-equal to the f32 restatement, nothing left unwritten"""
    names = ("film", "half", "length")
    bad = {}
    for n, g, w in zip(names, got, want):
        assert (g is None) == (w is None), (tag, n)
        if g is None:
            continue
        assert not np.isnan(g).any(), f"{tag}: {int(np.isnan(g).sum())} values of out_{n} not written"
        bad[n] = int((bits(g) != bits(w)).sum())
    log_line('{"test": "%s", "values": %d, "mismatching": %d}' % (tag, sum(g.size for g in got if g is not None), sum(bad.values())))
    assert not any(bad.values()), (tag, bad)


@pytest.mark.parametrize("half", [True, False], ids=["half", "nohalf"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_temporal_synthetic_parity(dev, shape, half):
    """Seeded synthetic frames (the two-plane step and the plane, HDR noise, NaN / inf / negative film values, a background band, previous
    lengths with zeros) at every shape, with and without a half film, without a previous frame and through every synthetic view (static:
    exact pixel centres; a 3-pixel shift; a move with a yaw; part of the frame outside the history; part of it behind the previous
    camera): every output value is bit-equal to the f32 restatement, nothing is left unwritten."""
    W, H = shape
    cur, _, _, spp = tr.synthetic(W, H, "static", "step", half)
    assert_bit_equal(dev.run(cur, spp), tr.accumulate(cur, spp), f"temporal_synthetic_{W}x{H}_{'half' if half else 'nohalf'}_first")
    for view in tr.VIEWS:
        for scene in (("step", "plane") if view == "shift3" else ("step",)):
            cur, prev, vw, spp = tr.synthetic(W, H, view, scene, half)
            want = tr.accumulate(cur, spp, prev, vw)
            assert_bit_equal(dev.run(cur, spp, prev, vw), want, f"temporal_synthetic_{W}x{H}_{'half' if half else 'nohalf'}_{view}_{scene}")


def test_temporal_synthetic_parity_other_parameters(dev):
    """the same at one shape with every parameter away from its default, and on the exact pixel grid (weights 1, 0, 0, 0 and 1/2, 1/2)"""
    W, H = 67, 35
    prm = tr.params(pos_tol=0.5, normal_cos=-1.0, min_weight=0.3, max_history=5.0)
    for view in tr.VIEWS:
        cur, prev, vw, spp = tr.synthetic(W, H, view, "step", True, spp=6)
        assert_bit_equal(dev.run(cur, spp, prev, vw, prm), tr.accumulate(cur, spp, prev, vw, prm), f"temporal_synthetic_params_{view}")
    gb = tr.grid_frame(W, H)
    rng = np.random.default_rng(2)
    cur = dict(gb, film=tr.hdr(rng, (H, W, 3)), half=None)
    prev = dict(gb, film=tr.hdr(rng, (H, W, 3)), half=None, length=np.full((H, W), 3.0, np.float32))
    for dx, dy in ((0.0, 0.0), (3.0, 2.0), (0.5, 0.0), (-1.0, -0.25), (float(W), 0.0), (-float(W) - 1.0, 0.0)):
        vw = tr.grid_view(W, H, dx, dy)
        assert_bit_equal(dev.run(cur, 1, prev, vw), tr.accumulate(cur, 1, prev, vw), f"temporal_grid_{dx}_{dy}")


# ---------------- rendered frames: scene 3 at 64 x 48 ----------------
@pytest.fixture(scope="module")
def handles(product, pkg):
    """scene 3 on two scene handles: the scene's camera, and the camera moved by (0.3, 0.1, -0.2) and yawed 0.05 rad"""
    move, yaw = tr.CAMERA_PAIRS["xyz_yaw"]
    return {"prev": tr.load_moved(product, pkg, 3, W3, H3), "cur": tr.load_moved(product, pkg, 3, W3, H3, move, yaw)}


def render_frame(product, pkg, handle, seed, spp=FRAME_SPP, guide_spp=GUIDE_SPP, albedo=False):
    """one frame's device films: the G-buffer sums at guide_spp, the half film [0, spp / 2) and the film [0, spp)"""
    import torch
    sc, cam, d65 = handle
    z = lambda: torch.zeros((H3, W3, 3), dtype=torch.float32, device="cuda")   # noqa: E731
    f = {k: z() for k in ("film", "half", "position", "shading_normal", "hit")}
    if albedo:
        f["albedo"] = z()
    g = {k: f[k].data_ptr() for k in ("albedo", "shading_normal", "position", "hit") if k in f}
    product.render_gbuffer_accum_device(sc, cam, pkg.make_params(guide_spp, "mis", "sobol", seed=seed), d65, 0, guide_spp, g)
    prm = pkg.make_params(spp, "mis", "sobol", seed=seed)
    product.render_accum_device(sc, cam, prm, 0, spp // 2, f["half"].data_ptr())
    torch.cuda.synchronize()
    f["film"].copy_(f["half"])
    product.render_accum_device(sc, cam, prm, spp // 2, spp, f["film"].data_ptr())
    torch.cuda.synchronize()
    return f


def frame_of(f, keys=tr.FILMS):
    return {k: f[k] for k in keys if k in f}


def host(f):
    return {k: v.cpu().numpy() for k, v in f.items()}


def test_temporal_rendered_parity_and_geometry(dev, product, pkg, handles):
    """Frame 0 (seed 0, the scene's camera) fed to frame 1 (seed 1, the moved camera): G-buffers at 16 spp, beauty and half at 4 spp.  Both
    accumulations are bit-equal to the restatement run on the same buffers read back, and the reprojection-geometry bars of
    tests/test_temporal.py (median <= 0.1 footprints, >= 0.97 under 0.25, interior >= 0.6 of the hit pixels) are met on the GPU's films."""
    f0, f1 = render_frame(product, pkg, handles["prev"], 0), render_frame(product, pkg, handles["cur"], 1)
    cam_p, cam_c = handles["prev"][1], handles["cur"][1]
    view = product.temporal_view_from_cameras(cam_c, cam_p)
    h0, h1 = host(f0), host(f1)
    a0 = dev.run_device(frame_of(f0), FRAME_SPP, None, None, None)
    assert_bit_equal([x.cpu().numpy() for x in a0], tr.accumulate(frame_of(h0), FRAME_SPP), "temporal_rendered_frame0")
    prev = dict(frame_of(f0, ("position", "shading_normal", "hit")), film=a0[0], half=a0[1], length=a0[2])
    a1 = dev.run_device(frame_of(f1), FRAME_SPP, prev, view, None)
    want = tr.accumulate(frame_of(h1), FRAME_SPP, host(prev), view, detail=True)
    assert_bit_equal([x.cpu().numpy() for x in a1], want[:3], "temporal_rendered_frame1")
    info = want[3]
    hit = h1["hit"][..., 1] > 0
    assert info["has"][hit].mean() > 0.5 and (~info["has"]).any()                   # both branches are exercised
    # the geometry: world-space positions as films
    cur_g, prev_g, prm = tr.geometry_frames(frame_of(h1, ("position", "shading_normal", "hit")), frame_of(h0, ("position", "shading_normal", "hit")),
                                            cam_c, cam_p, GUIDE_SPP)
    got = dev.run(cur_g, GUIDE_SPP, prev_g, view, prm)
    assert_bit_equal(got, tr.accumulate(cur_g, GUIDE_SPP, prev_g, view, prm), "temporal_rendered_geometry")
    fig = tr.geometry_figures(got[0], cur_g, prev_g, view, prm, cam_c, GUIDE_SPP)
    log_line('{"test": "temporal_geometry_gpu", "pair": "xyz_yaw", "median": %.4f, "share_under_quarter": %.4f, "interior_share": %.4f, "interior": %d, "hit": %d}'
             % (fig["median"], fig["share_under_quarter"], fig["interior_share"], fig["interior"], fig["hit"]))
    bars = tr.GEOMETRY_BARS
    assert fig["interior_share"] >= bars["interior_share"], fig
    assert fig["median"] <= bars["median"] and fig["share_under_quarter"] >= bars["share_under_quarter"], fig


@pytest.fixture(scope="module")
def static_run(dev, product, pkg, handles):
    """8 frames of 4 spp, seeds 0 .. 7, a static camera, the default parameters: the accumulated pair, the last frame's films"""
    acc, f = None, None
    view = product.temporal_view_from_cameras(handles["prev"][1], handles["prev"][1])
    for k in range(8):
        f = render_frame(product, pkg, handles["prev"], k, albedo=True)
        prev = None
        if acc is not None:
            prev = dict(frame_of(g, ("position", "shading_normal", "hit")), film=acc[0], half=acc[1], length=acc[2])
        acc = dev.run_device(frame_of(f), FRAME_SPP, prev, view if prev is not None else None, None)
        g = f
    return acc, f


def resolved(product, film_tensor, spp):
    import torch
    rgb = torch.empty_like(film_tensor)
    product.film_resolve_device(film_tensor.data_ptr(), W3 * H3, spp, rgb.data_ptr())
    torch.cuda.synchronize()
    return rgb.cpu().numpy().astype(np.float64)


def test_temporal_static_accumulation(product, pkg, handles, static_run):
    """RMSE after the resolve against the GPU's own 1024-spp frame: E_acc <= sqrt(E_4 E_32), the geometric midpoint between "did nothing"
    (a plain 4-spp frame) and "ideal" (a plain 32-spp frame), both measured here.  The 9 % of the pixels that find no history (normal-mapped
    and silhouette pixels) put the estimate at 1.3 E_32 against the bar's 1.68 E_32."""
    sc, cam, _ = handles["prev"]
    acc, _ = static_run
    rmse = lambda a, b: float(np.sqrt(np.mean((a - b) ** 2)))   # noqa: E731
    ref = product.render(sc, cam, pkg.make_params(1024, "mis", "sobol", seed=1000)).astype(np.float64)
    e4 = rmse(product.render(sc, cam, pkg.make_params(4, "mis", "sobol", seed=0)).astype(np.float64), ref)
    e32 = rmse(product.render(sc, cam, pkg.make_params(32, "mis", "sobol", seed=0)).astype(np.float64), ref)
    eacc = rmse(resolved(product, acc[0], 2), ref)
    length = acc[2].cpu().numpy()
    log_line('{"test": "temporal_static_accumulation", "E_4": %.5f, "E_32": %.5f, "E_acc": %.5f, "bar": %.5f, "E_acc_over_E_32": %.3f, "length_8_share": %.4f}'
             % (e4, e32, eacc, (e4 * e32) ** 0.5, eacc / e32, float((length == 8).mean())))
    assert e32 < e4
    assert eacc <= (e4 * e32) ** 0.5, (eacc, e4, e32)


def test_temporal_chain_with_the_variance_denoiser(product, static_run):
    """mi355pt_denoise_var_device(out_film, out_half, 2, ...) on the accumulated pair meets that filter's own bar — 8 x e32 of
    tests/denoise_var_reference.py — and its result resolves to finite values in [0, 1]."""
    import torch
    acc, f = static_run
    need = product.denoise_var_scratch_bytes(W3, H3)
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    out = torch.full((H3, W3, 3), float("nan"), dtype=torch.float32, device="cuda")
    product.denoise_var_device(acc[0].data_ptr(), acc[1].data_ptr(), 2, None, f["albedo"].data_ptr(), GUIDE_SPP, f["shading_normal"].data_ptr(), GUIDE_SPP,
                               W3, H3, product.denoise_var_params_default(), scratch.data_ptr(), need, out.data_ptr())
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    film, half, a, n = acc[0].cpu().numpy(), acc[1].cpu().numpy(), f["albedo"].cpu().numpy(), f["shading_normal"].cpu().numpy()
    ref64 = dv.denoise(film, half, 2, None, a, GUIDE_SPP, n, GUIDE_SPP, dtype=np.float64)
    e32 = dv.rel_err(dv.denoise(film, half, 2, None, a, GUIDE_SPP, n, GUIDE_SPP, dtype=np.float32), ref64)
    egpu = dv.rel_err(got, ref64)
    log_line('{"test": "temporal_chain_denoise_var", "e32": %.3e, "gpu": %.3e, "ratio": %.2f}' % (e32, egpu, egpu / e32 if e32 > 0 else 0.0))
    assert np.isfinite(got).all() and egpu <= 8.0 * e32, (egpu, e32)
    rgb = resolved(product, out, 1)
    assert np.isfinite(rgb).all() and rgb.min() >= 0.0 and rgb.max() <= 1.0


def test_temporal_is_deterministic_and_host_form_matches(dev, product, pkg):
    """Two calls are bit-equal; mi355pt_temporal_accumulate on host buffers is bit-equal to the device form, with and without a half film
    and a previous frame."""
    W, H = 67, 35
    for half in (True, False):
        cur, prev, vw, spp = tr.synthetic(W, H, "move", "step", half)
        for p, v in ((prev, vw), (None, None)):
            one, two = dev.run(cur, spp, p, v), dev.run(cur, spp, p, v)
            hostf = product.temporal_accumulate(cur, spp, p, ffi_view(pkg, v))
            for a, b, c in zip(one, two, hostf):
                assert (a is None) == (b is None) == (c is None)
                if a is not None:
                    assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a), bits(c))


def test_temporal_refusals_with_real_buffers(dev, product, pkg):
    """The refusals with device buffers return MI355PT_E_INVALID, the outputs stay untouched (all NaN), and the next valid call is
    bit-equal to the one before."""
    f = pkg.ffi
    W, H = 67, 35
    cur, prev, vw, spp = tr.synthetic(W, H, "move", "step", True)
    dc, dp = dev.up(cur), dev.up(prev)
    before = [x.cpu().numpy() for x in dev.run_device(dc, spp, dp, vw, None)]
    outs = dev.outputs(W, H, True)
    view, good = ffi_view(pkg, vw), product.temporal_params_default()
    frame = lambda d, **kw: f.TemporalFrame(*[dict({k: v.data_ptr() for k, v in d.items()}, **kw).get(k) for k in f.TEMPORAL_FILMS])   # noqa: E731
    o = [x.data_ptr() for x in outs]
    ref = lambda x: ctypes.byref(x) if x is not None else None   # noqa: E731

    def refused(fc, s, fp, v, w, h, p, of, oh, ol):
        rc = product.lib.mi355pt_temporal_accumulate_device(ref(fc), s, ref(fp), ref(v), w, h, ref(p), of, oh, ol, None)
        assert rc == -1 and b"temporal" in product.lib.mi355pt_last_error(), rc
    fc, fp = frame(dc), frame(dp)
    refused(None, spp, fp, view, W, H, good, *o)
    refused(frame(dc, hit=None), spp, fp, view, W, H, good, *o)
    refused(fc, spp, frame(dp, length=None), view, W, H, good, *o)
    refused(fc, spp, None, view, W, H, good, *o)
    refused(fc, spp, fp, None, W, H, good, *o)
    refused(fc, spp, frame(dp, half=None), view, W, H, good, *o)
    refused(fc, spp, fp, view, W, H, good, o[0], None, o[2])
    refused(fc, 0, fp, view, W, H, good, *o)
    refused(fc, 3, fp, view, W, H, good, *o)
    refused(fc, spp, fp, view, 0, H, good, *o)
    refused(fc, spp, fp, view, W, 0, good, *o)
    refused(fc, spp, fp, view, W, H, f.TemporalParams(), *o)
    for k, v in (("pos_tol", 0.0), ("min_weight", float("nan")), ("max_history", 0.5), ("normal_cos", 1.5)):
        p = product.temporal_params_default(); setattr(p, k, v)
        refused(fc, spp, fp, view, W, H, p, *o)
    refused(fc, spp, fp, view, W, H, good, dc["film"].data_ptr(), o[1], o[2])
    refused(fc, spp, fp, view, W, H, good, o[0], dp["half"].data_ptr(), o[2])
    refused(fc, spp, fp, view, W, H, good, o[0], o[1], dp["length"].data_ptr())
    refused(fc, spp, fp, view, W, H, good, o[0], o[0], o[2])
    dev.torch.cuda.synchronize()
    assert all(np.isnan(x.cpu().numpy()).all() for x in outs)
    after = [x.cpu().numpy() for x in dev.run_device(dc, spp, dp, vw, None, outs)]
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(before, after))


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


def replay(product, pkg, dev, frames, step, spp, guide_spp, variance):
    """the calls of `mi355pt --temporal-frames` through the ABI -> the u8 picture"""
    import torch
    sc = product.new_scene()
    cam = pkg.scenes.load_scene(sc, 3, W3, H3, build=False)
    d65 = sc.add_lut470(pkg.scenes.presets()["cie_illum_d6500"])
    base = np.array(list(cam.position), np.float32)
    acc, g, prev_cam = None, None, None
    for k in range(frames):
        pos = base + np.float32(k) * np.asarray(step, np.float32)
        for i in range(3):
            cam.position[i] = pos[i]
        if k == 0 or any(s != 0.0 for s in step):
            sc.build(cam)
        z = lambda: torch.zeros((H3, W3, 3), dtype=torch.float32, device="cuda")   # noqa: E731
        f = {n: z() for n in ("film", "position", "shading_normal", "hit")}
        gb = {n: f[n].data_ptr() for n in ("shading_normal", "position", "hit")}
        prm = pkg.make_params(spp, "mis", "sobol", seed=k)
        if variance:
            f["half"], f["albedo"] = z(), z()
            gb["albedo"] = f["albedo"].data_ptr()
        product.render_gbuffer_accum_device(sc, cam, pkg.make_params(guide_spp, "mis", "sobol", seed=k), d65, 0, guide_spp, gb)
        if variance:
            product.render_accum_device(sc, cam, prm, 0, spp // 2, f["half"].data_ptr())
            torch.cuda.synchronize()
            f["film"].copy_(f["half"])
            product.render_accum_device(sc, cam, prm, spp // 2, spp, f["film"].data_ptr())
        else:
            product.render_accum_device(sc, cam, prm, 0, spp, f["film"].data_ptr())
        torch.cuda.synchronize()
        prev, view = None, None
        if acc is not None:
            prev = dict(frame_of(g, ("position", "shading_normal", "hit")), film=acc[0], length=acc[2])
            if variance:
                prev["half"] = acc[1]
            view = product.temporal_view_from_cameras(cam, prev_cam)
        acc = dev.run_device(frame_of(f), spp, prev, view, None)
        g, prev_cam = f, pkg.ffi.Camera.from_buffer_copy(cam)
    film = acc[0]
    if variance:
        need = product.denoise_var_scratch_bytes(W3, H3)
        scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
        film = torch.zeros((H3, W3, 3), dtype=torch.float32, device="cuda")
        product.denoise_var_device(acc[0].data_ptr(), acc[1].data_ptr(), 2, None, g["albedo"].data_ptr(), guide_spp, g["shading_normal"].data_ptr(), guide_spp,
                                   W3, H3, product.denoise_var_params_default(), scratch.data_ptr(), need, film.data_ptr())
    rgb = torch.empty_like(film)
    product.film_resolve_device(film.data_ptr(), W3 * H3, 1, rgb.data_ptr())
    torch.cuda.synchronize()
    return product.quantize_u8(rgb.cpu().numpy())


@pytest.mark.parametrize("variance", [False, True], ids=["alone", "denoise_variance"])
def test_temporal_cli(product, pkg, dev, cli, tmp_path, variance):
    """`--temporal-frames 3 --camera-step 0.1,0,0` at 64 x 48, alone and with --denoise-variance: the PNG equals quantize_u8 of the same
    calls replayed through the ABI; a zero step (the scene is built once) likewise; the documented misuse cases exit 2."""
    from PIL import Image
    exe, env = cli
    base = [exe, "--scene", "3", "--renderer", "mis", "--sampler", "sobol", "--spp", str(FRAME_SPP), "--width", str(W3), "--height", str(H3),
            "--denoise-guide-spp", str(GUIDE_SPP), "--temporal-frames", "3"] + (["--denoise-variance"] if variance else [])
    for step, extra in (((0.1, 0.0, 0.0), ["--camera-step", "0.1,0,0"]), ((0.0, 0.0, 0.0), [])):
        path = str(tmp_path / f"t{len(extra)}.png")
        r = subprocess.run(base + extra + ["-o", path], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        got = np.asarray(Image.open(path).convert("RGB"))
        want = replay(product, pkg, dev, 3, step, FRAME_SPP, GUIDE_SPP, variance)
        assert got.shape == want.shape and np.array_equal(got, want), (step, int((got != want).sum()))
        assert got.mean() > 10.0
    if not variance:
        for args in tr.CLI_MISUSE:
            r = subprocess.run([exe, *args], env=env, capture_output=True, text=True, timeout=60, cwd=tmp_path)
            assert r.returncode == 2 and ("temporal" in r.stderr or "--camera-step" in r.stderr), (args, r.returncode, r.stderr)
