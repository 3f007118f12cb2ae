"""GPU tests of the rectified temporal accumulation (mi355pt_temporal_accumulate_rectified_device / mi355pt_temporal_accumulate_rectified,
csrc/pt_kernels_temporal_rectify.hip) against the NumPy restatement of tests/temporal_rectify_reference.py.  Every operation of the two
kernels is a single binary32 operation in the order the header states — square root included — so the bar is BIT EQUALITY on every output
value; the outputs start as NaN, so a value the kernels leave out shows."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import temporal_reference as tr  # noqa: E402
import temporal_rectify_reference as rr  # noqa: E402

pytestmark = pytest.mark.gpu

# (W, H): a frame smaller than the apron, ragged edges, windows that cross block edges (64 x 4 blocks) and frame edges, partial blocks
SHAPES = [(1, 1), (3, 2), (63, 5), (64, 4), (65, 9), (130, 70)]
VIEWS = ("static", "move", "outside", "behind")
W3, H3 = 64, 48                  # the rendered tests: scene 3
GUIDE_SPP, FRAME_SPP, HISTORY, AFTER = 16, 4, 8, 4


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


def ffi_rectify(product, rprm):
    p = product.temporal_rectify_params_default()
    if rprm is not None:
        p.radius, p.gamma = int(rprm.radius), float(rprm.gamma)
    return p


class Device:
    """frames on the device + one call of mi355pt_temporal_accumulate_rectified_device (or, rectified=False, of
    mi355pt_temporal_accumulate_device); the outputs start as NaN, the scratch as the byte 0x5a"""

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

    def scratch(self, W, H):
        return self.torch.full((self.product.temporal_rectify_scratch_bytes(W, H),), 0x5a, dtype=self.torch.uint8, device="cuda")

    def run_device(self, cur, spp, prev, view, prm=None, rprm=None, rectified=True, scratch=None):
        """cur / prev: dicts of device tensors -> the three output tensors (half None without a half film)"""
        H, W = cur["film"].shape[:2]
        of, oh, ol = self.outputs(W, H, "half" in cur)
        ptr = lambda d: {k: v.data_ptr() for k, v in d.items()} if d is not None else None   # noqa: E731
        tail = (of.data_ptr(), oh.data_ptr() if oh is not None else None, ol.data_ptr())
        if rectified:
            scratch = scratch if scratch is not None else self.scratch(W, H)
            self.product.temporal_accumulate_rectified_device(ptr(cur), spp, ptr(prev), ffi_view(self.pkg, view), W, H, ffi_params(self.product, prm),
                                                              ffi_rectify(self.product, rprm), scratch.data_ptr(), scratch.numel(), *tail)
        else:
            self.product.temporal_accumulate_device(ptr(cur), spp, ptr(prev), ffi_view(self.pkg, view), W, H, ffi_params(self.product, prm), *tail)
        self.torch.cuda.synchronize()
        return of, oh, ol

    def run(self, cur, spp, prev=None, view=None, prm=None, rprm=None, rectified=True):
        """host frames in, host arrays out"""
        of, oh, ol = self.run_device(self.up(cur), spp, self.up(prev), view, prm, rprm, rectified)
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
def test_temporal_rectify_synthetic_parity(dev, shape, half):
    """Seeded synthetic frames (the two-plane step, HDR noise, NaN / inf / negative current values, a background band, previous lengths with
    zeros — holes in the windows) at every shape, with and without a half film, radius 1, 2 and 3, through the static view, a move with a
    yaw, a view with part of the frame outside the history and one with part of it behind the previous camera: every output value is
    bit-equal to the f32 restatement, nothing is left unwritten."""
    W, H = shape
    for view in VIEWS:
        cur, prev, vw, spp = tr.synthetic(W, H, view, "step", half)
        dc, dp = dev.up(cur), dev.up(prev)
        for radius in (1, 2, 3):
            rprm = rr.params(radius=radius)
            got = [x.cpu().numpy() if x is not None else None for x in dev.run_device(dc, spp, dp, vw, None, rprm)]
            assert_bit_equal(got, rr.accumulate(cur, spp, prev, vw, rprm=rprm), f"temporal_rectify_synthetic_{W}x{H}_{'half' if half else 'nohalf'}_{view}_r{radius}")


def test_temporal_rectify_parity_other_parameters(dev):
    """gamma 0.5 and 8, every parameter of the reprojection away from its default (spp 6), and the exact pixel grid, where a shift of half a
    pixel gathers with the weights 1/2, 1/2 and a shift by the frame's width leaves no history at all."""
    W, H = 67, 35
    for gamma in (0.5, 8.0):
        for half in (True, False):
            cur, prev, vw, spp = tr.synthetic(W, H, "move", "step", half)
            rprm = rr.params(gamma=gamma, radius=2 if half else 3)
            assert_bit_equal(dev.run(cur, spp, prev, vw, None, rprm), rr.accumulate(cur, spp, prev, vw, rprm=rprm),
                             f"temporal_rectify_gamma_{gamma}_{'half' if half else 'nohalf'}")
    prm = tr.params(pos_tol=0.5, normal_cos=-1.0, min_weight=0.3, max_history=5.0)
    for view in VIEWS:
        cur, prev, vw, spp = tr.synthetic(W, H, view, "step", True, spp=6)
        assert_bit_equal(dev.run(cur, spp, prev, vw, prm), rr.accumulate(cur, spp, prev, vw, prm), f"temporal_rectify_params_{view}")
    gb = tr.grid_frame(W, H)
    rng = np.random.default_rng(2)
    cur = dict(gb, film=tr.hdr(rng, (H, W, 3)), half=None)
    prev = dict(gb, film=tr.hdr(rng, (H, W, 3)), half=None, length=np.full((H, W), 3.0, np.float32))
    for dx, dy in ((0.0, 0.0), (3.0, 2.0), (0.5, 0.0), (-1.0, -0.25), (float(W), 0.0)):
        vw = tr.grid_view(W, H, dx, dy)
        assert_bit_equal(dev.run(cur, 1, prev, vw), rr.accumulate(cur, 1, prev, vw), f"temporal_rectify_grid_{dx}_{dy}")


def test_temporal_rectify_first_frame_is_the_plain_one(dev, product):
    """prev == NULL: bit-equal to mi355pt_temporal_accumulate_device, and the scratch keeps every byte."""
    W, H = 67, 35
    for half in (True, False):
        cur, _, _, spp = tr.synthetic(W, H, "static", "step", half)
        dc = dev.up(cur)
        scratch = dev.scratch(W, H)
        got = dev.run_device(dc, spp, None, None, scratch=scratch)
        want = dev.run_device(dc, spp, None, None, rectified=False)
        for a, b in zip(got, want):
            assert (a is None) == (b is None)
            if a is not None:
                assert np.array_equal(bits(a.cpu().numpy()), bits(b.cpu().numpy()))
        assert bool((scratch == 0x5a).all())


def test_temporal_rectify_is_deterministic_and_host_form_matches(dev, product, pkg):
    """Two calls are bit-equal (a scratch that starts as other bytes included); mi355pt_temporal_accumulate_rectified on host buffers is
    bit-equal to the device form, with and without a half film and a previous frame."""
    W, H = 67, 35
    for half in (True, False):
        cur, prev, vw, spp = tr.synthetic(W, H, "move", "step", half)
        for p, v in ((prev, vw), (None, None)):
            one = dev.run(cur, spp, p, v)
            other = dev.scratch(W, H); other.fill_(0xff)                      # NaN bit patterns in every record before the gather
            two = [x.cpu().numpy() if x is not None else None for x in dev.run_device(dev.up(cur), spp, dev.up(p), v, scratch=other)]
            hostf = product.temporal_accumulate_rectified(cur, spp, p, ffi_view(pkg, v))
            for a, b, c in zip(one, two, hostf):
                assert (a is None) == (b is None) == (c is None)
                if a is not None:
                    assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a), bits(c))


def test_temporal_rectify_refusals_with_real_buffers(dev, product, pkg):
    """What the new header refuses, with device buffers: MI355PT_E_INVALID, the outputs and the scratch stay untouched."""
    f = pkg.ffi
    W, H = 67, 35
    cur, prev, vw, spp = tr.synthetic(W, H, "move", "step", True)
    dc, dp = dev.up(cur), dev.up(prev)
    outs = dev.outputs(W, H, True)
    scratch = dev.scratch(W, H)
    view, good, rgood = ffi_view(pkg, vw), product.temporal_params_default(), product.temporal_rectify_params_default()
    frame = lambda d: f.TemporalFrame(*[{k: v.data_ptr() for k, v in d.items()}.get(k) for k in f.TEMPORAL_FILMS])   # noqa: E731
    fc, fp, o = frame(dc), frame(dp), [x.data_ptr() for x in outs]
    ref = lambda x: ctypes.byref(x) if x is not None else None   # noqa: E731

    def refused(rp, sp, nbytes, p=good):
        rc = product.lib.mi355pt_temporal_accumulate_rectified_device(ref(fc), spp, ref(fp), ref(view), W, H, ref(p), ref(rp), sp, nbytes, *o, None)
        assert rc == -1 and b"temporal" in product.lib.mi355pt_last_error(), rc
    sp, need = scratch.data_ptr(), scratch.numel()
    refused(None, sp, need)
    refused(f.TemporalRectifyParams(), sp, need)
    refused(f.TemporalRectifyParams(0, 2.0), sp, need)
    refused(f.TemporalRectifyParams(4, 2.0), sp, need)
    refused(f.TemporalRectifyParams(2, 0.0), sp, need)
    refused(f.TemporalRectifyParams(2, float("nan")), sp, need)
    refused(rgood, None, need)
    refused(rgood, sp, need - 1)
    refused(rgood, sp + 4, need)
    refused(rgood, o[0], need)
    refused(rgood, dp["film"].data_ptr(), need)
    refused(rgood, sp, need, f.TemporalParams())
    dev.torch.cuda.synchronize()
    assert all(np.isnan(x.cpu().numpy()).all() for x in outs) and bool((scratch == 0x5a).all())


# ---------------- rendered frames: scene 3 at 64 x 48 ----------------
def render_frame(product, pkg, handle, seed, spp=FRAME_SPP, guide_spp=GUIDE_SPP):
    """one frame's device films: the G-buffer sums at guide_spp, the half film [0, spp / 2) and the film [0, spp)"""
    import torch
    sc, cam, d65 = handle
    z = lambda: torch.zeros((H3, W3, 3), dtype=torch.float32, device="cuda")   # noqa: E731
    f = {k: z() for k in ("film", "half", "position", "shading_normal", "hit")}
    g = {k: f[k].data_ptr() for k in ("shading_normal", "position", "hit")}
    product.render_gbuffer_accum_device(sc, cam, pkg.make_params(guide_spp, "mis", "sobol", seed=seed), d65, 0, guide_spp, g)
    prm = pkg.make_params(spp, "mis", "sobol", seed=seed)
    product.render_accum_device(sc, cam, prm, 0, spp // 2, f["half"].data_ptr())
    torch.cuda.synchronize()
    f["film"].copy_(f["half"])
    product.render_accum_device(sc, cam, prm, spp // 2, spp, f["film"].data_ptr())
    torch.cuda.synchronize()
    return f


def resolved(product, film_tensor, spp):
    import torch
    rgb = torch.empty_like(film_tensor)
    product.film_resolve_device(film_tensor.data_ptr(), W3 * H3, spp, rgb.data_ptr())
    torch.cuda.synchronize()
    return rgb.cpu().numpy().astype(np.float64)


def test_temporal_rectify_follows_a_fourfold_change_on_the_device(dev, product, pkg):
    """The x4 case of tests/test_temporal_rectify.py on device-rendered frames: a static camera, frames of 4 spp with seeds 0 .. 11 and
    G-buffers at 16 spp; the films of frames 0 .. 7 are scaled by 4 (the light was four times as bright), frames 8 .. 11 are the true ones.
    RMSE after the resolve against the GPU's own 1024-spp frame: E_rect <= sqrt(E_unrectified E_32), the same bar.  The CPU figures are
    0.094 against the bar 0.137 (profiles/temporal_rectify_cpu.json)."""
    handle = tr.load_moved(product, pkg, 3, W3, H3)
    sc, cam, _ = handle
    view = product.temporal_view_from_cameras(cam, cam)
    frames = [render_frame(product, pkg, handle, k) for k in range(HISTORY + AFTER)]
    geo = ("position", "shading_normal", "hit")
    acc = {}
    for name, rectified in (("rectified", True), ("unrectified", False)):
        prev = None
        for k, f in enumerate(frames):
            s = 4.0 if k < HISTORY else 1.0
            cur = dict({g: f[g] for g in geo}, film=f["film"] * s, half=f["half"] * s)
            out = dev.run_device(cur, FRAME_SPP, prev, view if prev is not None else None, rectified=rectified)
            prev = dict({g: f[g] for g in geo}, film=out[0], half=out[1], length=out[2])
        acc[name] = out
    rmse = lambda a, b: float(np.sqrt(np.mean((a - b) ** 2)))   # noqa: E731
    ref = product.render(sc, cam, pkg.make_params(1024, "mis", "sobol", seed=1000)).astype(np.float64)
    e32 = rmse(product.render(sc, cam, pkg.make_params(32, "mis", "sobol", seed=0)).astype(np.float64), ref)
    e_r, e_u = rmse(resolved(product, acc["rectified"][0], 2), ref), rmse(resolved(product, acc["unrectified"][0], 2), ref)
    cpu = json.load(open(os.path.join(pkg.ffi.ROOT, "profiles", "temporal_rectify_cpu.json")))["runs"]["x4"]
    log_line('{"test": "temporal_rectify_x4_gpu", "E_32": %.5f, "E_rect": %.5f, "E_unrectified": %.5f, "bar": %.5f, "cpu_E_rect": %.5f, "cpu_E_unrectified": %.5f}'
             % (e32, e_r, e_u, (e_u * e32) ** 0.5, cpu["E_rect"], cpu["E_unrectified"]))
    assert e_u > e32
    assert e_r <= (e_u * e32) ** 0.5, (e_r, e_u, e32)
    assert np.array_equal(acc["rectified"][2].cpu().numpy(), acc["unrectified"][2].cpu().numpy())      # out_length is the plain accumulation's


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


def replay(product, pkg, dev, frames, step, spp, guide_spp, rprm):
    """the calls of `mi355pt --temporal-frames N --temporal-rectify` (without --denoise-variance: no half film) through the ABI -> the u8 picture"""
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
        f = {n: torch.zeros((H3, W3, 3), dtype=torch.float32, device="cuda") for n in ("film", "position", "shading_normal", "hit")}
        gb = {n: f[n].data_ptr() for n in ("shading_normal", "position", "hit")}
        product.render_gbuffer_accum_device(sc, cam, pkg.make_params(guide_spp, "mis", "sobol", seed=k), d65, 0, guide_spp, gb)
        product.render_accum_device(sc, cam, pkg.make_params(spp, "mis", "sobol", seed=k), 0, spp, f["film"].data_ptr())
        torch.cuda.synchronize()
        prev, view = None, None
        if acc is not None:
            prev = dict({n: g[n] for n in ("position", "shading_normal", "hit")}, film=acc[0], length=acc[2])
            view = product.temporal_view_from_cameras(cam, prev_cam)
        acc = dev.run_device(f, spp, prev, view, None, rprm)
        g, prev_cam = f, pkg.ffi.Camera.from_buffer_copy(cam)
    rgb = torch.empty_like(acc[0])
    product.film_resolve_device(acc[0].data_ptr(), W3 * H3, 1, rgb.data_ptr())
    torch.cuda.synchronize()
    return product.quantize_u8(rgb.cpu().numpy())


def test_temporal_rectify_cli(product, pkg, dev, cli, tmp_path):
    """`--temporal-frames 3 --camera-step 0.1,0,0 --temporal-rectify` at 64 x 48, with the default parameters and with --temporal-rectify-radius 3
    --temporal-rectify-gamma 0.5: the PNG equals quantize_u8 of the same calls replayed through the ABI, and differs from the PNG without
    --temporal-rectify; the documented misuse cases exit 2."""
    from PIL import Image
    exe, env = cli
    base = [exe, "--scene", "3", "--renderer", "mis", "--sampler", "sobol", "--spp", str(FRAME_SPP), "--width", str(W3), "--height", str(H3),
            "--denoise-guide-spp", str(GUIDE_SPP), "--temporal-frames", "3", "--camera-step", "0.1,0,0"]

    def picture(extra, name):
        path = str(tmp_path / name)
        r = subprocess.run(base + extra + ["-o", path], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        return np.asarray(Image.open(path).convert("RGB"))
    plain = picture([], "plain.png")
    for i, (extra, rprm) in enumerate(((["--temporal-rectify"], rr.params()),
                                      (["--temporal-rectify", "--temporal-rectify-radius", "3", "--temporal-rectify-gamma", "0.5"], rr.params(radius=3, gamma=0.5)))):
        got = picture(extra, f"r{i}.png")
        want = replay(product, pkg, dev, 3, (0.1, 0.0, 0.0), FRAME_SPP, GUIDE_SPP, rprm)
        assert got.shape == want.shape and np.array_equal(got, want), (extra, int((got != want).sum()))
        assert got.mean() > 10.0 and not np.array_equal(got, plain)
    for args in rr.CLI_MISUSE:
        r = subprocess.run([exe, *args], env=env, capture_output=True, text=True, timeout=60, cwd=tmp_path)
        assert r.returncode == 2 and "--temporal-rectify" in r.stderr, (args, r.returncode, r.stderr)
