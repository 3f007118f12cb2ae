"""GPU tests of the G-buffer pass (include/mi355pt_gbuffer.h, csrc/pt_kernels_gbuffer.hip): against the existing albedo renderer, against
itself (a film never depends on which other films were asked for), against the CPU restatement of tests/gbuffer_reference.cpp, and through
the host entry point and the CLI.  Figures go to the file MI355PT_FRAME_LOG names (profiles/gbuffer_parity.jsonl)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gbuffer_reference  # noqa: E402

pytestmark = pytest.mark.gpu

FILMS = gbuffer_reference.FILMS
# the project's per-sample bars (tests/test_aov_gpu.py, profiles/aov_parity.jsonl): caps on what may be left out, not tolerances
PER_SAMPLE_MIN = 0.9995          # share within 1e-3 |c| + 1e-4
TIGHT_MIN = 0.997                # share within 1e-5 max(1, t)


@pytest.fixture(scope="module")
def ref():
    return gbuffer_reference.GbufferReference()


@pytest.fixture(scope="module")
def scenes(product, ref):
    """scene id -> {"gpu": (scene, camera, d65), "cpu": ...}, built once (the build depends on the camera's position only)"""
    cache = {}

    def get(scene_id, cpu=False):
        pair = cache.setdefault(scene_id, {})
        if "gpu" not in pair:
            pair["gpu"] = gbuffer_reference.load(product, scene_id, 64, 48)
        if cpu and "cpu" not in pair:
            pair["cpu"] = gbuffer_reference.load(ref, scene_id, 64, 48)
            ref.set_faithful(pair["cpu"][0], False)      # (faithful == fast for primary rays, bit for bit: tests/test_aov.py)
        return pair
    return get


def sized(cam, w, h, pkg):
    c = pkg.ffi.Camera.from_buffer_copy(cam)
    c.width, c.height = w, h
    return c


def log_line(text):
    if os.environ.get("MI355PT_FRAME_LOG"):
        with open(os.environ["MI355PT_FRAME_LOG"], "a") as f:
            f.write(text + "\n")


class Slab:
    """Four neighbouring film slots in ONE device buffer, NaN-filled; the wanted films' slots are zeroed (or take `init`).  After a launch
    the slots of the films that were not requested must still be all NaN: a film whose pointer is NULL is never written."""

    def __init__(self, w, h, want, init=None):
        import torch
        self.torch, self.w, self.h, self.want = torch, w, h, tuple(want)
        self.buf = torch.full((4, h, w, 3), float("nan"), dtype=torch.float32, device="cuda")
        for i, k in enumerate(FILMS):
            if k in self.want:
                self.buf[i] = 0.0 if init is None else torch.from_numpy(init[k]).cuda()

    def ptrs(self):
        return {k: self.buf[i].data_ptr() for i, k in enumerate(FILMS) if k in self.want}

    def films(self):
        self.torch.cuda.synchronize()
        host = self.buf.cpu().numpy()
        for i, k in enumerate(FILMS):
            if k not in self.want:
                assert np.isnan(host[i]).all(), f"the {k} film was not requested but its neighbouring slot was written"
        return {k: host[i] for i, k in enumerate(FILMS) if k in self.want}


def gpu_films(product, pkg, gpu, w, h, spp, want=FILMS, sampler="sobol", ranges=None, shards=1, stats=None):
    """the requested films after the launches of `ranges` ([(begin, end)], default the whole range) x `shards` into one zeroed slab"""
    sc, cam, d65 = gpu
    slab = Slab(w, h, want)
    for b, e in (ranges or [(0, spp)]):
        for shard in range(shards):
            prm = pkg.make_params(spp, "mis", sampler, shard_index=shard, shard_count=shards)
            product.render_gbuffer_accum_device(sc, sized(cam, w, h, pkg), prm, d65, b, e, slab.ptrs(), None, stats)
    return slab.films()


@pytest.mark.parametrize("sampler", ["sobol", "random"])
@pytest.mark.parametrize("scene_id", [0, 3, 17, 19, 30])
def test_gbuffer_albedo_bit_equal_to_aov(product, pkg, scenes, scene_id, sampler):
    """The albedo film of the four-film launch equals the film of mi355pt_render_aov_accum_device(MI355PT_AOV_ALBEDO) bit for bit, 64x48 at
    4 spp: the pass draws the albedo renderer's dimensions and shoots its rays (this pins the sampling schedule)."""
    import torch
    W, H, spp = 64, 48, 4
    sc, cam, d65 = scenes(scene_id)["gpu"]
    prm = pkg.make_params(spp, "mis", sampler)
    aov = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    product.render_aov_accum_device(sc, sized(cam, W, H, pkg), prm, pkg.ffi.AOV_ALBEDO, d65, 0, spp, aov.data_ptr(), None)
    torch.cuda.synchronize()
    want = aov.cpu().numpy()
    got = gpu_films(product, pkg, scenes(scene_id)["gpu"], W, H, spp, sampler=sampler)
    assert want.max() > 0.1 and np.isfinite(want).all()
    differ = int((got["albedo"].view(np.uint32) != want.view(np.uint32)).sum())
    print(scene_id, sampler, "albedo values differing", differ)
    assert differ == 0


@pytest.mark.parametrize("size", [(9, 7), (8, 8), (64, 48)])
@pytest.mark.parametrize("scene_id", [3, 19])
def test_gbuffer_independence_of_the_request(product, pkg, scenes, scene_id, size):
    """Each film rendered alone is bit-equal to the same film of the four-film launch — and the slots of the three films that were not
    requested stay NaN —; [0, 2) + [2, 4) is bit-equal to [0, 4); three shards are bit-equal to the whole frame; two runs are bit-equal;
    the stats block counts the samples and primary rays."""
    W, H = size
    spp = 4
    gpu = scenes(scene_id)["gpu"]
    st = pkg.ffi.Stats()
    whole = gpu_films(product, pkg, gpu, W, H, spp, stats=st)
    assert st.samples == st.closest_rays == W * H * spp and 0 < st.closest_hits <= st.samples and st.launches == 1 and st.kernel_ms > 0.0
    assert st.shadow_rays == 0 and st.bounces == 0
    hit = whole["hit"]
    assert st.closest_hits == int(hit[..., 1].sum()) and np.all(hit[..., 2] <= hit[..., 1]) and np.all(hit[..., 1] <= spp)
    for k in FILMS:
        assert np.isfinite(whole[k]).all(), k
        alone = gpu_films(product, pkg, gpu, W, H, spp, want=(k,))
        assert np.array_equal(alone[k].view(np.uint32), whole[k].view(np.uint32)), k
    pair = gpu_films(product, pkg, gpu, W, H, spp, want=("shading_normal", "hit"))
    assert all(np.array_equal(pair[k].view(np.uint32), whole[k].view(np.uint32)) for k in pair)
    for name, other in (("ranges", gpu_films(product, pkg, gpu, W, H, spp, ranges=[(0, 2), (2, 4)])),
                        ("shards", gpu_films(product, pkg, gpu, W, H, spp, shards=3)),
                        ("again", gpu_films(product, pkg, gpu, W, H, spp))):
        for k in FILMS:
            assert np.array_equal(other[k].view(np.uint32), whole[k].view(np.uint32)), (name, k)


@pytest.mark.parametrize("scene_id", [0, 3, 8, 17, 19, 30])
def test_gbuffer_parity_with_the_cpu_restatement(product, ref, pkg, scenes, scene_id):
    """One pixel = one sample (256x192 at 1 spp, Sobol) against tests/gbuffer_reference.cpp.  On every pixel where both sides hit the same
    class (BSDF surface / emitter / miss) shading_normal and hit.yz are bit-equal; position and hit.x meet the project's two per-sample
    bars over ALL pixels (a pixel whose classes differ counts as left out)."""
    W, H = 256, 192
    pair = scenes(scene_id, cpu=True)
    g = gpu_films(product, pkg, pair["gpu"], W, H, 1)
    sc, cam, d65 = pair["cpu"]
    c, cls = ref.render_gbuffer_accum(sc, sized(cam, W, H, pkg), pkg.make_params(1, "mis", "sobol"), d65, want_classes=True)
    for k in FILMS:
        assert np.array_equal(np.isnan(g[k]), np.isnan(c[k])), k
    g_class = np.where(g["hit"][..., 1] == 0, 2, np.where(g["hit"][..., 2] == 1, 1, 0))
    c_class = np.argmax(cls, axis=2)
    same = g_class == c_class
    assert np.array_equal(g["shading_normal"][same].view(np.uint32), c["shading_normal"][same].view(np.uint32))
    assert np.array_equal(g["hit"][..., 1:][same].view(np.uint32), c["hit"][..., 1:][same].view(np.uint32))
    t = c["hit"][..., 0]
    line = {"test": "per_sample", "scene": scene_id, "same_class": float(same.mean())}
    shares = {}
    for name, gv, cv in (("position", g["position"], c["position"]), ("hit_x", g["hit"][..., :1], c["hit"][..., :1])):
        d = np.abs(gv - cv)
        close = (np.all(d <= 1e-3 * np.abs(cv) + 1e-4, axis=2) & same).mean()
        tight = (np.all(d <= 1e-5 * np.maximum(1.0, t)[..., None], axis=2) & same).mean()
        shares[name] = (close, tight)
        line.update({f"{name}_close": round(float(close), 6), f"{name}_tight": round(float(tight), 6), f"{name}_max_dev": float(f"{d.max():.3e}"),
                     f"{name}_bit_equal": round(float(np.all(gv == cv, axis=2).mean()), 6)})
    line["albedo_max_dev"] = float(f"{np.abs(g['albedo'] - c['albedo']).max():.3e}")
    import json
    log_line(json.dumps(line))
    print(line)
    for name, (close, tight) in shares.items():
        assert close >= PER_SAMPLE_MIN, (name, close)
        assert tight >= TIGHT_MIN, (name, tight)


@pytest.mark.parametrize("scene_id", [3, 19])
def test_gbuffer_frame_rmse_is_recorded(product, ref, pkg, scenes, scene_id):
    """64x48 at 64 spp against the CPU restatement: there is no frame bar for these films, the RMSE of each film's mean is RECORDED
    (MI355PT_FRAME_LOG) together with the number of pixels whose hit counts differ; what is asserted is only that both sides are finite."""
    W, H, spp = 64, 48, 64
    pair = scenes(scene_id, cpu=True)
    g = gpu_films(product, pkg, pair["gpu"], W, H, spp)
    sc, cam, d65 = pair["cpu"]
    c = ref.render_gbuffer_accum(sc, sized(cam, W, H, pkg), pkg.make_params(spp, "mis", "sobol"), d65)
    import json
    line = {"test": "frame", "scene": scene_id}
    for k in FILMS:
        assert np.isfinite(g[k]).all() and np.isfinite(c[k]).all(), k
        line[f"{k}_rmse"] = float(f"{np.sqrt(np.mean((g[k] / spp - c[k] / spp) ** 2)):.3e}")
    line["hit_count_differs"] = int((g["hit"][..., 1] != c["hit"][..., 1]).sum())
    log_line(json.dumps(line))
    print(line)


def render_normalized(product, pkg, scenes, spp, sampler="sobol"):
    """scene 19, 64x48 at `spp`: the four sums and what mi355pt_gbuffer_normalize_device makes of shading_normal, position and hit"""
    import torch
    W, H = 64, 48
    sc, cam, d65 = scenes(19)["gpu"]
    slab = Slab(W, H, FILMS)
    product.render_gbuffer_accum_device(sc, sized(cam, W, H, pkg), pkg.make_params(spp, "mis", sampler), d65, 0, spp, slab.ptrs())
    out = torch.full((3, H, W, 3), float("nan"), dtype=torch.float32, device="cuda")
    ptrs = slab.ptrs()
    for i, k in enumerate(("shading_normal", "position", "hit")):
        product.gbuffer_normalize_device(ptrs[k], ptrs["hit"], W * H, out[i].data_ptr())
    sums = slab.films()
    host = out.cpu().numpy()
    return spp, sums, {k: host[i] for i, k in enumerate(("shading_normal", "position", "hit"))}


@pytest.fixture(scope="module")
def normalized(product, pkg, scenes):
    """4 spp: partly covered pixels with one, two and three hits (the quotient's divisors)"""
    return render_normalized(product, pkg, scenes, 4)


def test_gbuffer_normalize_is_the_quotient(normalized):
    """mi355pt_gbuffer_normalize_device equals the NumPy quotient film / hit.y bit for bit where hit.y > 0 and is 0 elsewhere; the frame
    has pixels with 0 < hit.y < spp (without one the input would prove nothing: a failure of the test's input, not a pass) and pixels
    with hit.y == 0; depth = hit.x / hit.y is the mean distance."""
    spp, sums, norm = normalized
    cnt = sums["hit"][..., 1]
    partial = (cnt > 0) & (cnt < spp)
    assert partial.sum() > 0, "the chosen frame has no partly covered pixel"
    assert (cnt == 0).sum() > 0 and (cnt == spp).sum() > 0
    for k, got in norm.items():
        with np.errstate(divide="ignore", invalid="ignore"):
            want = np.where(cnt[..., None] > 0, sums[k] / cnt[..., None], np.float32(0.0)).astype(np.float32)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), k
        assert np.all(got[cnt == 0] == 0.0)
    assert np.all(norm["hit"][..., 1][cnt > 0] == 1.0)
    depth = norm["hit"][..., 0]
    assert np.all(depth[cnt > 0] > 0.0)
    # dividing by the hit count, not by spp: on partly covered pixels the two differ
    assert np.all(depth[partial] > (sums["hit"][..., 0] / spp)[partial])


def test_gbuffer_normalized_silhouette_normals_are_unit(product, pkg, scenes, normalized):
    """On scene 19's silhouette pixels (0 < hit.y < spp) the coverage-normalised normal, decoded n * 2 - 1, has length within 1e-3 of 1,
    where sum / spp — what every AOV mean gives there — is biased towards 0 by the misses.  A partly covered pixel must exist in the frame.

    The frame is 64x48 at 2 spp, and the sample count is chosen by reasoning, not by trying: the film holds SUMS of n * 0.5 + 0.5 over the
    samples that hit, so film / hit.y decodes to the MEAN of those unit normals.  Two unit vectors an angle t apart have a mean of length
    cos(t / 2): whatever the divisor, the length is 1 only where the hits of a pixel agree on the normal, which is a property of the
    geometry under the pixel, not of the normalisation.  What dividing by the hit count — and only that — guarantees is that a pixel's mean
    is the mean over its HITS; 2 spp is the smallest count with partly covered pixels, and each of them has exactly one hit, so the mean is
    that hit's normal and the bound must hold on EVERY silhouette pixel, with 1e-3 against the 1e-7 of the rounding.  A normalisation that
    divided by spp, or by anything but hit.y, gives n / 2 - 1 / 2 there and fails by up to 1.  The sampler is the random one: the two
    Sobol samples of a pixel of this frame hit or miss together (the CPU restatement finds no partly covered pixel at 2 spp with Sobol,
    28 with the random sampler), and a frame without such a pixel is a failure of the test's input.
    At 4 spp the same pixels hold one to three hits and the geometry shows: on the dragons' silhouettes against the sky the hits land on
    differently oriented faces.  Those figures are printed and logged (MI355PT_FRAME_LOG), not asserted: the CPU restatement of
    tests/gbuffer_reference.cpp gives 29 of 58 partly covered pixels outside 1e-3 there, the worst by 0.394."""
    spp, sums, norm = render_normalized(product, pkg, scenes, 2, sampler="random")
    cnt = sums["hit"][..., 1]
    partial = (cnt > 0) & (cnt < spp)
    assert partial.sum() > 0, "the chosen frame has no partly covered pixel"
    dev = np.abs(np.linalg.norm(norm["shading_normal"][partial] * 2.0 - 1.0, axis=1) - 1.0)
    biased = np.abs(np.linalg.norm(sums["shading_normal"][partial] / np.float32(spp) * 2.0 - 1.0, axis=1) - 1.0)
    spp4, sums4, norm4 = normalized
    cnt4 = sums4["hit"][..., 1]
    partial4 = (cnt4 > 0) & (cnt4 < spp4)
    dev4 = np.abs(np.linalg.norm(norm4["shading_normal"][partial4] * 2.0 - 1.0, axis=1) - 1.0)
    print("2 spp: silhouette pixels", int(partial.sum()), "worst", float(dev.max()), "; sum / spp instead: worst", float(biased.max()))
    print("4 spp (recorded, not asserted): silhouette pixels", int(partial4.sum()), "outside 1e-3:", int((dev4 > 1e-3).sum()), "worst", float(dev4.max()))
    log_line(f'{{"test": "silhouette_normals", "scene": 19, "spp": 2, "sampler": "random", "partial_pixels": {int(partial.sum())}, "worst": {float(dev.max()):.3e}, '
             f'"worst_of_sum_over_spp": {float(biased.max()):.3e}, "recorded_4spp": {{"partial_pixels": {int(partial4.sum())}, '
             f'"outside_1e-3": {int((dev4 > 1e-3).sum())}, "worst": {float(dev4.max()):.3e}}}}}')
    assert dev.max() <= 1e-3, (int((dev > 1e-3).sum()), float(dev.max()))
    assert biased.max() > 1e-3                               # (the bias the normalisation divides out is there)


def test_gbuffer_host_entry_point(product, pkg, scenes):
    """mi355pt_render_gbuffer is bit-equal to device accumulation plus resolve (albedo through mi355pt_aov_resolve_device(ALBEDO), the
    other films sum / spp); a subset of the films comes back the same; its stats count the frame."""
    import torch
    W, H, spp = 64, 48, 4
    sc, cam, d65 = scenes(3)["gpu"]
    cam = sized(cam, W, H, pkg)
    prm = pkg.make_params(spp, "mis", "sobol")
    host, st = product.render_gbuffer(sc, cam, prm, d65, want_stats=True)
    assert st.samples == W * H * spp and st.launches == 1
    sums = gpu_films(product, pkg, scenes(3)["gpu"], W, H, spp)
    for k in FILMS:
        acc = torch.from_numpy(sums[k]).cuda()
        out = torch.empty_like(acc)
        product.aov_resolve_device(pkg.ffi.AOV_ALBEDO if k == "albedo" else pkg.ffi.AOV_SHADING_NORMAL, acc.data_ptr(), W * H, spp, out.data_ptr(), None)
        torch.cuda.synchronize()
        assert np.array_equal(host[k].view(np.uint32), out.cpu().numpy().view(np.uint32)), k
    assert np.array_equal(host["albedo"], product.render_aov(sc, cam, prm, pkg.ffi.AOV_ALBEDO, d65))
    two = product.render_gbuffer(sc, cam, prm, d65, films=("position", "hit"))
    assert sorted(two) == ["hit", "position"] and all(np.array_equal(two[k], host[k]) for k in two)


def test_gbuffer_errors_on_a_built_scene(product, pkg, scenes):
    """The refusals on a built scene leave the films untouched, and the next valid call succeeds."""
    f = pkg.ffi
    W, H, spp = 64, 48, 4
    sc, cam, d65 = scenes(0)["gpu"]
    cam = sized(cam, W, H, pkg)
    prm = pkg.make_params(spp, "mis", "sobol")
    slab = Slab(W, H, ())                                   # nothing wanted: every slot stays NaN
    p = [slab.buf[i].data_ptr() for i in range(4)]
    lib = product.lib

    def call(films, prm_=prm, lut=d65, b=0, e=spp, cam_=cam):
        return lib.mi355pt_render_gbuffer_accum_device(sc.h, ctypes.byref(cam_), ctypes.byref(prm_), lut, b, e, ctypes.byref(films), None, None)
    assert call(f.GbufferFilms(None, None, None, None)) == -1
    assert call(f.GbufferFilms(p[0], p[0], None, None)) == -1
    assert call(f.GbufferFilms(*p), lut=12345) == -1 and b"illuminant" in lib.mi355pt_last_error()
    assert call(f.GbufferFilms(*p), e=spp + 1) == -1 and call(f.GbufferFilms(*p), b=3, e=2) == -1
    assert call(f.GbufferFilms(*p), prm_=pkg.make_params(spp, "mis", "sobol", collect_stats=1)) == -1
    moved = f.Camera.from_buffer_copy(cam); moved.position[0] += 1.0
    assert call(f.GbufferFilms(*p), cam_=moved) == -1       # the camera position is baked into the build
    assert call(f.GbufferFilms(*p), b=2, e=2) == 0          # an empty range: nothing is launched
    slab.films()                                            # (asserts that all four slots are still NaN)
    got = gpu_films(product, pkg, scenes(0)["gpu"], W, H, spp, want=("position",))
    assert np.isfinite(got["position"]).all() and np.abs(got["position"]).max() > 0.1


@pytest.fixture(scope="module")
def cli(pkg, tmp_path_factory):
    root = pkg.ffi.ROOT
    exe = os.path.join(root, "toy-cpu-pathtracing_amd", "host", "mi355pt")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.dirname(exe)])
    assets_dir = str(tmp_path_factory.mktemp("assets"))
    subprocess.check_call([sys.executable, os.path.join(root, "tools", "export_assets.py"), assets_dir])
    return exe, dict(os.environ, MI355PT_ASSETS=assets_dir, MI355PT_DATA=os.path.join(root, "toy-cpu-pathtracing_amd", "data"))


def read_pfm(path):
    with open(path, "rb") as f:
        assert f.readline() == b"PF\n"
        w, h = (int(v) for v in f.readline().split())
        assert float(f.readline()) < 0.0                    # little endian
        data = np.frombuffer(f.read(), dtype="<f4")
    assert data.size == w * h * 3
    return data.reshape(h, w, 3)[::-1].copy()              # PFM rows run bottom to top


def test_gbuffer_cli_position_and_depth(product, pkg, cli, tmp_path):
    """The PFM `--renderer position` writes reads back bit-equal to the film the API gives — the position sums through
    mi355pt_gbuffer_normalize_device —, and `--renderer depth` is the normalised hit.x in all three channels."""
    import torch
    exe, env = cli
    W, H, spp = 96, 64, 8
    sc = product.new_scene()
    cam = pkg.scenes.load_scene(sc, 3, W, H, build=False)
    d65 = sc.add_lut470(pkg.scenes.presets()["cie_illum_d6500"])
    sc.build(cam)
    slab = Slab(W, H, ("position", "hit"))
    product.render_gbuffer_accum_device(sc, cam, pkg.make_params(spp, "mis", "sobol"), d65, 0, spp, slab.ptrs())
    out = torch.empty((2, H, W, 3), dtype=torch.float32, device="cuda")
    product.gbuffer_normalize_device(slab.ptrs()["position"], slab.ptrs()["hit"], W * H, out[0].data_ptr())
    product.gbuffer_normalize_device(slab.ptrs()["hit"], slab.ptrs()["hit"], W * H, out[1].data_ptr())
    torch.cuda.synchronize()
    want = out.cpu().numpy()
    base = [exe, "--scene", "3", "--sampler", "sobol", "--spp", str(spp), "--width", str(W), "--height", str(H)]
    for renderer in ("position", "depth"):
        path = str(tmp_path / f"{renderer}.pfm")
        r = subprocess.run(base + ["--renderer", renderer, "-o", path], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        assert "Finish rendering" in r.stdout
        got = read_pfm(path)
        ref_film = want[0] if renderer == "position" else np.repeat(want[1][..., :1], 3, axis=2)
        assert got.shape == ref_film.shape and np.array_equal(got.view(np.uint32), ref_film.view(np.uint32)), renderer
    assert np.abs(want[0]).max() > 0.5 and want[1][..., 0].max() > 1.0
    r = subprocess.run(base + ["--renderer", "depth", "-o", str(tmp_path / "x.png")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and ".pfm" in r.stderr


def test_gbuffer_cli_fused_guides(product, pkg, cli, tmp_path):
    """`--denoise-variance --fused-guides` equals its replay from the public entry points (the half film, the film, ONE G-buffer launch for
    the albedo and shading-normal films at the default 64 guide spp, mi355pt_denoise_var_device, the resolve with spp 1), pixel for pixel;
    `--fused-guides` without a denoise flag exits 2."""
    import torch
    from PIL import Image
    exe, env = cli
    W, H, spp, guide_spp = 64, 48, 16, 64
    sc = product.new_scene()
    cam = pkg.scenes.load_scene(sc, 3, W, H, build=False)
    d65 = sc.add_lut470(pkg.scenes.presets()["cie_illum_d6500"])
    sc.build(cam)
    prm = pkg.make_params(spp, "mis", "sobol")

    def dev():
        return torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    half, albedo, normal, out, rgb = dev(), dev(), dev(), dev(), dev()
    product.render_accum_device(sc, cam, prm, 0, spp // 2, half.data_ptr())
    torch.cuda.synchronize()
    film = half.clone()
    product.render_accum_device(sc, cam, prm, spp // 2, spp, film.data_ptr())
    product.render_gbuffer_accum_device(sc, cam, pkg.make_params(guide_spp, "mis", "sobol"), d65, 0, guide_spp,
                                        {"albedo": albedo.data_ptr(), "shading_normal": normal.data_ptr()})
    need = product.denoise_var_scratch_bytes(W, H)
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    product.denoise_var_device(film.data_ptr(), half.data_ptr(), spp, None, albedo.data_ptr(), guide_spp, normal.data_ptr(), guide_spp, W, H,
                               product.denoise_var_params_default(), scratch.data_ptr(), need, out.data_ptr())
    product.film_resolve_device(out.data_ptr(), W * H, 1, rgb.data_ptr())
    torch.cuda.synchronize()
    want = product.quantize_u8(rgb.cpu().numpy())
    base = [exe, "--scene", "3", "--renderer", "mis", "--sampler", "sobol", "--spp", str(spp), "--width", str(W), "--height", str(H), "--denoise-variance"]
    fused = str(tmp_path / "fused.png")
    r = subprocess.run(base + ["--fused-guides", "-o", fused], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = np.asarray(Image.open(fused).convert("RGB"))
    assert got.shape == want.shape and np.array_equal(got, want), int((got != want).sum())
    r = subprocess.run(base[:-1] + ["--fused-guides"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--fused-guides" in r.stderr
