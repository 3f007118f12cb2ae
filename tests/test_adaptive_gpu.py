"""GPU tests of adaptive sampling: path renders over an explicit tile list (mi355pt_render_accum_tiles_device, csrc/pt_kernels_tiles*.hip), the
noise step and the normalisation (csrc/pt_kernels_adaptive.hip) against the NumPy restatement of tests/adaptive_reference.py, and the driver
against a replay of its normative sequence from the public pieces.

Frame: 44 x 20 = 6 x 3 tiles, the last column 4 pixels wide and the last row 4 tall; maximum 64 spp, minimum 4.
Bars.  A list of ALL tiles, the replay and two runs of anything: bit-equal.  Another summation order of the same samples (a shorter list splits
the sample range differently; a range in pieces): the project's own bar for that, rtol 2e-4, atol 1e-4 * samples * 0.01
(tests/test_parity_gpu.py's accumulation test).  tile_err: the denoiser tests' measure max |x - ref64| / (|ref64| + 1e-3) with the GPU allowed
8 x what the float32 restatement shows on the same case, 2^-22 where that is 0."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adaptive_reference as ar  # noqa: E402

pytestmark = pytest.mark.gpu

W, H, MAX_SPP, MIN_SPP = 44, 20, 64, 4
TX, TY = 6, 3
NT = TX * TY
CASES = [(3, "mis", "sobol"), (17, "nee", "sobol"), (8, "pt", "sobol"), (3, "mis", "random")]   # deferral class, clearcoat units, MODE_PT, generic mode
CASE_IDS = [f"scene{s}-{st}-{sa}" for s, st, sa in CASES]
# with CASES, every (mode, feature-set class) pair once: the units CASES leaves out (MIS clearcoat, plain NEE, generic and pt clearcoat)
ALL_UNITS = CASES + [(17, "mis", "sobol"), (3, "nee", "sobol"), (17, "pt", "sobol"), (17, "mis", "random")]
ALL_UNIT_IDS = [f"scene{s}-{st}-{sa}" for s, st, sa in ALL_UNITS]
SPARSE = [2, 5, 11, 17]                     # 5 and 11 in the narrow right-hand column, 17 the bottom-right corner
DARK_EPS = 1e-3
FACTOR, FLOOR = 8.0, 2.0 ** -22


def log_line(text):
    print(text)
    if os.environ.get("MI355PT_FRAME_LOG"):
        with open(os.environ["MI355PT_FRAME_LOG"], "a") as f:
            f.write(text + "\n")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def order_bar(got, want, samples):
    np.testing.assert_allclose(got, want, rtol=2e-4, atol=1e-4 * samples * 0.01)


def tile_mask(tiles):
    m = np.zeros((TY, TX), bool)
    m.reshape(-1)[list(tiles)] = True
    return np.repeat(np.repeat(m, 8, 0), 8, 1)[:H, :W]


def err_bar(gpu_err, film, half, tile_spp, tag, which=None):
    """tile_err of the tiles `which` (default: all) against the float64 restatement on the same films and counts"""
    ref64 = ar.tile_errors(film, half, tile_spp, DARK_EPS, np.float64)
    ref32 = ar.tile_errors(film, half, tile_spp, DARK_EPS, np.float32)
    sel = np.ones(ref64.size, bool) if which is None else which
    e32 = ar.rel_err(ref32[sel], ref64[sel])
    egpu = ar.rel_err(np.asarray(gpu_err)[sel], ref64[sel])
    bar = FACTOR * e32 if e32 > 0 else FLOOR
    log_line(f'{{"test": "{tag}", "tiles": {int(sel.sum())}, "e32": {e32:.3e}, "gpu": {egpu:.3e}, "bar": {bar:.3e}}}')
    assert egpu <= bar, (tag, egpu, e32)


class Rig:
    """one scene on the device with its parameters, whole-frame films of [0, n) rendered once and shared, and the frame's adaptive state"""

    def __init__(self, product, pkg, case):
        import torch
        self.torch, self.product, self.pkg = torch, product, pkg
        scene_id, strategy, sampler = case
        self.sc = product.new_scene()
        self.cam = pkg.scenes.load_scene(self.sc, scene_id, W, H, tex_size=64)
        self.strategy, self.sampler = strategy, sampler
        self.prm = pkg.make_params(MAX_SPP, strategy, sampler)
        self._whole = {}

    def params(self, **kw):
        return self.pkg.make_params(MAX_SPP, self.strategy, self.sampler, **kw)

    def zeros(self):
        return self.torch.zeros((H, W, 3), dtype=self.torch.float32, device="cuda")

    def accum(self, film, b, e):
        self.product.render_accum_device(self.sc, self.cam, self.prm, b, e, film.data_ptr(), None)

    def whole(self, n):
        """the whole-frame film of [0, n) in one call of mi355pt_render_accum_device (host array, read-only)"""
        if n not in self._whole:
            f = self.zeros()
            self.accum(f, 0, n)
            self.torch.cuda.synchronize()
            a = f.cpu().numpy()
            a.setflags(write=False)
            self._whole[n] = a
        return self._whole[n]

    def tiles(self, film, tiles, b, e, prm=None):
        self.product.render_accum_tiles_device(self.sc, self.cam, prm or self.prm, tiles, b, e, film.data_ptr(), None)

    def state(self):
        t = self.torch
        return dict(film=self.zeros(), half=self.zeros(), spp=t.zeros(NT, dtype=t.int32, device="cuda"), err=t.zeros(NT, dtype=t.float32, device="cuda"),
                    lst=t.zeros(NT, dtype=t.int32, device="cuda"), cnt=t.zeros(1, dtype=t.int32, device="cuda"),
                    scratch=t.zeros(self.product.adaptive_scratch_bytes(W, H), dtype=t.uint8, device="cuda"))

    def step(self, st, ap, level, max_spp=MAX_SPP):
        """mi355pt_adaptive_step_device on the state -> the list, downloaded"""
        self.product.adaptive_step_device(st["film"].data_ptr(), st["half"].data_ptr(), W, H, st["spp"].data_ptr(), st["err"].data_ptr(), ap, level,
                                          max_spp, st["scratch"].data_ptr(), st["scratch"].numel(), st["lst"].data_ptr(), st["cnt"].data_ptr(), None)
        self.torch.cuda.synchronize()
        n = int(st["cnt"].cpu().numpy()[0])
        assert 0 <= n <= NT
        return st["lst"].cpu().numpy()[:n].astype(np.uint32)

    def driver(self, ap, prm=None):
        st = self.state()
        res = self.product.render_adaptive_device(self.sc, self.cam, prm or self.prm, ap, st["film"].data_ptr(), st["half"].data_ptr(), st["spp"].data_ptr(),
                                                  st["err"].data_ptr(), st["lst"].data_ptr(), st["scratch"].data_ptr(), st["scratch"].numel(), None)
        self.torch.cuda.synchronize()
        return host_state(st), res

    def replay(self, ap, prm=None):
        """the driver's normative sequence from the public pieces, the list going through the host"""
        prm = prm or self.prm
        lo, hi = ap.min_spp, prm.spp
        st = self.state()
        st["spp"].fill_(lo)
        self.product.render_accum_device(self.sc, self.cam, prm, 0, lo // 2, st["half"].data_ptr(), None)
        st["film"].copy_(st["half"])
        self.product.render_accum_device(self.sc, self.cam, prm, lo // 2, lo, st["film"].data_ptr(), None)
        level, passes = lo, 0
        while level <= hi:
            lst = self.step(st, ap, level, hi)
            passes += 1
            if lst.size == 0:
                break
            self.tiles(st["film"], lst, level, 2 * level, prm)
            level *= 2
        self.torch.cuda.synchronize()
        return host_state(st), passes


def host_state(st):
    return dict(film=st["film"].cpu().numpy(), half=st["half"].cpu().numpy(), spp=st["spp"].cpu().numpy().view(np.uint32),
                err=st["err"].cpu().numpy())


@pytest.fixture(scope="module")
def rigs(product, pkg):
    cache = {}

    def get(case):
        if case not in cache:
            cache[case] = Rig(product, pkg, case)
        return cache[case]
    return get


def adaptive_params(pkg, threshold, min_spp=MIN_SPP):
    return pkg.ffi.AdaptiveParams(threshold, DARK_EPS, min_spp)


# ---------------------------------------------------------------- 1, 2: tile lists
@pytest.mark.parametrize("case", ALL_UNITS, ids=ALL_UNIT_IDS)
def test_list_of_all_tiles_is_bit_equal_to_the_plain_render(rigs, case):
    """Every translation unit's kernels launched once through the plain lookup and once through the tile-list lookup (pt_kernels.hip
    find_pt_kernel): an empty or crossed slot of that table shows here."""
    r = rigs(case)
    f = r.zeros()
    r.tiles(f, np.arange(NT), 0, 16)
    r.torch.cuda.synchronize()
    ref = r.whole(16)
    assert ref.mean() > 0.01 * 16 * 0.1
    assert np.array_equal(bits(f.cpu().numpy()), bits(ref))


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_sparse_list(rigs, case):
    """Tiles [2, 5, 11, 17] onto a film pre-filled with a pattern (multiples of 1 / 64 in [3 / 64, 1): exact in binary32, small against the
    sums): outside the listed tiles the pattern bit for bit; inside, film - pattern is the whole-frame film up to summation order; two runs
    bit-equal; [0, 8) then [8, 16) likewise; and every refused call leaves the film alone."""
    r = rigs(case)
    torch = r.torch
    pattern = (((np.arange(H * W * 3) % 61) + 3) / 64.0).astype(np.float32).reshape(H, W, 3)
    inside = tile_mask(SPARSE)
    assert inside.sum() == 64 + 32 + 32 + 16
    ref = r.whole(16)

    def run(ranges):
        f = torch.from_numpy(pattern.copy()).cuda()
        for b, e in ranges:
            r.tiles(f, SPARSE, b, e)
        torch.cuda.synchronize()
        return f.cpu().numpy()
    one, two, pieces = run([(0, 16)]), run([(0, 16)]), run([(0, 8), (8, 16)])
    assert np.array_equal(bits(one[~inside]), bits(pattern[~inside]))
    assert np.array_equal(bits(pieces[~inside]), bits(pattern[~inside]))
    assert np.array_equal(bits(one), bits(two))
    order_bar((one - pattern)[inside], ref[inside], 16)
    order_bar((pieces - pattern)[inside], ref[inside], 16)
    assert ref[inside].mean() > 0.01 * 16 * 0.1
    # refused before anything touches the device: the film stays the pattern
    f = torch.from_numpy(pattern.copy()).cuda()
    lib = r.product.lib

    def call(tiles, prm):
        t = np.ascontiguousarray(tiles, np.uint32)
        return lib.mi355pt_render_accum_tiles_device(r.sc.h, ctypes.byref(r.cam), ctypes.byref(prm), t.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                                     t.size, 0, 16, ctypes.c_void_p(f.data_ptr()), None, None)
    bad = {"descending": ([5, 2], r.prm), "repeated": ([2, 5, 5, 11], r.prm), "index = tile count": ([2, NT], r.prm),
           "shard_count 2": (SPARSE, r.params(shard_index=0, shard_count=2)), "collect_stats 1": (SPARSE, r.params(collect_stats=1))}
    for name, (tiles, prm) in bad.items():
        assert call(tiles, prm) == -1, name
        assert len(lib.mi355pt_last_error()) > 0, name
    torch.cuda.synchronize()
    assert np.array_equal(bits(f.cpu().numpy()), bits(pattern))


# ---------------------------------------------------------------- 3: the step on synthetic films
@pytest.mark.parametrize("shape", [(1, 1), (9, 7), (44, 20), (130, 70)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_step_on_synthetic_films(product, pkg, shape):
    """Host-built films with mixed tile_spp, HDR values to about 100, negative channels and one NaN pixel, every tile's error at most half the
    threshold or at least twice it (tests/test_adaptive.py checks the construction): tile_err to the bar, the list = np.nonzero(active)
    ascending with its count, tile_spp doubled exactly on active tiles, H := F bit for bit on their in-frame pixels and untouched elsewhere, F
    untouched, tiles at other counts untouched in every buffer; two runs bit-equal."""
    import torch
    w, h = shape
    thr, level = 0.05, 8
    film, half, spp, err0 = ar.synthetic(w, h, level, thr, DARK_EPS)
    nt = spp.size
    ap = pkg.ffi.AdaptiveParams(thr, DARK_EPS, MIN_SPP)
    need = product.adaptive_scratch_bytes(w, h)

    def run():
        d = dict(film=torch.from_numpy(film).cuda(), half=torch.from_numpy(half).cuda(), spp=torch.from_numpy(spp.view(np.int32)).cuda(),
                 err=torch.from_numpy(err0).cuda(), lst=torch.full((nt,), -1, dtype=torch.int32, device="cuda"),
                 cnt=torch.full((1,), -1, dtype=torch.int32, device="cuda"), scratch=torch.zeros(need, dtype=torch.uint8, device="cuda"))
        product.adaptive_step_device(d["film"].data_ptr(), d["half"].data_ptr(), w, h, d["spp"].data_ptr(), d["err"].data_ptr(), ap, level, MAX_SPP,
                                     d["scratch"].data_ptr(), need, d["lst"].data_ptr(), d["cnt"].data_ptr(), None)
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in d.items() if k != "scratch"}
    got, again = run(), run()
    for k in got:
        assert np.array_equal(bits(got[k]), bits(again[k])), k
    half_ref, spp_ref, err_ref, list_ref, active = ar.step(film, half, spp, err0, thr, DARK_EPS, level, MAX_SPP, np.float64)
    at_level = spp == level
    if nt >= NT:                                             # (the two larger frames: every kind of tile occurs)
        assert active.any() and (at_level & ~active).any() and (~at_level).any()
    err_bar(got["err"], film, half, np.where(at_level, spp, 2), f"step_synthetic_{w}x{h}", which=at_level)
    assert np.array_equal(bits(got["err"][~at_level]), bits(err0[~at_level]))                        # other counts: the start value, untouched
    n = int(got["cnt"][0])
    assert n == list_ref.size and np.array_equal(got["lst"][:n].view(np.uint32), list_ref)
    assert np.array_equal(got["lst"][n:], np.full(nt - n, -1, np.int32))                              # nothing written past the count
    assert np.array_equal(got["spp"].view(np.uint32), spp_ref)
    assert np.array_equal(got["film"].view(np.uint32), film.view(np.uint32))
    assert np.array_equal(got["half"].view(np.uint32), half_ref.view(np.uint32))


# ---------------------------------------------------------------- 4: normalise
def test_normalize_tiles(product):
    import torch
    rng = np.random.default_rng(5)
    film = rng.uniform(0.0, 300.0, (H, W, 3)).astype(np.float32)
    film[3, 7] = (0.0, -2.5, 1e-20)

    def resolve(f, spp):
        out = torch.empty_like(f)
        product.film_resolve_device(f.data_ptr(), H * W, spp, out.data_ptr(), None)
        torch.cuda.synchronize()
        return out.cpu().numpy()

    def normalise(spp):
        f = torch.from_numpy(film).cuda()
        mean = torch.full((H, W, 3), float("nan"), dtype=torch.float32, device="cuda")
        product.film_normalize_tiles_device(f.data_ptr(), torch.from_numpy(spp.view(np.int32)).cuda().data_ptr(), W, H, mean.data_ptr(), None)
        torch.cuda.synchronize()
        return mean
    for n in (1, 4, 48, 64):
        mean = normalise(np.full(NT, n, np.uint32))
        assert np.array_equal(bits(resolve(mean, 1)), bits(resolve(torch.from_numpy(film).cuda(), n))), n
    mixed = (MIN_SPP << rng.integers(0, 5, NT)).astype(np.uint32)
    assert len(set(mixed.tolist())) > 2
    assert np.array_equal(bits(normalise(mixed).cpu().numpy()), bits(ar.normalize(film, mixed)))


# ---------------------------------------------------------------- 5: the driver
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_driver_with_min_equal_to_max(rigs, pkg, case):
    """min_spp == spp: the film is [0, max / 2) copied plus [max / 2, max) through mi355pt_render_accum_device, bit for bit; every count is
    max; one step ran (it activates nothing and leaves the errors)."""
    r = rigs(case)
    ap = adaptive_params(pkg, 1e-6, min_spp=MAX_SPP)
    st, res = r.driver(ap)
    half = r.zeros()
    r.accum(half, 0, MAX_SPP // 2)
    film = half.clone()
    r.accum(film, MAX_SPP // 2, MAX_SPP)
    r.torch.cuda.synchronize()
    assert np.array_equal(bits(st["film"]), bits(film.cpu().numpy())) and np.array_equal(bits(st["half"]), bits(half.cpu().numpy()))
    assert np.array_equal(st["spp"], np.full(NT, MAX_SPP, np.uint32))
    assert (res.passes, res.tiles_at_max, res.total_samples) == (1, NT, MAX_SPP * W * H)
    err_bar(st["err"], st["film"], st["half"], st["spp"], f"driver_min_eq_max_{case[0]}_{case[1]}_{case[2]}")


@pytest.fixture(scope="module")
def measured_threshold(rigs, pkg):
    """the median of tile_err after a first step at min_spp, measured on the frame itself (a threshold nothing exceeds: the step then only
    writes the errors)"""
    cache = {}

    def get(case):
        if case not in cache:
            r = rigs(case)
            st = r.state()
            st["spp"].fill_(MIN_SPP)
            r.accum(st["half"], 0, MIN_SPP // 2)
            st["film"].copy_(st["half"])
            r.accum(st["film"], MIN_SPP // 2, MIN_SPP)
            assert r.step(st, adaptive_params(pkg, 3e38), MIN_SPP).size == 0
            err = st["err"].cpu().numpy()
            assert np.isfinite(err).all()
            cache[case] = float(np.median(err))
            assert cache[case] > 0
        return cache[case]
    return get


@pytest.fixture(scope="module")
def replayed(rigs, pkg, measured_threshold):
    cache = {}

    def get(case):
        if case not in cache:
            cache[case] = rigs(case).replay(adaptive_params(pkg, measured_threshold(case)))
        return cache[case]
    return get


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_driver_at_a_measured_threshold(rigs, pkg, measured_threshold, case):
    r = rigs(case)
    thr = measured_threshold(case)
    st, res = r.driver(adaptive_params(pkg, thr))
    spp, err = st["spp"], st["err"]
    counts = sorted(set(spp.tolist()))
    log_line(f'{{"test": "driver_counts", "case": "{case[0]}_{case[1]}_{case[2]}", "threshold": {thr:.4e}, "passes": {res.passes}, '
             f'"counts": {dict((n, int((spp == n).sum())) for n in counts)}}}')
    assert len(counts) > 1                                                                 # non-uniform
    assert all(n in (4, 8, 16, 32, 64) for n in counts)
    assert np.all(err[spp < MAX_SPP] <= np.float32(thr))
    in_frame = ar.in_frame(W, H).sum(1)
    assert res.total_samples == int((spp.astype(np.int64) * in_frame).sum()) and res.tiles_at_max == int((spp == MAX_SPP).sum())
    assert res.passes == (max(counts) // MIN_SPP).bit_length()          # steps at min, 2 min, .. , the largest count (which finds nothing active)
    err_bar(err, st["film"], st["half"], spp, f"driver_threshold_{case[0]}_{case[1]}_{case[2]}")
    for n in counts:
        m = tile_mask(np.nonzero(spp == n)[0])
        order_bar(st["film"][m], r.whole(n)[m], n)
        order_bar(st["half"][m], r.whole(n // 2)[m], n // 2)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_driver_equals_its_replay_from_the_public_pieces(rigs, pkg, measured_threshold, replayed, case):
    st, res = rigs(case).driver(adaptive_params(pkg, measured_threshold(case)))
    rp, passes = replayed(case)
    for k in ("film", "half", "spp", "err"):
        assert np.array_equal(bits(st[k]), bits(rp[k])), k
    assert res.passes == passes


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_host_entry_is_resolve_of_normalise_of_the_replay(rigs, pkg, measured_threshold, replayed, case):
    r = rigs(case)
    torch = r.torch
    img, spp, res = r.product.render_adaptive(r.sc, r.cam, r.prm, adaptive_params(pkg, measured_threshold(case)))
    rp, passes = replayed(case)
    assert np.array_equal(spp.reshape(-1), rp["spp"]) and res.passes == passes
    film = torch.from_numpy(rp["film"]).cuda()
    mean, out = torch.empty_like(film), torch.empty_like(film)
    r.product.film_normalize_tiles_device(film.data_ptr(), torch.from_numpy(rp["spp"].view(np.int32)).cuda().data_ptr(), W, H, mean.data_ptr(), None)
    r.product.film_resolve_device(mean.data_ptr(), H * W, 1, out.data_ptr(), None)
    torch.cuda.synchronize()
    assert np.array_equal(bits(img), bits(out.cpu().numpy()))
    assert np.isfinite(img).all() and img.min() >= 0.0 and img.max() <= 1.0


def test_adaptive_cli(pkg, tmp_path):
    """mi355pt --adaptive-threshold exits 0 and writes the frame and the spp map; it composes with --denoise; with an AOV renderer or
    --gpus 2 it exits 2."""
    import subprocess
    root = pkg.ffi.ROOT
    exe = os.path.join(root, "toy-cpu-pathtracing_amd", "host", "mi355pt")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.dirname(exe)])
    assets_dir = str(tmp_path / "assets")
    subprocess.check_call([sys.executable, os.path.join(root, "tools", "export_assets.py"), assets_dir])
    env = dict(os.environ, MI355PT_ASSETS=assets_dir, MI355PT_DATA=os.path.join(root, "toy-cpu-pathtracing_amd", "data"))
    base = [exe, "--scene", "3", "--renderer", "mis", "--sampler", "sobol", "--spp", "32", "--width", "64", "--height", "48", "--adaptive-min-spp", "4"]
    out, spp_map, den = str(tmp_path / "a.png"), str(tmp_path / "spp.png"), str(tmp_path / "d.png")
    r = subprocess.run(base + ["--adaptive-threshold", "0.05", "--spp-map", spp_map, "-o", out], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "Finish rendering" in r.stdout and "adaptive:" in r.stdout
    assert len(open(out, "rb").read()) > 100 and len(open(spp_map, "rb").read()) > 100
    r = subprocess.run(base + ["--adaptive-threshold", "0.05", "--denoise", "-o", den], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert open(den, "rb").read() != open(out, "rb").read()
    r = subprocess.run([exe, "--scene", "3", "--renderer", "albedo", "--adaptive-threshold", "0.05"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--adaptive-threshold" in r.stderr
    r = subprocess.run(base + ["--adaptive-threshold", "0.05", "--gpus", "2"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "one GPU" in r.stderr
