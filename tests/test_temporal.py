"""The temporal reprojection (include/mi355pt_temporal.h), the part that needs no GPU: the ABI surface of the cross-compiled library, the view
of a camera pair against a NumPy double computation, the refusals that happen before anything touches the device, the properties of the
NumPy restatement (tests/temporal_reference.py) that the GPU tests lean on, the reprojection geometry on G-buffers rendered by the CPU
restatement of the G-buffer pass, and the CLI's argument errors."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gbuffer_reference  # noqa: E402
import temporal_reference as tr  # noqa: E402

NEW_SYMBOLS = ["mi355pt_temporal_params_default", "mi355pt_temporal_view_from_cameras", "mi355pt_temporal_accumulate_device", "mi355pt_temporal_accumulate"]
E_INVALID = -1
DTYPES = [np.float32, np.float64]


def log_line(text):
    print(text)
    if os.environ.get("MI355PT_FRAME_LOG"):
        with open(os.environ["MI355PT_FRAME_LOG"], "a") as f:
            f.write(text + "\n")


def ffi_camera(pkg, c):
    return pkg.make_camera(c.position, c.direction, c.up, c.width, c.height, c.fov_deg)


def scene3_camera(pkg, W=64, H=48):
    """scene 3's camera, from a scene that is described but never built (no device)"""
    return pkg.scenes.load_scene(pkg.Product().new_scene(), 3, W, H, tex_size=16, build=False)


def moved(pkg, cam, move=(0.3, 0.1, -0.2), yaw=0.05, scale=1.0):
    c = pkg.ffi.Camera.from_buffer_copy(cam)
    d = tr.yawed(tuple(cam.direction), yaw)
    for i in range(3):
        c.position[i] += move[i]
        c.direction[i] = d[i] * scale
    return c


def test_temporal_abi_surface(pkg):
    """The header declares the four entry points and the three structs, mi355pt.h includes it ahead of the variance-guided denoiser's and
    declares nothing itself, the library exports the symbols, the ctypes mirror and the generated Rust binding name them."""
    lib = ctypes.CDLL(pkg.ffi.LIB_PATH)
    root = pkg.ffi.ROOT
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "mi355pt_temporal.h")).read(), flags=re.S)
    main = open(os.path.join(root, "include", "mi355pt.h")).read()
    rs = open(os.path.join(root, "bindings", "rust", "mi355pt_sys.rs")).read()
    assert 0 < main.index('#include "mi355pt_temporal.h"') < main.index('#include "mi355pt_denoise_var.h"')
    declared = sorted(set(re.findall(r"\b(mi355pt_[a-z0-9_]+)\s*\(", code)))
    assert declared == sorted(NEW_SYMBOLS)
    assert sorted("mi355pt_" + s for s in pkg.ffi.TEMPORAL_SYMBOLS) == declared
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(r"pub fn %s\(" % name, rs), name
    for struct in ("mi355pt_temporal_view", "mi355pt_temporal_params", "mi355pt_temporal_frame"):
        assert re.search(r"typedef struct %s \{.*?\} %s;" % (struct, struct), code, flags=re.S), struct
    assert re.search(r"pub struct TemporalFrame \{\s*pub film: \*const f32,\s*pub half: \*const f32,\s*pub length: \*const f32,\s*pub position: \*const f32,"
                     r"\s*pub shading_normal: \*const f32,\s*pub hit: \*const f32,\s*\}", rs)
    assert re.search(r"pub struct TemporalView \{\s*pub delta: \[f32; 3\],\s*pub rows: \[f32; 9\],\s*pub sx: f32,\s*pub sy: f32,\s*pub cx: f32,\s*pub cy: f32,\s*\}", rs)
    assert ctypes.sizeof(pkg.ffi.TemporalView) == 16 * 4 and ctypes.sizeof(pkg.ffi.TemporalParams) == 16
    assert ctypes.sizeof(pkg.ffi.TemporalFrame) == 6 * ctypes.sizeof(ctypes.c_void_p)
    assert subprocess.call([sys.executable, os.path.join(root, "tools", "gen_rust_binding.py"), "--check"]) == 0
    p = pkg.Product().temporal_params_default()
    assert (p.pos_tol, p.normal_cos, p.min_weight, p.max_history) == tuple(np.float32(v) for v in (0.01, 0.9, 0.01, 32.0))
    assert {k: float(np.float32(v)) for k, v in tr.DEFAULTS.items()} == {k: getattr(p, k) for k in tr.DEFAULTS}


def test_temporal_view_matches_double_computation(pkg):
    """mi355pt_temporal_view_from_cameras against the NumPy double computation rounded to f32, on scene 3's camera, the same camera moved
    by (0.3, 0.1, -0.2) and yawed 0.05 rad, and a non-unit direction: every entry within 1 f32 ulp (both sides are double evaluations of
    the same well-conditioned expressions: they differ only where a rounding tie is straddled)."""
    prod = pkg.Product()
    base = scene3_camera(pkg)
    cams = {"base": base, "moved": moved(pkg, base), "nonunit": moved(pkg, base, scale=3.7)}
    cams["nonunit"].up[1] = 2.5
    worst = 0.0
    for a, b in (("moved", "base"), ("base", "moved"), ("nonunit", "base"), ("base", "nonunit"), ("base", "base"), ("moved", "nonunit")):
        got, want = tr.view_entries(prod.temporal_view_from_cameras(cams[a], cams[b])), tr.view_entries(tr.view_from_cameras(cams[a], cams[b]))
        ulps = np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.maximum(np.abs(got), np.abs(want)))
        worst = max(worst, float(ulps.max()))
        assert ulps.max() <= 1.0, (a, b, got, want)
    log_line(f'{{"test": "temporal_view_ulps", "worst_ulp": {worst:.2f}}}')
    # the rows are those of a rotation, and a non-unit direction gives the unit one's view
    v = tr.view_entries(prod.temporal_view_from_cameras(cams["base"], cams["nonunit"]))
    r = v[3:12].reshape(3, 3).astype(np.float64)
    assert np.abs(r @ r.T - np.eye(3)).max() < 1e-6


def test_temporal_view_refusals(pkg):
    prod = pkg.Product()
    lib, f = prod.lib, pkg.ffi
    base = scene3_camera(pkg)
    out = f.TemporalView()

    def call(cur, prev, o=out):
        rc = lib.mi355pt_temporal_view_from_cameras(ctypes.byref(cur) if cur is not None else None, ctypes.byref(prev) if prev is not None else None,
                                                    ctypes.byref(o) if o is not None else None)
        return rc, lib.mi355pt_last_error()

    def variant(**kw):
        c = f.Camera.from_buffer_copy(base)
        for k, v in kw.items():
            if isinstance(v, tuple):
                for i in range(3):
                    getattr(c, k)[i] = v[i]
            else:
                setattr(c, k, v)
        return c
    assert call(base, base)[0] == 0
    bad = [(None, base, out), (base, None, out), (base, base, None), (variant(width=32), base, out), (base, variant(height=24), out),
           (variant(width=0), variant(width=0), out), (variant(height=0), variant(height=0), out), (variant(fov_deg=60.0), base, out),
           (base, variant(direction=(0.0, 0.0, 0.0)), out), (base, variant(up=(0.0, 0.0, 0.0)), out),
           (base, variant(direction=(0.0, 2.0, 0.0), up=(0.0, 1.0, 0.0)), out), (base, variant(direction=(0.0, -1.0, 0.0), up=(0.0, 3.0, 0.0)), out)]
    for cur, prev, o in bad:
        rc, msg = call(cur, prev, o)
        assert rc == E_INVALID and b"temporal" in msg, msg


def test_temporal_view_round_trip(pkg):
    """64 x 48: for each pixel centre of the previous camera the ray of camera.rs:51-65 in double, a point at t = 5 on it, pushed through
    the f32 view, comes back as (i + 0.5, j + 0.5) within 1e-3 pixel (f32 rounding gives about 64 * 2^-23 times a small factor)."""
    prod = pkg.Product()
    base = scene3_camera(pkg)
    for cur, prev in ((moved(pkg, base), base), (base, moved(pkg, base)), (base, base)):
        view = prod.temporal_view_from_cameras(cur, prev)
        P = tr.pixel_rays(prev) * 5.0 + np.array(list(prev.position), np.float64)            # world
        X = (P - np.array(list(cur.position), np.float64)).astype(np.float32)                  # the current frame's render space
        for dt in DTYPES:
            fx, fy, zc = tr.project(view, X, dt)
            ii, jj = np.meshgrid(np.arange(64) + 0.5, np.arange(48) + 0.5)
            err = max(np.abs(fx - ii).max(), np.abs(fy - jj).max())
            assert (zc > 0).all() and err <= 1e-3, (dt, err)


def _frames(W=8, H=4, half=True):
    cur, prev, view, spp = tr.synthetic(W, H, "static", "step", half, bad=False)
    return cur, prev, view, spp


def test_temporal_refusals_before_the_device(pkg):
    """Every refusal the header lists returns MI355PT_E_INVALID with a message that names "temporal", from both entry points, with no
    device present (a call that got past the checks would answer MI355PT_E_DEVICE), and the outputs stay untouched."""
    f = pkg.ffi
    prod = pkg.Product()
    lib = prod.lib
    W, H = 8, 4
    cur, prev, view, spp = _frames(W, H)
    cview = f.TemporalView((ctypes.c_float * 3)(*view.delta), (ctypes.c_float * 9)(*view.rows), view.sx, view.sy, view.cx, view.cy)
    outs = [np.full((H, W, 3), 7.0, np.float32), np.full((H, W, 3), 7.0, np.float32), np.full((H, W), 7.0, np.float32)]
    o = [a.ctypes.data for a in outs]

    def frame(d, **kw):
        q = {k: (d[k].ctypes.data if d.get(k) is not None else None) for k in f.TEMPORAL_FILMS}
        q.update(kw)
        return f.TemporalFrame(*[q[k] for k in f.TEMPORAL_FILMS])
    good = prod.temporal_params_default()

    def both(fc, s, fp, v, w, h, p, of, oh, ol):
        ref = lambda x: ctypes.byref(x) if x is not None else None   # noqa: E731
        args = (ref(fc), s, ref(fp), ref(v), w, h, ref(p), of, oh, ol)
        for rc in (lib.mi355pt_temporal_accumulate_device(*args, None), lib.mi355pt_temporal_accumulate(*args)):
            assert rc == E_INVALID and b"temporal" in lib.mi355pt_last_error(), (rc, lib.mi355pt_last_error())
    fc, fp = frame(cur), frame(prev)
    # required pointers
    both(None, spp, fp, cview, W, H, good, *o)
    both(fc, spp, fp, cview, W, H, None, *o)
    both(fc, spp, fp, cview, W, H, good, None, o[1], o[2])
    both(fc, spp, fp, cview, W, H, good, o[0], o[1], None)
    for k in ("film", "position", "shading_normal", "hit"):
        both(frame(cur, **{k: None}), spp, fp, cview, W, H, good, *o)
        both(fc, spp, frame(prev, **{k: None}), cview, W, H, good, *o)
    both(fc, spp, frame(prev, length=None), cview, W, H, good, *o)
    # prev and view: both or neither
    both(fc, spp, None, cview, W, H, good, *o)
    both(fc, spp, fp, None, W, H, good, *o)
    # the half pointers: all or none
    both(frame(cur, half=None), spp, fp, cview, W, H, good, *o)
    both(fc, spp, frame(prev, half=None), cview, W, H, good, *o)
    both(fc, spp, fp, cview, W, H, good, o[0], None, o[2])
    both(frame(cur, half=None), spp, frame(prev, half=None), cview, W, H, good, *o)
    both(frame(cur, half=None), spp, None, None, W, H, good, *o)
    # spp, the frame
    both(fc, 0, fp, cview, W, H, good, *o)
    both(fc, 3, fp, cview, W, H, good, *o)
    both(frame(cur, half=None), 0, frame(prev, half=None), cview, W, H, good, o[0], None, o[2])
    both(fc, spp, fp, cview, 0, H, good, *o)
    both(fc, spp, fp, cview, W, 0, good, *o)
    # the parameters: a zero-initialised struct, then each field
    both(fc, spp, fp, cview, W, H, f.TemporalParams(), *o)
    for k, values in (("pos_tol", (0.0, -1.0, np.inf, np.nan)), ("min_weight", (0.0, -0.5, np.inf, np.nan)), ("max_history", (0.0, 0.5, -2.0, np.inf, np.nan)),
                      ("normal_cos", (1.5, -1.5, np.nan, np.inf))):
        for v in values:
            p = prod.temporal_params_default(); setattr(p, k, v)
            both(fc, spp, fp, cview, W, H, p, *o)
    # aliasing: an output equal to an input or to another output
    for k in ("film", "half", "position", "shading_normal", "hit"):
        for i in range(3):
            q = list(o); q[i] = cur[k].ctypes.data
            both(fc, spp, fp, cview, W, H, good, *q)
    for k in ("film", "half", "length", "position", "shading_normal", "hit"):
        for i in range(3):
            q = list(o); q[i] = prev[k].ctypes.data
            both(fc, spp, fp, cview, W, H, good, *q)
    both(fc, spp, fp, cview, W, H, good, o[0], o[0], o[2])
    both(fc, spp, fp, cview, W, H, good, o[0], o[1], o[0])
    both(fc, spp, fp, cview, W, H, good, o[0], o[1], o[1])
    assert all((a == 7.0).all() for a in outs)


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_restatement_first_frame(dt):
    """Without a previous frame: out = c, length 1; with a half film out_half = c1 and out_film = c1 + c2; bad film values come out as 0."""
    cur, _, _, spp = tr.synthetic(67, 35, "static", "step", True)
    film, half, L, info = tr.accumulate(cur, spp, dtype=dt, detail=True)
    c1, c2 = info["c"]
    assert np.array_equal(half, c1) and np.array_equal(film, c1 + c2) and np.array_equal(L, np.ones((35, 67), dt))
    assert np.isfinite(film).all() and (film >= 0).all() and film.dtype == dt and L.dtype == dt
    B, Hf = np.asarray(cur["film"], dt), np.asarray(cur["half"], dt)
    with np.errstate(all="ignore"):
        fine = np.isfinite(B) & np.isfinite(Hf) & (Hf > 0) & (B - Hf > 0)
        assert np.array_equal(c1[fine], (Hf / dt(spp // 2))[fine]) and np.array_equal(c2[fine], ((B - Hf) / dt(spp // 2))[fine])
    assert (c1[~np.isfinite(Hf) | (Hf < 0)] == 0).all() and (~fine).sum() > 0
    one = dict(cur, half=None)
    film1, half1, L1, info1 = tr.accumulate(one, spp, dtype=dt, detail=True)
    assert half1 is None and np.array_equal(film1, info1["c"][0]) and np.array_equal(L1, np.ones((35, 67), dt))


@pytest.mark.parametrize("half", [True, False], ids=["half", "nohalf"])
@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_restatement_static_plane_is_a_running_mean(dt, half):
    """A static view on the plane of the exact pixel grid: the length runs 1, 2, 3, ... and stops at max_history; after k frames the output
    equals the arithmetic mean of the k cleaned frames within k * 2^-23 relative.  (The frames are positive with values in [0.5, 1.5]: a
    step m + (c - m) / k then adds at most 2^-24 (|m'| + 3 |c - m| / k) <= 2^-24 |m'| (1 + 3 / k) to an error that it scales by
    (k - 1) / k, which stays below k * 2^-24 plus one rounding of the pair's sum: half the bound.)"""
    W, H, spp, max_history, frames = 13, 9, 4, 6.0, 9
    gb, view, prm = tr.grid_frame(W, H), tr.grid_view(W, H), tr.params(max_history=max_history)
    rng = np.random.default_rng(11)
    prev, sums, count = None, None, 0
    for k in range(1, frames + 1):
        h1 = (rng.random((H, W, 3)) + 0.5).astype(np.float32) * np.float32(spp // 2)
        film = h1 + (rng.random((H, W, 3)) + 0.5).astype(np.float32) * np.float32(spp // 2)
        cur = dict(gb, film=film, half=h1 if half else None)
        of, oh, L, info = tr.accumulate(cur, spp, prev, view if prev is not None else None, prm, dtype=dt, detail=True)
        assert np.array_equal(L, np.full((H, W), min(k, max_history), dt)), k
        c = [x.astype(np.float64) for x in info["c"]]
        if k <= max_history:
            sums = c if sums is None else [s + x for s, x in zip(sums, c)]
            count = k
            mean = sum(sums) / count
            rel = np.abs(of.astype(np.float64) - mean) / mean
            assert rel.max() <= k * 2.0 ** -23, (k, rel.max())
            if half:
                assert (np.abs(oh.astype(np.float64) - sums[0] / count) / (sums[0] / count)).max() <= k * 2.0 ** -23
        prev = dict(gb, film=of, half=oh, length=L)


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_restatement_three_pixel_shift(dt):
    """A view that shifts the fronto-parallel plane by exactly 3 pixels (and 2 rows) moves the history by 3 pixels (and 2 rows): pixel
    (i, j) takes the previous pixel (i + 3, j + 2) alone, pixels whose source is outside the frame have no history.  A half-pixel shift
    takes the mean of two neighbours."""
    W, H, spp = 13, 9, 2
    gb = tr.grid_frame(W, H)
    rng = np.random.default_rng(5)
    pf = tr.hdr(rng, (H, W, 3))
    cur = dict(gb, film=tr.hdr(rng, (H, W, 3)) * np.float32(spp), half=None)
    prev = dict(gb, film=pf, half=None, length=np.full((H, W), 3.0, np.float32))
    of, _, L, info = tr.accumulate(cur, spp, prev, tr.grid_view(W, H, 3.0, 2.0), dtype=dt, detail=True)
    c = info["c"][0]
    want = c.copy(); wantL = np.ones((H, W), dt)
    src = np.asarray(pf, dt)[2:, 3:]
    want[:H - 2, :W - 3] = src + (c[:H - 2, :W - 3] - src) * (dt(1) / dt(4))
    wantL[:H - 2, :W - 3] = 4
    assert np.array_equal(of, want) and np.array_equal(L, wantL)
    of, _, L, info = tr.accumulate(cur, spp, prev, tr.grid_view(W, H, 0.5, 0.0), dtype=dt, detail=True)
    hist = (np.asarray(pf, dt)[:, :-1] * dt(0.5) + np.asarray(pf, dt)[:, 1:] * dt(0.5)) / dt(1)
    assert np.array_equal(info["hist"][0][:, :-1], hist) and (L[:, :-1] == 4).all()
    # the last column: its right tap is outside, the left one alone has the weight 0.5 and the history is its value
    assert np.array_equal(info["hist"][0][:, -1], (np.asarray(pf, dt)[:, -1] * dt(0.5)) / dt(0.5))


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_restatement_step_scene_disocclusion(dt):
    """The two-plane step seen from a camera that moved sideways: pixels disoccluded by the move (far-plane pixels whose four taps all saw
    the near plane) come out as c with length 1, and a tap across the step never contributes."""
    W, H, spp = 67, 35, 4
    rng = np.random.default_rng(3)
    cam_c, cam_p = tr.camera(position=(1.5, 0.0, 0.0), width=W, height=H), tr.camera(width=W, height=H)
    cur, _ = tr.gbuffer_sums(cam_c, "step", rng)
    prev, _ = tr.gbuffer_sums(cam_p, "step", rng)
    cur.update(film=tr.hdr(rng, (H, W, 3)) * np.float32(spp), half=tr.hdr(rng, (H, W, 3)))
    prev.update(film=tr.hdr(rng, (H, W, 3)) + 200.0, half=tr.hdr(rng, (H, W, 3)), length=np.full((H, W), 5.0, np.float32))
    view = tr.view_from_cameras(cam_c, cam_p)
    of, oh, L, info = tr.accumulate(cur, spp, prev, view, dtype=dt, detail=True)

    def plane_of(cam):      # 1 near, 2 far, 0 background
        X, t, hit = tr.raycast(cam, "step")
        return np.where(hit, np.where(np.abs(X[..., 2] + cam.position[2] + tr.STEP_NEAR) < 1e-6, 1, 2), 0)
    pc, pp = plane_of(cam_c), plane_of(cam_p)
    all_near = info["ok"] & (pc == 2)
    crossing = 0
    for k in range(4):
        qx, qy = info["x0"] + (k & 1), info["y0"] + (k >> 1)
        inside = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
        tap_plane = pp[np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)]
        v = info["valid"][k]
        assert (tap_plane[v] == pc[v]).all()                                     # a valid tap lies on the current pixel's plane
        crossing += int((inside & info["ok"] & (tap_plane != pc) & (tap_plane > 0) & (pc > 0)).sum())
        all_near &= inside & (tap_plane == 1)
    assert crossing > 20 and all_near.sum() >= 10, (crossing, int(all_near.sum()))
    c1, c2 = info["c"]
    assert np.array_equal(oh[all_near], c1[all_near]) and np.array_equal(of[all_near], (c1 + c2)[all_near]) and (L[all_near] == 1).all()
    assert (np.abs(L[info["has"]] - 6) < 1e-5).all() and (L[~info["has"]] == 1).all() and info["has"].sum() > 0.4 * W * H
    assert (of[info["has"]] > 40.0).all()                                       # (the history, near 200, took part there)


@pytest.mark.parametrize("view", tr.VIEWS)
@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_restatement_pair_and_bad_values(dt, view):
    """On every synthetic view: out_half is m1 and out_film - out_half reproduces m2 (within a rounding of the sum: 2^-23 |out_film| in f32);
    NaN / inf / negative film values give finite, non-negative output; every length is in [1, max_history]."""
    cur, prev, vw, spp = tr.synthetic(67, 35, view, "step", True)
    assert not np.isfinite(cur["film"]).all() and not np.isfinite(cur["half"]).all()
    of, oh, L, info = tr.accumulate(cur, spp, prev, vw, dtype=dt, detail=True)
    m1, m2 = info["m"]
    eps = 2.0 ** -23 if dt == np.float32 else 2.0 ** -52
    assert np.array_equal(oh, m1) and (np.abs((of.astype(np.float64) - oh.astype(np.float64)) - m2) <= eps * np.abs(of)).all()
    assert np.isfinite(of).all() and np.isfinite(oh).all() and (of >= 0).all() and (oh >= 0).all()
    assert (L >= 1).all() and (L <= 32).all() and (L[~info["has"]] == 1).all()
    assert info["has"].any() and (~info["has"]).any()


@pytest.fixture(scope="module")
def ref():
    return gbuffer_reference.GbufferReference()


@pytest.fixture(scope="module")
def rendered(ref, pkg):
    """scene 3, 64 x 48, 16 spp, mis + ZSobol, tex_size 128, from the CPU restatement of the G-buffer pass: the previous frame (seed 0) and
    the current frames (seed 1) of the static camera and of the two moved ones"""
    W, H, spp = 64, 48, 16
    out = {}
    for name, (move, yaw) in dict(tr.CAMERA_PAIRS, prev=((0.0, 0.0, 0.0), 0.0), static=((0.0, 0.0, 0.0), 0.0)).items():
        sc, cam, d65 = tr.load_moved(ref, pkg, 3, W, H, move, yaw)
        ref.set_faithful(sc, False)
        gb = ref.render_gbuffer_accum(sc, cam, pkg.make_params(spp, "mis", "sobol", seed=0 if name == "prev" else 1), d65,
                                      want=("shading_normal", "position", "hit"))
        out[name] = (gb, cam)
    return out, spp


@pytest.mark.parametrize("pair", list(tr.CAMERA_PAIRS))
def test_reprojection_geometry_on_rendered_gbuffers(pkg, rendered, pair):
    """The previous film holds the previous frame's world-space mean position, the current beauty the current frame's: the gathered history
    must be the current position on interior pixels, in units of the pixel footprint.  Bars: median <= 0.1, share under 0.25 >= 0.97, with
    an interior set of >= 0.6 of the pixels that hit geometry.  A NumPy sketch of the rule gave medians 0.005 / 0.012 and shares 0.9987 /
    0.9857 on these two pairs, and medians of 0.47 / 0.93 with no pixel under 0.25 for offsets of a quarter / half pixel in both axes."""
    frames, spp = rendered
    (gb_c, cam_c), (gb_p, cam_p) = frames[pair], frames["prev"]
    view = pkg.Product().temporal_view_from_cameras(cam_c, cam_p)
    cur, prev, prm = tr.geometry_frames(gb_c, gb_p, cam_c, cam_p, spp)
    of, _, _ = tr.accumulate(cur, spp, prev, view, prm)
    fig = tr.geometry_figures(of, cur, prev, view, prm, cam_c, spp)
    log_line('{"test": "temporal_geometry_cpu", "pair": "%s", "median": %.4f, "share_under_quarter": %.4f, "interior_share": %.4f, "interior": %d, "hit": %d}'
             % (pair, fig["median"], fig["share_under_quarter"], fig["interior_share"], fig["interior"], fig["hit"]))
    bars = tr.GEOMETRY_BARS
    assert fig["interior_share"] >= bars["interior_share"], fig
    assert fig["median"] <= bars["median"] and fig["share_under_quarter"] >= bars["share_under_quarter"], fig
    # the check can fail: the same frames through a view that is half a pixel off in x miss both bars
    off = pkg.ffi.TemporalView.from_buffer_copy(view); off.cx += 0.5
    bad = tr.geometry_figures(tr.accumulate(cur, spp, prev, off, prm)[0], cur, prev, off, prm, cam_c, spp)
    assert bad["median"] > bars["median"] and bad["share_under_quarter"] < bars["share_under_quarter"], bad


def test_static_camera_history_share(pkg, rendered):
    """A static camera and the default parameters: the share of the pixels that hit geometry which find a valid history (normal-mapped and
    silhouette pixels fail the tests).  Logged; the bar is only that most pixels do."""
    frames, spp = rendered
    (gb_c, cam_c), (gb_p, cam_p) = frames["static"], frames["prev"]
    view = pkg.Product().temporal_view_from_cameras(cam_c, cam_p)
    cur, prev, _ = tr.geometry_frames(gb_c, gb_p, cam_c, cam_p, spp)
    _, _, L, info = tr.accumulate(cur, spp, prev, view, detail=True)
    hit = gb_c["hit"][..., 1] > 0
    share = float(info["has"][hit].mean())
    log_line('{"test": "temporal_static_history_share", "with_history": %d, "hit": %d, "share": %.4f}' % (int(info["has"][hit].sum()), int(hit.sum()), share))
    assert share > 0.8 and not info["has"][~hit].any()


def test_temporal_cli_argument_errors(pkg, tmp_path):
    """--temporal-frames 0, with --gpus 2, with an AOV / position / depth renderer, with --adaptive-threshold or --denoise, and
    --camera-step without --temporal-frames: exit status 2 with a message, before any scene is loaded (no device needed)."""
    exe = os.path.join(pkg.ffi.ROOT, "toy-cpu-pathtracing_amd", "host", "mi355pt")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.dirname(exe)])
    for args in tr.CLI_MISUSE:
        r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=60, cwd=tmp_path)
        assert r.returncode == 2 and ("temporal" in r.stderr or "--camera-step" in r.stderr), (args, r.returncode, r.stderr)
    r = subprocess.run([exe, "--renderer", "mis", "--temporal-frames", "2", "--camera-step", "1,2"], capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert r.returncode == 2 and "--camera-step" in r.stderr
    r = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--temporal-frames" in r.stdout and "--camera-step" in r.stdout
    assert not os.listdir(tmp_path)
