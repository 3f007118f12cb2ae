"""The rectified temporal accumulation (include/mi355pt_temporal_rectify.h), the part that needs no GPU: the ABI surface of the cross-compiled
library, the refusals that happen before anything touches the device, the properties of the NumPy restatement
(tests/temporal_rectify_reference.py) that the GPU tests lean on, the CLI's argument errors, and the quality of the RULE on oracle films
(tools/temporal_rectify_cpu.py): it costs a static view nothing and recovers from a change of illumination in both directions."""
import ctypes
import importlib.util
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import temporal_reference as tr  # noqa: E402
import temporal_rectify_reference as rr  # noqa: E402

NEW_SYMBOLS = ["mi355pt_temporal_rectify_params_default", "mi355pt_temporal_rectify_scratch_bytes", "mi355pt_temporal_accumulate_rectified_device",
               "mi355pt_temporal_accumulate_rectified"]
E_INVALID = -1
DTYPES = [np.float32, np.float64]


def log_line(text):
    print(text)
    if os.environ.get("MI355PT_FRAME_LOG"):
        with open(os.environ["MI355PT_FRAME_LOG"], "a") as f:
            f.write(text + "\n")


def test_temporal_rectify_abi_surface(pkg):
    """The new header declares exactly the four entry points and the one struct, mi355pt.h includes it right after mi355pt_temporal.h and
    declares nothing itself, the library exports the symbols, the ctypes mirror and the generated Rust binding name them, the defaults are
    radius 2 and gamma 2, and the scratch is 32 bytes per pixel (0 when that does not fit a size_t)."""
    lib = ctypes.CDLL(pkg.ffi.LIB_PATH)
    root = pkg.ffi.ROOT
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "mi355pt_temporal_rectify.h")).read(), flags=re.S)
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "mi355pt.h")).read(), flags=re.S)
    rs = open(os.path.join(root, "bindings", "rust", "mi355pt_sys.rs")).read()
    assert re.search(r'#include "mi355pt_temporal.h"\s*#include "mi355pt_temporal_rectify.h"', main)
    assert "mi355pt_temporal_rectify_" not in main.replace('#include "mi355pt_temporal_rectify.h"', "") and "accumulate_rectified" not in main
    declared = sorted(set(re.findall(r"\b(mi355pt_[a-z0-9_]+)\s*\(", code)))
    assert declared == sorted(NEW_SYMBOLS)
    assert sorted("mi355pt_" + s for s in pkg.ffi.TEMPORAL_RECTIFY_SYMBOLS) == declared
    assert not set(pkg.ffi.TEMPORAL_RECTIFY_SYMBOLS) & set(pkg.ffi.TEMPORAL_SYMBOLS)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(r"pub fn %s\(" % name, rs), name
    assert re.search(r"typedef struct mi355pt_temporal_rectify_params \{.*?\} mi355pt_temporal_rectify_params;", code, flags=re.S)
    assert re.search(r"pub struct TemporalRectifyParams \{\s*pub radius: u32,\s*pub gamma: f32,\s*\}", rs)
    assert ctypes.sizeof(pkg.ffi.TemporalRectifyParams) == 8
    assert pkg.ffi.TemporalRectifyParams.radius.offset == 0 and pkg.ffi.TemporalRectifyParams.gamma.offset == 4
    assert subprocess.call([sys.executable, os.path.join(root, "tools", "gen_rust_binding.py"), "--check"]) == 0
    prod = pkg.Product()
    p = prod.temporal_rectify_params_default()
    assert (p.radius, p.gamma) == (2, 2.0) and (rr.DEFAULTS["radius"], rr.DEFAULTS["gamma"]) == (p.radius, p.gamma)
    assert prod.temporal_rectify_scratch_bytes(64, 48) == 32 * 64 * 48 and prod.temporal_rectify_scratch_bytes(1, 1) == 32
    assert prod.temporal_rectify_scratch_bytes(0, 7) == 0
    assert prod.temporal_rectify_scratch_bytes(2 ** 32 - 1, 2 ** 32 - 1) == 0              # 32 (2^32 - 1)^2 does not fit 64 bits
    assert prod.temporal_rectify_scratch_bytes(2 ** 24, 2 ** 24) == 32 * 2 ** 48


def _frames(W=8, H=4, half=True):
    return tr.synthetic(W, H, "static", "step", half, bad=False)


def test_temporal_rectify_refusals_before_the_device(pkg):
    """Every refusal of mi355pt_temporal_accumulate_device, and the ones the new header adds (NULL rectify_params, a zero-initialised struct,
    radius outside 1 .. 3, gamma not finite or not > 0, a NULL / too small / misaligned scratch, a scratch that is an input or an output),
    return MI355PT_E_INVALID with a message that names "temporal", from both entry points, with no device present (a call that got past
    the checks would answer MI355PT_E_DEVICE), and the outputs and the scratch stay untouched."""
    f = pkg.ffi
    prod = pkg.Product()
    lib = prod.lib
    W, H = 8, 4
    cur, prev, view, spp = _frames(W, H)
    cview = f.TemporalView((ctypes.c_float * 3)(*view.delta), (ctypes.c_float * 9)(*view.rows), view.sx, view.sy, view.cx, view.cy)
    outs = [np.full((H, W, 3), 7.0, np.float32), np.full((H, W, 3), 7.0, np.float32), np.full((H, W), 7.0, np.float32)]
    o = [a.ctypes.data for a in outs]
    need = prod.temporal_rectify_scratch_bytes(W, H)
    raw = np.full(need + 64, 7, np.uint8)
    sp = (raw.ctypes.data + 15) & ~15                                            # a 16-byte aligned host address inside `raw`

    def frame(d, **kw):
        q = {k: (d[k].ctypes.data if d.get(k) is not None else None) for k in f.TEMPORAL_FILMS}
        q.update(kw)
        return f.TemporalFrame(*[q[k] for k in f.TEMPORAL_FILMS])
    good, rgood = prod.temporal_params_default(), prod.temporal_rectify_params_default()
    ref = lambda x: ctypes.byref(x) if x is not None else None   # noqa: E731
    calls = [0]

    def refused(rc):
        calls[0] += 1
        assert rc == E_INVALID and b"temporal" in lib.mi355pt_last_error(), (rc, lib.mi355pt_last_error())

    def both(fc, s, fp, v, w, h, p, of, oh, ol, rp=rgood, scratch=sp, nbytes=need):
        """refused by both entry points (the host form has no scratch: `scratch` / `nbytes` go to the device form alone)"""
        refused(lib.mi355pt_temporal_accumulate_rectified_device(ref(fc), s, ref(fp), ref(v), w, h, ref(p), ref(rp), scratch, nbytes, of, oh, ol, None))
        refused(lib.mi355pt_temporal_accumulate_rectified(ref(fc), s, ref(fp), ref(v), w, h, ref(p), ref(rp), of, oh, ol))

    def device_only(scratch, nbytes, fc, fp, v):
        refused(lib.mi355pt_temporal_accumulate_rectified_device(ref(fc), spp, ref(fp), ref(v), W, H, ref(good), ref(rgood), scratch, nbytes, *o, None))
    fc, fp = frame(cur), frame(prev)
    # ---- what mi355pt_temporal_accumulate_device refuses: required pointers
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
    both(fc, spp, fp, cview, 2 ** 24 + 1, H, good, *o)
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
    # ---- what the new header adds: the rectification's parameters (with and without a previous frame)
    for fpx, vx in ((fp, cview), (None, None)):
        both(fc, spp, fpx, vx, W, H, good, *o, rp=None)
        both(fc, spp, fpx, vx, W, H, good, *o, rp=f.TemporalRectifyParams())
        for radius in (0, 4, 5, 2 ** 32 - 1):
            both(fc, spp, fpx, vx, W, H, good, *o, rp=f.TemporalRectifyParams(radius, 2.0))
        for gamma in (0.0, -2.0, np.inf, -np.inf, np.nan):
            both(fc, spp, fpx, vx, W, H, good, *o, rp=f.TemporalRectifyParams(2, gamma))
        # ... and the device form's scratch: NULL, too small, not 16-byte aligned, an input, an output
        device_only(None, need, fc, fpx, vx)
        device_only(sp, need - 1, fc, fpx, vx)
        device_only(sp, 0, fc, fpx, vx)
        for off in (4, 8, 12, 1):
            device_only(sp + off, need, fc, fpx, vx)
        for ptr in o:
            device_only(ptr, 1 << 20, fc, fpx, vx)
        for k in ("film", "half", "position", "shading_normal", "hit"):
            device_only(cur[k].ctypes.data, 1 << 20, fc, fpx, vx)
    for k in ("film", "half", "length", "position", "shading_normal", "hit"):
        device_only(prev[k].ctypes.data, 1 << 20, fc, fp, cview)
    assert calls[0] > 200
    assert all((a == 7.0).all() for a in outs) and (raw == 7).all()


# ---------------- properties of the restatement ----------------
def _grid_case(W, H, half, rng, scale=1.0, length=3.0):
    """the exact pixel grid, a static view: the history IS the current frame's values times `scale` (c1 = half / (spp / 2) exactly: spp = 2)"""
    gb = tr.grid_frame(W, H)
    h1 = tr.hdr(rng, (H, W, 3))
    film = h1 + tr.hdr(rng, (H, W, 3))
    cur = dict(gb, film=film, half=h1 if half else None)
    s = np.float32(scale)
    prev = dict(gb, film=(h1 * s + (film - h1) * s) if half else film * s, half=h1 * s if half else None, length=np.full((H, W), length, np.float32))
    return cur, prev, tr.grid_view(W, H), (2 if half else 1)


@pytest.mark.parametrize("half", [True, False], ids=["half", "nohalf"])
@pytest.mark.parametrize("radius", [1, 2, 3])
def test_restatement_history_equal_to_current_is_left_alone(radius, half):
    """f32, the exact pixel grid: a history equal to the current values gives k = 1 EXACTLY at every pixel and channel (the two window sums
    are the same numbers added in the same order, so muh == mu, which lies in [lo, hi]), and the output is bit-equal to the unrectified
    accumulation's."""
    rng = np.random.default_rng(17)
    W, H = 13, 9
    cur, prev, view, spp = _grid_case(W, H, half, rng)
    if half:                                             # make hist2 = film - half exact: c2 = (B - H) / 1 is the same subtraction
        prev["film"] = prev["half"] + (cur["film"] - cur["half"])
        cur["film"] = prev["film"].copy()
    want = tr.accumulate(cur, spp, prev, view)
    got = rr.accumulate(cur, spp, prev, view, rprm=rr.params(radius=radius), detail=True)
    assert (got[3]["k"] == 1).all() and got[3]["has"].all()
    for a, b in zip(got[:3], want):
        assert (a is None) == (b is None)
        if a is not None:
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("radius", [1, 2, 3])
def test_restatement_constant_frame_pulls_a_scaled_history_back(dt, radius):
    """A constant current frame (se = 0, so lo = hi = mu) and a history 4 times as bright, itself not constant: the rectified history's
    window mean equals mu at every pixel, to the rounding of k and of the sums (a few 2^-24 in f32)."""
    rng = np.random.default_rng(23)
    W, H = 13, 9
    gb = tr.grid_frame(W, H)
    cur = dict(gb, film=np.full((H, W, 3), 0.75, np.float32), half=None)
    hist = (4.0 * 0.75 * (0.5 + rng.random((H, W, 3)))).astype(np.float32)
    prev = dict(gb, film=hist, half=None, length=np.full((H, W), 5.0, np.float32))
    *_, info = rr.accumulate(cur, 1, prev, tr.grid_view(W, H), rprm=rr.params(radius=radius), dtype=dt, detail=True)
    assert (info["se"] == 0).all() and (info["mu"] == dt(0.75)).all() and info["has"].all()
    # the window mean of the history, scaled by the pixel's own k, is mu
    scaled_mean = info["muh"].astype(np.float64) * info["k"].astype(np.float64)
    assert np.abs(scaled_mean / 0.75 - 1.0).max() <= (8 * 2.0 ** -24 if dt == np.float32 else 1e-14)
    assert (info["k"] < 0.6).all() and (info["k"] > 0.1).all()                           # (the history was about 4 times too bright)


@pytest.mark.parametrize("view", ["static", "move", "outside", "behind"])
@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_restatement_pair_keeps_its_ratio_and_bad_values_stay_out(dt, view):
    """On the synthetic views (bad current values, previous lengths with zeros): hist1' / hist2' = hist1 / hist2 because both take the same
    k (checked as hist1' hist2 = hist2' hist1 within 3 roundings); NaN, inf and negative current values give finite, non-negative output;
    out_length is the unrectified accumulation's; out_half is m1 and out_film = m1 + m2."""
    cur, prev, vw, spp = tr.synthetic(67, 35, view, "step", True)
    assert not np.isfinite(cur["film"]).all() and not np.isfinite(cur["half"]).all()
    of, oh, L, info = rr.accumulate(cur, spp, prev, vw, dtype=dt, detail=True)
    plain = tr.accumulate(cur, spp, prev, vw, dtype=dt)
    has = info["has"]
    assert has.any() and (~has).any()
    assert np.array_equal(L, plain[2]) and (L[~has] == 1).all()
    assert np.isfinite(of).all() and np.isfinite(oh).all() and (of >= 0).all() and (oh >= 0).all()
    assert np.array_equal(oh, info["m"][0]) and np.array_equal(of, info["m"][0] + info["m"][1])
    eps = 2.0 ** -23 if dt == np.float32 else 2.0 ** -52
    h1, h2 = [x[has].astype(np.float64) for x in info["hist"]]
    r1, r2 = [x[has].astype(np.float64) for x in info["rect"]]
    assert (np.abs(r1 * h2 - r2 * h1) <= 3 * eps * np.abs(r1 * h2)).all()
    assert np.isfinite(info["k"][has]).all() and (info["k"][has] >= 0).all() and (info["k"][has] != 1).any()
    # a pixel without history comes out as c
    assert np.array_equal(oh[~has], info["c"][0][~has]) and np.array_equal(of[~has], (info["c"][0] + info["c"][1])[~has])


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_restatement_pixel_without_history_is_no_member(dt):
    """A pixel whose previous length is 0 has no history (static view on the exact grid: one tap): it comes out as c with L = 1, and whatever
    the previous films hold under it — here 1e6 instead of HDR noise — changes no other pixel.  (The history is 8 times the current frame:
    k < 1 everywhere, since hi < 8 mu needs only that the window's squared coefficient of variation is below 49 n / 4, and it is at most n - 1.)"""
    rng = np.random.default_rng(29)
    W, H = 13, 9
    cur, prev, view, spp = _grid_case(W, H, True, rng, scale=8.0)
    holes = [(4, 6), (0, 0), (8, 12), (4, 7)]
    for j, i in holes:
        prev["length"][j, i] = 0.0
    a = rr.accumulate(cur, spp, prev, view, dtype=dt, detail=True)
    other = {k: v.copy() if isinstance(v, np.ndarray) else v for k, v in prev.items()}
    for j, i in holes:
        other["film"][j, i], other["half"][j, i] = 1e6, 3e5
    b = rr.accumulate(cur, spp, other, view, dtype=dt)
    for x, y in zip(a[:3], b):
        assert np.array_equal(x, y)
    for j, i in holes:
        assert a[2][j, i] == 1 and np.array_equal(a[1][j, i], a[3]["c"][0][j, i]) and not a[3]["has"][j, i]
    assert a[3]["n"][4, 6] == 25 - 2 and a[3]["n"][0, 0] == 9 - 1 and (a[3]["k"][a[3]["has"]] < 1).all()


def test_window_sum_order_and_edges():
    """window_sum is the header's order: row sums left to right from 0, then top to bottom from 0 — against a plain loop in f32 on values
    whose sum depends on the order — and counts only in-frame values."""
    rng = np.random.default_rng(31)
    H, W, r = 5, 6, 2
    x = (rng.random((H, W)) * 10.0 ** rng.integers(-3, 4, (H, W))).astype(np.float32)
    want = np.zeros((H, W), np.float32)
    for j in range(H):
        for i in range(W):
            s = np.float32(0)
            for dy in range(-r, r + 1):
                row = np.float32(0)
                for dx in range(-r, r + 1):
                    inside = 0 <= j + dy < H and 0 <= i + dx < W
                    row = np.float32(row + (x[j + dy, i + dx] if inside else np.float32(0)))
                s = np.float32(s + row)
            want[j, i] = s
    assert np.array_equal(rr.window_sum(x, r), want)
    assert np.array_equal(rr.window_sum(np.ones((3, 2), np.float32), 3), np.full((3, 2), 6, np.float32))


def test_temporal_rectify_cli_argument_errors(pkg, tmp_path):
    """The rectify flags without --temporal-frames, radius and gamma without --temporal-rectify, a radius outside 1 .. 3 and a gamma that is
    not finite and above 0: exit status 2 with a message that names "temporal", before any scene is loaded (no device needed).  --help
    lists the new flags."""
    exe = os.path.join(pkg.ffi.ROOT, "toy-cpu-pathtracing_amd", "host", "mi355pt")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.dirname(exe)])
    for args in rr.CLI_MISUSE:
        r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=60, cwd=tmp_path)
        assert r.returncode == 2 and "--temporal-rectify" in r.stderr, (args, r.returncode, r.stderr)
    r = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and all(k in r.stdout for k in ("--temporal-rectify]", "--temporal-rectify-radius", "--temporal-rectify-gamma"))
    assert not os.listdir(tmp_path)


# ---------------- the quality of the rule on oracle films ----------------
@pytest.fixture(scope="module")
def figures(pkg):
    spec = importlib.util.spec_from_file_location("temporal_rectify_cpu", os.path.join(pkg.ffi.ROOT, "tools", "temporal_rectify_cpu.py"))
    tool = importlib.util.module_from_spec(spec); spec.loader.exec_module(tool)
    return tool.figures()


def test_rectification_costs_a_static_view_nothing(figures):
    """(a) 8 static frames of 4 spp: E_rect <= sqrt(E_4 E_32), the bar of the unrectified accumulation.  The NumPy study that chose the rule
    gave E_rect / E_unrectified = 0.995."""
    run = figures["runs"]["static"]
    log_line(json.dumps({"test": "temporal_rectify_static_cpu", "E_4": figures["E_4"], "E_32": figures["E_32"], **{k: run[k] for k in run if k != "rmse"}}))
    assert figures["E_32"] < figures["E_4"]
    assert run["rmse"]["rectified"]["history"] <= (figures["E_4"] * figures["E_32"]) ** 0.5, run


@pytest.mark.parametrize("case", ["x0.25", "x4", "split"])
def test_rectification_follows_a_change_of_illumination(figures, case):
    """(b) The history is built from 8 frames whose films are scaled by 0.25, by 4, or by 0.25 on the left half and 4 on the right; four true
    frames follow.  E_rect <= sqrt(E_unrectified E_32) after them.  The study gave 0.096 against 0.109, 0.094 against 0.137 and 0.100 against
    0.128."""
    run = figures["runs"][case]
    log_line(json.dumps({"test": "temporal_rectify_change_cpu", "case": case, "E_32": figures["E_32"], **run}))
    e_r, e_u = run["rmse"]["rectified"]["after_4"], run["rmse"]["unrectified"]["after_4"]
    assert e_u > figures["E_32"]                                                    # (the stale history does hurt the unrectified run)
    assert e_r <= (e_u * figures["E_32"]) ** 0.5, run
