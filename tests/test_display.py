"""The display stage (include/mi355pt_display.h), the part that needs no GPU: the ABI surface of the cross-compiled library, the defaults, the
refusals that happen before anything touches the device, the plan of the meter's first launch through a host check program, the properties of
the NumPy restatement (tests/display_reference.py) that the GPU tests lean on, and the CLI's argument errors."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import display_reference as dr  # noqa: E402
import sensor_reference as sr  # noqa: E402
from test_film_log import oracle_resolve_error  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["mi355pt_display_params_default", "mi355pt_display_scratch_bytes", "mi355pt_display_meter_device", "mi355pt_display_device",
               "mi355pt_display_meter", "mi355pt_display"]
E_INVALID = -1
F32 = np.float32


def ffi_params(product, prm):
    p = product.display_params_default()
    for k in dr.DEFAULTS:
        setattr(p, k, (float if k in dr.FLOAT_FIELDS else int)(getattr(prm, k)))
    return p


# ---------------- the ABI surface, the defaults ----------------
def test_display_abi_surface_and_defaults(pkg):
    """The header declares the six entry points, the struct and the enums; mi355pt.h includes it right after the upsample block's and declares
    nothing of it itself; the library exports the symbols; the ctypes mirror has the header struct's size and the documented defaults; the
    generated Rust binding names everything and is what the headers generate."""
    lib = ctypes.CDLL(pkg.ffi.LIB_PATH)
    root = pkg.ffi.ROOT
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "mi355pt_display.h")).read(), flags=re.S)
    main = open(os.path.join(root, "include", "mi355pt.h")).read()
    rs = open(os.path.join(root, "bindings", "rust", "mi355pt_sys.rs")).read()
    assert 0 < main.index('#include "mi355pt_upsample.h"') < main.index('#include "mi355pt_display.h"') < main.index('#include "mi355pt_denoise_var.h"')
    between = main[main.index('#include "mi355pt_upsample.h"') + len('#include "mi355pt_upsample.h"'):main.index('#include "mi355pt_display.h"')]
    assert "#include" not in between
    declared = sorted(set(re.findall(r"\b(mi355pt_[a-z0-9_]+)\s*\(", code)))
    assert declared == sorted(NEW_SYMBOLS)
    assert sorted("mi355pt_" + s for s in pkg.ffi.DISPLAY_SYMBOLS) == declared
    assert not set(pkg.ffi.DISPLAY_SYMBOLS) & set(pkg.ffi.ABI_SYMBOLS)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(r"pub fn %s\(" % name, rs), name
    m = re.search(r"typedef struct mi355pt_display_params \{(.*?)\} mi355pt_display_params;", code, flags=re.S)
    fields = [n.strip() for decl in m.group(1).split(";") if decl.strip() for n in decl.strip().split(" ", 1)[1].split(",")]
    assert fields == [f[0] for f in pkg.ffi.DisplayParams._fields_] == list(dr.DEFAULTS)
    assert ctypes.sizeof(pkg.ffi.DisplayParams) == 4 * len(fields) == 44           # eleven 32-bit fields, no padding
    assert re.search(r"pub struct DisplayParams \{\s*" + r"\s*".join(r"pub %s: (u32|i32|f32)," % f for f in fields) + r"\s*\}", rs)
    enums = dict(re.findall(r"(MI355PT_(?:TONE|ENCODE)_\w+) = (\d+)", code))
    assert {k: int(v) for k, v in enums.items()} == {"MI355PT_TONE_NONE": 0, "MI355PT_TONE_REINHARD": 1, "MI355PT_TONE_REINHARD_EXT": 2, "MI355PT_TONE_ACES": 3,
                                                     "MI355PT_TONE_HABLE": 4, "MI355PT_ENCODE_LINEAR": 0, "MI355PT_ENCODE_SRGB": 1}
    assert pkg.ffi.TONE == dr.TONES and pkg.ffi.ENCODE == {"linear": dr.ENCODE_LINEAR, "srgb": dr.ENCODE_SRGB}
    assert (pkg.ffi.DISPLAY_RECORD_WORDS, pkg.ffi.DISPLAY_HIST_WORDS) == (dr.RECORD_WORDS, dr.HIST_WORDS) == (8, 258)
    assert subprocess.call([sys.executable, os.path.join(root, "tools", "gen_rust_binding.py"), "--check"]) == 0
    p = pkg.Product().display_params_default()
    want = dict(tone=1, encode=1, exposure=1.0, white=F32(11.2), log2_lum_min=-16, trim_low=102, trim_high=51, key=F32(0.18), e_min=2.0 ** -10, e_max=2.0 ** 10,
                adapt=1.0)
    assert {k: getattr(p, k) for k in want} == {k: (float(v) if k in dr.FLOAT_FIELDS else v) for k, v in want.items()}
    d = dr.params()
    assert {k: getattr(p, k) for k in want} == {k: (float(getattr(d, k)) if k in dr.FLOAT_FIELDS else getattr(d, k)) for k in want}
    o = dr.params(**dr.OTHER)
    assert all(getattr(o, k) != getattr(d, k) for k in dr.DEFAULTS)                # OTHER moves every field


# ---------------- the plan of the meter's first launch ----------------
@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("display_plan") / "display_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "toy-cpu-pathtracing_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "display_plan_check.cpp")], check=True)

    def run(cases):
        text = "".join(f"{w} {h}\n" for w, h in cases)
        r = subprocess.run([exe], input=text, capture_output=True, text=True, check=True)
        rows = [tuple(int(v) for v in line.split()) for line in r.stdout.splitlines()]
        assert len(rows) == len(cases)
        return [dict(zip(("pixels", "chunks", "rows", "trips", "scratch", "covered", "twice"), row)) for row in rows]
    return run


PLAN_SIZES = [(1, 1), (1, 3), (63, 1), (64, 1), (65, 1), (255, 1), (256, 1), (257, 1), (1023, 1), (1024, 1), (1025, 1), (66, 34), (130, 70), (512, 512), (511, 513), (1024, 256), (1025, 256),
              (1920, 1080), (3840, 2160), (4096, 4096), (1 << 24, 1), (1, 1 << 24), (1 << 24, 1 << 7), (1 << 7, 1 << 24), ((1 << 24) - 1, 255), (65536, 65535)]


def test_display_plan_covers_every_pixel_once(pkg, planner):
    """display_plan.hpp through the host check program: for frames from 1 pixel to 2^24 x 2^7 the blocks' trips reach every pixel exactly once,
    rows is min(chunks of 1024 pixels, 256), no trip is wasted, the scratch size is rows x 258 x 4 bytes and equals mi355pt_display_scratch_bytes; frames the
    meter refuses have an empty plan and a scratch size of 0."""
    lib = pkg.Product().lib
    for (w, h), p in zip(PLAN_SIZES, planner(PLAN_SIZES)):
        n = w * h
        assert p["pixels"] == n and p["chunks"] == -(-n // 1024), (w, h, p)
        assert p["rows"] == min(p["chunks"], 256) and p["trips"] == -(-p["chunks"] // p["rows"]), (w, h, p)
        assert p["rows"] * (p["trips"] - 1) < p["chunks"] <= p["rows"] * p["trips"], (w, h, p)
        assert p["covered"] == n and p["twice"] == 0, (w, h, p)
        assert p["scratch"] == p["rows"] * 258 * 4 == lib.mi355pt_display_scratch_bytes(w, h), (w, h, p)
    bad = [(0, 5), (5, 0), ((1 << 24) + 1, 1), (1, (1 << 24) + 1), (1 << 16, 1 << 16), (1 << 24, 1 << 8), (1 << 24, 1 << 24)]
    for (w, h), p in zip(bad, planner(bad)):
        assert p["rows"] == 0 and p["scratch"] == 0 and lib.mi355pt_display_scratch_bytes(w, h) == 0, (w, h, p)
    (p,) = planner([(1920, 1080)])
    assert (p["rows"], p["trips"]) == (256, 8)                                     # the size the GPU tests use for "more than one trip"


# ---------------- the refusals ----------------
def test_display_refusals_before_the_device(pkg):
    """Every refusal the header lists returns MI355PT_E_INVALID with a message that names "display", from the device and the host entry
    points, with no device present (a call that got past the checks would answer MI355PT_E_DEVICE), and the outputs stay untouched."""
    f = pkg.ffi
    prod = pkg.Product()
    lib = prod.lib
    W, H, spp = 8, 4, 4
    film, _ = dr.frame(W, H, "mid", spp=spp)
    out = np.full((H, W, 3), 7.0, np.float32)
    rec = np.full(8, 7, np.uint32)
    prev = np.full(8, 7, np.uint32)
    hist = np.full(258, 7, np.uint32)
    need = prod.display_scratch_bytes(W, H)
    assert need == 258 * 4
    scratch = np.full(need // 4 + 4, 7, np.uint32)
    good = prod.display_params_default()
    ref = lambda x: ctypes.byref(x) if x is not None else None   # noqa: E731
    P = lambda a: a.ctypes.data if a is not None else None   # noqa: E731

    def refused(rc):
        assert rc == E_INVALID and b"display" in lib.mi355pt_last_error(), (rc, lib.mi355pt_last_error())

    def meter(fl=film, w=W, h=H, s=spp, p=good, pv=P(prev), sc=P(scratch), nb=need, rc=P(rec), hs=P(hist), host=True):
        refused(lib.mi355pt_display_meter_device(P(fl) if isinstance(fl, np.ndarray) else fl, w, h, s, ref(p), pv, sc, nb, rc, hs, None))
        if host:
            refused(lib.mi355pt_display_meter(P(fl) if isinstance(fl, np.ndarray) else fl, w, h, s, ref(p), pv, rc, hs))

    def display(fl=film, w=W, h=H, s=spp, p=good, rc=P(rec), o=P(out)):
        refused(lib.mi355pt_display_device(P(fl) if isinstance(fl, np.ndarray) else fl, w, h, s, ref(p), rc, o, None))
        refused(lib.mi355pt_display(P(fl) if isinstance(fl, np.ndarray) else fl, w, h, s, ref(p), rc, o))
    # NULL pointers
    meter(p=None); meter(fl=None); meter(rc=None); meter(sc=None, host=False)
    display(p=None); display(fl=None); display(o=None)
    # spp, sizes
    meter(s=0); display(s=0)
    for w, h in ((0, H), (W, 0), ((1 << 24) + 1, 1), (1, (1 << 24) + 1), (1 << 16, 1 << 16), (1 << 24, 1 << 8)):
        meter(w=w, h=h); display(w=w, h=h)
    meter(nb=need - 1, host=False); meter(nb=0, host=False)
    # alignment
    meter(sc=P(scratch) + 2, host=False); meter(rc=P(rec) + 1); meter(pv=P(prev) + 2); meter(hs=P(hist) + 3); display(rc=P(rec) + 2)
    # the parameters: a zero-initialised struct, then each field, by both operations
    bad_fields = (("tone", (5, 77, 0xffffffff)), ("encode", (2, 9)), ("exposure", (0.0, -1.0, np.inf, np.nan)),
                  ("white", (0.0, -2.0, 2.0 ** -17, 2.0 ** 17, np.inf, np.nan)), ("log2_lum_min", (-127, 96, -2 ** 31, 2 ** 31 - 1)),
                  ("key", (0.0, -0.18, np.inf, np.nan)), ("e_min", (0.0, -1.0, np.inf, np.nan, 2048.0)), ("e_max", (0.0, -1.0, np.inf, np.nan, 2.0 ** -11)),
                  ("adapt", (-0.01, 1.01, np.nan, np.inf)))
    meter(p=f.DisplayParams()); display(p=f.DisplayParams())
    for k, values in bad_fields:
        for v in values:
            p = prod.display_params_default(); setattr(p, k, v)
            meter(p=p); display(p=p)
    for lo, hi in ((1024, 0), (0, 1024), (512, 512), (1000, 24), (0xffffffff, 1), (0xfffffc00, 0x400)):
        p = prod.display_params_default(); p.trim_low, p.trim_high = lo, hi
        meter(p=p); display(p=p)
    # aliasing
    fb = film.nbytes
    meter(rc=P(film)); meter(rc=P(film) + fb - 4); meter(hs=P(film) + 8); meter(pv=P(film))
    meter(rc=P(scratch), host=False); meter(hs=P(scratch) + need - 4, host=False); meter(pv=P(scratch) + 4, host=False)
    meter(hs=P(rec)); meter(rc=P(hist) + 257 * 4); meter(hs=P(prev) + 4, pv=P(prev)); meter(pv=P(hist))
    both = np.full(16, 7, np.uint32)
    meter(rc=P(both), pv=P(both) + 16)                                             # overlapping without being the same record
    display(o=P(film)); display(o=P(film) + fb - 4); display(o=P(film) - fb + 4); display(rc=P(out) + 16)
    for a in (out, rec, prev, hist, scratch, both):
        assert (a == 7).all()
    # calls that pass every check reach the device layer: anything but MI355PT_E_INVALID here (there may be no device)
    p = prod.display_params_default(); p.trim_low, p.trim_high, p.adapt, p.log2_lum_min, p.tone, p.encode = 1023, 0, 0.0, 95, 4, 0
    assert lib.mi355pt_display_meter(P(film), W, H, spp, ref(p), P(rec), P(rec), None) != E_INVALID          # prev == record is allowed
    assert lib.mi355pt_display(P(film), W, H, spp, ref(p), None, P(out)) != E_INVALID


# ---------------- properties of the restatement ----------------
def test_restatement_scaling_shifts_bins_and_keeps_the_picture():
    """On a film whose luminances lie within octaves 8 .. 24 of the range, scaling by 2^j shifts the histogram by 8 j bins, scales L_avg by
    exactly 2^j and E_t by exactly 2^-j (bit patterns: the exponent field moves by j), and leaves the auto-exposed picture bit-equal, for
    every tone operator."""
    W, H = 66, 34
    film, spp = dr.frame(W, H, "mid")
    prm = dr.params()
    rec0, hist0, info0 = dr.meter(film, spp, prm)
    assert hist0[256] == hist0[257] == 0 and hist0[:64].sum() == 0 and hist0[192:256].sum() == 0 and info0["N"] == W * H
    assert F32(prm.e_min) < info0["E_t"] < F32(prm.e_max) and info0["cut_lo"] > 0 and info0["cut_hi"] > 0
    for j in (-4, -1, 3):
        scaled = (film * F32(2.0 ** j)).astype(np.float32)
        rec, hist, info = dr.meter(scaled, spp, prm)
        assert np.array_equal(np.roll(hist0[:256], 8 * j), hist[:256]) and hist[256] == hist[257] == 0
        assert int(rec[2]) == int(rec0[2]) + (j << 23) and int(rec[1]) == int(rec0[1]) - (j << 23) and rec[0] == rec[1]
        assert F32(prm.e_min) < info["E_t"] < F32(prm.e_max)
        assert np.array_equal(rec[3:], rec0[3:])
        for t in range(5):
            for enc in (dr.ENCODE_LINEAR, dr.ENCODE_SRGB):
                q = dr.params(tone=t, encode=enc)
                assert np.array_equal(dr.bits(dr.display(scaled, spp, q, rec)), dr.bits(dr.display(film, spp, q, rec0))), (j, t, enc)
    assert not np.array_equal(dr.display(scaled, spp, prm), dr.display(film, spp, prm))      # a fixed exposure does tell them apart


def test_restatement_trims_remove_exactly_their_counts():
    """N' = N - cut_lo - cut_hi always, and N' >= 1 whenever N >= 1 — for random histograms and trims, for a trim that ends exactly on a bin
    boundary and for one that ends inside a bin."""
    rng = np.random.default_rng(5)
    for _ in range(300):
        bins = rng.integers(0, 50, 256) * (rng.random(256) < rng.random())
        lo = int(rng.integers(0, 1024)); hi = int(rng.integers(0, 1024 - lo))
        N = int(bins.sum())
        cl, ch = (N * lo) >> 10, (N * hi) >> 10
        n = dr.trim(bins, cl, ch)
        assert sum(n) == N - cl - ch and all(0 <= a <= b for a, b in zip(n, bins))
        assert sum(n) >= 1 or N == 0
        assert sum(bins[:next((k for k, v in enumerate(n) if v), 256)]) <= cl       # everything under the first kept bin went to the low trim
    for N in (1, 2, 9, 10, 11, 1023, 1024, 1025):                                  # one pixel up: N' >= 1 with the largest trims
        for lo, hi in ((1023, 0), (0, 1023), (512, 511)):
            bins = np.zeros(256, int); bins[7] = N
            assert sum(dr.trim(bins, (N * lo) >> 10, (N * hi) >> 10)) >= 1
    # 1024 pixels, 4 per bin: trim_low 100 -> 100 pixels = exactly bins 0 .. 24; trim_high 50 -> bins 255 .. 244 and 2 of the 4 in bin 243
    hist = np.zeros(258, np.uint32); hist[:256] = 4
    rec, info = dr.finish(hist, dr.params(trim_low=100, trim_high=50))
    n = info["trimmed"]
    assert (info["cut_lo"], info["cut_hi"]) == (100, 50) and n[:25] == [0] * 25 and n[25] == 4 and n[243] == 2 and n[244:] == [0] * 12 and n[242] == 4
    assert info["Np"] == 1024 - 150 == rec[6] and rec[3] == 1024
    # ... and the mean bin of what is left, by hand: S / N' on the pseudo-log scale
    S = sum(k * v for k, v in enumerate(n))
    assert int(rec[2]) == (dr.hist_base(dr.params()) << 20) + ((S << 20) // 874) + (1 << 19)


def test_restatement_fallback_and_adaptation():
    """An all-black or all-out-of-range frame has N' = 0: E_t is 1 without a previous record and the previous E with one.  With adapt == 1 and
    with no previous record E is E_t in bits; otherwise E = E_prev + (E_t - E_prev) adapt in three f32 steps."""
    W, H = 16, 8
    prev = np.zeros(8, np.uint32); prev[0] = dr.bits(np.array([3.25], np.float32))[0]
    for kind in ("black", "below", "above"):
        film, spp = dr.frame(W, H, kind)
        rec, hist, info = dr.meter(film, spp)
        assert info["N"] == info["Np"] == 0 and rec[2] == 0 and hist[:256].sum() == 0 and hist[256] + hist[257] == W * H
        assert (hist[257] == W * H) == (kind == "above")
        assert dr.from_bits(rec[:2]).tolist() == [1.0, 1.0]
        for adapt in (0.0, 0.25, 1.0):
            rec, _, _ = dr.meter(film, spp, dr.params(adapt=adapt), prev)
            assert dr.from_bits(rec[:2]).tolist() == [3.25, 3.25]
    film, spp = dr.frame(W, H, "mid")
    rec1, _, info = dr.meter(film, spp, dr.params(adapt=0.3))                       # no previous record: adapt is not looked at
    assert rec1[0] == rec1[1]
    rec2, _, _ = dr.meter(film, spp, dr.params(adapt=1.0), prev)
    assert rec2[0] == rec2[1] == rec1[1]
    for adapt in (0.0, 0.25, 0.5):
        rec3, _, _ = dr.meter(film, spp, dr.params(adapt=adapt), prev)
        et, ep = dr.from_bits(rec3[1:2])[0], F32(3.25)
        want = F32(ep + F32(F32(et - ep) * F32(adapt)))
        assert rec3[1] == rec1[1] and dr.from_bits(rec3[:1])[0] == want
        assert (adapt == 0.0) == (want == ep)


def tone_grid():
    """0, then 64 points per octave from 2^-24 to 2^10 — a relative step of 1.1 %.  The curves' slopes make a step of that size change the
    value by far more than the few f32 roundings of a curve (each 2^-24 relative) can: at the flattest place used, x = 2^10, Reinhard moves by
    1e-5 and Hable by 3e-5 per step against 6e-8 for an ulp of 1; where a curve is clamped it is exactly flat."""
    return np.concatenate([[0.0], np.exp2(np.arange(-24 * 64, 10 * 64 + 1) / 64.0)]).astype(np.float32)


@pytest.mark.parametrize("name", list(dr.TONES))
def test_restatement_tone_operators(name):
    """Each operator is monotone non-decreasing on a dense grid in [0, 2^10] (grey input, so REINHARD_EXT is exercised on its luminance
    axis), maps 0 to 0 exactly, and NONE, REINHARD and ACES stay in [0, 1]; REINHARD_EXT maps the luminance `white` to 1 and HABLE the value
    `white` to 1; no operator produces a NaN anywhere up to the cap, specials included."""
    t = dr.TONES[name]
    x = tone_grid()
    assert (np.diff(x) > 0).all() and x[-1] == 1024.0
    for white in (11.2, 1.0, 100.0):
        prm = dr.params(tone=t, white=white)
        v = dr.tone(np.repeat(x[:, None], 3, 1), prm)
        assert np.isfinite(v).all() and dr.bits(v[0]).tolist() == [0, 0, 0]
        assert (np.diff(v, axis=0) >= 0).all(), name
        assert (v >= 0).all()
        if name in ("none", "reinhard", "aces"):
            assert (v <= 1).all()
        if name == "hable":
            assert dr.tone(np.full((1, 3), white, np.float32), prm).tolist() == [[1.0, 1.0, 1.0]]
        if name == "reinhard-ext":
            g = dr.tone(np.full((1, 3), white, np.float32), prm)
            assert np.allclose(g, 1.0, rtol=1e-6)
        hard = np.array([0.0, 1e-45, 1e-38, 1.0, 2.0 ** 31, 2.0 ** 32], np.float32)
        hv = dr.tone(np.stack([hard, hard[::-1], hard], 1), prm)
        assert np.isfinite(hv).all() and (hv >= 0).all()
    film = np.array([[dr.SPECIALS, dr.SPECIALS[::-1], np.roll(dr.SPECIALS, 5)]], np.float32).transpose(0, 2, 1).copy()
    for enc in (dr.ENCODE_LINEAR, dr.ENCODE_SRGB):
        out = dr.display(film, 1, dr.params(tone=t, encode=enc, exposure=1024.0))
        assert np.isfinite(out).all() and (out >= 0).all()


def test_restatement_reinhard_srgb_is_the_resolve(oracle):
    """REINHARD + ENCODE_SRGB + E = 1 against sensor_reference.resolve_reference (float64) over the resolve test's inputs and sample counts:
    within E, the deviation test_film_log.py measures for the oracle's own f32 Sensor::to_rgb over the same inputs.  (+inf is left out: the
    display cleans it to 0, the resolve turns it into NaN; the header promises the agreement on finite films.)"""
    e_oracle = oracle_resolve_error(oracle)
    _, pool = sr.resolve_inputs()
    pool = pool[~np.isposinf(pool)]
    pad = np.resize(pool, -(-pool.size // 3) * 3).reshape(1, -1, 3)
    worst = 0.0
    for spp in sr.RESOLVE_SPP:
        got = dr.display(pad, spp, dr.params())
        want = sr.resolve_reference(pad, spp)
        assert not np.isnan(got).any() and not np.isnan(want).any()
        worst = max(worst, float(sr.ulp_distance(got, want).max()))
    print(f"restatement's REINHARD + sRGB against the float64 resolve: {worst:.3f} ulp (the oracle's own E = {e_oracle:.3f})")
    assert worst <= e_oracle, (worst, e_oracle)


def test_restatement_frames_cross_what_they_should():
    """The synthetic frames the GPU tests use do reach what they are for: both range ends, every bin edge with both neighbours, the special
    values, every histogram word."""
    prm = dr.params()
    film, spp = dr.frame(130, 70, "loguniform")
    _, hist, info = dr.meter(film, spp, prm)
    assert hist[256] > 100 and hist[257] > 100 and (hist[:256] > 0).all() and not np.isfinite(film).all() and (film < 0).any()
    for p in (prm, dr.params(**dr.OTHER)):
        film, spp = dr.frame(130, 70, "edges", prm=p)
        t = dr.bits(dr.luminance(dr.clean(film, spp))).ravel()
        base = dr.hist_base(p)
        edges = (np.arange(257, dtype=np.int64) + base) << 20
        for off in (-1, 0, 1):
            assert np.isin(edges + off, t).all()
        _, hist, _ = dr.meter(film, spp, p)
        assert hist[256] >= 1 and hist[257] >= 2 and (hist[:256] >= 2).all()
    film, spp = dr.frame(66, 34, "constant")
    _, hist, _ = dr.meter(film, spp, prm)
    assert (hist > 0).sum() == 1 and hist.max() == 66 * 34


def test_display_cli_argument_errors(pkg, tmp_path):
    """The display flags' misuse — an unknown curve, an AOV renderer, --gpus 2, a dependent flag without its parent, values out of range: exit
    status 2 with a message naming the flag, before any scene is loaded (no device needed); --help lists the flags."""
    exe = os.path.join(pkg.ffi.ROOT, "toy-cpu-pathtracing_amd", "host", "mi355pt")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.dirname(exe)])
    for args, flag in dr.CLI_MISUSE:
        r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=60, cwd=tmp_path)
        assert r.returncode == 2 and flag in r.stderr and "Start build scene" not in r.stdout, (args, r.returncode, r.stderr)
    r = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and all(k in r.stdout for k in ("--tone-map", "--white", "--auto-exposure", "--exposure-key", "--exposure-adapt", "--exposure-trim"))
    assert not os.listdir(tmp_path)
