"""NumPy restatement of include/mi355pt_display.h — the display stage: the METER (a trimmed pseudo-log luminance histogram whose mean bin gives
an exposure, blended with the previous frame's) and the DISPLAY (exposure, tone curve, encoding) — and the seeded synthetic frames its tests
use.  Written from the header's text, not from the kernels: every float step is one np.float32 operation (NumPy rounds each array operation
on its own, it never fuses), every integer step a Python integer.  tests/test_display.py checks its properties without a GPU;
tests/test_display_gpu.py holds the kernels of csrc/pt_kernels_display.hip to it bit for bit."""
from types import SimpleNamespace

import numpy as np

F32 = np.float32
TONE_NONE, TONE_REINHARD, TONE_REINHARD_EXT, TONE_ACES, TONE_HABLE = range(5)
ENCODE_LINEAR, ENCODE_SRGB = 0, 1
TONES = {"none": TONE_NONE, "reinhard": TONE_REINHARD, "reinhard-ext": TONE_REINHARD_EXT, "aces": TONE_ACES, "hable": TONE_HABLE}
RECORD_WORDS, HIST_WORDS = 8, 258
FLT_MAX = np.finfo(np.float32).max
X_MAX = F32(2.0 ** 32)

# mi355pt_display_params_default, and a set with EVERY field off its default (tone and encode are the test's to choose)
DEFAULTS = dict(tone=TONE_REINHARD, encode=ENCODE_SRGB, exposure=1.0, white=11.2, log2_lum_min=-16, trim_low=102, trim_high=51, key=0.18,
                e_min=2.0 ** -10, e_max=2.0 ** 10, adapt=1.0)
OTHER = dict(tone=TONE_HABLE, encode=ENCODE_LINEAR, exposure=0.37, white=4.5, log2_lum_min=-9, trim_low=300, trim_high=7, key=0.11, e_min=0.02, e_max=50.0, adapt=0.7)
FLOAT_FIELDS = ("exposure", "white", "key", "e_min", "e_max", "adapt")
INT_FIELDS = ("tone", "encode", "log2_lum_min", "trim_low", "trim_high")


def params(**kw):
    d = dict(DEFAULTS)
    d.update(kw)
    return SimpleNamespace(**{k: (F32(v) if k in FLOAT_FIELDS else int(v)) for k, v in d.items()})


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def from_bits(u):
    return np.ascontiguousarray(u, dtype=np.uint32).view(np.float32)


def clean(film, spp):
    """c = F / spp where that is > 0 and finite, +0 otherwise (mi355pt_denoise_var.h)"""
    with np.errstate(all="ignore"):
        c = np.asarray(film, dtype=np.float32) / F32(spp)
        return np.where((c > 0) & (c <= FLT_MAX), c, F32(0)).astype(np.float32)


def luminance(c):
    with np.errstate(over="ignore"):
        return ((F32(0.2126) * c[..., 0] + F32(0.7152) * c[..., 1]) + F32(0.0722) * c[..., 2]).astype(np.float32)


def hist_base(prm):
    return (prm.log2_lum_min + 127) << 3


def histogram(film, spp, prm):
    """-> 258 uint32: the 256 bins, below, above"""
    t = (bits(luminance(clean(film, spp))).astype(np.int64) >> 20).ravel()
    base = hist_base(prm)
    slot = np.where(t < base, 256, np.where(t >= base + 256, 257, t - base))
    return np.bincount(slot, minlength=HIST_WORDS).astype(np.uint32)


def trim(bins, cut_lo, cut_hi):
    """cut_lo pixels off the bins in ascending order, then cut_hi off what is left in descending order -> list of ints"""
    n = [int(v) for v in bins]
    rem = cut_lo
    for k in range(256):
        r = min(n[k], rem); n[k] -= r; rem -= r
    rem = cut_hi
    for k in range(255, -1, -1):
        r = min(n[k], rem); n[k] -= r; rem -= r
    return n


def finish(hist, prm, prev=None):
    """the meter's second launch on the summed histogram -> (record: 8 uint32, info)"""
    bins = [int(v) for v in hist[:256]]
    N = sum(bins)
    cut_lo, cut_hi = (N * prm.trim_low) >> 10, (N * prm.trim_high) >> 10
    n = trim(bins, cut_lo, cut_hi)
    Np = sum(n)
    S = sum(v * k for k, v in enumerate(n))
    has_prev = prev is not None
    e_prev = from_bits(np.asarray(prev, dtype=np.uint32)[:1])[0] if has_prev else F32(1)
    L, Et = F32(0), e_prev
    if Np > 0:
        pos = (S << 20) // Np
        L = from_bits(np.array([(hist_base(prm) << 20) + pos + (1 << 19)], np.uint32))[0]
        q = F32(prm.key) / L
        Et = np.minimum(np.maximum(q, F32(prm.e_min)), F32(prm.e_max))
    E = Et
    if has_prev and F32(prm.adapt) != F32(1):
        d = F32(Et - e_prev)
        m = F32(d * F32(prm.adapt))
        E = F32(e_prev + m)
    rec = np.zeros(RECORD_WORDS, np.uint32)
    rec[0:3] = bits(np.array([E, Et, L], np.float32))
    rec[3:7] = (N, int(hist[256]), int(hist[257]), Np)
    return rec, dict(N=N, Np=Np, S=S, cut_lo=cut_lo, cut_hi=cut_hi, trimmed=n, E=F32(E), E_t=F32(Et), L_avg=F32(L))


def meter(film, spp, prm=None, prev=None):
    """mi355pt_display_meter -> (record, hist, info)"""
    prm = prm if prm is not None else params()
    hist = histogram(film, spp, prm)
    rec, info = finish(hist, prm, prev)
    return rec, hist, info


def hable(x):
    x = np.asarray(x, dtype=np.float32)
    A, B, DF, K1, K0 = F32(0.15), F32(0.5), F32(0.06), F32(0.056), F32(0.001)
    p = A * x
    n, d = x * (K1 * p + K0), DF * (x * (p + B) + DF)
    return (n / d).astype(np.float32)


def tone(x, prm):
    """x: (..., 3) exposed, capped values -> the tone-mapped values, f32"""
    x = np.asarray(x, dtype=np.float32)
    one = F32(1)
    with np.errstate(all="ignore"):
        if prm.tone == TONE_NONE:
            v = np.minimum(x, one)
        elif prm.tone == TONE_REINHARD:
            v = x / (one + x)
        elif prm.tone == TONE_REINHARD_EXT:
            Y = luminance(x)
            w2 = F32(F32(prm.white) * F32(prm.white))
            a = Y / w2
            b = one + a
            n, d = Y * b, one + Y
            Yp = n / d
            s = Yp / Y
            v = np.where((Y == 0)[..., None], F32(0), x * s[..., None])
        elif prm.tone == TONE_ACES:
            n = x * (F32(2.51) * x + F32(0.03))
            d = x * (F32(2.43) * x + F32(0.59)) + F32(0.14)
            v = np.minimum(np.maximum(n / d, F32(0)), one)
        elif prm.tone == TONE_HABLE:
            v = hable(x) / hable(F32(prm.white))
        else:
            raise ValueError(prm.tone)
    return v.astype(np.float32)


def srgb_oetf32(v):
    """the resolve's device function in f32 steps, its powf taken as the correctly rounded one (float64 power, rounded once)"""
    v = np.asarray(v, dtype=np.float32)
    e = float(F32(1) / F32(2.4))
    with np.errstate(all="ignore"):
        p = np.power(v.astype(np.float64), e).astype(np.float32)
        return np.where(v <= F32(0.0031308), F32(12.92) * v, F32(1.055) * p - F32(0.055)).astype(np.float32)


def srgb_oetf64(v):
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.where(v <= 0.0031308, 12.92 * v, 1.055 * np.power(v, 1.0 / 2.4) - 0.055)


def exposed(film, spp, prm, record=None):
    E = from_bits(np.asarray(record, dtype=np.uint32)[:1])[0] if record is not None else F32(prm.exposure)
    with np.errstate(over="ignore"):
        return np.minimum(clean(film, spp) * E, X_MAX).astype(np.float32)


def display(film, spp, prm=None, record=None):
    """mi355pt_display -> (H, W, 3) f32"""
    prm = prm if prm is not None else params()
    v = tone(exposed(film, spp, prm, record), prm)
    return srgb_oetf32(v) if prm.encode == ENCODE_SRGB else v


def ulp_distance(got_f32, want_f64):
    """|got - want| in units of the f32 spacing at want"""
    want32 = np.abs(np.asarray(want_f64)).astype(np.float32)
    return np.abs(np.asarray(got_f32).astype(np.float64) - want_f64) / np.spacing(want32).astype(np.float64)


# ---------------- seeded synthetic frames ----------------
SPECIALS = np.array([0.0, -0.0, -1.0, -1e-30, np.nan, np.inf, -np.inf, 1e-41, 7e-45, -3e38, FLT_MAX, 1e30], dtype=np.float32)


def pixels_for_lum(y):
    """pixels (0, g, b) of sums (spp 1) whose luminance ((0 + 0.7152f g) + 0.0722f b) is EXACTLY the f32 y > 0: the green product lands a few
    ulps under y, the blue one supplies the difference, which is a small multiple of y's spacing and so far inside blue's resolution"""
    y = np.asarray(y, dtype=np.float32)
    g = from_bits((bits((y / F32(0.7152)).astype(np.float32)).astype(np.int64) - 4).astype(np.uint32))
    p = (F32(0.7152) * g).astype(np.float32)
    b = ((y - p).astype(np.float32) / F32(0.0722)).astype(np.float32)
    out = np.stack([np.zeros_like(g), g, b], -1)
    assert (b > 0).all() and np.array_equal(bits(luminance(out)), bits(y))
    return out


def frame(W, H, kind, seed=0, prm=None, spp=4, specials=True):
    """-> (film sums (H, W, 3) f32, spp).  kind:
       loguniform  luminance log-uniform over 2^-24 .. 2^24 (both ends of the default range are crossed), random chroma; with `specials`,
                   zeros, negatives, NaN, +-inf, subnormals and huge values in all three channels at seeded places
       edges       green-and-blue pixels (spp 1) whose luminance is exactly on every bin edge of `prm` — the two range ends with them — and one
                   ulp to either side
       constant    one value everywhere: every lane of every wave on one bin
       below / above / black   a frame entirely out of range
       mid         luminance log-uniform within octaves 8 .. 24 of the default range, chroma in [0.25, 1]: the scaling tests' frame"""
    prm = prm if prm is not None else params()
    rng = np.random.default_rng(seed + 1000 * W + H)
    n = W * H
    if kind == "edges":
        base = hist_base(prm)
        edge = (np.arange(257, dtype=np.int64) + base) << 20
        yb = np.stack([edge - 1, edge, edge + 1], 1).ravel().astype(np.uint32)
        px = pixels_for_lum(from_bits(rng.permutation(yb)))
        return np.resize(px, (n, 3)).reshape(H, W, 3).copy(), 1
    if kind == "constant":
        return np.tile(np.array([0.3, 0.5, 0.2], np.float32) * F32(spp), (H, W, 1)).astype(np.float32), spp
    if kind in ("below", "above", "black"):
        v = {"below": 2.0 ** -30, "above": 2.0 ** 40, "black": 0.0}[kind]
        return np.full((H, W, 3), v * spp, np.float32), spp
    lo, hi = (-24.0, 24.0) if kind == "loguniform" else (-5.9, 7.9)      # (the luminance is 0.25 .. 1 times this: 2^-7.9 .. 2^7.9)
    lum = np.exp2(rng.uniform(lo, hi, n))
    chroma = rng.uniform(0.25, 1.0, (n, 3))
    film = (lum[:, None] * chroma * spp).astype(np.float32)
    if kind == "loguniform" and specials:
        k = max(1, n // 5)
        at = rng.choice(n, k, replace=False)
        film[at, rng.integers(0, 3, k)] = np.resize(SPECIALS, k)
        for ch in range(3):                                           # ... and whole pixels of them, so that Y itself is special
            film[at[ch::7], :] = np.resize(SPECIALS, at[ch::7].size)[:, None]
    return film.reshape(H, W, 3), spp


def sequence(W, H, seed=0, frames=4, step_after=2, factor=4.0, spp=4):
    """the films of an adapting sequence: `frames` seeded mid-range frames, multiplied by `factor` after frame `step_after`"""
    out = []
    for k in range(frames):
        f, _ = frame(W, H, "mid", seed + k, spp=spp)
        out.append((f * F32(factor)).astype(np.float32) if k >= step_after else f)
    return out, spp


def run_sequence(films, spp, prm):
    """meter frame after frame, each with the previous frame's record -> the records"""
    recs, prev = [], None
    for f in films:
        prev, _, _ = meter(f, spp, prm, prev)
        recs.append(prev)
    return recs


# the CLI's documented misuse: each exits 2 with a message naming the flag, before any scene is loaded
CLI_MISUSE = [
    (["--renderer", "mis", "--tone-map", "filmic"], "--tone-map"),
    (["--renderer", "normal", "--tone-map", "aces"], "--tone-map"),
    (["--renderer", "albedo", "--auto-exposure"], "--auto-exposure"),
    (["--renderer", "mis", "--gpus", "2", "--auto-exposure"], "--auto-exposure"),
    (["--renderer", "mis", "--white", "4"], "--white"),
    (["--renderer", "mis", "--tone-map", "hable", "--white", "0"], "--white"),
    (["--renderer", "mis", "--exposure-key", "0.2"], "--exposure-key"),
    (["--renderer", "mis", "--auto-exposure", "--exposure-key", "-1"], "--exposure-key"),
    (["--renderer", "mis", "--auto-exposure", "--exposure-adapt", "1.5"], "--exposure-adapt"),
    (["--renderer", "mis", "--auto-exposure", "--exposure-trim", "900,200"], "--exposure-trim"),
    (["--renderer", "mis", "--auto-exposure", "--exposure-trim", "12"], "--exposure-trim"),
]
