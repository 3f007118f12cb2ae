"""NumPy restatement of include/mi355pt_bloom.h — the bloom stage: bright pass, firefly weights, the [1 3 3 1] reductions, the bilinear
expansions of the up pass, the composite — with the scratch buffer's layout, and the seeded synthetic films its tests use.  Written from the
header's text, not from the kernels: every float step is one np.float32 array operation (NumPy rounds each on its own, it never fuses), min
and max are np.fmin / np.fmax (a NaN operand is ignored).  tests/test_bloom.py checks its properties without a GPU; tests/test_bloom_gpu.py
holds the kernels of csrc/pt_kernels_bloom.hip to it bit for bit."""
from types import SimpleNamespace

import numpy as np

F32 = np.float32
FLT_MAX = np.finfo(np.float32).max
CAP = F32(2.0 ** 32)
MAX_LEVELS = 8
RECORD_WORDS = 8

# mi355pt_bloom_params_default
DEFAULTS = dict(levels=6, firefly=1, threshold=0.0, knee=0.5, scatter=0.7, base=float(F32(1) - F32(0.04)), intensity=0.04, exposure=1.0)
FIELDS = ("levels", "firefly", "threshold", "knee", "scatter", "base", "intensity", "exposure")
INT_FIELDS = ("levels", "firefly")
FLOAT_FIELDS = ("threshold", "knee", "scatter", "base", "intensity", "exposure")
SHAPES = [(1, 1), (1, 64), (64, 1), (7, 5), (33, 17), (67, 19), (130, 10)]      # (width, height)


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


def level_sizes(width, height, levels):
    """[(W_l, H_l)] for l = 0 .. levels"""
    out = [(width, height)]
    for _ in range(levels):
        w, h = out[-1]
        out.append(((w + 1) >> 1, (h + 1) >> 1))
    return out


def level_offsets(width, height, levels):
    """-> ([offset of level l in records, l = 0 .. levels; level 0 is not in the buffer: 0], records of the whole buffer)"""
    offs, total = [0], 0
    for w, h in level_sizes(width, height, levels)[1:]:
        offs.append(total)
        total += w * h
    return offs, total


def scratch_bytes(width, height, levels):
    if not (1 <= width <= 1 << 24 and 1 <= height <= 1 << 24 and width * height < 1 << 32 and 1 <= levels <= MAX_LEVELS):
        return 0
    return 16 * level_offsets(width, height, levels)[1]


def exposure_of(prm, record):
    return from_bits(np.asarray(record, np.uint32)[:1])[0] if record is not None else F32(prm.exposure)


def bright_pass(cc, prm, record=None):
    """cc: (H, W, 3), cleaned and capped -> p"""
    with np.errstate(all="ignore"):
        E = exposure_of(prm, record)
        T = F32(F32(prm.threshold) / E)
        k = F32(T * F32(prm.knee))
        m = np.fmax(np.fmax(cc[..., 0], cc[..., 1]), cc[..., 2])
        a = (m - T).astype(np.float32)
        s = np.fmin(np.fmax((a + k).astype(np.float32), F32(0)), F32(k + k))
        q = ((s * s).astype(np.float32) / F32(F32(4) * k)).astype(np.float32) if k != 0 else np.zeros_like(m)
        g = np.fmax(q, a)
        f = np.where(m == 0, F32(0), (g / m).astype(np.float32)).astype(np.float32)
        return (cc * f[..., None]).astype(np.float32)


def luminance(c):
    return ((F32(0.2126) * c[..., 0] + F32(0.7152) * c[..., 1]) + F32(0.0722) * c[..., 2]).astype(np.float32)


def reduce(S):
    """R(S): (H, W, C) -> ((H + 1) >> 1, (W + 1) >> 1, C), the separable [1 3 3 1] / 8 with clamped borders"""
    H, W = S.shape[:2]
    dw, dh = (W + 1) >> 1, (H + 1) >> 1
    with np.errstate(all="ignore"):
        x = [np.clip(2 * np.arange(dw) - 1 + a, 0, W - 1) for a in range(4)]
        h = ((S[:, x[0]] + S[:, x[3]]).astype(np.float32) + F32(3) * (S[:, x[1]] + S[:, x[2]]).astype(np.float32)).astype(np.float32)
        y = [np.clip(2 * np.arange(dh) - 1 + b, 0, H - 1) for b in range(4)]
        v = ((h[y[0]] + h[y[3]]).astype(np.float32) + F32(3) * (h[y[1]] + h[y[2]]).astype(np.float32)).astype(np.float32)
        return (v * F32(1.0 / 64.0)).astype(np.float32)


def _taps(n_dst, n_src):
    x = np.arange(n_dst)
    i = x >> 1
    n = np.where(x & 1, i + 1, i - 1)
    return np.clip(i, 0, n_src - 1), np.clip(n, 0, n_src - 1)


def expand(U, width, height):
    """X(U): (h, w, C) -> (height, width, C), bilinear with aligned centres and clamped borders"""
    i, n = _taps(width, U.shape[1])
    j, nj = _taps(height, U.shape[0])
    with np.errstate(all="ignore"):
        e = (F32(3) * U[:, i] + U[:, n]).astype(np.float32)
        r = (F32(3) * e[j] + e[nj]).astype(np.float32)
        return (r * F32(1.0 / 16.0)).astype(np.float32)


def pyramid(film, spp, prm, record=None):
    """-> (c, [None, D_1 .. D_L]): the cleaned film and the levels of the down pass, each (H_l, W_l, 3)"""
    c = clean(film, spp)
    cc = np.fmin(c, CAP)
    p = bright_pass(cc, prm, record)
    with np.errstate(all="ignore"):
        if prm.firefly:
            y1 = (F32(1) + luminance(p)).astype(np.float32)
            w = (F32(1) / y1).astype(np.float32)
            planes = np.concatenate([(p * w[..., None]).astype(np.float32), w[..., None]], axis=-1)
            r = reduce(planes)
            d = (r[..., :3] / r[..., 3:4]).astype(np.float32)
        else:
            d = reduce(p)
    D = [None, d]
    for _ in range(2, prm.levels + 1):
        D.append(reduce(D[-1]))
    return c, D


def bloom(film, spp, prm, record=None):
    """mi355pt_bloom on a (H, W, 3) float32 film of sums -> SimpleNamespace(out, B, D, U, scratch): the composite, the bloom alone, the levels of
    the down pass, those of the up pass, and the scratch buffer as the call leaves it, (records, 4) float32"""
    film = np.asarray(film, np.float32)
    H, W = film.shape[:2]
    L = prm.levels
    c, D = pyramid(film, spp, prm, record)
    s1 = F32(prm.scatter)
    s0 = F32(F32(1) - s1)
    U = [None] * (L + 1)
    U[L] = D[L]
    with np.errstate(all="ignore"):
        for l in range(L - 1, 0, -1):
            X = expand(U[l + 1], D[l].shape[1], D[l].shape[0])
            U[l] = ((D[l] * s0).astype(np.float32) + (X * s1).astype(np.float32)).astype(np.float32)
        B = expand(U[1], W, H)
        out = ((c * F32(prm.base)).astype(np.float32) + (B * F32(prm.intensity)).astype(np.float32)).astype(np.float32)
    scratch = np.concatenate([np.concatenate([U[l].reshape(-1, 3), np.zeros((U[l].shape[0] * U[l].shape[1], 1), np.float32)], axis=1) for l in range(1, L + 1)])
    assert scratch.shape[0] * 16 == scratch_bytes(W, H, L)
    return SimpleNamespace(out=out, B=B, D=D, U=U, scratch=scratch)


# ---------------- the films of the tests ----------------
SPECIALS = np.array([np.nan, np.inf, -np.inf, -1.0, -0.0, 0.0, 1e-45, 1e-39, 1.1754944e-38, 3.4028235e38, 1e30, 2.0 ** 33], np.float32)


def film(width, height, kind, seed=0, spp=4):
    """-> ((H, W, 3) float32 sums, spp).  "hdr": log-uniform radiance over 2^-12 .. 2^12 with a few 1e4 emitter texels; "specials": the same
    with NaN, infinities, negatives, zeros, subnormals and huge values strewn over a quarter of the values; "bits": arbitrary u32 patterns"""
    rng = np.random.default_rng(1000 * width + height + 7919 * seed)
    if kind == "bits":
        f = from_bits(rng.integers(0, 1 << 32, (height, width, 3), dtype=np.uint64).astype(np.uint32)).copy()
        if f.size >= 4 * SPECIALS.size:                                            # (an infinity has two patterns in 2^32: planted)
            f.reshape(-1)[rng.choice(f.size, SPECIALS.size, replace=False)] = SPECIALS
        return f, spp
    f = np.exp2(rng.uniform(-12, 12, (height, width, 3))).astype(np.float32)
    hot = rng.random((height, width)) < 0.02
    f[hot] = (f[hot] * F32(1e4)).astype(np.float32)
    if kind == "specials":
        pick = rng.random(f.shape) < 0.25
        f[pick] = rng.choice(SPECIALS, int(pick.sum()))
    else:
        assert kind == "hdr", kind
    with np.errstate(all="ignore"):
        return (f * F32(spp)).astype(np.float32), spp


# the parameter sets every shape is run with on the GPU: (name, params overrides, with a display record?)
RECORD_E = 0.37
VARIANTS = [
    ("defaults", dict(), False),
    ("plain", dict(firefly=0), False),
    ("hard-threshold", dict(threshold=2.0, knee=0.0, base=1.0, intensity=0.5), False),
    ("soft-threshold-firefly-off", dict(firefly=0, threshold=1.5, knee=0.5, base=1.0, intensity=0.25), False),
    ("soft-threshold-record", dict(threshold=1.5, knee=0.5, exposure=3.0), True),
    ("record-no-threshold", dict(exposure=5.0), True),
    ("exposure", dict(threshold=1.0, knee=0.5, exposure=0.125), False),
    ("scatter-0", dict(scatter=0.0), False),
    ("scatter-1", dict(scatter=1.0, firefly=0), False),
]


def record(E=RECORD_E):
    r = np.zeros(RECORD_WORDS, np.uint32)
    r[0] = bits(np.array([E], np.float32))[0]
    return r


# ---------------- the CLI's argument errors: (arguments, what the message names) ----------------
CLI_MISUSE = [
    (["--bloom-levels", "3"], "--bloom-levels"), (["--bloom-threshold", "1"], "--bloom-threshold"), (["--bloom-knee", "0.5"], "--bloom-knee"),
    (["--bloom-scatter", "0.5"], "--bloom-scatter"), (["--bloom-intensity", "0.1"], "--bloom-intensity"), (["--bloom-additive"], "--bloom-additive"),
    (["--bloom-no-firefly"], "--bloom-no-firefly"),
    (["--bloom", "--renderer", "normal"], "--bloom"), (["--bloom", "--renderer", "albedo"], "--bloom"), (["--bloom", "--gpus", "2"], "--bloom"),
    (["--bloom", "--bloom-levels", "0"], "--bloom-levels"), (["--bloom", "--bloom-levels", "9"], "--bloom-levels"), (["--bloom", "--bloom-levels", "x"], "--bloom-levels"),
    (["--bloom", "--bloom-threshold", "-1"], "--bloom-threshold"), (["--bloom", "--bloom-threshold", "nan"], "--bloom-threshold"),
    (["--bloom", "--bloom-threshold", "70000"], "--bloom-threshold"), (["--bloom", "--bloom-knee", "1.5"], "--bloom-knee"),
    (["--bloom", "--bloom-scatter", "-0.1"], "--bloom-scatter"), (["--bloom", "--bloom-scatter", "2"], "--bloom-scatter"),
    (["--bloom", "--bloom-intensity", "17"], "--bloom-intensity"), (["--bloom", "--bloom-intensity", "-1"], "--bloom-intensity"),
    (["--bloom", "--bloom-intensity", "2"], "--bloom-intensity"),      # the energy-conserving form needs base = 1 - intensity in [0, 1]
]
