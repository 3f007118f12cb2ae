"""NumPy restatement of include/mi355pt_robust.h (the robust film: a per-pixel trimmed mean of K bucket means whose trim comes from their Gini
coefficient) and a seeded generator of bucket stacks.  Every step is one binary32 operation in the order the header states — arrays and
scalars are np.float32 throughout, so NumPy rounds each operation on its own — and the GPU tests hold the kernel to BIT EQUALITY with it.
Not a test module; tests/test_robust.py and tests/test_robust_gpu.py import it."""
import numpy as np

F32 = np.float32
MEAN, MOM, GMON = 0, 1, 2                     # MI355PT_ROBUST_*
MODES = {"mean": MEAN, "mom": MOM, "gmon": GMON}
BUCKET_COUNTS = (4, 8, 16, 32)
SET_SIZES = (2, 4, 8, 16, 32)

# the CLI's refusals (tests/test_robust.py): (arguments, the text the message must name)
CLI_MISUSE = [
    (["--renderer", "mis", "--robust-buckets", "5"], "--robust-buckets"),
    (["--renderer", "mis", "--robust-buckets", "64"], "--robust-buckets"),
    (["--renderer", "mis", "--spp", "20", "--robust-buckets", "8"], "--spp"),
    (["--renderer", "normal", "--robust-buckets", "8"], "--renderer"),
    (["--renderer", "albedo", "--robust-buckets", "8"], "--renderer"),
    (["--renderer", "depth", "--robust-buckets", "8"], "--renderer"),
    (["--renderer", "mis", "--robust-buckets", "8", "--gpus", "2"], "--gpus"),
    (["--renderer", "mis", "--robust-buckets", "8", "--adaptive-threshold", "0.05"], "--adaptive-threshold"),
    (["--renderer", "mis", "--robust-buckets", "8", "--half-res"], "--half-res"),
    (["--renderer", "mis", "--robust-buckets", "8", "--temporal-frames", "2"], "--temporal-frames"),
    (["--renderer", "mis", "--robust-buckets", "8", "--robust-mode", "median"], "--robust-mode"),
    (["--renderer", "mis", "--robust-buckets", "8", "--robust-scale", "-1"], "--robust-scale"),
    (["--renderer", "mis", "--robust-buckets", "8", "--robust-scale", "nan"], "--robust-scale"),
    (["--renderer", "mis", "--robust-mode", "mom"], "--robust-buckets"),
    (["--renderer", "mis", "--robust-scale", "2"], "--robust-buckets"),
]


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def clean_means(sums, spp_bucket):
    """step 1: v = B / (float)spp_bucket; v where it is finite and > 0, +0 otherwise"""
    with np.errstate(all="ignore"):
        v = np.asarray(sums, dtype=F32) / F32(spp_bucket)
        ok = np.isfinite(v) & (v > 0)
    return np.where(ok, v, F32(0)).astype(F32)


def luminance(m):
    """step 2 on (..., 3) cleaned means"""
    return (((m[..., 0] + m[..., 1]) + m[..., 2]) / F32(3)).astype(F32)


def ranks(l):
    """step 3 on (N, P) luminances: r_k = #{j != k : l_j < l_k or (l_j == l_k and j < k)}"""
    n = l.shape[0]
    r = np.zeros(l.shape, np.int32)
    for k in range(n):
        for j in range(n):
            if j != k:
                r[k] += (l[j] < l[k]) | ((l[j] == l[k]) & (j < k))
    return r


def gini(l, r):
    """steps 4 and 5 without the scale: (S, Q, G)"""
    n = l.shape[0]
    s = np.zeros(l.shape[1:], F32)
    q = np.zeros(l.shape[1:], F32)
    for k in range(n):
        s = (s + l[k]).astype(F32)
        w = (2 * r[k] - (n - 1)).astype(F32)
        wl = (w * l[k]).astype(F32)
        q = (q + wl).astype(F32)
    with np.errstate(all="ignore"):
        den = (F32(n - 1) * s).astype(F32)
        g = np.where(s > 0, q / den, F32(0)).astype(F32)
    return s, q, g


def trim_count(g_raw, n, mode, gini_scale):
    """steps 5 (scale, clamp) and 6"""
    if mode == MEAN:
        return np.zeros(g_raw.shape, np.int32)
    if mode == MOM:
        return np.full(g_raw.shape, n // 2 - 1, np.int32)
    assert mode == GMON
    sg = (F32(gini_scale) * g_raw).astype(F32)
    g = np.minimum(F32(1), np.maximum(F32(0), sg)).astype(F32)
    tf = np.floor((g * F32(n // 2)).astype(F32))
    return np.minimum(n // 2 - 1, tf.astype(np.int32)).astype(np.int32)


def combine_set(m, mode, gini_scale):
    """steps 2 - 7 over one set: m (N, P, 3) cleaned means in ascending bucket index -> (theta (P, 3) f32, t (P,) int32)"""
    n = m.shape[0]
    l = luminance(m)
    r = ranks(l)
    _, _, g = gini(l, r)
    t = trim_count(g, n, mode, gini_scale)
    acc = np.zeros(m.shape[1:], F32)
    for k in range(n):
        keep = (r[k] >= t) & (r[k] < n - t)
        acc = np.where(keep[:, None], (acc + m[k]).astype(F32), acc)
    kept = (n - 2 * t).astype(F32)
    return (acc / kept[:, None]).astype(F32), t


def combine(sums, spp_bucket, mode=GMON, gini_scale=1.0, pair=False):
    """mi355pt_robust_combine_device on a (K, H, W, 3) stack of sums -> (out (H, W, 3), out_half or None, trim (H, W, 2) uint8)"""
    sums = np.asarray(sums, dtype=F32)
    k, h, w = sums.shape[:3]
    assert k in BUCKET_COUNTS and sums.shape[3] == 3
    m = clean_means(sums, spp_bucket).reshape(k, h * w, 3)
    trim = np.zeros((h * w, 2), np.uint8)
    if not pair:
        theta, t = combine_set(m, mode, gini_scale)
        trim[:, 0] = t
        return theta.reshape(h, w, 3), None, trim.reshape(h, w, 2)
    th0, t0 = combine_set(m[0::2], mode, gini_scale)
    th1, t1 = combine_set(m[1::2], mode, gini_scale)
    trim[:, 0] = t0
    trim[:, 1] = t1
    return (th0 + th1).astype(F32).reshape(h, w, 3), th0.reshape(h, w, 3), trim.reshape(h, w, 2)


def set_diagnostics(sums, spp_bucket, gini_scale=1.0):
    """for the coverage tests, over one set (N, P, 3) of sums: t under GMON, pixels with a luminance tie, S == 0, a cleaned entry"""
    sums = np.asarray(sums, dtype=F32)
    n = sums.shape[0]
    m = clean_means(sums, spp_bucket)
    l = luminance(m)
    r = ranks(l)
    s, _, g = gini(l, r)
    t = trim_count(g, n, GMON, gini_scale)
    srt = np.sort(l, axis=0)
    tie = (srt[1:] == srt[:-1]).any(axis=0)
    with np.errstate(all="ignore"):
        v = sums / F32(spp_bucket)
        cleaned = (~np.isfinite(v) | (v < 0)).any(axis=(0, 2))
    return dict(t=t, tie=tie, s_zero=(s == 0), cleaned=cleaned, ranks=r)


def make_stack(k, height, width, seed, spp_bucket=4):
    """A seeded (K, H, W, 3) stack of bucket SUMS over spp_bucket samples that exercises every branch of the definition at every set size:
    gamma-distributed means of several shapes (the Gini term from near 0 to near 1), 2 % of the buckets with a spike of 50 ... 500 x the
    mean, dark pixels with one bright bucket, all-zero pixels, pixels quantised to a few grey levels (luminance TIES between buckets),
    pixels with j of their buckets equal and the others zero (every trim count of GMON, in the set of all K and — the non-zero buckets
    being spread evenly over even and odd indices — in the two sets of K / 2), and NaN, +inf, -inf and negative entries."""
    rng = np.random.default_rng(seed)
    p = height * width
    mean = np.zeros((k, p, 3), np.float64)
    kind = rng.choice(6, size=p, p=[0.40, 0.10, 0.05, 0.20, 0.20, 0.05])
    colour = rng.uniform(0.05, 2.0, (p, 3))
    # 0: gamma means
    shape = rng.choice([0.5, 2.0, 8.0, 50.0], size=p)
    gam = rng.gamma(shape[None, :], 1.0 / shape[None, :], (k, p))
    sel = kind == 0
    mean[:, sel] = gam[:, sel, None] * colour[None, sel]
    # 1: dark pixels with one bright bucket
    sel = np.flatnonzero(kind == 1)
    mean[:, sel] = 1e-3 * gam[:, sel, None] * colour[None, sel]
    mean[rng.integers(0, k, sel.size), sel] = rng.uniform(5.0, 50.0, (sel.size, 1)) * colour[sel]
    # 2: all-zero pixels (nothing to do)
    # 3: a few grey levels
    sel = kind == 3
    levels = np.array([0.0, 0.25, 0.5, 1.0])
    mean[:, sel] = levels[rng.integers(0, 4, (k, int(sel.sum())))][:, :, None]
    # 4: j consecutive buckets (cyclically) equal, the others zero: they fall alternately on even and odd indices, so both half sets sweep too
    sel = np.flatnonzero(kind == 4)
    for i in sel:
        j = int(rng.integers(1, k + 1))
        first = int(rng.integers(0, k))
        idx = (first + np.arange(j)) % k
        mean[idx, i] = rng.choice([0.5, 1.0, 3.0]) * (colour[i] if rng.random() < 0.5 else 1.0)
    # 5: gamma means, quantised coarsely (ties among noisy values)
    sel = kind == 5
    mean[:, sel] = np.round(gam[:, sel, None] * 2.0) / 2.0 * np.ones(3)
    # spikes: 2 % of all buckets
    spike = rng.random((k, p)) < 0.02
    base = np.maximum(mean.mean(axis=(0, 2)), 1e-3)
    mean += spike[:, :, None] * (rng.uniform(50.0, 500.0, (k, p)) * base[None, :])[:, :, None] * colour[None]
    sums = (mean.astype(F32) * F32(spp_bucket)).astype(F32)
    # entries the cleaning removes: 1 % of the values
    bad = rng.random(sums.shape)
    sums[bad < 0.0025] = np.nan
    sums[(bad >= 0.0025) & (bad < 0.005)] = np.inf
    sums[(bad >= 0.005) & (bad < 0.0075)] = -np.inf
    neg = (bad >= 0.0075) & (bad < 0.01)
    sums[neg] = -np.abs(sums[neg]) - F32(0.5)
    return sums.reshape(k, height, width, 3)


def firefly_model(k, pixels, seed, shape=8.0, p_spike=0.02, spike=200.0):
    """the model of the block's motivation: bucket means Gamma(shape, 1 / shape) (expectation 1) with probability p_spike of an added
    `spike`, grey -> (K, 1, pixels, 3) sums with spp_bucket 1"""
    rng = np.random.default_rng(seed)
    v = rng.gamma(shape, 1.0 / shape, (k, pixels)) + spike * (rng.random((k, pixels)) < p_spike)
    return np.repeat(v.astype(F32)[:, None, :, None], 3, axis=3)


def exact_stack(k, pixels, seed):
    """(K, 1, pixels, 3) sums with spp_bucket 1 on which every step up to the Gini quotient is EXACT in binary32: grey bucket means
    3 j / 16 with integer j <= 112 (so l = 3 j / 16, and S and Q are sums of small multiples of 1 / 16), a share of them zero, many ties.
    Here the order of the sums does not matter, so what holds in exact arithmetic — t does not depend on the order of the buckets — holds
    bit for bit."""
    rng = np.random.default_rng(seed)
    spread = rng.choice([1, 4, 16, 64], size=pixels)
    offset = rng.choice([0, 8, 48], size=pixels)                               # (an offset lowers the Gini term: the small trim counts)
    j = offset[None, :] + rng.integers(0, spread[None, :] + 1, (k, pixels))
    j[rng.random((k, pixels)) < rng.choice([0.0, 0.05, 0.1, 0.3, 0.8], size=pixels)[None, :]] = 0
    v = (j.astype(F32) * F32(3)) / F32(16)
    return np.repeat(v[:, None, :, None], 3, axis=3)
