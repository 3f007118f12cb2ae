"""NumPy restatement of the denoiser of include/mi355pt_denoise.h (csrc/pt_kernels_denoise.hip), parametrised by dtype: float32 is the
filter as a straightforward f32 program, float64 the value both it and the GPU are measured against.  Test infrastructure: written
from the header's text, taps in the order dy, dx = -2 .. 2, no shortcut the kernel takes (no reciprocals, no exp2, no fused records).

Also the seeded synthetic inputs of the GPU parity tests and the error measure, so that the CPU tests and the GPU tests use the same."""
import numpy as np

H5 = (1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0)
DEFAULTS = dict(levels=5, sigma_color=1.0, sigma_normal=0.5, sigma_albedo=0.3, albedo_eps=0.01)


def prepass(beauty, spp_b, albedo=None, spp_a=0, normal=None, spp_n=0, albedo_eps=0.01, dtype=np.float32):
    """-> c, a (None without albedo), n (None without normal), bg (H, W) bool, irr; the divisions by spp in `dtype` on the f32 sums"""
    T = dtype
    with np.errstate(all="ignore"):
        c = np.asarray(beauty, np.float32).astype(T) / T(spp_b)
        c = np.where(np.isfinite(c) & (c > 0), c, T(0))                 # non-finite -> 0, then max(c, 0) (a -0 becomes +0)
        a = n = None
        bg = np.zeros(c.shape[:2], bool)
        if normal is not None:
            ns = np.asarray(normal, np.float32)
            bg = np.all(ns == 0, axis=2)
            n = T(2) * (ns.astype(T) / T(spp_n)) - T(1)
        irr = c
        if albedo is not None:
            a = np.asarray(albedo, np.float32).astype(T) / T(spp_a)
            a = np.where(a > 0, a, T(0))
            irr = c / (a + T(albedo_eps))
    return c, a, n, bg, irr.astype(T)


def level(irr, a, n, bg, i, sigma_color, sigma_normal, sigma_albedo, dtype=np.float32):
    """one a-trous level, step 2^i: irr' of every non-background pixel; background pixels keep their value"""
    T = dtype
    Hh, W, _ = irr.shape
    s = 1 << i
    t = irr / (T(1) + irr)
    kc = T(4 ** i) / (T(sigma_color) * T(sigma_color))
    sw = np.zeros((Hh, W), T)
    acc = np.zeros((Hh, W, 3), T)
    for jy in range(5):
        dy = (jy - 2) * s
        y0, y1 = max(0, -dy), min(Hh, Hh - dy)                         # rows p for which q = p + dy is inside
        if y0 >= y1:
            continue
        for jx in range(5):
            dx = (jx - 2) * s
            x0, x1 = max(0, -dx), min(W, W - dx)
            if x0 >= x1:
                continue
            P = (slice(y0, y1), slice(x0, x1))
            Q = (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))
            dt = t[P] - t[Q]
            d = np.sum(dt * dt, axis=2) * kc
            if n is not None:
                dn = n[P] - n[Q]
                d = d + np.sum(dn * dn, axis=2) / (T(sigma_normal) * T(sigma_normal))
            if a is not None:
                da = a[P] - a[Q]
                d = d + np.sum(da * da, axis=2) / (T(sigma_albedo) * T(sigma_albedo))
            w = (T(H5[jx]) * T(H5[jy])) * np.exp(-d)
            w = np.where(bg[Q], T(0), w).astype(T)
            sw[P] += w
            acc[P] += w[..., None] * irr[Q]
    with np.errstate(all="ignore"):
        out = acc / sw[..., None]
    return np.where(bg[..., None], irr, out).astype(T)


def denoise(beauty, spp_b, albedo=None, spp_a=0, normal=None, spp_n=0, levels=5, sigma_color=1.0, sigma_normal=0.5, sigma_albedo=0.3,
            albedo_eps=0.01, dtype=np.float32, want_levels=False):
    """the whole filter on (H, W, 3) f32 films of sums -> (H, W, 3) `dtype` linear mean (and, on request, irr after every level)"""
    T = dtype
    c, a, n, bg, irr = prepass(beauty, spp_b, albedo, spp_a, normal, spp_n, albedo_eps, T)
    per_level = []
    for i in range(levels):
        irr = level(irr, a, n, bg, i, sigma_color, sigma_normal, sigma_albedo, T)
        per_level.append(irr)
    out = irr * (a + T(albedo_eps)) if a is not None else irr
    out = np.where(bg[..., None], c, out).astype(T)
    return (out, per_level) if want_levels else out


def rel_err(x, ref64):
    """max |x - ref64| / (|ref64| + 1e-3): the measure of e32 (x = the f32 restatement) and of the GPU's deviation"""
    return float(np.max(np.abs(np.asarray(x, np.float64) - ref64) / (np.abs(ref64) + 1e-3)))


def background(normal):
    return np.all(np.asarray(normal) == 0, axis=2)


def synthetic(width, height, spp_b, spp_a, spp_n, seed=0):
    """Seeded inputs (films of SUMS, f32): piecewise-planar normals and albedos over a few Voronoi regions, one of which is background
    (normal sums 0), HDR noise up to about 100 on the beauty, and a few NaN, +inf, -inf and negative beauty values.
    -> beauty, albedo, normal"""
    rng = np.random.default_rng([seed, width, height, spp_b])
    ys, xs = np.mgrid[0:height, 0:width]
    k = 5
    cx, cy = rng.uniform(0, width, k), rng.uniform(0, height, k)
    region = np.argmin((xs[..., None] - cx) ** 2 + (ys[..., None] - cy) ** 2, axis=2)
    nrm = rng.normal(size=(k, 3)); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    n_mean = (nrm[region] * 0.5 + 0.5).astype(np.float32)               # what the shading-normal AOV stores
    alb = rng.uniform(0.05, 0.9, (k, 3))
    tilt = rng.uniform(-0.2, 0.2, (k, 3)) / max(width, height)          # planar, not constant: a gradient inside each region
    a_mean = np.clip(alb[region] + tilt[region] * (xs + ys)[..., None], 0.0, None).astype(np.float32)
    bgm = region == 0
    if width * height < 4:
        bgm[:] = False                                                   # (a one-pixel frame stays a surface)
    n_sum = (n_mean * np.float32(spp_n)).astype(np.float32); n_sum[bgm] = 0.0
    a_sum = (a_mean * np.float32(spp_a)).astype(np.float32); a_sum[bgm] = 0.0
    light = rng.uniform(0.2, 3.0, (k, 3))[region]
    noise = rng.gamma(0.6, 1.0 / 0.6, (height, width, 3))               # mean 1, heavy tail
    fire = rng.random((height, width, 1)) < 0.02                        # fireflies up to about 100
    b_mean = a_mean * light * noise + fire * rng.uniform(10.0, 100.0, (height, width, 3))
    b_mean[bgm] = rng.uniform(0.0, 2.0, (int(bgm.sum()), 3))            # the background shows an environment
    b_sum = (b_mean * spp_b).astype(np.float32)
    flat = b_sum.reshape(-1)
    bad = rng.choice(flat.size, size=min(flat.size, max(3, flat.size // 200)), replace=False)
    vals = [np.nan, np.inf, -np.inf, -1.5, -0.0]
    if flat.size >= 8:
        for j, idx in enumerate(bad):
            flat[idx] = vals[j % len(vals)]
    return b_sum, a_sum, n_sum
