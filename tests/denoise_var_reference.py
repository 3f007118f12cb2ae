"""NumPy restatement of the variance-guided denoiser of include/mi355pt_denoise_var.h (csrc/pt_kernels_denoise_var.hip), parametrised by
dtype: float32 is the filter as a straightforward f32 program, float64 the value both it and the GPU are measured against.  Test
infrastructure: written from the header's text, taps in the order dy, dx = -2 .. 2, no shortcut the kernel takes (plain divisions, np.exp,
the luminance as the header writes it, no records, no sentinel in the variance).

The beauty film and the guides are denoise_reference.synthetic's; the half film is a second seeded draw with the same mean."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import denoise_reference as dr  # noqa: E402

H5 = dr.H5
G3 = (1.0 / 16.0, 2.0 / 16.0, 1.0 / 16.0)                               # one factor of the 3 x 3 binomial (1 2 1; 2 4 2; 1 2 1) / 16 is G3[i] * G3[j] * 16
DEFAULTS = dict(levels=5, sigma_lum=4.0, sigma_normal=0.5, sigma_albedo=0.3, albedo_eps=0.01, lum_eps=1e-4)
rel_err = dr.rel_err
background = dr.background


def pixel_counts(shape, spp_b, tile_spp):
    """(H, W) sample count of every pixel: spp_b, or the count of the pixel's 8 x 8 tile (tile_spp: one value per tile, row-major)"""
    Hh, W = shape
    if tile_spp is None:
        return np.full((Hh, W), spp_b, np.uint32)
    assert spp_b == 0
    t = np.asarray(tile_spp, np.uint32).reshape((Hh + 7) // 8, (W + 7) // 8)
    return np.repeat(np.repeat(t, 8, axis=0), 8, axis=1)[:Hh, :W]


def lum(x, T):
    return ((x[..., 0] + x[..., 1]) + x[..., 2]) / T(3)


def prepass(beauty, half, spp_b, tile_spp=None, albedo=None, spp_a=0, normal=None, spp_n=0, albedo_eps=0.01, dtype=np.float32):
    """-> c, a (None without albedo), n (None without normal), bg (H, W) bool, irr, var (H, W)"""
    T = dtype
    B = np.asarray(beauty, np.float32)
    Hf = np.asarray(half, np.float32)
    cnt = pixel_counts(B.shape[:2], spp_b, tile_spp)
    nf = cnt.astype(T)[..., None]
    hf = (cnt // 2).astype(T)[..., None]

    def clean(v):
        return np.where(np.isfinite(v) & (v > 0), v, T(0))              # non-finite or negative -> 0 (a -0 becomes +0)
    with np.errstate(all="ignore"):
        c = clean(B.astype(T) / nf)
        c1 = clean(Hf.astype(T) / hf)
        c2 = clean((B.astype(T) - Hf.astype(T)) / hf)
        a = n = None
        bg = np.zeros(c.shape[:2], bool)
        if normal is not None:
            ns = np.asarray(normal, np.float32)
            bg = np.all(ns == 0, axis=2)
            n = T(2) * (ns.astype(T) / T(spp_n)) - T(1)
        irr, irr1, irr2 = c, c1, c2
        if albedo is not None:
            a = np.asarray(albedo, np.float32).astype(T) / T(spp_a)
            a = np.where(a > 0, a, T(0))
            den = a + T(albedo_eps)
            irr, irr1, irr2 = c / den, c1 / den, c2 / den
        dl = (lum(irr1, T) - lum(irr2, T)) / T(2)
        var = dl * dl
    return c, a, n, bg, irr.astype(T), var.astype(T)


def smooth_sd(var, bg, dtype=np.float32):
    """sd = sqrt(G(var)): the 3 x 3 binomial over the in-frame, non-background pixels around p, rows top to bottom and left to right, divided
    by the sum of the weights it used (background p: 0, never read)"""
    T = dtype
    Hh, W = var.shape
    gs = np.zeros((Hh, W), T)
    gw = np.zeros((Hh, W), T)
    for jy in range(3):
        dy = jy - 1
        y0, y1 = max(0, -dy), min(Hh, Hh - dy)
        if y0 >= y1:
            continue
        for jx in range(3):
            dx = jx - 1
            x0, x1 = max(0, -dx), min(W, W - dx)
            if x0 >= x1:
                continue
            P = (slice(y0, y1), slice(x0, x1))
            Q = (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))
            k = np.where(bg[Q], T(0), T(G3[jx]) * T(G3[jy]) * T(16)).astype(T)
            gs[P] += k * np.where(bg[Q], T(0), var[Q])
            gw[P] += k
    with np.errstate(all="ignore"):
        sd = np.sqrt(gs / gw)
    return np.where(bg, T(0), sd).astype(T)


def level(irr, var, a, n, bg, i, sigma_lum, sigma_normal, sigma_albedo, lum_eps, dtype=np.float32):
    """one a-trous level, step 2^i: irr' and var' of every non-background pixel; background pixels keep their values"""
    T = dtype
    Hh, W, _ = irr.shape
    s = 1 << i
    sd = smooth_sd(var, bg, T)
    den = T(sigma_lum) * sd + T(lum_eps)
    l = lum(irr, T)
    sw = np.zeros((Hh, W), T)
    acc = np.zeros((Hh, W, 3), T)
    accv = np.zeros((Hh, W), T)
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
            with np.errstate(all="ignore"):
                d = np.abs(l[P] - l[Q]) / den[P]
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
            accv[P] += (w * w) * np.where(bg[Q], T(0), var[Q])
    with np.errstate(all="ignore"):
        out = acc / sw[..., None]
        outv = accv / (sw * sw)
    return np.where(bg[..., None], irr, out).astype(T), np.where(bg, var, outv).astype(T)


def denoise(beauty, half, spp_b, tile_spp=None, albedo=None, spp_a=0, normal=None, spp_n=0, levels=5, sigma_lum=4.0, sigma_normal=0.5,
            sigma_albedo=0.3, albedo_eps=0.01, lum_eps=1e-4, dtype=np.float32, want_levels=False):
    """the whole filter on (H, W, 3) f32 films of sums -> (H, W, 3) `dtype` linear mean (and, on request, (irr, var) after every level)"""
    T = dtype
    c, a, n, bg, irr, var = prepass(beauty, half, spp_b, tile_spp, albedo, spp_a, normal, spp_n, albedo_eps, T)
    per_level = []
    for i in range(levels):
        irr, var = level(irr, var, a, n, bg, i, sigma_lum, sigma_normal, sigma_albedo, lum_eps, T)
        per_level.append((irr, var))
    out = irr * (a + T(albedo_eps)) if a is not None else irr
    out = np.where(bg[..., None], c, out).astype(T)
    return (out, per_level) if want_levels else out


def synthetic(width, height, spp_b, spp_a, spp_n, seed=0):
    """denoise_reference.synthetic's beauty and guides, and a half film: an independent seeded draw of the same per-pixel mean over
    spp_b / 2 samples (its own gamma noise, no fireflies), with a few NaN, +inf, -inf and negative values of its own.
    -> beauty, half, albedo, normal"""
    b_sum, a_sum, n_sum = dr.synthetic(width, height, spp_b, spp_a, spp_n, seed)
    rng = np.random.default_rng([seed, width, height, spp_b, 1])
    bg = dr.background(n_sum)
    with np.errstate(all="ignore"):
        mean = np.where(np.isfinite(b_sum) & (b_sum > 0), b_sum, 0.0).astype(np.float64) / spp_b
    mean = np.minimum(mean, 4.0)                                         # (the beauty's fireflies are not the mean)
    h_mean = mean * rng.gamma(2.0, 0.5, (height, width, 3))              # mean 1
    h_mean[bg] = mean[bg]                                                # the environment is noise-free
    h_sum = (h_mean * (spp_b // 2)).astype(np.float32)
    flat = h_sum.reshape(-1)
    vals = [np.inf, -2.5, np.nan, -np.inf, -0.0]
    if flat.size >= 8:
        bad = rng.choice(flat.size, size=min(flat.size, max(3, flat.size // 200)), replace=False)
        for j, idx in enumerate(bad):
            flat[idx] = vals[j % len(vals)]
    return b_sum, h_sum, a_sum, n_sum


def synthetic_tiles(width, height, spp_a, spp_n, seed=0):
    """the same with per-tile counts drawn from {2, 4, 8}: -> beauty, half, tile_spp ((tiles_y, tiles_x) uint32), albedo, normal; the
    films are the count-1 means of synthetic(.., spp_b=2, ..) scaled by every pixel's own n and n / 2 (exact: powers of two)"""
    b, h, a, n = synthetic(width, height, 2, spp_a, spp_n, seed)
    rng = np.random.default_rng([seed, width, height, 7])
    t = rng.choice(np.array([2, 4, 8], np.uint32), size=((height + 7) // 8, (width + 7) // 8))
    cnt = pixel_counts((height, width), 0, t).astype(np.float32)[..., None]
    with np.errstate(all="ignore"):
        return (b * (cnt / np.float32(2))).astype(np.float32), (h * (cnt / np.float32(2))).astype(np.float32), t, a, n
