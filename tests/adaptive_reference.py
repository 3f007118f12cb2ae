"""NumPy restatement of include/mi355pt_adaptive.h — the per-tile noise estimate, the step and the per-tile normalisation — parametrised by
dtype (float32: the header's arithmetic, operation for operation and in its order; float64: the same formulas, the yardstick).  It follows
the header's text, shares nothing with csrc/pt_kernels_adaptive.hip and is what tests/test_adaptive.py and tests/test_adaptive_gpu.py
compare against.  Films are (H, W, 3) arrays of linear sums; per-tile arrays are flat, tile t = (t % tiles_x, t // tiles_x)."""
import numpy as np


def tiles_of(width, height):
    return (width + 7) // 8, (height + 7) // 8


def tile_view(a, width, height, fill):
    """(H, W, ...) -> (tiles_y, tiles_x, 64, ...) with l = 8 (y & 7) + (x & 7); pixels outside the frame hold `fill`"""
    tx, ty = tiles_of(width, height)
    pad = np.full((ty * 8, tx * 8) + a.shape[2:], fill, dtype=a.dtype)
    pad[:height, :width] = a
    v = pad.reshape((ty, 8, tx, 8) + a.shape[2:])
    v = np.moveaxis(v, 2, 1)                                     # (ty, tx, 8, 8, ...)
    return v.reshape((ty, tx, 64) + a.shape[2:])


def in_frame(width, height):
    """(tiles, 64) bool: pixel l of tile t lies inside the frame"""
    return tile_view(np.ones((height, width), bool), width, height, False).reshape(-1, 64)


def pixel_errors(film, half, n_pix, dark_eps, dtype):
    """e_p per pixel, (H, W); n_pix: (H, W) sample count n of the pixel's tile (n even)"""
    dt = np.dtype(dtype).type
    with np.errstate(all="ignore"):
        n_full = n_pix.astype(dtype)[..., None]
        n_half = (n_pix // 2).astype(dtype)[..., None]
        m = film.astype(dtype) / n_full
        h = half.astype(dtype) / n_half
        a = np.abs(m - h)
        d = (a[..., 0] + a[..., 1]) + a[..., 2]
        lum = (m[..., 0] + m[..., 1]) + m[..., 2]
        s = np.where(lum > 0, lum, dt(0)) + dt(np.float32(dark_eps))          # max(lum, 0); a NaN lum comes with a NaN d, so e_p is NaN either way
        return (d / np.sqrt(s)).astype(dtype)


def tile_errors(film, half, tile_spp, dark_eps, dtype=np.float32):
    """e_t of EVERY tile from its own tile_spp, (tiles,) of dtype: the pairwise tree over the 64 pixel slots, then / in-frame pixels"""
    H, W, _ = film.shape
    tx, ty = tiles_of(W, H)
    n_pix = np.repeat(np.repeat(np.asarray(tile_spp, np.uint32).reshape(ty, tx), 8, 0), 8, 1)[:H, :W]
    e = pixel_errors(film, half, n_pix, dark_eps, dtype)
    v = tile_view(e, W, H, np.dtype(dtype).type(0)).reshape(-1, 64)
    with np.errstate(all="ignore"):
        for k in (32, 16, 8, 4, 2, 1):
            v = v[:, :k] + v[:, k:2 * k]
        count = in_frame(W, H).sum(1).astype(dtype)
        return (v[:, 0] / count).astype(dtype)


def step(film, half, tile_spp, tile_err, threshold, dark_eps, level_spp, max_spp, dtype=np.float32):
    """mi355pt_adaptive_step_device -> (half', tile_spp', tile_err' (dtype), list, active (bool per tile)); the inputs are not modified"""
    H, W, _ = film.shape
    tile_spp = np.asarray(tile_spp, np.uint32).reshape(-1)
    at_level = tile_spp == level_spp
    safe_spp = np.where(at_level, tile_spp, 2).astype(np.uint32)                 # tiles at other counts are not estimated at all
    e = tile_errors(film, half, safe_spp, dark_eps, dtype)
    with np.errstate(invalid="ignore"):
        active = at_level & ~(e <= np.dtype(dtype).type(np.float32(threshold))) & (level_spp < max_spp)
    err = np.asarray(tile_err).astype(dtype).copy()
    err[at_level] = e[at_level]
    spp = tile_spp.copy()
    spp[active] = 2 * level_spp
    tx, ty = tiles_of(W, H)
    act_pix = np.repeat(np.repeat(active.reshape(ty, tx), 8, 0), 8, 1)[:H, :W]
    half2 = half.copy()
    half2[act_pix] = film[act_pix]
    return half2, spp, err, np.nonzero(active)[0].astype(np.uint32), active


def normalize(film, tile_spp):
    """mi355pt_film_normalize_tiles_device in float32"""
    H, W, _ = film.shape
    tx, ty = tiles_of(W, H)
    n = np.repeat(np.repeat(np.asarray(tile_spp, np.uint32).reshape(ty, tx), 8, 0), 8, 1)[:H, :W].astype(np.float32)
    with np.errstate(all="ignore"):
        return (film.astype(np.float32) / n[..., None]).astype(np.float32)


def rel_err(x, ref64):
    """max |x - ref64| / (|ref64| + 1e-3) over the finite entries of ref64 (the denoiser tests' measure); NaN positions must agree"""
    x = np.asarray(x, np.float64); ref64 = np.asarray(ref64, np.float64)
    assert np.array_equal(np.isnan(x), np.isnan(ref64)), "NaN errors in different tiles"
    ok = ~np.isnan(ref64)
    return float(np.max(np.abs(x[ok] - ref64[ok]) / (np.abs(ref64[ok]) + 1e-3))) if ok.any() else 0.0


def synthetic(width, height, level_spp, threshold, dark_eps, seed=0, nan_pixel=True):
    """A frame for the step at level_spp, built backwards from the answer: per tile a class — quiet (every pixel's e_p in (0.1 .. 0.9) x
    threshold / 2) or noisy ((2.5 .. 10) x threshold) — so that no decision hangs on rounding; means m are HDR (log-uniform up to about 100)
    with some negative channels, h = m + delta with |delta| summing to e_p sqrt(s).  tile_spp is mixed: about two thirds of the tiles at
    level_spp, the rest at level_spp / 2 and 2 level_spp with unrelated films.  One in-frame pixel of a tile at level_spp gets a NaN in F.
    -> film, half (float32 sums), tile_spp (uint32), tile_err (float32, a recognisable start value)"""
    rng = np.random.default_rng(1000 * seed + width * 7 + height)
    tx, ty = tiles_of(width, height)
    nt = tx * ty
    tile_spp = rng.choice([level_spp, level_spp, level_spp // 2, 2 * level_spp], size=nt).astype(np.uint32)
    tile_spp[rng.integers(nt)] = level_spp                                          # at least one tile at the level
    noisy = rng.random(nt) < 0.5
    up = lambda t: np.repeat(np.repeat(t.reshape(ty, tx), 8, 0), 8, 1)[:height, :width]   # noqa: E731
    m = np.exp(rng.uniform(np.log(1e-3), np.log(100.0), (height, width, 3)))
    m *= np.where(rng.random((height, width, 3)) < 0.08, -0.3, 1.0)                  # negative channels
    m[: height // 3] *= np.where(rng.random((height // 3, width, 1)) < 0.2, 0.0, 1.0)   # black pixels: dark_eps alone under the root
    s = np.maximum(m.sum(2), 0) + dark_eps
    u = np.where(up(noisy), rng.uniform(2.5, 10.0, (height, width)), rng.uniform(0.1, 0.9, (height, width)) * 0.5)
    total = u * threshold * np.sqrt(s)
    w = rng.dirichlet((1.0, 1.0, 1.0), (height, width))
    delta = total[..., None] * w * rng.choice([-1.0, 1.0], (height, width, 3))
    n = up(tile_spp).astype(np.float64)[..., None]
    film = (m * n).astype(np.float32)
    half = ((m + delta) * (n / 2)).astype(np.float32)
    if nan_pixel and nt > 1:
        t = int(np.nonzero(tile_spp == level_spp)[0][-1])
        film[(t // tx) * 8, (t % tx) * 8, 1] = np.nan
    tile_err = np.full(nt, -7.0, np.float32)
    return film, half, tile_spp, tile_err
