"""Float64 restatement of the sensor: the linear sRGB contribution of one finished path, from its spectral radiance L[4], its wavelengths
lambda[4] and their pdf[4] (renderer/src/sensor.rs:41-78 with spectrum/src/sampled_spectrum.rs:346-365 and color/src/gamut.rs:29-63), written
from what the reference does, not from the kernels' film_rgb (csrc/pt_path.hpp): tests/test_film_log.py ties it to the oracle's Sensor, and
tests/test_film_log_gpu.py then reconciles every path kernel's film with the sum of it over the kernel's own per-sample log.

Per wavelength k that is still alive (pdf[k] != 0; a path whose secondary wavelengths were terminated keeps pdf[0] / 4 and zeros):
    c_k = L[k] / pdf[k] / 4,   XYZ += c_k * cmf[floor(lambda[k] - 360)]   (index 470 wraps to 0)
then rgb = M * XYZ * exposure with M the XYZ -> sRGB matrix.  The colour-matching functions are the f32 table values taken exactly
(pkg.scenes.cmf_xyz(); tests/test_oracle.py pins them to tests/golden/cie_d65.json); everything else is float64.

Beside the value, the ABSOLUTE MASS of each sample and channel,
    A = exposure * sum_k sum_j |M[ch][j]| * |c_k| * |cmf_j[k]|,
is returned: the sum of the magnitudes of the terms an f32 evaluation rounds, which is what a rounding bound is proportional to."""
import numpy as np

LAMBDA_MIN, LAMBDA_MAX, N_CMF, N_WL = 360.0, 830.0, 470, 4
U = 2.0 ** -24                               # unit roundoff of f32
ABS_FLOOR = 1e-37                            # the denormal range, where an f32 rounding is absolute
RESOLVE_SPP = (1, 3, 64, 1000)               # the sample counts of the resolve test


def xyz_to_srgb():
    """The XYZ -> linear sRGB matrix in float64, derived from the primaries and the white point (gamut.rs:29-63): the columns of RGB -> XYZ
    are the primaries' XYZ (Y = 1) scaled so that RGB (1, 1, 1) is the white point; XYZ -> RGB is its inverse.  Row `ch` gives channel ch."""
    def xyz(x, y):
        return np.array([x / y, 1.0, (1.0 - x - y) / y], dtype=np.float64)
    prim = np.stack([xyz(0.64, 0.33), xyz(0.30, 0.60), xyz(0.15, 0.06)], axis=1)            # columns r, g, b
    scale = np.linalg.solve(prim, xyz(0.3127, 0.3290))
    return np.linalg.inv(prim * scale[None, :])


def sensor_reference(L, lam, pdf, cmf, exposure=1.0):
    """L, lam, pdf: (..., 4) arrays; cmf: (3, 470) f32 table -> (value, mass), both (..., 3) float64.
    Non-finite radiance gives non-finite values (and masses) in the channels it reaches, as it does in the reference."""
    L = np.asarray(L, dtype=np.float64); lam = np.asarray(lam, dtype=np.float64); pdf = np.asarray(pdf, dtype=np.float64)
    cmf = np.asarray(cmf, dtype=np.float64)
    assert L.shape == lam.shape == pdf.shape and L.shape[-1] == N_WL and cmf.shape == (3, N_CMF)
    alive = pdf != 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        c = np.where(alive, L / np.where(alive, pdf, 1.0) / N_WL, 0.0)                      # (..., 4)
        idx = np.where(alive, np.floor(lam - LAMBDA_MIN), 0.0).astype(np.int64)
        idx = np.where(idx == N_CMF, 0, idx)
        assert ((idx >= 0) & (idx < N_CMF)).all(), "a live wavelength outside [360, 830]"
        m = np.moveaxis(cmf[:, idx], 0, -1)                                                # (..., 4, 3): cmf_j at wavelength k
        xyz = (c[..., None] * m).sum(axis=-2)                                              # (..., 3)
        xyz_abs = (np.abs(c)[..., None] * np.abs(m)).sum(axis=-2)
        M = xyz_to_srgb()
        value = (xyz @ M.T) * float(exposure)
        mass = (xyz_abs @ np.abs(M).T) * abs(float(exposure))
    return value, mass


def resolve_reference(accum, spp):
    """Sensor::to_rgb in float64 (sensor.rs:81-88, tone_map.rs:20-28, eotf.rs:54-61): mean -> clip at 0 -> c / (1 + c) -> sRGB OETF.
    The clip is f32::max, which returns the other operand for a NaN: a NaN sum resolves to 0, and only +inf (inf / inf) gives NaN."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        c = np.fmax(np.asarray(accum, dtype=np.float64) / float(spp), 0.0)
        c = c / (1.0 + c)
        return np.where(c <= 0.0031308, 12.92 * c, 1.055 * np.power(c, 1.0 / 2.4) - 0.055)


def resolve_inputs(seed=0):
    """The film values of the resolve test: the special values — each in every residue class of a 256-thread block, because their number
    is odd and they are laid out cyclically over 256 x that many slots — and then 4096 log-uniform values in [1e-6, 1e3]."""
    knee = np.float32(0.0031308)
    special = np.array([0.0, -0.0, -1.0, -1e-30, -3.0e38, np.finfo(np.float32).tiny, 1e-41, 7e-45,
                        np.nextafter(knee, np.float32(0)), knee, np.nextafter(knee, np.float32(1)), 1.0, 1e4, 1e30, np.finfo(np.float32).max,
                        np.inf, np.nan, -np.inf, 0.5], dtype=np.float32)
    # the knee is met AFTER the mean and c / (1 + c): the sums whose tone-mapped mean is the knee, for every spp of the test, +-2 ulp
    pre = np.float32(0.0031308 / (1.0 - 0.0031308))
    near = [pre]
    for _ in range(2):
        near = [np.nextafter(near[0], np.float32(0))] + near + [np.nextafter(near[-1], np.float32(1))]
    special = np.concatenate([special, np.outer(np.array(RESOLVE_SPP, dtype=np.float32), np.array(near, dtype=np.float32)).ravel()])
    assert special.size % 2 == 1
    rng = np.random.default_rng(seed)
    logu = np.exp(rng.uniform(np.log(1e-6), np.log(1e3), 4096)).astype(np.float32)
    return special, np.concatenate([np.resize(special, special.size * 256), logu])


def ulp_distance(got_f32, want_f64):
    """|got - want| in units of the f32 spacing at want (finite entries only; the caller pairs up the NaN)"""
    want32 = np.abs(np.asarray(want_f64)).astype(np.float32)
    return np.abs(got_f32.astype(np.float64) - want_f64) / np.spacing(want32).astype(np.float64)


def reconcile_bound(n_s, k_roundings, mass):
    """|film - sum of sensor_reference| per pixel and channel, for n_s samples summed in f32 in any order, each after at most k_roundings
    roundings of a term of its mass (the derivation is in tests/test_film_log_gpu.py)."""
    return (n_s + k_roundings) * U * mass * (1.0 + 1e-3) + ABS_FLOOR
