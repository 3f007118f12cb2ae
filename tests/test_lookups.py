"""CPU tests that pin the REFERENCE side of the texture and environment-map lookups before the GPU is compared with it
(tests/test_lookups_gpu.py): the oracle's own functions (through the probes of tests/lookup_reference.cpp) against the plain NumPy
restatements of tests/lookup_reference.py, the properties an environment light's pdf and sampler must have, and the oracle's faithful mode
against its fast mode on every scene of tests/lookup_cases.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lookup_cases as lc  # noqa: E402
import lookup_reference as lr  # noqa: E402

F = np.float32
CONTENTS = ["noise", "seamless"]


@pytest.fixture(scope="module")
def ref():
    return lr.LookupReference()


@pytest.fixture(scope="module")
def uvs():
    """20 000 UVs in [-4, 4]^2, then the planted constant values and the corners of every UV set"""
    rng = np.random.default_rng(31)
    planted = list(lc.CONSTANT_UVS) + [(u, v) for (u0, u1, v0, v1) in lc.UV_SETS.values() for u in (u0, u1) for v in (v0, v1)]
    return np.concatenate([rng.uniform(-4.0, 4.0, (20000, 2)), np.array(planted)]).astype(F)


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("size", lc.TEX_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_bilinear_matches_numpy(ref, uvs, size, content):
    """The oracle's bilinear_sample_rgb against sampler.rs:6-45 restated in NumPy.  The texels read are equal: the first and last column and
    row that carry weight in the oracle's lookup (measured from outside, on one-hot textures) are x0, x1 (x0 alone where fx == 0), y0, y1 of
    the restatement, and the weights it gave them are the restatement's to an ulp.  The values agree within 1e-6 absolute: three nested
    float32 lerps of values <= 1 are at most 9 roundings of 2^-24, about 5.4e-7."""
    img = lc.texture(size, content)
    got = ref.bilinear(img, uvs)
    want, (x0, y0, x1, y1, fx, fy) = lr.bilinear_numpy(img, uvs)
    assert np.isfinite(got).all() and got.min() >= 0.0 and got.max() <= 1.0 + 1e-6
    assert np.abs(got - want).max() <= 1e-6, np.abs(got - want).max()
    if content == "noise":                                   # (the footprint depends on the size alone)
        idx, wt = ref.footprint(size, uvs)
        assert np.array_equal(idx[:, 0], x0) and np.array_equal(idx[:, 1], y0)
        assert np.array_equal(idx[:, 2], np.where(fx > 0, x1, x0)) and np.array_equal(idx[:, 3], np.where(fy > 0, y1, y0))
        one = x1 == x0                                       # a single column (w == 1, or the clamp at the last one) carries both weights
        wx_lo = np.where(one | (fx == 0), 1.0, 1.0 - fx.astype(np.float64)); wx_hi = np.where(one | (fx == 0), 1.0, fx.astype(np.float64))
        one = y1 == y0
        wy_lo = np.where(one | (fy == 0), 1.0, 1.0 - fy.astype(np.float64)); wy_hi = np.where(one | (fy == 0), 1.0, fy.astype(np.float64))
        for k, w in enumerate((wx_lo, wy_lo, wx_hi, wy_hi)):
            assert np.abs(wt[:, k] - w).max() <= 4 * 2.0 ** -24, (k, np.abs(wt[:, k] - w).max())
    # the wrap itself, on the planted values: integer v lands on row h - 1, integer u on column 0, and -0.0 is 0.0
    h, w = size
    for (u, v) in [(0.0, 0.0), (-0.0, -0.0), (1.0, 1.0), (-1.0, -1.0), (1.0, 0.0), (0.0, 1.0)]:
        assert np.abs(ref.bilinear(img, [(u, v)])[0] - img[h - 1, 0] / 255.0).max() <= 1e-6
    assert np.abs(ref.bilinear(img, [(2.0, 0.5)])[0] - lr.bilinear_numpy(img, [(0.0, -0.5)])[0][0]).max() <= 1e-6   # repeat and mirror


@pytest.mark.parametrize("flip_y", [0, 1])
@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("size", lc.TEX_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_normal_map_matches_numpy(ref, uvs, size, content, flip_y):
    """sample_normal_map against normal_texture.rs:39-66 restated, on the unit normal.  The bound follows the arithmetic: the components
    before the normalisation carry 2 x 5.4e-7 (the bilinear value, doubled) + 2^-24, the normalisation divides that by the length |n| it
    removes, and three more normalisations (Normal::new, Normal::from) add 2^-23 each: 2.5e-6 / |n| + 5e-7 per component."""
    img = lc.texture(size, content)
    got = ref.normal_map(img, flip_y, uvs)
    want, ln = lr.normal_map_numpy(img, flip_y, uvs)
    ok = ln > 1e-4                                          # (a blend within 1e-4 of mid-grey in all three channels: none occurs)
    assert ok.all()
    assert np.abs(np.linalg.norm(got.astype(np.float64), axis=1) - 1.0).max() <= 4 * 2.0 ** -24
    err = np.abs(got - want).max(axis=1)
    assert np.all(err <= 2.5e-6 / ln + 5e-7), float((err * ln).max())


ENV_MAPS = [(s, "noise") for s in lc.ENV_SIZES] + [((6, 9), "sun"), ((17, 33), "tophalf"), ((7, 5), "black")]
ENV_IDS = [f"{c}_{s[0]}x{s[1]}" for s, c in ENV_MAPS]


def _inner_directions(env_np, rng, per_texel=4):
    """render-space directions inside every texel, between 10 % and 90 % of its extent: the floor in calculate_direction_pdf cannot flip"""
    ys, xs = np.mgrid[0:env_np.h, 0:env_np.w]
    xs, ys = np.repeat(xs.ravel(), per_texel), np.repeat(ys.ravel(), per_texel)
    u = (xs + rng.uniform(0.1, 0.9, xs.size)) / env_np.w; v = (ys + rng.uniform(0.1, 0.9, ys.size)) / env_np.h
    return env_np.direction(u, v), xs, ys


@pytest.mark.parametrize("xf", ["id", "rot"])
@pytest.mark.parametrize("size,content", ENV_MAPS, ids=ENV_IDS)
def test_environment_matches_numpy(ref, size, content, xf):
    """EnvLight::build, direction_pdf, the sampler and sample_texture against environment_light.rs restated: sampled texels equal, floats
    within 1e-5 relative (float32 running sums of at most 64 terms against float64 ones).  The pdf is asked inside the texels and the sampler
    away from the CDF's steps, where the answer does not hang on an ulp."""
    rgb, M = lc.env_map(size, content), lc.TRANSFORMS[xf]
    probe, env = ref.env(rgb, M), lr.EnvNumpy(rgb, M)
    marg, cond, total = probe.tables()
    assert np.allclose(marg, env.marginal, rtol=1e-5, atol=0.0) and np.allclose(cond, env.conditional, rtol=1e-5, atol=0.0)
    assert np.isclose(total, env.total_weight, rtol=1e-5, atol=0.0)
    if content == "black":
        assert total == 0.0 and np.array_equal(marg, ((np.arange(size[0]) + 1.0) / size[0]).astype(F)) and not cond.any()
    rng = np.random.default_rng(17)
    dirs, xs, ys = _inner_directions(env, rng)
    tx, ty, _ = env.texel_of(dirs)
    assert np.array_equal(tx, xs) and np.array_equal(ty, ys)              # (the restatement finds the texel the direction was made in)
    assert np.allclose(probe.pdf(dirs), env.pdf(dirs), rtol=1e-5, atol=0.0)
    # the sampler: three points inside every step of the marginal CDF x three inside every step of that row's conditional CDF
    if total > 0.0:
        us = []
        for y in range(env.h):
            lo, hi = (env.marginal[y - 1] if y else 0.0), env.marginal[y]
            if hi - lo <= 1e-4:
                continue
            for x in range(env.w):
                clo, chi = (env.conditional[y, x - 1] if x else 0.0), env.conditional[y, x]
                if chi - clo > 1e-4:
                    us += [(lo + a * (hi - lo), clo + b * (chi - clo)) for a in (0.25, 0.5, 0.75) for b in (0.25, 0.5, 0.75)]
        us = np.array(us, F)
        texel, wi, pdf = probe.sample(us)
        assert np.array_equal(texel, env.sample(us))
        centre = env.centre_direction(texel[:, 0], texel[:, 1])
        assert np.abs(wi - centre).max() <= 1e-6                         # sample() goes to the centre of the texel the two searches found
        assert np.allclose(pdf, env.pdf(centre), rtol=1e-5, atol=0.0) and np.all(pdf > 0.0)
    # sample_texture (:124-160): the bilinear lookup over (w - 1, h - 1), clamped
    uv = np.concatenate([rng.uniform(-0.2, 1.2, (2000, 2)), [(0.0, 0.0), (1.0, 1.0), (0.5, 0.5), (1.0, 0.0)]]).astype(F)
    u, v = np.clip(uv[:, 0], F(0), F(1)), np.clip(uv[:, 1], F(0), F(1))
    x, y = (u * F(size[1] - 1)).astype(F), (v * F(size[0] - 1)).astype(F)
    x0, y0 = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, size[1] - 1), np.minimum(y0 + 1, size[0] - 1)
    fx, fy = (x - x0.astype(F)).astype(np.float64)[:, None], (y - y0.astype(F)).astype(np.float64)[:, None]
    t = rgb.astype(np.float64)
    want = (t[y0, x0] * (1 - fx) + t[y0, x1] * fx) * (1 - fy) + (t[y1, x0] * (1 - fx) + t[y1, x1] * fx) * fy
    assert np.allclose(probe.sample_texture(uv), want, rtol=1e-5, atol=1e-5 * float(rgb.max()))


@pytest.mark.parametrize("xf", ["id", "rot"])
@pytest.mark.parametrize("size,content", [m for m in ENV_MAPS if m[1] != "black"], ids=[i for i in ENV_IDS if not i.startswith("black")])
def test_environment_properties(ref, size, content, xf):
    """The oracle alone.  The pdf integrates to one: sum over the texels of pdf(centre) sin(theta) (pi / h) (2 pi / w) = 1 within 1e-4.  And
    for u in (0, 1) the sampler never returns a texel of zero weight — random u, and u on, just below and just above every value of the CDFs."""
    rgb, M = lc.env_map(size, content), lc.TRANSFORMS[xf]
    h, w = size
    probe, env = ref.env(rgb, M), lr.EnvNumpy(rgb, M)
    ys, xs = np.mgrid[0:h, 0:w]
    theta = (ys.ravel() + 0.5) / h * np.pi
    pdf = probe.pdf(env.centre_direction(xs.ravel(), ys.ravel())).astype(np.float64)
    total = float((pdf * np.sin(theta)).sum() * (np.pi / h) * (2.0 * np.pi / w))
    assert abs(total - 1.0) <= 1e-4, total
    marg, cond, _ = probe.tables()
    rng = np.random.default_rng(23)
    edge = lambda c: np.concatenate([c, np.nextafter(c, F(0)), np.nextafter(c, F(1))])
    um, uc = edge(marg), edge(cond.ravel())
    u = np.concatenate([rng.uniform(0.0, 1.0, (20000, 2)), np.stack([um[rng.integers(0, um.size, 20000)], uc[rng.integers(0, uc.size, 20000)]], 1),
                        np.stack([um[rng.integers(0, um.size, 5000)], rng.uniform(0.0, 1.0, 5000)], 1)]).astype(F)
    u = u[np.all((u > 0.0) & (u < 1.0), axis=1)]
    texel, _, pdf = probe.sample(u)
    weight = env.weight[texel[:, 1], texel[:, 0]]
    assert np.all(weight > 0.0), int((weight == 0.0).sum())
    assert np.all(pdf > 0.0)


@pytest.fixture(scope="module")
def srgb(pkg):
    return pkg.scenes.srgb_table()


@pytest.mark.parametrize("name", lc.NAMES + [lc.TWIN])
def test_oracle_fast_equals_faithful(oracle, pkg, srgb, name):
    """Every lookup scene at 48 x 36 x 4 spp under pt, nee and mis: the oracle's fast mode renders the film of its faithful mode bit for bit
    (no sample is left out on these inputs: they are well defined), the films are finite, and something is lit."""
    sc, cam, _ = lc.build_scene(oracle, name, 48, 36)
    for strategy in ("pt", "nee", "mis"):
        prm = pkg.make_params(4, strategy, "sobol")
        films = []
        for faithful in (True, False):
            oracle.set_faithful(sc, faithful)
            films.append(oracle.render(sc, cam, prm))
        assert np.isfinite(films[0]).all()
        assert np.array_equal(films[0], films[1])
        assert films[0].mean() > 1e-3, (strategy, films[0].mean())
