"""GPU tests of the texture and environment-map lookups (fetch_texel, bilinear_rgb, rgb2spec_lookup, eval_spectrum of csrc/pt_device.hpp;
env_spherical, env_radiance, env_pdf, env_sample_cdf, env_sample of csrc/pt_path.hpp; the CDF build of csrc/scene_lower.cpp and the host's
intensity_avg of csrc/api_scene.cpp) on the cases of tests/lookup_cases.py: odd and one-texel-wide textures at odd texel offsets, wrapped,
mirrored and seam-crossing UVs, tiny, tall, partly and wholly black environment maps under a general rotation.  The reference side of every
comparison is pinned on the CPU by tests/test_lookups.py; every bar is one the project already holds (tests/test_aov_gpu.py,
tests/test_parity_gpu.py).  One line per comparison goes to the file MI355PT_FRAME_LOG names (profiles/lookup_parity.jsonl)."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aov_reference  # noqa: E402
import lookup_cases as lc  # noqa: E402
from test_aov_gpu import FRAME_BAR, PER_SAMPLE_MIN, TIGHT_MIN  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref():
    return aov_reference.AovReference()


@pytest.fixture(scope="module")
def scenes(product, oracle, ref):
    """(case, side) -> (scene, camera, d65), built once; side: "gpu" | "cpu" (the oracle, fast mode) | "aov" (AovReference)"""
    cache = {}
    backends = {"gpu": product, "cpu": oracle, "aov": ref}

    def get(name, side):
        if (name, side) not in cache:
            cache[name, side] = lc.build_scene(backends[side], name)
            if side != "gpu":
                backends[side].set_faithful(cache[name, side][0], False)      # (faithful == fast on every case: tests/test_lookups.py)
        return cache[name, side]
    return get


def sized(cam, w, h, pkg):
    c = pkg.ffi.Camera.from_buffer_copy(cam)
    c.width, c.height = w, h
    return c


def log_line(record):
    if os.environ.get("MI355PT_FRAME_LOG"):
        with open(os.environ["MI355PT_FRAME_LOG"], "a") as f:
            f.write(json.dumps(record) + "\n")


@pytest.mark.parametrize("name,kind", [("lambert_albedo", "albedo"), ("simple_pbr", "albedo"), ("clearcoat", "albedo"), ("lambert_normal", "shading_normal"),
                                       ("simple_pbr", "shading_normal")])
def test_aov_per_lookup(product, ref, pkg, scenes, name, kind):
    """One pixel = one lookup (256 x 192 at 1 spp, Sobol): the albedo AOV of the walls with a textured base colour and the shading-normal
    AOV of the normal-mapped walls against the CPU reference, with the two per-sample bars of tests/test_aov_gpu.py.  A wrong texel of a
    base colour is a wrong pixel.  The shading-normal AOV shows the interpolated normal BEFORE the normal map (the extension follows
    normal_renderer.rs, which never reads one): on these walls it pins the quads, not the map.  The normal-map lookup itself is compared
    through the light it turns, by test_per_sample_radiance and test_frames on the same walls."""
    k = pkg.ffi.AOV[kind]
    prm = pkg.make_params(1, "mis", "sobol")
    (sg, cg, dg), (sc, cc, dc) = scenes(name, "gpu"), scenes(name, "aov")
    g = product.render_aov(sg, cg, prm, k, dg)
    c = ref.render_aov(sc, cc, prm, k, dc)
    assert np.array_equal(np.isnan(g), np.isnan(c))
    d = np.abs(g - c)
    close = np.all(d <= 1e-3 * np.abs(c) + 1e-4, axis=2)
    tight = np.all(d <= 1e-5, axis=2)
    log_line({"test": "aov", "case": name, "kind": kind, "close": round(float(close.mean()), 6), "tight": round(float(tight.mean()), 6),
              "bit_equal": round(float(np.all(g == c, axis=2).mean()), 6), "max_dev": float(f"{d.max():.3e}")})
    print(name, kind, "close", close.mean(), "tight", tight.mean(), "max", d.max())
    assert c.std() > 0.05                                   # (the wall is in the picture)
    assert close.mean() >= PER_SAMPLE_MIN, close.mean()
    assert tight.mean() >= TIGHT_MIN, tight.mean()


@pytest.mark.parametrize("strategy", ["pt", "nee", "mis"])
@pytest.mark.parametrize("name", lc.NAMES)
def test_per_sample_radiance(pkg, scenes, name, strategy):
    """Every material family and every environment case: the spectral radiance of 20 000 (x, y, sample) triples, strategy by strategy (the
    reference samples an environment map at texel centres only, so on small maps pt, nee and mis legitimately disagree with each other).  The
    assertions of test_per_sample_radiance_parity (tests/test_parity_gpu.py) with PER_SAMPLE_MIN."""
    rng = np.random.default_rng(41)
    n = 20000
    xys = np.stack([rng.integers(0, lc.W, n), rng.integers(0, lc.H, n), rng.integers(0, 64, n)], 1).astype(np.uint32)
    prm = pkg.make_params(64, strategy, "sobol")
    (sg, cg, _), (sc, cc, _) = scenes(name, "gpu"), scenes(name, "cpu")
    Lg, lg, pg = sg.probe_radiance(cg, prm, xys)
    Lc, lc_, pc = sc.probe_radiance(cc, prm, xys)
    # The reference accumulates NaN samples without complaint (sensor.rs:42 only logs), and the glass wall, whose roughness map holds texels
    # of 0 and 1 / 255, makes a few in 20 000 (as scene 11 does, tests/test_parity_gpu.py): a NaN sample agrees with a NaN sample, and the
    # means are taken over the samples that are numbers on the CPU
    with np.errstate(invalid="ignore"):
        d = np.abs(Lg - Lc)
        close = np.all((d <= 1e-3 * np.abs(Lc) + 1e-4) | (np.isnan(Lg) & np.isnan(Lc)), axis=1)
    num = ~np.isnan(Lc).any(axis=1)
    mean_g, mean_c = float(Lg[num].mean()), float(Lc[num].mean())
    log_line({"test": "radiance", "case": name, "strategy": strategy, "close": round(float(close.mean()), 6), "mean_gpu": float(f"{mean_g:.6e}"),
              "mean_cpu": float(f"{mean_c:.6e}"), "max_dev": float(f"{np.nanmax(d):.3e}"), "nan_cpu": int((~num).sum()),
              "same_wavelengths": bool(np.array_equal(lg, lc_)), "same_termination": bool(np.array_equal(pg, pc))})
    print(name, strategy, "close", close.mean(), "means", mean_g, mean_c, "nan", int((~num).sum()))
    assert np.array_equal(lg, lc_)              # wavelengths come straight from Sobol bits
    assert np.array_equal(pg, pc)
    assert mean_c > 0.0 and (~num).sum() <= 20
    assert close.mean() >= PER_SAMPLE_MIN, close.mean()
    assert abs(mean_g - mean_c) <= 1e-3 * mean_c


@pytest.mark.parametrize("strategy", ["pt", "nee", "mis"])
@pytest.mark.parametrize("name", lc.NAMES)
def test_frames(product, oracle, pkg, scenes, name, strategy):
    """64 x 48 at 64 spp against the oracle in fast mode: FRAME_BAR as it stands for test_frames_match_the_oracle_sample_for_sample."""
    prm = pkg.make_params(64, strategy, "sobol")
    (sg, cg, _), (sc, cc, _) = scenes(name, "gpu"), scenes(name, "cpu")
    g = product.render(sg, sized(cg, 64, 48, pkg), prm)
    c = oracle.render(sc, sized(cc, 64, 48, pkg), prm)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(np.isnan(g), np.isnan(c))
        d = np.nan_to_num(g - c)
    rmse = float(np.sqrt(np.mean(d ** 2)))
    off = int((np.abs(d).max(axis=2) > 0.01).sum())
    log_line({"test": "frame", "case": name, "strategy": strategy, "rmse": float(f"{rmse:.3e}"), "off": off, "nan_px": int(np.isnan(g).any(axis=2).sum()),
              "mean": round(float(np.nanmean(c)), 4)})
    print(name, strategy, "rmse", rmse, "off", off)
    assert rmse <= FRAME_BAR[0] and off <= FRAME_BAR[1], (rmse, off)


def test_texel_offsets(product, pkg, scenes):
    """All sixteen textures in one scene, laid end to end at offsets that are a multiple of nothing, and the twin that adds the same textures
    in reverse order: other ids, other offsets, the same picture.  The films are bit-equal at 16 spp under mis; only the offset arithmetic
    (t.offset + y * t.w + x) stands between them."""
    prm = pkg.make_params(16, "mis", "sobol")
    sa, ca, _ = scenes("lambert_albedo", "gpu")
    sb, cb, _ = scenes(lc.TWIN, "gpu")
    a, b = product.render(sa, ca, prm), product.render(sb, cb, prm)
    differ = int((a != b).any(axis=2).sum())
    log_line({"test": "texel_offsets", "pixels_differing": differ, "mean": round(float(a.mean()), 4)})
    assert np.isfinite(a).all() and a.std() > 0.01
    assert np.array_equal(a, b), differ


@pytest.mark.parametrize("name", lc.ENV_NAMES + ["emissive"])
def test_device_tables(product, name):
    """What was uploaded is what the host lowered (texels, marginal and conditional CDFs, DevEnv records, the emitters' materials with their
    light-pick intensity): the digests of the device's arrays equal the digests of the host lowering, which the CPU tests pin."""
    sc, cam, _ = lc.build_scene(product, name, builder="host")
    got, want = sc.debug_device_digest(), sc.debug_lowering_digest(cam)
    differ = [n for n in want[0] if got[0].get(n) != want[0][n]]
    log_line({"test": "device_tables", "case": name, "arrays": len(want[0]), "differ": differ})
    assert list(got[0]) == list(want[0]) and not differ and got[1] == want[1]
