"""CPU-side checks of adaptive sampling (include/mi355pt_adaptive.h): the ABI surface and the argument checks — none of which needs a
device — and the NumPy restatement of the noise estimate and the step (tests/adaptive_reference.py) against properties that follow from
the header's definition.  The GPU kernels are compared with that restatement in tests/test_adaptive_gpu.py."""
import ctypes
import importlib.util
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adaptive_reference as ar  # noqa: E402

DTYPES = [np.float32, np.float64]


# ---------------------------------------------------------------- ABI
def test_header_declares_and_library_exports_adaptive_sampling(pkg):
    """mi355pt.h declares mi355pt_render_accum_tiles_device and includes mi355pt_adaptive.h, which declares the two structs and five functions;
    the library exports them; the ctypes mirrors and the generated Rust binding have the header's layouts and argument counts."""
    inc = os.path.join(pkg.ffi.ROOT, "include")
    main = open(os.path.join(inc, "mi355pt.h")).read()
    assert re.search(r'^#include "mi355pt_adaptive.h"', main, flags=re.M)
    assert "render_accum_tiles_device" in pkg.ffi.ABI_SYMBOLS
    spec = importlib.util.spec_from_file_location("gen_rust_binding", os.path.join(pkg.ffi.ROOT, "tools", "gen_rust_binding.py"))
    g = importlib.util.module_from_spec(spec); spec.loader.exec_module(g)
    structs, funcs, _, _ = g.parse_header(os.path.join(inc, "mi355pt_adaptive.h"))
    assert structs == {"mi355pt_adaptive_params": [("threshold", "float", None), ("dark_eps", "float", None), ("min_spp", "uint32_t", None)],
                       "mi355pt_adaptive_result": [("passes", "uint32_t", None), ("tiles_at_max", "uint32_t", None), ("total_samples", "uint64_t", None)]}
    declared = sorted(name for name, _, _ in funcs)
    assert declared == sorted("mi355pt_" + s for s in pkg.ffi.ADAPTIVE_SYMBOLS) and len(declared) == 5
    lib = ctypes.CDLL(pkg.ffi.LIB_PATH)
    for name in declared + ["mi355pt_render_accum_tiles_device"]:
        assert hasattr(lib, name), f"{name} declared but not exported"
    rs = open(os.path.join(pkg.ffi.ROOT, "bindings", "rust", "mi355pt_sys.rs")).read()
    c_scalars = {"uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "float": ctypes.c_float}
    r_scalars = {"u32": ctypes.c_uint32, "u64": ctypes.c_uint64, "f32": ctypes.c_float}
    for cname, mirror, size in (("mi355pt_adaptive_params", pkg.ffi.AdaptiveParams, 12), ("mi355pt_adaptive_result", pkg.ffi.AdaptiveResult, 16)):
        m = re.search(r"pub struct %s \{(.*?)\n\}" % g.rust_struct_name(cname), rs, flags=re.S)
        assert m, cname

        class FromRust(ctypes.Structure):
            _fields_ = [(n, r_scalars[t]) for n, t in re.findall(r"pub (\w+): (\w+),", m.group(1))]

        class FromHeader(ctypes.Structure):
            _fields_ = [(n, c_scalars[t]) for n, t, _ in structs[cname]]
        assert ctypes.sizeof(FromRust) == ctypes.sizeof(FromHeader) == ctypes.sizeof(mirror) == size, cname
        assert [n for n, _ in mirror._fields_] == [n for n, _, _ in structs[cname]]
        for n, _ in mirror._fields_:
            assert getattr(FromRust, n).offset == getattr(FromHeader, n).offset == getattr(mirror, n).offset, (cname, n)
    for name, _, args in funcs:
        fm = re.search(r"pub fn %s\((.*?)\)" % name, rs)
        assert fm, f"{name} missing from the Rust binding"
        assert len([a for a in fm.group(1).split(",") if a.strip()]) == len(args), name


def test_scratch_size(pkg):
    prod = pkg.Product()
    for w, h in ((1, 1), (9, 7), (44, 20), (130, 70), (1920, 1080)):
        tiles = ((w + 7) // 8) * ((h + 7) // 8)
        b = prod.adaptive_scratch_bytes(w, h)
        assert b >= tiles * 4 + 4 and b % 16 == 0, (w, h, b)             # a flag per tile and the drivers' count
    assert prod.adaptive_scratch_bytes(0, 5) == 0 and prod.adaptive_scratch_bytes(5, 0) == 0
    assert prod.adaptive_scratch_bytes(2 ** 20, 2 ** 20) == 0             # 2^34 tiles


def test_invalid_arguments_are_refused_without_a_device(pkg):
    """A zeroed params struct and each bad field, and every other MI355PT_E_INVALID case of mi355pt_adaptive_step_device and
    mi355pt_film_normalize_tiles_device: -1 with a message, before anything touches the device (without a GPU the pointers are made-up
    addresses the checks never dereference; there is deliberately no valid call with them)."""
    prod = pkg.Product()
    lib, f = prod.lib, pkg.ffi
    import torch
    W, H = 44, 20
    need = prod.adaptive_scratch_bytes(W, H)
    ptrs = [0x10000 * (i + 1) for i in range(7)]
    if torch.cuda.device_count() > 0:        # the suite on a GPU box: real buffers, so that not even a mistake in this test could reach a bad address
        keep = [torch.zeros(max(need, W * H * 12), dtype=torch.uint8, device="cuda") for _ in range(7)]
        ptrs = [t.data_ptr() for t in keep]
    F, Hf, SPP, ERR, S, L, CNT = ptrs

    def params(**kw):
        p = f.AdaptiveParams(0.05, 1e-3, 4)
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    good = params()

    def step(film=F, half=Hf, w=W, h=H, spp=SPP, err=ERR, p=good, level=4, mx=64, s=S, sbytes=need, lst=L, cnt=CNT):
        vp = ctypes.c_void_p
        return lib.mi355pt_adaptive_step_device(vp(film), vp(half), w, h, vp(spp), vp(err), ctypes.byref(p) if p is not None else None, level, mx,
                                                vp(s), sbytes, vp(lst), vp(cnt), None)
    cases = {
        "zeroed params": dict(p=f.AdaptiveParams()),
        "threshold 0": dict(p=params(threshold=0.0)), "threshold < 0": dict(p=params(threshold=-1.0)),
        "threshold nan": dict(p=params(threshold=float("nan"))), "threshold inf": dict(p=params(threshold=float("inf"))),
        "dark_eps 0": dict(p=params(dark_eps=0.0)), "dark_eps < 0": dict(p=params(dark_eps=-1e-3)), "dark_eps nan": dict(p=params(dark_eps=float("nan"))),
        "dark_eps inf": dict(p=params(dark_eps=float("inf"))),
        "min_spp 0": dict(p=params(min_spp=0)), "min_spp 1": dict(p=params(min_spp=1)), "min_spp 6": dict(p=params(min_spp=6)),
        "null params": dict(p=None), "null film": dict(film=0), "null half": dict(half=0), "null tile_spp": dict(spp=0), "null tile_err": dict(err=0),
        "null list": dict(lst=0), "null count": dict(cnt=0), "null scratch": dict(s=0), "scratch too small": dict(sbytes=need - 1),
        "scratch misaligned": dict(s=S + 2), "width 0": dict(w=0), "height 0": dict(h=0), "level 0": dict(level=0), "level odd": dict(level=3),
        "max below level": dict(level=8, mx=4),
    }
    for name, kw in cases.items():
        assert step(**kw) == -1, name
        assert len(lib.mi355pt_last_error()) > 0 and b"adaptive" in lib.mi355pt_last_error(), name
    vp = ctypes.c_void_p
    for name, args in {"null film": (0, SPP, W, H, Hf), "null spp": (F, 0, W, H, Hf), "null mean": (F, SPP, W, H, 0), "width 0": (F, SPP, 0, H, Hf),
                       "height 0": (F, SPP, W, 0, Hf)}.items():
        assert lib.mi355pt_film_normalize_tiles_device(vp(args[0]), vp(args[1]), args[2], args[3], vp(args[4]), None) == -1, name
        assert b"normalize" in lib.mi355pt_last_error(), name
    with pytest.raises(RuntimeError, match="min_spp"):                      # and through the Python wrapper
        prod.adaptive_step_device(F, Hf, W, H, SPP, ERR, params(min_spp=3), 4, 64, S, need, L, CNT)


# ---------------------------------------------------------------- the restatement
def films(shape, value=None, seed=0):
    h, w = shape
    rng = np.random.default_rng(seed)
    return (np.full((h, w, 3), value, np.float32) if value is not None else rng.uniform(0.05, 20.0, (h, w, 3)).astype(np.float32))


@pytest.mark.parametrize("dtype", DTYPES)
def test_constant_films_have_no_error(dtype):
    """F = n c and H = (n / 2) c for a constant c: m = h exactly (n and n / 2 are powers of two), so every e_p and e_t is exactly 0"""
    for (w, h) in ((1, 1), (9, 7), (44, 20)):
        tx, ty = ar.tiles_of(w, h)
        n = 16
        F = films((h, w), 0.75 * n); Hh = films((h, w), 0.75 * (n // 2))
        e = ar.tile_errors(F, Hh, np.full(tx * ty, n, np.uint32), 1e-3, dtype)
        assert e.dtype == dtype and np.array_equal(e, np.zeros(tx * ty, dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_film_twice_the_half_has_no_error(dtype):
    """F = 2 H exactly (a power-of-two scale is exact in binary32): the second half of the samples brought what the first did, error 0 —
    whatever the values, negative and zero channels included"""
    w, h, n = 44, 20, 8
    Hh = films((h, w), seed=3); Hh[2::5] *= -1; Hh[::7] = 0
    F = (Hh * np.float32(2)).astype(np.float32)
    tx, ty = ar.tiles_of(w, h)
    e = ar.tile_errors(F, Hh, np.full(tx * ty, n, np.uint32), 1e-3, dtype)
    assert np.array_equal(e, np.zeros(tx * ty, dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_scaling_both_films_by_four_doubles_the_error(dtype):
    """e_p = d / sqrt(s) with d linear and s linear (dark_eps negligible: 1e-30 against sums of 0.15 and more) in the films: 4 x the films =
    2 x the error, exactly up to the roundings of one square root and one quotient per pixel and of the division by the count — the scale
    by 4 itself is exact, and so is the doubling through the sums.  Bound: 4 eps relative."""
    w, h, n = 44, 20, 8
    F, Hh = films((h, w), seed=1), (films((h, w), seed=2) * np.float32(0.5)).astype(np.float32)
    tx, ty = ar.tiles_of(w, h)
    spp = np.full(tx * ty, n, np.uint32)
    e1 = ar.tile_errors(F, Hh, spp, 1e-30, dtype)
    e4 = ar.tile_errors(F * np.float32(4), Hh * np.float32(4), spp, 1e-30, dtype)
    assert (e1 > 0).all()
    assert np.all(np.abs(e4 - 2 * e1) <= 4 * float(np.finfo(dtype).eps) * 2 * e1)


@pytest.mark.parametrize("dtype", DTYPES)
def test_partial_tiles_average_over_in_frame_pixels_only(dtype):
    """44 x 20: the last tile column is 4 pixels wide, the last row 4 tall.  With the same e_p on every pixel, every tile — whole, narrow,
    short or the 4 x 4 corner — has e_t = e_p (a mean over 64, 32, 32 or 16 equal values: sums of a power-of-two count of equal values and the
    division are exact); a mean over 64 slots would give a half or a quarter of it."""
    w, h, n = 44, 20, 4
    tx, ty = ar.tiles_of(w, h)
    assert (tx, ty) == (6, 3) and sorted(set(ar.in_frame(w, h).sum(1))) == [16, 32, 64]
    F = films((h, w), 2.0 * n); Hh = films((h, w), 1.0 * (n // 2))
    e = ar.tile_errors(F, Hh, np.full(tx * ty, n, np.uint32), 1e-3, dtype)
    dt = np.dtype(dtype).type
    e_p = (dt(1) + dt(1) + dt(1)) / np.sqrt(dt(6) + dt(np.float32(1e-3)))
    assert np.array_equal(e, np.full(tx * ty, e_p, dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_pixel_makes_its_tile_active_up_to_the_maximum(dtype):
    w, h, n = 44, 20, 8
    tx, ty = ar.tiles_of(w, h)
    F = films((h, w), 0.5 * n); Hh = films((h, w), 0.5 * (n // 2))
    F[9, 41, 2] = np.nan                                                     # tile 1 * 6 + 5, in the narrow column
    spp0 = np.full(tx * ty, n, np.uint32)
    half2, spp, err, lst, active = ar.step(F, Hh, spp0, np.zeros(tx * ty, np.float32), 0.05, 1e-3, n, 64, dtype)
    assert lst.tolist() == [11] and np.isnan(err[11]) and np.array_equal(np.delete(err, 11), np.zeros(tx * ty - 1, dtype))
    assert spp[11] == 2 * n and np.array_equal(np.delete(spp, 11), np.delete(spp0, 11))
    assert np.array_equal(half2[8:16, 40:44].view(np.uint32), F[8:16, 40:44].view(np.uint32))      # H := F on the tile's in-frame pixels
    mask = np.ones((h, w), bool); mask[8:16, 40:44] = False
    assert np.array_equal(half2[mask], Hh[mask])
    # at the maximum nothing is active, NaN or not, and the error is still written
    _, spp, err, lst, _ = ar.step(F, Hh, spp0, np.zeros(tx * ty, np.float32), 0.05, 1e-3, n, n, dtype)
    assert lst.size == 0 and np.array_equal(spp, spp0) and np.isnan(err[11])


def test_step_leaves_other_counts_alone_and_synthetic_decisions_are_unambiguous():
    """The synthetic frames of the GPU test: every tile at the level is at most half the threshold or at least twice it (or NaN) in the float64
    restatement, both classes occur, float32 and float64 decide alike, and tiles at other counts keep their error, count and half film."""
    thr, eps, level = 0.05, 1e-3, 8
    for (w, h) in ((1, 1), (9, 7), (44, 20), (130, 70)):
        F, Hh, spp, err0 = ar.synthetic(w, h, level, thr, eps)
        e64 = ar.tile_errors(F, Hh, np.where(spp == level, spp, 2), eps, np.float64)[spp == level]
        assert np.all(np.isnan(e64) | (e64 <= thr / 2) | (e64 >= 2 * thr)), (w, h)
        if w * h > 64:
            assert (e64 <= thr / 2).any() and (e64 >= 2 * thr).any() and np.isnan(e64).sum() == 1
        r32 = ar.step(F, Hh, spp, err0, thr, eps, level, 64, np.float32)
        r64 = ar.step(F, Hh, spp, err0, thr, eps, level, 64, np.float64)
        assert np.array_equal(r32[3], r64[3]) and np.array_equal(r32[1], r64[1])
        other = spp != level
        assert np.array_equal(r32[1][other], spp[other]) and np.array_equal(r32[2][other], err0[other])
        assert ar.rel_err(r32[2], r64[2]) < 1e-5
