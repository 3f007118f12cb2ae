"""CPU-side checks of the denoiser (include/mi355pt_denoise.h): the ABI surface, the argument checks — none of which needs a device — and the
NumPy restatement of the filter (tests/denoise_reference.py) against properties that follow from the filter's definition.  The GPU kernels are
compared with that restatement in tests/test_denoise_gpu.py."""
import ctypes
import importlib.util
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import denoise_reference as dr  # noqa: E402

F32_EPS = float(np.finfo(np.float32).eps)


def log_line(text):
    print(text)
    if os.environ.get("MI355PT_FRAME_LOG"):
        with open(os.environ["MI355PT_FRAME_LOG"], "a") as f:
            f.write(text + "\n")


# ---------------------------------------------------------------- ABI
def test_header_declares_and_library_exports_the_denoiser(pkg):
    """mi355pt.h includes mi355pt_denoise.h, which declares mi355pt_denoise_params and the four functions; the library exports them; the
    ctypes mirror and the generated Rust binding have the struct's layout and the functions' argument counts."""
    inc = os.path.join(pkg.ffi.ROOT, "include")
    main = open(os.path.join(inc, "mi355pt.h")).read()
    assert re.search(r'^#include "mi355pt_denoise.h"', main, flags=re.M)
    spec = importlib.util.spec_from_file_location("gen_rust_binding", os.path.join(pkg.ffi.ROOT, "tools", "gen_rust_binding.py"))
    g = importlib.util.module_from_spec(spec); spec.loader.exec_module(g)
    structs, funcs, _, _ = g.parse_header(os.path.join(inc, "mi355pt_denoise.h"))
    assert list(structs) == ["mi355pt_denoise_params"]
    assert structs["mi355pt_denoise_params"] == [("levels", "uint32_t", None), ("sigma_color", "float", None), ("sigma_normal", "float", None),
                                                 ("sigma_albedo", "float", None), ("albedo_eps", "float", None)]
    declared = sorted(name for name, _, _ in funcs)
    assert declared == sorted("mi355pt_" + s for s in pkg.ffi.DENOISE_SYMBOLS) and len(declared) == 4
    lib = ctypes.CDLL(pkg.ffi.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), f"{name} declared but not exported"
    P = pkg.ffi.DenoiseParams
    assert ctypes.sizeof(P) == 20
    assert [(n, getattr(P, n).offset) for n, _ in P._fields_] == [("levels", 0), ("sigma_color", 4), ("sigma_normal", 8), ("sigma_albedo", 12),
                                                                  ("albedo_eps", 16)]
    rs = open(os.path.join(pkg.ffi.ROOT, "bindings", "rust", "mi355pt_sys.rs")).read()
    m = re.search(r"pub struct DenoiseParams \{(.*?)\n\}", rs, flags=re.S)
    assert m and re.findall(r"pub (\w+): (\w+),", m.group(1)) == [("levels", "u32"), ("sigma_color", "f32"), ("sigma_normal", "f32"),
                                                                   ("sigma_albedo", "f32"), ("albedo_eps", "f32")]
    # the struct re-parsed from the Rust TEXT and laid out by C rules, against the header's struct and the ctypes mirror: size and every offset
    # (what tests/test_abi.py does for the structs of mi355pt.h)
    r_scalars = {"u32": ctypes.c_uint32, "f32": ctypes.c_float}
    c_scalars = {"uint32_t": ctypes.c_uint32, "float": ctypes.c_float}

    class FromRust(ctypes.Structure):
        _fields_ = [(n, r_scalars[t]) for n, t in re.findall(r"pub (\w+): (\w+),", m.group(1))]

    class FromHeader(ctypes.Structure):
        _fields_ = [(n, c_scalars[t]) for n, t, _ in structs["mi355pt_denoise_params"]]
    assert ctypes.sizeof(FromRust) == ctypes.sizeof(FromHeader) == ctypes.sizeof(P) == 20
    for n, _ in P._fields_:
        assert getattr(FromRust, n).offset == getattr(FromHeader, n).offset == getattr(P, n).offset, n
    for name, _, args in funcs:
        fm = re.search(r"pub fn %s\((.*?)\)" % name, rs)
        assert fm, f"{name} missing from the Rust binding"
        assert len([a for a in fm.group(1).split(",") if a.strip()]) == len(args), name


def test_defaults_and_scratch_size(pkg):
    prod = pkg.Product()
    d = prod.denoise_params_default()
    got = (d.levels, d.sigma_color, d.sigma_normal, d.sigma_albedo, d.albedo_eps)
    assert got == (5, 1.0, 0.5, float(np.float32(0.3)), float(np.float32(0.01)))
    assert {k: dr.DEFAULTS[k] for k in dr.DEFAULTS} == dict(levels=5, sigma_color=1.0, sigma_normal=0.5, sigma_albedo=0.3, albedo_eps=0.01)
    sizes = [(1, 1), (3, 2), (7, 5), (64, 1), (1, 64), (67, 35), (130, 70), (1920, 1080), (65536, 65536)]
    sizes.sort(key=lambda s: s[0] * s[1])
    b = [prod.denoise_scratch_bytes(w, h) for w, h in sizes]
    assert all(x > 0 for x in b)
    for (s0, b0), (s1, b1) in zip(zip(sizes, b), zip(sizes[1:], b[1:])):      # monotone in W * H
        assert b1 >= b0 and (b1 > b0 or s0[0] * s0[1] == s1[0] * s1[1]), (s0, s1)
    assert prod.denoise_scratch_bytes(64, 1) == prod.denoise_scratch_bytes(1, 64)
    assert prod.denoise_scratch_bytes(1920, 1080) >= 1920 * 1080 * 64        # the four 16-byte records per pixel of DESIGN.md 4.7


def test_invalid_arguments_are_refused_without_a_device(pkg):
    """Every MI355PT_E_INVALID case of mi355pt_denoise_device and mi355pt_denoise: -1 with a message, before anything touches the device
    (without a GPU the device pointers below are made-up addresses: every call here is refused by the argument checks, which never
    dereference them; there is deliberately no valid call with them)."""
    prod = pkg.Product()
    lib = prod.lib
    import torch
    W, H = 16, 8
    need = prod.denoise_scratch_bytes(W, H)
    B, A, N, S, O = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
    if torch.cuda.device_count() > 0:        # the suite on a GPU box: real buffers, so that not even a mistake in this test could reach a bad address
        keep = [torch.zeros(max(need, W * H * 12), dtype=torch.uint8, device="cuda") for _ in range(5)]
        B, A, N, S, O = (t.data_ptr() for t in keep)
    good = prod.denoise_params_default()

    def params(**kw):
        p = prod.denoise_params_default()
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def dev(b=B, sb=4, a=A, sa=64, n=N, sn=64, w=W, h=H, p=good, s=S, sbytes=need, o=O):
        return lib.mi355pt_denoise_device(ctypes.c_void_p(b), sb, ctypes.c_void_p(a), sa, ctypes.c_void_p(n), sn, w, h,
                                          ctypes.byref(p) if p is not None else None, ctypes.c_void_p(s), sbytes, ctypes.c_void_p(o), None)
    cases = {
        "levels 0": dict(p=params(levels=0)), "levels 9": dict(p=params(levels=9)),
        "zeroed params": dict(p=pkg.ffi.DenoiseParams()),
        "sigma_color 0": dict(p=params(sigma_color=0.0)), "sigma_color < 0": dict(p=params(sigma_color=-1.0)),
        "sigma_normal nan": dict(p=params(sigma_normal=float("nan"))), "sigma_albedo inf": dict(p=params(sigma_albedo=float("inf"))),
        "albedo_eps 0": dict(p=params(albedo_eps=0.0)), "albedo_eps nan": dict(p=params(albedo_eps=float("nan"))),
        "spp_beauty 0": dict(sb=0), "spp_albedo 0": dict(sa=0), "spp_normal 0": dict(sn=0),
        "width 0": dict(w=0), "height 0": dict(h=0),
        "null beauty": dict(b=0), "null out": dict(o=0), "null params": dict(p=None),
        "null scratch": dict(s=0), "scratch too small": dict(sbytes=need - 1), "scratch 0 bytes": dict(sbytes=0),
        "out = beauty": dict(o=B), "out = albedo": dict(o=A), "out = normal": dict(o=N),
    }
    for name, kw in cases.items():
        assert dev(**kw) == -1, name
        assert len(lib.mi355pt_last_error()) > 0 and b"denoise" in lib.mi355pt_last_error(), name
    # a buffer that is not given takes no spp: these are NOT refused for the spp, so they are only made in their refused-elsewhere form
    assert dev(a=0, sa=0, n=0, sn=0, p=params(levels=0)) == -1 and b"levels" in lib.mi355pt_last_error()
    # the host-buffer form: the same checks (scratch aside), before any allocation
    b = np.ones((H, W, 3), np.float32); out = np.zeros_like(b)
    fp = ctypes.POINTER(ctypes.c_float)

    def host(b_=b, sb=4, a_=b, sa=64, n_=b, sn=64, w=W, h=H, p=good, o_=out):
        ptr = lambda x: x.ctypes.data_as(fp) if x is not None else None   # noqa: E731
        return lib.mi355pt_denoise(ptr(b_), sb, ptr(a_), sa, ptr(n_), sn, w, h, ctypes.byref(p) if p is not None else None, ptr(o_))
    for name, kw in {"levels": dict(p=params(levels=0)), "zeroed": dict(p=pkg.ffi.DenoiseParams()), "sigma": dict(p=params(sigma_normal=-0.5)),
                     "spp": dict(sb=0), "spp_a": dict(sa=0), "spp_n": dict(sn=0), "width": dict(w=0), "height": dict(h=0), "beauty": dict(b_=None),
                     "out": dict(o_=None), "params": dict(p=None), "alias": dict(o_=b)}.items():
        assert host(**kw) == -1, name
        assert b"denoise" in lib.mi355pt_last_error(), name
    with pytest.raises(RuntimeError, match="levels"):                       # and through the Python wrapper
        prod.denoise(b, 4, params=params(levels=12))


# ---------------------------------------------------------------- the restatement
GUIDES = {"both": (True, True), "normal": (False, True), "albedo": (True, False), "none": (False, False)}


def run_ref(films, spps, guides, dtype, **kw):
    b, a, n = films
    use_a, use_n = GUIDES[guides]
    return dr.denoise(b, spps[0], a if use_a else None, spps[1], n if use_n else None, spps[2], dtype=dtype, **kw)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_constant_irradiance_is_a_fixed_point(dtype):
    """A constant irr under arbitrary guides comes back within rounding: every level is a weighted mean of equal values.  The bound is the
    worst case of the arithmetic: with u = eps / 2, a level's two 25-term sums carry at most 25 u (products and 24 additions) and 24 u, the
    quotient one more: 25 eps per level, 125 eps for the five.  With an albedo the beauty is the f32 film of k (a + eps), so irr is k only up
    to the f32 roundings of that film, of a + eps and of the quotient, and the product back adds one: 4 f32 eps on top, in either type."""
    eps = float(np.finfo(dtype).eps)
    W, H, k = 37, 23, 1.75
    _, a_sum, n_sum = dr.synthetic(W, H, 1, 64, 64, seed=3)
    a = np.maximum(a_sum / np.float32(64), 0)
    for guides in GUIDES:
        use_a, _ = GUIDES[guides]
        mean = (k * (a.astype(np.float64) + np.float32(0.01))) if use_a else np.full((H, W, 3), k)
        b_sum = (mean * 4).astype(np.float32)
        out = run_ref((b_sum, a_sum, n_sum), (4, 64, 64), guides, dtype)
        c = b_sum.astype(dtype) / dtype(4)
        tol = 125 * eps + (4 * F32_EPS if use_a else 0.0)
        assert out.dtype == dtype
        assert np.all(np.abs(out - c) <= tol * np.abs(c)), (guides, float(np.max(np.abs(out - c) / np.abs(c))))


def test_background_is_bit_equal_and_never_a_tap():
    """Background pixels come back as c bit for bit (also where the beauty holds NaN / inf / negative values: c = 0 there), and changing a
    background pixel's beauty changes no other pixel: it is never read as a tap."""
    W, H = 67, 35
    b, a, n = dr.synthetic(W, H, 4, 64, 64, seed=1)
    bg = dr.background(n)
    assert 0 < bg.sum() < W * H
    for dtype in (np.float32, np.float64):
        out = dr.denoise(b, 4, a, 64, n, 64, dtype=dtype)
        with np.errstate(all="ignore"):
            c = b.astype(dtype) / dtype(4)
        c = np.where(np.isfinite(c) & (c > 0), c, dtype(0))
        assert np.array_equal(out[bg].view(np.uint32 if dtype == np.float32 else np.uint64), c[bg].view(np.uint32 if dtype == np.float32 else np.uint64))
        b2 = b.copy(); b2[bg] = 1000.0
        out2 = dr.denoise(b2, 4, a, 64, n, 64, dtype=dtype)
        assert np.array_equal(out2[~bg], out[~bg])


def test_bad_inputs_give_finite_output():
    """NaN, +-inf and negative beauty values become 0 in the prepass: the output is finite and >= 0 everywhere, for every guide set."""
    W, H = 33, 17
    b, a, n = dr.synthetic(W, H, 4, 64, 64, seed=2)
    b.reshape(-1)[::7] = np.nan; b.reshape(-1)[1::11] = np.inf; b.reshape(-1)[2::13] = -np.inf; b.reshape(-1)[3::17] = -3.0
    for guides in GUIDES:
        for dtype in (np.float32, np.float64):
            out = run_ref((b, a, n), (4, 64, 64), guides, dtype, levels=6)
            assert np.isfinite(out).all() and (out >= 0).all(), (guides, dtype)
    allbad = np.full((5, 7, 3), np.nan, np.float32)
    assert np.array_equal(dr.denoise(allbad, 1, dtype=np.float32), np.zeros((5, 7, 3), np.float32))


def test_step_beyond_the_image_is_the_identity():
    """levels = 8 on a 67 x 35 image: at step 128 (and at step 64 = level 7, which no tap survives either on 67 columns) only the centre tap
    is inside, so the level returns (w irr) / w — irr up to the two roundings of that product and quotient."""
    W, H = 67, 35
    b, a, n = dr.synthetic(W, H, 4, 64, 64, seed=4)
    for dtype in (np.float32, np.float64):
        eps = float(np.finfo(dtype).eps)
        _, lv = dr.denoise(b, 4, a, 64, n, 64, levels=8, dtype=dtype, want_levels=True)
        assert len(lv) == 8
        assert np.all(np.abs(lv[7] - lv[6]) <= 2 * eps * np.abs(lv[6]))
        assert not np.array_equal(lv[5], lv[4])                               # (step 32 still has taps inside)
        out7 = dr.denoise(b, 4, a, 64, n, 64, levels=7, dtype=dtype)
        out8 = dr.denoise(b, 4, a, 64, n, 64, levels=8, dtype=dtype)
        assert np.all(np.abs(out8 - out7) <= 4 * eps * np.abs(out7))


def test_f32_restatement_error_is_logged():
    """e32 = max |ref32 - ref64| / (|ref64| + 1e-3) on the synthetic inputs of the GPU parity test (the GPU's bar there is 8 e32 of the same
    case).  Logged, and bounded here only by what f32 arithmetic allows: 1e-4 would mean a different filter, not rounding."""
    for (w, h) in ((7, 5), (67, 35), (130, 70)):
        for spps in ((4, 64, 64), (1, 1, 1)):
            films = dr.synthetic(w, h, *spps)
            for guides in GUIDES:
                for levels in (1, 5, 8):
                    e32 = dr.rel_err(run_ref(films, spps, guides, np.float32, levels=levels), run_ref(films, spps, guides, np.float64, levels=levels))
                    log_line(f'{{"test": "e32_synthetic", "shape": [{w}, {h}], "spp": {list(spps)}, "guides": "{guides}", "levels": {levels}, "e32": {e32:.3e}}}')
                    assert e32 < 1e-4, (w, h, spps, guides, levels, e32)
