"""Per-pixel motion vectors (include/mi355pt_flow.h), the part that needs no GPU: the ABI surface of the cross-compiled library; every
refusal that is decided before a device is touched; the restatement (tests/flow_reference.py) against the restatements it is built on
and against float64; and csrc/flow_checks.hpp on its own (tests/flow_checks_check.cpp, also under the host sanitizers).
tests/test_flow_gpu.py holds the kernels to the restatement bit for bit."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_reference as fr  # noqa: E402
import temporal_rectify_reference as rr  # noqa: E402
import temporal_reference as tr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "toy-cpu-pathtracing_amd", "csrc")
F = np.float32
NEW_SYMBOLS = ["mi355pt_scene_flow_mark", "mi355pt_scene_flow_marked", "mi355pt_render_flow_device", "mi355pt_render_flow",
               "mi355pt_temporal_accumulate_flow_device", "mi355pt_temporal_accumulate_flow", "mi355pt_temporal_accumulate_rectified_flow_device",
               "mi355pt_temporal_accumulate_rectified_flow"]
DEBUG_SYMBOLS = ["mi355pt_render_flow_debug", "mi355pt_scene_export_flow_mark", "mi355pt_scene_export_triangle_ids"]
INVALID, NOT_BUILT = -1, -3


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_flow_abi_surface(pkg):
    """The header declares the eight entry points and the struct, mi355pt.h includes it right after mi355pt_deform.h and declares nothing
    itself, the library exports the symbols (the debug surface's too), ffi.FLOW_SYMBOLS and the generated Rust binding name them; the
    record is 32 bytes with the header's offsets in NumPy and in the Rust text."""
    f = pkg.ffi
    lib = ctypes.CDLL(f.LIB_PATH)
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(f.ROOT, "include", "mi355pt_flow.h")).read(), flags=re.S)
    main = open(os.path.join(f.ROOT, "include", "mi355pt.h")).read()
    debug = re.sub(r"/\*.*?\*/", "", open(os.path.join(f.ROOT, "include", "mi355pt_debug.h")).read(), flags=re.S)
    rs = open(os.path.join(f.ROOT, "bindings", "rust", "mi355pt_sys.rs")).read()
    includes = re.findall(r'#include "(mi355pt_\w+\.h)"', main)
    assert includes.index("mi355pt_deform.h") + 1 == includes.index("mi355pt_flow.h") and includes[-1] == "mi355pt_denoise_var.h"
    declared = sorted(set(re.findall(r"\b(mi355pt_[a-z0-9_]+)\s*\(", code)))
    assert declared == sorted(NEW_SYMBOLS) == sorted("mi355pt_" + s for s in f.FLOW_SYMBOLS)
    assert not any(n in re.sub(r"/\*.*?\*/", "", main, flags=re.S) for n in NEW_SYMBOLS)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(r"pub fn %s\(" % name, rs), name
    assert sorted(DEBUG_SYMBOLS) == sorted("mi355pt_" + s for s in f.FLOW_DEBUG_SYMBOLS)
    for name in DEBUG_SYMBOLS:
        assert hasattr(lib, name) and re.search(r"\b%s\s*\(" % name, debug), name
    assert re.search(r"typedef struct mi355pt_flow_pixel \{.*?\} mi355pt_flow_pixel;", code, flags=re.S)
    assert re.search(r"pub struct FlowPixel \{\s*pub d: \[f32; 3\],\s*pub id: u32,\s*pub dn: \[f32; 3\],\s*pub pad: u32,\s*\}", rs)
    for dt in (f.FLOW_PIXEL, fr.FLOW_PIXEL):
        assert dt.itemsize == 32 and [dt.fields[k][1] for k in ("d", "id", "dn", "pad")] == [0, 12, 16, 28]
    assert f.FLOW_HIT.itemsize == 16 == fr.FLOW_HIT.itemsize
    assert subprocess.call([sys.executable, os.path.join(f.ROOT, "tools", "gen_rust_binding.py"), "--check"]) == 0
    # sizeof(mi355pt_flow_pixel) as a C compiler sees the header
    src = '#include "mi355pt.h"\n_Static_assert(sizeof(mi355pt_flow_pixel) == 32, "32 bytes");\nint main(void) { return 0; }\n'
    r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.join(f.ROOT, "include"), "-x", "c", "-"], input=src, text=True, capture_output=True)
    assert r.returncode == 0, r.stderr
    text = open(os.path.join(f.ROOT, "include", "mi355pt_flow.h")).read()
    assert "THE LIMIT OF dn" in text and "NOT renormalised" in text and "DROPS" in text


def test_refusals_without_a_device(pkg):
    """What is decided before a device is touched.  The mark: a null scene is MI355PT_E_INVALID, an unbuilt one MI355PT_E_NOT_BUILT, and
    mi355pt_scene_flow_marked says 0 for both.  The flow pass: a null, a misaligned (device form only) and an aliased record buffer, null
    scene / camera / params, a zero-sized frame, collect_stats are MI355PT_E_INVALID, an unbuilt scene MI355PT_E_NOT_BUILT; the debug pass
    likewise, plus its null hit buffer.  The accumulations: null records, misaligned records (device forms only), previous ids without
    current ones, records or ids that are an output (or the scratch) are MI355PT_E_INVALID, after the existing checks have passed."""
    f = pkg.ffi
    prod = pkg.Product()
    lib = prod.lib
    err = lambda: lib.mi355pt_last_error()   # noqa: E731
    sc = prod.new_scene()
    cam = pkg.scenes.load_scene(sc, 3, 16, 8, tex_size=16, build=False)
    prm = pkg.make_params(1)
    assert lib.mi355pt_scene_flow_mark(None, None) == INVALID
    assert lib.mi355pt_scene_flow_mark(sc.h, None) == NOT_BUILT and b"not built" in err()
    assert lib.mi355pt_scene_flow_marked(None) == 0 and lib.mi355pt_scene_flow_marked(sc.h) == 0 and not prod.scene_flow_marked(sc)
    n = ctypes.c_uint32(0)
    assert lib.mi355pt_scene_export_flow_mark(sc.h, None, ctypes.byref(n)) == NOT_BUILT and lib.mi355pt_scene_export_flow_mark(None, None, ctypes.byref(n)) == INVALID
    assert lib.mi355pt_scene_export_triangle_ids(sc.h, None, ctypes.byref(n)) == NOT_BUILT and lib.mi355pt_scene_export_triangle_ids(sc.h, None, None) == INVALID

    buf = np.zeros(16 * 8 * 8 + 8, F)
    base = buf.ctypes.data + (-buf.ctypes.data % 16)                  # 16-byte aligned; base + 4 is not
    ids = np.zeros((8, 16), np.uint32)
    hits = np.zeros((8, 16, 4), F)
    c, p = ctypes.byref(cam), ctypes.byref(prm)
    dev, host, dbg = lib.mi355pt_render_flow_device, lib.mi355pt_render_flow, lib.mi355pt_render_flow_debug
    assert dev(sc.h, c, p, None, None, None, None) == INVALID and b"null record buffer" in err()
    assert dev(sc.h, c, p, base + 4, None, None, None) == INVALID and b"16-byte aligned" in err()
    assert dev(sc.h, c, p, base, base, None, None) == INVALID and b"must not be the id buffer" in err()
    assert host(sc.h, c, p, None, None, None) == INVALID and host(sc.h, c, p, base, base, None) == INVALID
    assert host(sc.h, c, p, base + 4, None, None) == NOT_BUILT                                       # no alignment asked of host buffers
    assert dbg(sc.h, c, p, base, None, None, None) == INVALID and b"null hit buffer" in err()
    assert dbg(sc.h, c, p, None, None, hits.ctypes.data, None) == INVALID
    for fn, tail in ((dev, (base, ids.ctypes.data, None, None)), (host, (base, ids.ctypes.data, None)), (dbg, (base, ids.ctypes.data, hits.ctypes.data, None))):
        assert fn(None, c, p, *tail) == INVALID and fn(sc.h, None, p, *tail) == INVALID and fn(sc.h, c, None, *tail) == INVALID
        empty = f.Camera.from_buffer_copy(cam); empty.width = 0
        assert fn(sc.h, ctypes.byref(empty), p, *tail) == INVALID and b"zero-sized" in err()
        stats = pkg.make_params(1); stats.collect_stats = 1
        assert fn(sc.h, c, ctypes.byref(stats), *tail) == INVALID and b"collect_stats" in err()
        assert fn(sc.h, c, p, *tail) == NOT_BUILT and b"not built" in err()
    assert not buf.any() and not ids.any() and not hits.any()

    # the accumulations: host arrays stand in for the buffers, every call below is refused before a launch
    W, H = 6, 4
    cur, prev, vw, spp = tr.synthetic(W, H, "move", "step", True)
    keep = [{k: np.ascontiguousarray(v, F) for k, v in fr_.items() if v is not None} for fr_ in (cur, prev)]
    frames = [f.TemporalFrame(*[k_[n_].ctypes.data if n_ in k_ else None for n_ in f.TEMPORAL_FILMS]) for k_ in keep]
    view = f.TemporalView((ctypes.c_float * 3)(*vw.delta), (ctypes.c_float * 9)(*vw.rows), vw.sx, vw.sy, vw.cx, vw.cy)
    tp, rp = prod.temporal_params_default(), prod.temporal_rectify_params_default()
    of, oh, ol = np.zeros((H, W, 3), F), np.zeros((H, W, 3), F), np.zeros((H, W), F)
    fbuf = np.zeros(W * H * 8 + 8, F)
    fl = fbuf.ctypes.data + (-fbuf.ctypes.data % 16)
    ic, ip = np.zeros((H, W), np.uint32), np.zeros((H, W), np.uint32)
    scratch = np.zeros(prod.temporal_rectify_scratch_bytes(W, H) + 16, np.uint8)
    sp = scratch.ctypes.data + (-scratch.ctypes.data % 16)
    head = (ctypes.byref(frames[0]), spp, ctypes.byref(frames[1]), ctypes.byref(view), W, H, ctypes.byref(tp))
    outs = (of.ctypes.data, oh.ctypes.data, ol.ctypes.data)
    forms = [
        (lib.mi355pt_temporal_accumulate_flow_device, head, outs + (None,), True),
        (lib.mi355pt_temporal_accumulate_flow, head, outs, False),
        (lib.mi355pt_temporal_accumulate_rectified_flow_device, head + (ctypes.byref(rp), sp, scratch.size - 16), outs + (None,), True),
        (lib.mi355pt_temporal_accumulate_rectified_flow, head + (ctypes.byref(rp),), outs, False),
    ]
    for fn, hd, tl, device_form in forms:
        assert fn(*hd, ic.ctypes.data, ip.ctypes.data, None, *tl) == INVALID and b"null record buffer" in err(), fn.__name__
        assert fn(*hd, None, ip.ctypes.data, fl, *tl) == INVALID and b"need the current" in err(), fn.__name__
        for alias in (0, 1, 2):
            bad = list(tl); bad[alias] = fl
            assert fn(*hd, ic.ctypes.data, ip.ctypes.data, fl, *bad) == INVALID, fn.__name__
            bad = list(tl); bad[alias] = ic.ctypes.data
            assert fn(*hd, ic.ctypes.data, None, fl, *bad) == INVALID, fn.__name__
        if device_form:
            assert fn(*hd, ic.ctypes.data, ip.ctypes.data, fl + 4, *tl) == INVALID and b"16-byte aligned" in err(), fn.__name__
        assert fn(*hd[:1], 0, *hd[2:], ic.ctypes.data, ip.ctypes.data, fl, *tl) == INVALID                  # an existing check still comes first: spp == 0
    fn, hd, tl, _ = forms[2]
    assert fn(*hd[:-2], fl, hd[-1], ic.ctypes.data, ip.ctypes.data, fl, *tl) == INVALID                     # the scratch is the records
    assert not of.any() and not oh.any() and not ol.any()


@pytest.mark.parametrize("half", [True, False], ids=["half", "nohalf"])
@pytest.mark.parametrize("view", ["static", "move", "outside", "behind"])
def test_restatement_with_zero_records_is_the_static_restatement(view, half):
    """flow_reference.accumulate_flow with all-zero records and no previous ids IS temporal_reference.accumulate at delta = 0, bit for bit,
    and the rectified pair likewise; with the view's delta in every record it is temporal_reference.accumulate at that delta (the same
    addition); with a displaced band, a dn or previous ids it is not."""
    W, H = 70, 50
    cur, prev, vw, spp = tr.synthetic(W, H, view, "step", half)
    v0 = fr.zero_delta(vw)
    zero = fr.zero_records(W, H)
    carried = fr.zero_records(W, H); carried["d"] = np.asarray(vw.delta, F)
    for flow, v in ((zero, v0), (carried, vw)):
        for want, got in ((tr.accumulate(cur, spp, prev, v), fr.accumulate_flow(cur, spp, prev, vw, None, None, flow)),
                          (rr.accumulate(cur, spp, prev, v), fr.accumulate_rectified_flow(cur, spp, prev, vw, None, None, flow))):
            for a, b in zip(want, got):
                assert (a is None) == (b is None)
                if a is not None:
                    assert np.array_equal(bits(a), bits(b))
    assert rr.tr is tr                                                   # the rectified restatement has its own gather back
    if view in ("static", "move"):
        base = tr.accumulate(cur, spp, prev, vw)
        moved = fr.synthetic_flow(W, H, vw)
        assert not np.array_equal(bits(fr.accumulate_flow(cur, spp, prev, vw, None, None, moved)[0]), bits(base[0]))
        ids_cur = moved["id"]; ids_prev = np.roll(ids_cur, 2, axis=1)
        assert not np.array_equal(bits(fr.accumulate_flow(cur, spp, prev, vw, ids_cur, ids_prev, carried)[0]), bits(base[0]))
    first = fr.accumulate_flow(cur, spp, None, None, None, None, zero)
    assert np.array_equal(bits(first[0]), bits(tr.accumulate(cur, spp)[0]))


def random_triangles(rng, n, scale):
    t = np.zeros((n, 12), F)
    t[:, :9] = rng.uniform(-scale, scale, (n, 9)).astype(F)
    t[:, 9] = rng.integers(0, 7, n).astype(np.uint32).view(F)
    return t


def test_equal_triangle_arrays_give_zero_records():
    """bytewise-equal current and marked arrays: every record's d and dn is exactly +0 (x - x), the id is the instance + 1; degenerate and
    overflowing triangles included (their dn is 0 by the rule); a miss is all zero"""
    rng = np.random.default_rng(3)
    tris = random_triangles(rng, 64, 50.0)
    tris[5, 3:9] = np.tile(tris[5, 0:3], 2)                              # a point: zero cross product
    tris[6, :9] *= F(1e19)                                               # squared length overflows
    n = 500
    tri = rng.integers(0, 64, n)
    b = rng.dirichlet((1.0, 1.0, 1.0), n).astype(F)
    hit = rng.random(n) < 0.8
    rec = fr.records(hit, tri, b, tris, tris.copy())
    assert not bits(rec["d"]).any() and not bits(rec["dn"]).any() and not rec["pad"].any()
    assert np.array_equal(rec["id"], np.where(hit, fr.instances(tris)[tri] + 1, 0))
    assert not rec[~hit].view(np.uint32).any()


def test_records_against_float64():
    """The record against the same formulas in float64 from the same f32 inputs.  DERIVATION of the bound on d, per component, with
    u = 2^-24 (the unit roundoff of binary32) and M = max |P| over both triangles:
      an interpolation  (b0 P0 + b1 P1) + b2 P2  has three products, each within u |b_k P_k| of exact, and two sums, each within u of
      its own value; with b_k >= 0 and b0 + b1 + b2 <= 1 + 3u (the barycentrics of a hit) every partial sum is at most (1 + 3u) M, so
      the computed value is within  (3 + 2)(1 + O(u)) u M  <= 5.01 u M of the exact one;
      d = Xv - Xc  subtracts two such values (2 x 5.01 u M) and rounds once more, at most u |d| <= 2.01 u M.
    Together |d - d64| <= 12.03 u M: the test holds every component to 13 x 2^-24 x max|P|.
    dn is a difference of unit vectors: each normal's components carry about 10 roundings relative to edge products that can cancel, so
    its bound depends on the triangle's shape, not on M; it is held bit for bit by the GPU test instead, and here only for well-shaped
    triangles (|cross| >= 0.1 x the product of the edge lengths) to 64 u."""
    rng = np.random.default_rng(11)
    u = 2.0 ** -24
    worst = 0.0
    for scale in (1.0, 37.0, 1e4):
        cur_t, prev_t = random_triangles(rng, 200, scale), random_triangles(rng, 200, scale)
        prev_t[:100, :9] = cur_t[:100, :9] + rng.normal(0, 1e-3 * scale, (100, 9)).astype(F)       # small motions: heavy cancellation in d
        prev_t[:, 9] = cur_t[:, 9]
        n = 4000
        tri = rng.integers(0, 200, n)
        b = rng.dirichlet((1.0, 1.0, 1.0), n).astype(F)
        rec = fr.records(np.ones(n, bool), tri, b, cur_t, prev_t)
        Pc, Pv = fr.positions(cur_t)[tri].astype(np.float64), fr.positions(prev_t)[tri].astype(np.float64)
        b64 = b.astype(np.float64)
        d64 = fr.interpolate(b64, Pv, np.float64) - fr.interpolate(b64, Pc, np.float64)
        M = max(np.abs(Pc).max(), np.abs(Pv).max())
        err = np.abs(rec["d"].astype(np.float64) - d64).max()
        worst = max(worst, err / (u * M))
        assert err <= 13.0 * u * M, (scale, err / (u * M))
        (nc, _), (nv, _) = fr.facet_normal(Pc, np.float64), fr.facet_normal(Pv, np.float64)
        e1, e2 = Pc[:, 1] - Pc[:, 0], Pc[:, 2] - Pc[:, 0]
        f1, f2 = Pv[:, 1] - Pv[:, 0], Pv[:, 2] - Pv[:, 0]
        shaped = (np.linalg.norm(np.cross(e1, e2), axis=1) >= 0.1 * np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1)) & \
                 (np.linalg.norm(np.cross(f1, f2), axis=1) >= 0.1 * np.linalg.norm(f1, axis=1) * np.linalg.norm(f2, axis=1)) & \
                 (np.linalg.norm(e1, axis=1) > 0.05 * scale) & (np.linalg.norm(e2, axis=1) > 0.05 * scale) & \
                 (np.linalg.norm(f1, axis=1) > 0.05 * scale) & (np.linalg.norm(f2, axis=1) > 0.05 * scale)
        assert shaped.sum() > 500
        assert np.abs(rec["dn"].astype(np.float64) - (nv - nc))[shaped].max() <= 64.0 * u
    assert worst > 0.5                                                   # the bound is not vacuous: errors of its order occur


@pytest.fixture(scope="module")
def checks_check(tmp_path_factory):
    """tests/flow_checks_check.cpp built with plain g++ (the header needs no HIP) and, a second time, with the host sanitizers"""
    def build(name, extra):
        exe = str(tmp_path_factory.mktemp(name) / "flow_checks_check")
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + extra + ["-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "flow_checks_check.cpp")],
                       check=True)
        return exe
    return build("plain", []), build("sanitized", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def test_checks_header_is_pure(checks_check):
    text = open(os.path.join(CSRC, "flow_checks.hpp")).read()
    assert not re.search(r"#\s*include\s*[<\"]hip|getenv|chrono|clock_gettime|gettimeofday|atomic", text)


@pytest.mark.parametrize("seed,n", [(1, 0), (2, 100), (3, 5000)])
def test_checks_predicates(checks_check, seed, n):
    """the stand-alone program's own checks — the order of the verdicts, the host forms' alignment, every alias — plain and under
    ASan + UBSan"""
    for exe in checks_check:
        r = subprocess.run([exe, str(seed), str(n)], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
