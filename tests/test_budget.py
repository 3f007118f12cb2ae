"""The sample budget by reprojected history (include/mi355pt_budget.h), the part that needs no GPU: the ABI surface of the cross-compiled
library; every refusal that is decided before a device is touched, with its message; the budget formula at its corners, in the restatement
(tests/budget_reference.py) and in csrc/budget_plan.hpp (tests/budget_plan_check.cpp, plain and under the host sanitizers); and, in the
restatement alone, the identity that ties the probe to the accumulation: out_length == where(P > 0, min(P + 1, max_history), 1).
tests/test_budget_gpu.py holds the kernels to the restatement bit for bit."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import budget_reference as br  # noqa: E402
import flow_reference as fr  # noqa: E402
import motion_reference as mr  # noqa: E402
import temporal_reference as tr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "toy-cpu-pathtracing_amd", "csrc")
F = np.float32
NEW_SYMBOLS = ["mi355pt_temporal_budget_device", "mi355pt_temporal_budget", "mi355pt_render_budget_device", "mi355pt_film_pair_normalize_tiles_device",
               "mi355pt_film_pair_normalize_tiles", "mi355pt_temporal_length_credit_device"]
INVALID, NOT_BUILT = -1, -3


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def f32_bits(x):
    return int(np.array([x], F).view(np.uint32)[0])


def test_budget_abi_surface(pkg):
    """The header declares the six entry points and the two structs, mi355pt.h includes it right after mi355pt_flow.h and declares nothing
    itself, the library exports the symbols, ffi.BUDGET_SYMBOLS and the generated Rust binding name them, the ctypes structs have the C
    layout, and the header states the known limit."""
    f = pkg.ffi
    lib = ctypes.CDLL(f.LIB_PATH)
    text = open(os.path.join(f.ROOT, "include", "mi355pt_budget.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    main = open(os.path.join(f.ROOT, "include", "mi355pt.h")).read()
    rs = open(os.path.join(f.ROOT, "bindings", "rust", "mi355pt_sys.rs")).read()
    includes = re.findall(r'#include "(mi355pt_\w+\.h)"', main)
    assert includes.index("mi355pt_flow.h") + 1 == includes.index("mi355pt_budget.h") and includes[-1] == "mi355pt_denoise_var.h"
    declared = sorted(set(re.findall(r"\b(mi355pt_[a-z0-9_]+)\s*\(", code)))
    assert declared == sorted(NEW_SYMBOLS) == sorted("mi355pt_" + s for s in f.BUDGET_SYMBOLS)
    assert not any(n in re.sub(r"/\*.*?\*/", "", main, flags=re.S) for n in NEW_SYMBOLS)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(r"pub fn %s\(" % name, rs), name
    assert re.search(r"pub struct BudgetParams \{\s*pub base_spp: u32,\s*pub max_spp: u32,\s*pub target_history: f32,\s*\}", rs)
    assert re.search(r"pub struct BudgetMotion \{\s*pub ids_cur: \*const u32,\s*pub ids_prev: \*const u32,\s*pub table: \*const MotionXform,\s*"
                     r"pub n_entries: u32,\s*pub flow: \*const FlowPixel,\s*\}", rs)
    assert subprocess.call([sys.executable, os.path.join(f.ROOT, "tools", "gen_rust_binding.py"), "--check"]) == 0
    # the structs as a C compiler sees the header, against the ctypes ones
    src = ('#include <stddef.h>\n#include "mi355pt.h"\n'
           '_Static_assert(sizeof(mi355pt_budget_params) == %d, "params");\n_Static_assert(sizeof(mi355pt_budget_motion) == %d, "motion");\n'
           '_Static_assert(offsetof(mi355pt_budget_motion, n_entries) == %d && offsetof(mi355pt_budget_motion, flow) == %d, "offsets");\n'
           'int main(void) { return 0; }\n') % (ctypes.sizeof(f.BudgetParams), ctypes.sizeof(f.BudgetMotion), f.BudgetMotion.n_entries.offset,
                                               f.BudgetMotion.flow.offset)
    r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.join(f.ROOT, "include"), "-x", "c", "-"], input=src, text=True, capture_output=True)
    assert r.returncode == 0, r.stderr
    assert "THE KNOWN LIMIT" in text and "under-weighted" in text and "not variance-optimal" in text and "never trusted" in text


def test_refusals_without_a_device(pkg):
    """Every refusal of the six entry points, each with its message; host arrays stand in for the buffers, every call below is refused
    before a launch, and no output is written."""
    f = pkg.ffi
    prod = pkg.Product()
    lib = prod.lib
    err = lambda: lib.mi355pt_last_error()   # noqa: E731
    ref = ctypes.byref
    W, H = 12, 9
    cur, prev, vw, _ = tr.synthetic(W, H, "move", "step", True)
    keep = [{k: np.ascontiguousarray(v, F) for k, v in fr_.items() if v is not None} for fr_ in (cur, prev)]

    def frame(k_, drop=()):
        return f.TemporalFrame(*[k_[n_].ctypes.data if n_ in k_ and n_ not in drop else None for n_ in f.TEMPORAL_FILMS])
    fc, fp = frame(keep[0]), frame(keep[1])
    view = f.TemporalView((ctypes.c_float * 3)(*vw.delta), (ctypes.c_float * 9)(*vw.rows), vw.sx, vw.sy, vw.cx, vw.cy)
    tp, bp = prod.temporal_params_default(), f.BudgetParams(4, 32, 8.0)
    pred, tl, ts = np.zeros((H, W), F), np.zeros((2, 2), F), np.zeros((2, 2), np.uint32)
    outs = (pred.ctypes.data, tl.ctypes.data, ts.ctypes.data)
    ic, ip = np.zeros((H, W), np.uint32), np.zeros((H, W), np.uint32)
    tbuf, fbuf = np.zeros(3 * 24 + 8, F), np.zeros(W * H * 8 + 8, F)
    tab, fl = tbuf.ctypes.data + (-tbuf.ctypes.data % 16), fbuf.ctypes.data + (-fbuf.ctypes.data % 16)

    for fn, tail, device_form in ((lib.mi355pt_temporal_budget_device, outs + (None,), True), (lib.mi355pt_temporal_budget, outs, False)):
        def call(cur_=fc, prev_=fp, view_=view, w=W, h=H, tp_=tp, mo=None, bp_=bp, tail_=tail):
            return fn(ref(cur_) if cur_ is not None else None, ref(prev_) if prev_ is not None else None, ref(view_) if view_ is not None else None, w, h,
                      ref(tp_) if tp_ is not None else None, ref(mo) if mo is not None else None, ref(bp_) if bp_ is not None else None, *tail_)

        def refused(text, **kw):
            assert call(**kw) == INVALID and text in err(), (fn.__name__, text, err())
        refused(b"null current frame", cur_=None)
        refused(b"null current frame", tp_=None)
        refused(b"null current frame", tail_=(tail[0], None) + tail[2:])
        refused(b"null current frame", tail_=tail[:2] + (None,) + tail[3:])
        refused(b"null budget_params", bp_=None)
        refused(b"base_spp must be a power of two >= 2", bp_=f.BudgetParams())                       # a zeroed struct
        refused(b"base_spp must be a power of two >= 2", bp_=f.BudgetParams(1, 32, 8.0))
        refused(b"base_spp must be a power of two >= 2", bp_=f.BudgetParams(6, 32, 8.0))
        refused(b"max_spp must be a power of two >= base_spp", bp_=f.BudgetParams(4, 2, 8.0))
        refused(b"max_spp must be a power of two >= base_spp", bp_=f.BudgetParams(4, 24, 8.0))
        refused(b"target_history must be finite and >= 1", bp_=f.BudgetParams(4, 32, 0.5))
        refused(b"target_history must be finite and >= 1", bp_=f.BudgetParams(4, 32, float("inf")))
        refused(b"target_history must be finite and >= 1", bp_=f.BudgetParams(4, 32, float("nan")))
        refused(b"both be given or both be NULL", prev_=None)
        refused(b"both be given or both be NULL", view_=None)
        for name in ("position", "shading_normal", "hit"):
            refused(b"the current frame needs", cur_=frame(keep[0], (name,)))
        for name in ("length", "position", "shading_normal", "hit"):
            refused(b"the previous frame needs", prev_=frame(keep[1], (name,)))
        refused(b"zero width or height", w=0)
        refused(b"zero width or height", h=0)
        refused(b"frame too large", w=(1 << 24) + 1)
        refused(b"must be finite and > 0", tp_=f.TemporalParams())                                   # a zeroed struct
        refused(b"max_history must be >= 1", tp_=f.TemporalParams(0.01, 0.9, 0.01, 0.5))
        refused(b"normal_cos must be in [-1, 1]", tp_=f.TemporalParams(0.01, 1.5, 0.01, 32.0))
        refused(b"both a table and flow records", mo=f.BudgetMotion(ic.ctypes.data, None, tab, 3, fl))
        refused(b"without a table or flow records", mo=f.BudgetMotion(ic.ctypes.data, None, None, 0, None))
        refused(b"without a table or flow records", mo=f.BudgetMotion(None, None, None, 2, None))
        refused(b"needs the current id buffer", mo=f.BudgetMotion(None, None, tab, 3, None))
        refused(b"n_entries must be > 0", mo=f.BudgetMotion(ic.ctypes.data, None, tab, 0, None))
        refused(b"must not be an output", mo=f.BudgetMotion(ic.ctypes.data, ip.ctypes.data, tab, 3, None), tail_=(ip.ctypes.data,) + tail[1:])
        refused(b"need the current frame's", mo=f.BudgetMotion(None, ip.ctypes.data, None, 0, fl))
        refused(b"must not be an output", mo=f.BudgetMotion(ic.ctypes.data, None, None, 0, fl), tail_=(tail[0], fl) + tail[2:])
        if device_form:
            refused(b"table must be 16-byte aligned", mo=f.BudgetMotion(ic.ctypes.data, None, tab + 4, 3, None))
            refused(b"record buffer must be 16-byte aligned", mo=f.BudgetMotion(None, None, None, 0, fl + 4))
        refused(b"must not be one of the films that are read", tail_=(keep[1]["length"].ctypes.data,) + tail[1:])
        refused(b"must not be one of the films that are read", tail_=(tail[0], keep[0]["hit"].ctypes.data) + tail[2:])
        refused(b"two outputs are the same buffer", tail_=(tail[0], tail[1], tail[1]) + tail[3:])
        # without a previous frame the motion is still checked
        refused(b"both a table and flow records", prev_=None, view_=None, mo=f.BudgetMotion(ic.ctypes.data, None, tab, 3, fl))
    assert not pred.any() and not tl.any() and not ts.any()

    # the driver: the scene checks of the tile-list render first, then the budget's own
    sc = prod.new_scene()
    cam = pkg.scenes.load_scene(sc, 3, 16, 8, tex_size=16, build=False)
    prm = pkg.make_params(32)
    buf = np.zeros(16 * 8 * 3, F)
    half, lst = np.zeros_like(buf), np.zeros(2, np.uint32)
    scratch = np.zeros(prod.adaptive_scratch_bytes(16, 8) + 4, np.uint8)
    sp = scratch.ctypes.data + (-scratch.ctypes.data % 4)
    drv = lib.mi355pt_render_budget_device

    def drive(s_=sc.h, cam_=cam, p_=prm, bp_=bp, spp_=ts.ctypes.data, film=buf.ctypes.data, half_=half.ctypes.data, lst_=lst.ctypes.data, sp_=sp,
              nbytes=scratch.size - 4):
        return drv(s_, ref(cam_) if cam_ is not None else None, ref(p_) if p_ is not None else None, ref(bp_) if bp_ is not None else None, spp_, film, half_,
                   lst_, sp_, nbytes, None, None)
    assert drive(s_=None) == INVALID and drive(cam_=None) == INVALID and drive(p_=None) == INVALID
    assert drive() == NOT_BUILT and b"not built" in err()
    # (the remaining checks come after the scene's: they are reached on a built scene, tests/test_budget_gpu.py)
    shards = pkg.make_params(32); shards.shard_count = 2
    stats = pkg.make_params(32); stats.collect_stats = 1
    for p_ in (shards, stats):
        assert drive(p_=p_) in (INVALID, NOT_BUILT)

    # the pair normalise and the length credit
    film, hf = np.ones((H, W, 3), F), np.ones((H, W, 3), F)
    of, oh = np.zeros((H, W, 3), F), np.zeros((H, W, 3), F)
    for fn, tail in ((lib.mi355pt_film_pair_normalize_tiles_device, (None,)), (lib.mi355pt_film_pair_normalize_tiles, ())):
        good = [film.ctypes.data, hf.ctypes.data, ts.ctypes.data, W, H, of.ctypes.data, oh.ctypes.data]
        for i in (0, 1, 2, 5, 6):
            bad = list(good); bad[i] = None
            assert fn(*bad, *tail) == INVALID and b"pair normalize: null buffer" in err()
        bad = list(good); bad[3] = 0
        assert fn(*bad, *tail) == INVALID and b"zero width or height" in err()
        bad = list(good); bad[4] = (1 << 24) + 1
        assert fn(*bad, *tail) == INVALID and b"frame too large" in err()
        bad = list(good); bad[6] = bad[5]
        assert fn(*bad, *tail) == INVALID and b"the two outputs are the same buffer" in err()
        bad = list(good); bad[5] = bad[1]
        assert fn(*bad, *tail) == INVALID and b"the other film's input" in err()
        bad = list(good); bad[6] = bad[0]
        assert fn(*bad, *tail) == INVALID and b"the other film's input" in err()
    assert not of.any() and not oh.any()
    credit = lib.mi355pt_temporal_length_credit_device
    ln = np.ones((H, W), F)
    assert credit(None, ts.ctypes.data, 4, 32.0, W, H, None) == INVALID and b"length credit: null buffer" in err()
    assert credit(ln.ctypes.data, None, 4, 32.0, W, H, None) == INVALID and b"length credit: null buffer" in err()
    assert credit(ln.ctypes.data, ts.ctypes.data, 4, 32.0, 0, H, None) == INVALID and b"zero width or height" in err()
    for base in (0, 1, 6):
        assert credit(ln.ctypes.data, ts.ctypes.data, base, 32.0, W, H, None) == INVALID and b"base_spp must be a power of two >= 2" in err()
    for mh in (0.5, float("inf"), float("nan")):
        assert credit(ln.ctypes.data, ts.ctypes.data, 4, mh, W, H, None) == INVALID and b"max_history must be finite and >= 1" in err()
    assert (ln == 1).all()


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    """tests/budget_plan_check.cpp built with plain g++ (the header needs no HIP) and, a second time, with the host sanitizers"""
    def build(name, extra):
        exe = str(tmp_path_factory.mktemp(name) / "budget_plan_check")
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + extra + ["-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "budget_plan_check.cpp")],
                       check=True)
        return exe
    return build("plain", []), build("sanitized", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def test_plan_header_is_pure(plan_check):
    text = open(os.path.join(CSRC, "budget_plan.hpp")).read()
    assert not re.search(r"#\s*include\s*[<\"]hip|getenv|chrono|clock_gettime|gettimeofday|atomic", text)


@pytest.mark.parametrize("seed,n", [(1, 0), (2, 100), (3, 20000)])
def test_plan_predicates_and_formula(plan_check, seed, n):
    """the stand-alone program's own checks — the verdicts in their order, the formula at its corners and against its definition by
    search, the clamp and the credit — plain and under ASan + UBSan"""
    for exe in plan_check:
        r = subprocess.run([exe, str(seed), str(n)], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr


# (Lmin, base, max, target) -> tile_spp, worked out by hand from the header's formula
below8 = float(np.nextafter(F(7), F(0)))
CORNERS = [
    (0.0, 4, 32, 8.0, 32),            # Lmin = 0: (0 + 1) 2^3 >= 8
    (0.0, 4, 16, 8.0, 16),            # ... capped at max_spp
    (below8, 4, 32, 8.0, 8),          # Lmin + 1 one ulp below the target (8 - ulp is a binary32 number)
    (7.0, 4, 32, 8.0, 4),             # at the target
    (7.5, 4, 32, 8.0, 4),             # above it
    (float(np.nextafter(F(1), F(0))), 4, 32, 2.0, 4),      # (1 - 2^-24) + 1 rounds to 2: Lmin + 1 is rounded once, then compared
    (3.0, 4, 32, 8.0, 8), (2.9, 4, 32, 8.0, 16), (1.0, 4, 32, 8.0, 16), (0.9, 4, 32, 8.0, 32),
    (0.0, 4, 32, 1.0, 4), (31.0, 4, 32, 1.0, 4),           # target_history = 1: every tile gets base_spp
    (0.0, 8, 8, 32.0, 8), (5.0, 8, 8, 32.0, 8),            # base_spp == max_spp
    (0.0, 4, 64, 5.0, 32), (1.5, 4, 64, 5.0, 8), (1.4, 4, 64, 5.0, 16), (4.0, 4, 64, 5.0, 4), (3.9, 4, 64, 5.0, 8),      # a target that is no power of two
    (float("inf"), 4, 32, 8.0, 4),
]


def test_formula_corners(plan_check):
    """the budget formula at its corners: the restatement and csrc/budget_plan.hpp's budget_spp (the text the probe kernel compiles) both give
    the value worked out by hand"""
    for lmin, base, mx, target, want in CORNERS:
        b = br.budget(base, mx, target)
        assert int(br.spp_of(np.array([lmin], F), b)[0]) == want, (lmin, base, mx, target)
        for exe in plan_check:
            r = subprocess.run([exe, "spp", str(f32_bits(lmin)), str(base), str(mx), str(f32_bits(target))], capture_output=True, text=True)
            assert r.returncode == 0 and int(r.stdout) == want, (lmin, base, mx, target, r.stdout, r.stderr)
    # every tile of a frame at target 1 and at base == max
    lmin = np.random.default_rng(5).random((7, 9)).astype(F) * F(40)
    assert (br.spp_of(lmin, br.budget(4, 32, 1.0)) == 4).all() and (br.spp_of(lmin, br.budget(16, 16, 9.0)) == 16).all()
    got = br.spp_of(lmin, br.budget(4, 32, 8.0))
    assert set(np.unique(got)) <= {4, 8, 16, 32} and (got[lmin + F(1) >= 8] == 4).all()


def test_tile_minimum_and_credit_restatement():
    """a P that is not > 0 counts as 0; ragged tiles take their in-frame pixels only; the pair normalise and the credit as the header says"""
    P = np.full((9, 9), 5.0, F)
    P[0, 0], P[8, 8], P[3, 8] = np.nan, 2.0, -1.0
    lmin = br.tile_min(P)
    assert lmin.shape == (2, 2) and lmin.tolist() == [[0.0, 0.0], [5.0, 2.0]]
    spp = np.array([[4, 8], [32, 2]], np.uint32)
    film, half = np.full((9, 9, 3), 12.0, F), np.full((9, 9, 3), 6.0, F)
    of, oh = br.pair_normalize(film, half, spp)
    assert of[0, 0, 0] == 6 and of[0, 8, 0] == 3 and of[8, 0, 0] == 0.75 and of[8, 8, 0] == 12 and oh[0, 8, 1] == 1.5
    ln = np.full((9, 9), 30.0, F)
    out = br.length_credit(ln, spp, 4, 32.0)
    assert out[0, 0] == 30 and out[0, 8] == 31 and out[8, 0] == 32 and out[8, 8] == 30
    assert br.rendered_count(np.array([0, 4, 6, 8, 33, 1000]), br.budget(4, 32, 8.0)).tolist() == [4, 4, 8, 8, 32, 32]
    levels = br.driver_levels(np.array([4, 8, 16, 4, 32, 8]), br.budget(4, 32, 8.0))
    assert [(lv, t.tolist()) for lv, t in levels] == [(4, [1, 2, 4, 5]), (8, [2, 4]), (16, [4])]
    assert [(lv, t.tolist()) for lv, t in br.driver_levels(np.array([4, 4]), br.budget(4, 32, 8.0))] == [(4, [])]


@pytest.mark.parametrize("scene", ["plane", "step"])
@pytest.mark.parametrize("view", tr.VIEWS)
def test_probe_identity_in_the_restatement(view, scene):
    """In the restatement alone, on the synthetic frames of the existing temporal tests: temporal_reference's out_length ==
    where(P > 0, min(P + 1, max_history), 1), bit for bit — with and without the half film (the length does not depend on it), at two
    max_history; and the same with a motion table and with flow records, previous ids included."""
    W, H = 70, 50
    cur, prev, vw, spp = tr.synthetic(W, H, view, scene, True)
    for mh in (32.0, 5.0):
        prm = tr.params(max_history=mh)
        P = br.gathered_length(cur, prev, vw, prm)
        want = br.expected_out_length(P, mh)
        for half in (True, False):
            c, p = dict(cur), dict(prev)
            if not half:
                c["half"], p["half"] = None, None
            assert np.array_equal(bits(tr.accumulate(c, spp, p, vw, prm)[2]), bits(want))
        ids_cur, ids_prev = mr.synthetic_ids(W, H)
        table = mr.static_table(vw, 3); table[1] = mr.moved_entry(vw)
        flow = fr.synthetic_flow(W, H, vw, big=True)
        for ip in (None, ids_prev):
            Pm = br.gathered_length(cur, prev, vw, prm, ids_cur=ids_cur, ids_prev=ip, table=table)
            assert np.array_equal(bits(mr.accumulate_motion(cur, spp, prev, vw, ids_cur, ip, table, prm)[2]), bits(br.expected_out_length(Pm, mh)))
            Pf = br.gathered_length(cur, prev, vw, prm, ids_cur=ids_cur, ids_prev=ip, flow=flow)
            assert np.array_equal(bits(fr.accumulate_flow(cur, spp, prev, vw, ids_cur, ip, flow, prm)[2]), bits(br.expected_out_length(Pf, mh)))
    if view in ("static", "shift3", "move"):
        assert (P > 0).sum() > W * H // 4 and (P == 0).sum() > 0                   # both kinds of pixels occur
    # without a previous frame every P is 0
    assert not br.gathered_length(cur, None, None).any()
