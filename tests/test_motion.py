"""Object motion vectors (include/mi355pt_motion.h), the part that needs no GPU: the ABI surface of the cross-compiled library; the motion
table against a NumPy float64 computation, its exact static entries and its refusals; the round trip of an object's points through an
entry and the previous view's projection; the restatement (tests/motion_reference.py) against the restatements it is built on; and
csrc/motion_plan.hpp on its own (tests/motion_plan_check.cpp, also under the host sanitizers).  tests/test_motion_gpu.py holds the
kernels to the restatement bit for bit."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import motion_reference as mr  # noqa: E402
import temporal_rectify_reference as rr  # noqa: E402
import temporal_reference as tr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "toy-cpu-pathtracing_amd", "csrc")
F = np.float32
NEW_SYMBOLS = ["mi355pt_render_ids_device", "mi355pt_render_ids", "mi355pt_motion_table", "mi355pt_temporal_accumulate_motion_device",
               "mi355pt_temporal_accumulate_motion", "mi355pt_temporal_accumulate_rectified_motion_device", "mi355pt_temporal_accumulate_rectified_motion"]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def ffi_camera(pkg, c):
    return pkg.make_camera(c.position, c.direction, c.up, c.width, c.height, c.fov_deg)


def trs(t=(0.0, 0.0, 0.0), axis=(0.0, 1.0, 0.0), angle=0.0, s=(1.0, 1.0, 1.0)):
    """T(t) R(axis, angle) S(s) as a float32 4 x 4 (row-major, as add_instance takes it)"""
    ax = np.asarray(axis, np.float64); ax = ax / np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)
    m = np.eye(4)
    m[:3, :3] = R @ np.diag(s)
    m[:3, 3] = t
    return m.astype(F)


# (previous matrix, current matrix): unmoved; translation; rotation; non-uniform scale change; all of them on a rotated and scaled object
POSES = [
    (trs((1.0, 0.5, -3.0)), trs((1.0, 0.5, -3.0))),
    (trs((1.0, 0.5, -3.0)), trs((1.25, 0.4, -2.5))),
    (trs((0.3, 0.0, -4.0), (0.0, 1.0, 0.0), 0.2), trs((0.3, 0.0, -4.0), (0.0, 1.0, 0.0), 0.55)),
    (trs((0.0, 1.0, -2.0), s=(1.0, 1.0, 1.0)), trs((0.0, 1.0, -2.0), s=(1.3, 0.8, 1.1))),
    (trs((-2.0, 0.2, -5.0), (1.0, 2.0, -0.5), 1.1, (0.7, 1.6, 1.2)), trs((-1.6, 0.3, -5.5), (1.0, 2.0, -0.5), 1.4, (0.75, 1.5, 1.2))),
]
CAMERAS = [   # (current, previous): the same camera; a camera move with a yaw
    (tr.camera(position=(0.1, 1.2, 3.4)), tr.camera(position=(0.1, 1.2, 3.4))),
    (tr.camera(position=(0.4, 1.3, 3.2)), tr.camera(position=(0.1, 1.2, 3.4), direction=tr.yawed((0.0, 0.0, -1.0), 0.05))),
]


def test_motion_abi_surface(pkg):
    """The header declares the seven entry points and the struct, mi355pt.h includes it right after mi355pt_instances.h and declares nothing
    itself, the library exports the symbols, ffi.MOTION_SYMBOLS and the generated Rust binding name them; the record is 96 bytes with the
    header's offsets in ctypes and in the Rust text."""
    f = pkg.ffi
    lib = ctypes.CDLL(f.LIB_PATH)
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(f.ROOT, "include", "mi355pt_motion.h")).read(), flags=re.S)
    main = open(os.path.join(f.ROOT, "include", "mi355pt.h")).read()
    rs = open(os.path.join(f.ROOT, "bindings", "rust", "mi355pt_sys.rs")).read()
    includes = re.findall(r'#include "(mi355pt_\w+\.h)"', main)
    assert includes.index("mi355pt_instances.h") + 1 == includes.index("mi355pt_motion.h") and includes[-1] == "mi355pt_denoise_var.h"
    declared = sorted(set(re.findall(r"\b(mi355pt_[a-z0-9_]+)\s*\(", code)))
    assert declared == sorted(NEW_SYMBOLS) == sorted("mi355pt_" + s for s in f.MOTION_SYMBOLS)
    assert not any(n in re.sub(r"/\*.*?\*/", "", main, flags=re.S) for n in NEW_SYMBOLS)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(r"pub fn %s\(" % name, rs), name
    assert re.search(r"typedef struct mi355pt_motion_xform \{.*?\} mi355pt_motion_xform;", code, flags=re.S)
    assert re.search(r"pub struct MotionXform \{\s*pub a: \[f32; 9\],\s*pub b: \[f32; 3\],\s*pub n: \[f32; 9\],\s*pub pad: \[f32; 3\],\s*\}", rs)
    assert ctypes.sizeof(f.MotionXform) == 96 == 4 * mr.ENTRY_WORDS
    assert (f.MotionXform.a.offset, f.MotionXform.b.offset, f.MotionXform.n.offset, f.MotionXform.pad.offset) == (0, 36, 48, 84)
    assert subprocess.call([sys.executable, os.path.join(f.ROOT, "tools", "gen_rust_binding.py"), "--check"]) == 0


@pytest.mark.parametrize("cams", [0, 1], ids=["camera_fixed", "camera_moved"])
def test_motion_table_matches_float64(pkg, cams):
    """mi355pt_motion_table against NumPy float64 (numpy.linalg.inv, the header's formulas as written) for translations, rotations, a
    non-uniform scale change and all of them under a camera move.  Every entry is within ONE f32 rounding of the float64 value: half an
    f32 ulp of the value, plus what two float64 evaluations of the entry by different routes can differ by — 1e-13 of the largest term of
    the entry's sum, which for b (a difference of terms of a few units) is the only part that counts near zero.  Entry 0 and the entry of a
    bytewise unmoved instance are EXACTLY identity and delta — delta with the bits of mi355pt_temporal_view_from_cameras — and pad is 0."""
    prod = pkg.Product()
    cur, prev = CAMERAS[cams]
    fc, fp = ffi_camera(pkg, cur), ffi_camera(pkg, prev)
    l2w_prev, l2w_cur = [p for p, _ in POSES], [c for _, c in POSES]
    got = prod.motion_table(fc, fp, l2w_cur, l2w_prev)
    want = mr.table64(cur, prev, l2w_cur, l2w_prev)
    assert got.shape == want.shape == (len(POSES) + 1, mr.ENTRY_WORDS)
    delta = np.array(list(prod.temporal_view_from_cameras(fc, fp).delta), F)
    static = mr.static_table(tr.view_from_cameras(cur, prev), 1)[0]
    assert np.array_equal(bits(static[9:12]), bits(delta))
    for e in (0, 1):                                                     # the static entry, and POSES[0], which did not move
        assert np.array_equal(bits(got[e]), bits(static)), e
    assert not got[:, 21:].any()
    cc = np.abs(np.asarray(cur.position, np.float64)).max() + np.abs(np.asarray(prev.position, np.float64)).max()
    for e in range(2, len(POSES) + 1):
        w = want[e]
        scale = np.abs(w[0:9]).max() * (cc + 10.0) + 10.0               # the largest term of any sum behind an entry (positions below 10)
        tol = 0.5 * np.spacing(np.abs(w).astype(F)).astype(np.float64) + 1e-13 * scale
        err = np.abs(got[e].astype(np.float64) - w)
        assert (err <= tol).all(), (e, np.argmax(err - tol), err.max())
        assert not np.array_equal(got[e, :21], static[:21])


def test_motion_table_refusals(pkg):
    """MI355PT_E_INVALID for null pointers, n == 0, a non-finite and a singular matrix (also of an instance that did not move); the output
    keeps its bytes"""
    prod = pkg.Product()
    cur, prev = CAMERAS[1]
    fc, fp = ffi_camera(pkg, cur), ffi_camera(pkg, prev)
    good = np.ascontiguousarray(np.stack([trs((1.0, 0.0, -3.0)), trs((0.0, 1.0, -2.0), angle=0.3)]).transpose(0, 2, 1)).reshape(2, 16)   # column-major, as the C ABI takes them
    out = np.full((3, mr.ENTRY_WORDS), 7.0, F)
    fn = prod.lib.mi355pt_motion_table
    call = lambda a, b, mc, mp, n, o: fn(ctypes.byref(a) if a is not None else None, ctypes.byref(b) if b is not None else None,   # noqa: E731
                                         mc.ctypes.data if mc is not None else None, mp.ctypes.data if mp is not None else None, n,
                                         o.ctypes.data if o is not None else None)
    assert call(fc, fp, good, good, 2, out) == 0
    out[:] = 7.0
    for args in ((None, fp, good, good, 2, out), (fc, None, good, good, 2, out), (fc, fp, None, good, 2, out), (fc, fp, good, None, 2, out),
                 (fc, fp, good, good, 2, None), (fc, fp, good, good, 0, out)):
        assert call(*args) == -1 and b"motion table" in prod.lib.mi355pt_last_error()
    for k, v in ((5, np.nan), (12, np.inf)):
        bad = good.copy(); bad[1, k] = v
        assert call(fc, fp, bad, good, 2, out) == -1 and call(fc, fp, good, bad, 2, out) == -1
    flat = good.copy(); flat[0, [0, 4, 8]] = 0.0                          # a zero row: singular
    assert call(fc, fp, flat, good, 2, out) == -1 and call(fc, fp, good, flat, 2, out) == -1 and call(fc, fp, flat, flat, 2, out) == -1
    assert b"singular" in prod.lib.mi355pt_last_error()
    assert (out == 7.0).all()


@pytest.mark.parametrize("cams", [0, 1], ids=["camera_fixed", "camera_moved"])
def test_round_trip_through_entry_and_previous_view(pkg, cams):
    """Local points of an object placed by l2w_cur, in the current render space, carried through the object's entry (binary32, the header's
    order) and then through project() of the previous view, land where the same local points placed by l2w_prev land in the previous
    image.  The tolerance is derived per point from the f32 roundings involved, in pixels:
      coordinates   the current render-space point is rounded to f32 (2^-24 |X| per component); the entry's twelve numbers are f32 (2^-24
                    of each term); the three products and three sums per component round once each: <= 8 x 2^-24 x (sum of the terms'
                    magnitudes) per component of Xp;
      projection    a coordinate error d at depth zc moves the pixel by at most  d (1 + |v| / zc) sx / zc  (the quotient rule), and the
                    view's own f32 entries and the quotient's roundings add  8 x 2^-24 x (|f| + |c|);
    doubled for the two routes."""
    prod = pkg.Product()
    cur, prev = CAMERAS[cams]
    view = tr.view_from_cameras(cur, prev)
    table = prod.motion_table(ffi_camera(pkg, cur), ffi_camera(pkg, prev), [c for _, c in POSES], [p for p, _ in POSES])
    rng = np.random.default_rng(5)
    local = rng.uniform(-0.5, 0.5, (200, 3))
    u = 2.0 ** -24
    for i, (mp, mc) in enumerate(POSES):
        Xc = (local @ mr.mat4(mc)[:3, :3].T + mr.mat4(mc)[:3, 3]) - np.asarray(cur.position, np.float64)
        Xw_prev = (local @ mr.mat4(mp)[:3, :3].T + mr.mat4(mp)[:3, 3]) - np.asarray(cur.position, np.float64)   # as the static projection takes it: + delta
        e = table[i + 1]
        Xp = mr.apply_entry(e, Xc.astype(F), F)
        fx, fy, zc = tr.project(view, Xp.astype(np.float64) - np.asarray(view.delta, np.float64))
        wx, wy, wz = tr.project(view, Xw_prev)
        keep = (zc > 0.5) & (wz > 0.5)
        assert keep.sum() > 100
        mag = np.abs(Xc) @ np.abs(e[0:9].reshape(3, 3).astype(np.float64)).T + np.abs(e[9:12].astype(np.float64))
        d = 8.0 * u * mag.max(axis=1)
        r = np.asarray(view.rows, np.float64)
        v = np.abs(Xp.astype(np.float64) @ r.reshape(3, 3).T).max(axis=1)
        s = max(float(view.sx), float(view.sy))
        tol = 2.0 * (d * 3.0 * (1.0 + v / zc) * s / zc + 8.0 * u * (np.abs(fx) + np.abs(fy) + float(view.cx) + float(view.cy)))
        err = np.maximum(np.abs(fx - wx), np.abs(fy - wy))
        assert (err[keep] <= tol[keep]).all(), (i, float(err[keep].max()), float(tol[keep].min()))
        assert tol[keep].max() < 1e-2                                     # the derived tolerance is far below a pixel


@pytest.mark.parametrize("half", [True, False], ids=["half", "nohalf"])
@pytest.mark.parametrize("view", ["static", "move", "outside", "behind"])
def test_restatement_with_static_entries_is_the_static_restatement(view, half):
    """motion_reference.accumulate_motion with a table of static entries and no previous ids IS temporal_reference.accumulate, bit for bit —
    whatever the ids are, ids above the table included — and the rectified pair likewise; with a moved entry or with previous ids it is not."""
    W, H = 70, 50
    cur, prev, vw, spp = tr.synthetic(W, H, view, "step", half)
    ids_cur, ids_prev = mr.synthetic_ids(W, H)
    table = mr.static_table(vw, 3)
    for want, got in ((tr.accumulate(cur, spp, prev, vw), mr.accumulate_motion(cur, spp, prev, vw, ids_cur, None, table)),
                      (rr.accumulate(cur, spp, prev, vw), mr.accumulate_rectified_motion(cur, spp, prev, vw, ids_cur, None, table))):
        for a, b in zip(want, got):
            assert (a is None) == (b is None)
            if a is not None:
                assert np.array_equal(bits(a), bits(b))
    assert rr.tr is tr                                                   # the rectified restatement has its own gather back
    base = tr.accumulate(cur, spp, prev, vw)
    if view in ("static", "move"):
        moved = table.copy(); moved[1] = mr.moved_entry(vw)
        assert not np.array_equal(bits(mr.accumulate_motion(cur, spp, prev, vw, ids_cur, None, moved)[0]), bits(base[0]))
        assert not np.array_equal(bits(mr.accumulate_motion(cur, spp, prev, vw, ids_cur, ids_prev, table)[0]), bits(base[0]))
    first = mr.accumulate_motion(cur, spp, None, None, ids_cur, None, table)
    assert np.array_equal(bits(first[0]), bits(tr.accumulate(cur, spp)[0]))


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    """tests/motion_plan_check.cpp built with plain g++ (the header needs no HIP) and, a second time, with the host sanitizers"""
    def build(name, extra):
        exe = str(tmp_path_factory.mktemp(name) / "motion_plan_check")
        subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror"] + extra +
                       ["-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "motion_plan_check.cpp")], check=True)
        return exe
    return build("plain", []), build("sanitized", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def test_plan_header_is_pure(plan_check):
    text = open(os.path.join(CSRC, "motion_plan.hpp")).read()
    assert not re.search(r"#\s*include\s*[<\"]hip|getenv|chrono|clock_gettime|gettimeofday|atomic", text)


@pytest.mark.parametrize("seed,n", [(1, 0), (2, 1), (3, 5), (4, 64), (5, 1000)])
def test_plan_arithmetic(plan_check, seed, n):
    """the stand-alone program's own checks — exact static entries, the round trip in long double, n^T a = I, the refusals — plain and
    under ASan + UBSan"""
    for exe in plan_check:
        r = subprocess.run([exe, str(seed), str(n)], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
