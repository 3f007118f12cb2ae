"""The bloom stage (include/mi355pt_bloom.h), the part that needs no GPU: the ABI surface of the cross-compiled library, the defaults, the
refusals of tests/golden/bloom_refusals.json through the library and through the pure predicate's check program, the plan of
csrc/bloom_plan.hpp through a host check program, the properties of the NumPy restatement (tests/bloom_reference.py) that the GPU tests lean
on, and the CLI's argument errors."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bloom_reference as br  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "toy-cpu-pathtracing_amd", "csrc")
NEW_SYMBOLS = ["mi355pt_bloom_params_default", "mi355pt_bloom_scratch_bytes", "mi355pt_bloom_device", "mi355pt_bloom"]
E_INVALID = -1
F32 = np.float32
U = 2.0 ** -24      # the unit roundoff of binary32: one rounded operation moves a value by at most this, relatively


def ffi_params(product, prm):
    p = product.bloom_params_default()
    for k in br.FIELDS:
        setattr(p, k, (float if k in br.FLOAT_FIELDS else int)(getattr(prm, k)))
    return p


# ---------------- the ABI surface, the defaults ----------------
def test_bloom_abi_surface_and_defaults(pkg):
    """The header declares the four entry points and the struct; mi355pt.h includes it right after the edit block's, ahead of the
    variance-guided denoiser's (which stays last), and declares nothing of it itself; the library exports the symbols; the ctypes mirror has
    the header struct's fields, 32 bytes, and the documented defaults; the generated Rust binding names everything and is what the headers
    generate.  (Fails on a tree without the stage: there is no such header.)"""
    lib = ctypes.CDLL(pkg.ffi.LIB_PATH)
    root = pkg.ffi.ROOT
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "mi355pt_bloom.h")).read(), flags=re.S)
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "mi355pt.h")).read(), flags=re.S)
    rs = open(os.path.join(root, "bindings", "rust", "mi355pt_sys.rs")).read()
    includes = re.findall(r'#include "(mi355pt_\w+\.h)"', main)
    assert includes.index("mi355pt_edit.h") + 1 == includes.index("mi355pt_bloom.h") == len(includes) - 2 and includes[-1] == "mi355pt_denoise_var.h"
    assert "mi355pt_bloom_" not in main
    declared = sorted(set(re.findall(r"\b(mi355pt_[a-z0-9_]+)\s*\(", code)))
    assert declared == sorted(NEW_SYMBOLS)
    assert sorted("mi355pt_" + s for s in pkg.ffi.BLOOM_SYMBOLS) == declared
    assert not set(pkg.ffi.BLOOM_SYMBOLS) & set(pkg.ffi.ABI_SYMBOLS)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(r"pub fn %s\(" % name, rs), name
    m = re.search(r"typedef struct mi355pt_bloom_params \{(.*?)\} mi355pt_bloom_params;", code, flags=re.S)
    fields = [n.strip() for decl in m.group(1).split(";") if decl.strip() for n in decl.strip().split(" ", 1)[1].split(",")]
    assert fields == [f[0] for f in pkg.ffi.BloomParams._fields_] == list(br.FIELDS) == list(br.DEFAULTS)
    assert ctypes.sizeof(pkg.ffi.BloomParams) == 4 * len(fields) == 32             # eight 32-bit fields, no padding
    assert re.search(r"pub struct BloomParams \{\s*" + r"\s*".join(r"pub %s: (u32|f32)," % f for f in fields) + r"\s*\}", rs)
    assert re.search(r"#define MI355PT_BLOOM_MAX_LEVELS 8\b", code) and pkg.ffi.BLOOM_MAX_LEVELS == br.MAX_LEVELS == 8
    assert subprocess.call([sys.executable, os.path.join(root, "tools", "gen_rust_binding.py"), "--check"]) == 0
    p = pkg.Product().bloom_params_default()
    want = dict(levels=6, firefly=1, threshold=0.0, knee=0.5, scatter=float(F32(0.7)), base=float(F32(1) - F32(0.04)), intensity=float(F32(0.04)), exposure=1.0)
    assert {k: getattr(p, k) for k in want} == want
    d = br.params()
    assert {k: getattr(p, k) for k in want} == {k: (float(getattr(d, k)) if k in br.FLOAT_FIELDS else getattr(d, k)) for k in want}


# ---------------- the plan ----------------
def compile_check(tmp_path_factory, name):
    exe = str(tmp_path_factory.mktemp(name) / name)
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", name + ".cpp")], check=True)
    return exe


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    exe = compile_check(tmp_path_factory, "bloom_plan_check")

    def run(cases):
        r = subprocess.run([exe], input="".join("%d %d %d\n" % c for c in cases), capture_output=True, text=True, check=True)
        rows = [[int(v) for v in line.split()] for line in r.stdout.splitlines()]
        assert len(rows) == len(cases)
        return [dict(levels=row[0], scratch=row[1], tile=tuple(row[2:6]), level=[tuple(row[6 + 5 * i:11 + 5 * i]) for i in range((len(row) - 6) // 5)]) for row in rows]
    return run


PLAN_SIZES = br.SHAPES + [(63, 15), (64, 16), (65, 17), (256, 64), (2, 2), (3, 1), (1920, 1080), (3840, 2160), (4097, 4095), (1 << 24, 1), (1, 1 << 24), (1 << 24, 1 << 7),
                          ((1 << 24) - 1, 255), (65536, 65535)]


def test_bloom_plan_matches_the_restatement(pkg, planner):
    """bloom_plan.hpp through the host check program, for frames from 1 x 1 to 2^24 wide and every level count: the level sizes halve rounding
    up and stay at 1, the offsets are the running sum of the sizes, the scratch size is 16 bytes per record and equals
    mi355pt_bloom_scratch_bytes and the restatement's, the reductions' grids cover every destination pixel with their tiles and the expansions'
    with their blocks, and neither grid exceeds what a one-dimensional launch takes; calls the stage refuses have an empty plan and size 0."""
    lib = pkg.Product().lib
    cases = [(w, h, L) for w, h in PLAN_SIZES for L in range(1, 9)]
    for (w, h, L), p in zip(cases, planner(cases)):
        tx, ty, ux, uy = p["tile"]
        sizes, (offs, total) = br.level_sizes(w, h, L), br.level_offsets(w, h, L)
        assert p["levels"] == L and len(p["level"]) == L + 1, (w, h, L, p)
        assert p["scratch"] == 16 * total == br.scratch_bytes(w, h, L) == lib.mi355pt_bloom_scratch_bytes(w, h, L), (w, h, L, p)
        for l, (lw, lh, off, down, up) in enumerate(p["level"]):
            assert (lw, lh) == sizes[l] and off == offs[l], (w, h, L, l, p)
            assert down == (0 if l == 0 else -(-lw // tx) * -(-lh // ty)) and up == (0 if l == L else -(-lw // ux) * -(-lh // uy)), (w, h, L, l, p)
            assert down < 1 << 31 and up < 1 << 31
        if L == 8 and max(w, h) <= 256:
            assert sizes[-1] == (1, 1)                                            # the chain bottoms out
    assert planner([(1, 1, 8)])[0]["scratch"] == 16 * 8 and planner([(64, 64, 3)])[0]["scratch"] == 16 * (32 * 32 + 16 * 16 + 8 * 8)
    bad = [(0, 5, 1), (5, 0, 1), ((1 << 24) + 1, 1, 1), (1, (1 << 24) + 1, 1), (1 << 16, 1 << 16, 1), (1 << 24, 1 << 8, 1), (8, 8, 0), (8, 8, 9), (8, 8, 0xffffffff)]
    for (w, h, L), p in zip(bad, planner(bad)):
        assert p["levels"] == 0 and p["scratch"] == 0 and p["level"] == [] and lib.mi355pt_bloom_scratch_bytes(w, h, L) == 0 == br.scratch_bytes(w, h, L), (w, h, L, p)
    assert planner([(8, 8, 1)])[0]["tile"] == (32, 8, 64, 4)                      # what tests/test_bloom_gpu.py takes its edge shapes from


# ---------------- the refusals ----------------
def refusal_cases():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "bloom_refusals.json")))


def params_of(case, f):
    if case["params"] is None:
        return None
    p = f.BloomParams()
    for k, v in case["params"].items():
        setattr(p, k, float(br.from_bits(np.array([v], np.uint32))[0]) if k in br.FLOAT_FIELDS else v)
    return p


def test_bloom_refusals_before_the_device(pkg):
    """Every case of the fixture through the library: a refusal returns MI355PT_E_INVALID with a message that names "bloom" — from the device
    form and, where the case applies to it, from the host form —, with no device present (a call that got past the checks would answer
    MI355PT_E_DEVICE), and no buffer is touched; a case the checks let through comes back from the host form with anything but E_INVALID."""
    doc = refusal_cases()
    prod = pkg.Product()
    lib = prod.lib
    lib.mi355pt_last_error.restype = ctypes.c_char_p
    arena = np.full(doc["arena_bytes"] + 16, 7, np.uint8)
    base = (arena.ctypes.data + 15) & ~15
    at = lambda off: None if off is None else base + off   # noqa: E731
    assert len(doc["cases"]) > 60 and {c["verdict"] for c in doc["cases"]} >= {"NULL_POINTER", "SPP_ZERO", "EMPTY_FRAME", "FRAME_TOO_LARGE", "LEVELS", "FIREFLY", "THRESHOLD", "KNEE",
                                                                              "SCATTER", "BASE", "INTENSITY", "EXPOSURE", "SCRATCH_TOO_SMALL", "MISALIGNED", "OVERLAP", "OK"}
    for c in doc["cases"]:
        p = params_of(c, pkg.ffi)
        ref = ctypes.byref(p) if p is not None else None
        if c["verdict"] == "OK":
            if c["forms"] == "both":
                assert lib.mi355pt_bloom(at(c["film"]), c["width"], c["height"], c["spp"], ref, at(c["record"]), at(c["out"])) != E_INVALID, c["name"]
                arena[:] = 7
            continue
        rc = lib.mi355pt_bloom_device(at(c["film"]), c["width"], c["height"], c["spp"], ref, at(c["record"]), at(c["scratch"]), c["scratch_bytes"], at(c["out"]), None)
        assert rc == E_INVALID and b"bloom" in lib.mi355pt_last_error(), (c["name"], rc, lib.mi355pt_last_error())
        if c["forms"] == "both":
            rc = lib.mi355pt_bloom(at(c["film"]), c["width"], c["height"], c["spp"], ref, at(c["record"]), at(c["out"]))
            assert rc == E_INVALID and b"bloom" in lib.mi355pt_last_error(), (c["name"], rc, lib.mi355pt_last_error())
        assert (arena == 7).all(), c["name"]


def test_bloom_refusals_through_the_pure_predicate(tmp_path_factory):
    """The same fixture through csrc/bloom_checks.hpp alone, compiled with plain g++ (no HIP, no library): the verdict of every case, for the
    device form and, where the case applies to it, the host form — which never looks at the scratch buffer."""
    exe = compile_check(tmp_path_factory, "bloom_checks_check")
    doc = refusal_cases()
    base = 1 << 28
    lines, want = [], []
    for c in doc["cases"]:
        p = c["params"] or {k: 0 for k in br.FIELDS}
        for device in ((1, 0) if c["forms"] == "both" else (1,)):
            lines.append(" ".join(str(v) for v in [device] + [0 if c[k] is None else base + c[k] for k in ("film", "out", "scratch", "record")] +
                                  [c["scratch_bytes"], c["width"], c["height"], c["spp"], int(c["params"] is not None)] + [p[k] for k in br.FIELDS]))
            want.append(c["verdict"])
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
    got = r.stdout.split()
    assert len(got) == len(want)
    assert [(c, g) for c, g, w in zip(lines, got, want) if g != w] == []


# ---------------- properties of the restatement ----------------
def ops_on_the_path(levels, firefly=False):
    """The longest chain of rounded operations between a film value and a value of B (the weights of every step are positive, so a sum's
    relative error is at most its operands' worst plus its own rounding): the clean's division 1; a reduction 6 (per axis: the inner sum, the
    product by 3, the outer sum; the scalings by powers of two are exact), with the weights 8 more on the first (the product by w, the
    quotient, and the denominator's own six); an expansion 4 (per axis the product by 3 and the sum); a mix 3 (a product, the sum, and
    s0 + s1 differing from 1 by a rounding of s0)."""
    return 1 + 6 * levels + (8 if firefly else 0) + 4 * levels + 3 * (levels - 1)


def test_restatement_scales_exactly():
    """threshold 0, no weights: the whole stage is linear, and every rounding commutes with a power of two — a film times 2^j gives exactly out
    times 2^j, at every shape of the GPU tests and for 1, 3 and 8 levels (no value becomes subnormal or overflows: asserted)."""
    for (w, h) in br.SHAPES:
        film, spp = br.film(w, h, "hdr")
        for L in (1, 3, 8):
            prm = br.params(levels=L, firefly=0)
            ref = br.bloom(film, spp, prm)
            assert ref.out.min() > 2.0 ** -100 and ref.out.max() < 2.0 ** 100
            for j in (-7, 5):
                got = br.bloom((film * F32(2.0 ** j)).astype(np.float32), spp, prm)
                assert np.array_equal(br.bits(got.out), br.bits((ref.out * F32(2.0 ** j)).astype(np.float32))), (w, h, L, j)
                assert np.array_equal(br.bits(got.scratch), br.bits((ref.scratch * F32(2.0 ** j)).astype(np.float32))), (w, h, L, j)


@pytest.mark.parametrize("firefly", [0, 1])
def test_restatement_sub_threshold_film_is_untouched(firefly):
    """A film wholly below T - k: B is +0 everywhere and out is c base, bit for bit — with a record's exposure and with params.exposure."""
    film, spp = br.film(67, 19, "hdr")
    c = br.clean(film, spp)
    top = float(c.max())
    for record, exposure in ((None, 0.5), (br.record(0.25), 1.0)):
        E = exposure if record is None else 0.25
        prm = br.params(firefly=firefly, threshold=4.0 * top * E, knee=0.5, base=0.75, intensity=2.0, exposure=exposure, levels=5)
        assert float(prm.threshold) / E * 0.5 > top                                # T - k = T / 2 is above every value
        ref = br.bloom(film, spp, prm, record)
        assert not br.bits(ref.B).any() and not br.bits(ref.scratch).any()
        assert np.array_equal(br.bits(ref.out), br.bits((c * F32(0.75)).astype(np.float32)))
    ref = br.bloom(film, spp, br.params(firefly=firefly, threshold=top * 0.01, knee=0.5, levels=5))
    assert ref.B.min() > 0                                                          # ... and a threshold inside the range lets light through


@pytest.mark.parametrize("firefly, threshold", [(0, 0.0), (1, 0.0), (0, 1.5), (1, 1.5)])
def test_restatement_arbitrary_bit_patterns_give_no_nan(firefly, threshold):
    """Films of arbitrary u32 patterns — NaN, both infinities, negatives, subnormals, huge values — and the films of specials of the GPU
    tests: every level and the output hold no NaN and nothing negative (no -0 either); the bloom itself is finite; +inf appears in the output
    only where c base + B intensity overflows binary32 (computed in float64)."""
    flt_max = float(np.finfo(np.float32).max)
    for (w, h), kind, seed in (((33, 17), "bits", 0), ((67, 19), "bits", 1), ((130, 10), "bits", 2), ((1, 64), "bits", 3), ((33, 17), "specials", 0)):
        film, spp = br.film(w, h, kind, seed)
        assert np.isnan(film).any() and np.isinf(film).any() and (film < 0).any()
        for base, intensity in ((0.96, 0.04), (1.0, 16.0)):
            prm = br.params(firefly=firefly, threshold=threshold, knee=0.5, base=base, intensity=intensity)
            ref = br.bloom(film, spp, prm)
            for a in (ref.out, ref.scratch, ref.B, *ref.D[1:]):
                assert not np.isnan(a).any() and not np.signbit(a).any()
            assert np.isfinite(ref.B).all() and np.isfinite(ref.scratch).all()
            exact = br.clean(film, spp).astype(np.float64) * float(prm.base) + ref.B.astype(np.float64) * float(prm.intensity)
            assert not (np.isinf(ref.out) & (exact < flt_max)).any()


def test_restatement_impulse_keeps_its_energy():
    """One interior texel of 100 in a 64 x 64 frame (every level's size is even down to 8 x 8 and 4 x 4, where the clamped borders keep the
    weights' sums: a reduction takes a quarter of the sum, an expansion gives four times it), no threshold, no weights, any scatter: the sum
    of B is the impulse's energy within ops_on_the_path(L) roundings, relatively."""
    for L in (3, 4):
        for scatter in (0.7, 0.0, 1.0):
            film = np.zeros((64, 64, 3), np.float32)
            film[29, 37] = (100.0, 50.0, 25.0)
            ref = br.bloom(film, 1, br.params(levels=L, firefly=0, scatter=scatter))
            total = ref.B.astype(np.float64).sum(axis=(0, 1))
            bound = 1.001 * ops_on_the_path(L) * U
            rel = np.abs(total / np.array([100.0, 50.0, 25.0]) - 1.0)
            print(f"impulse, L = {L}, scatter {scatter}: sum of B = {total[0]:.6f} for 100 (relative error {rel.max():.3g}, bound {bound:.3g})")
            assert (rel <= bound).all(), (L, scatter, total, bound)
            assert (ref.B > 0).sum() > 9 * 3 and ref.B.max() < 100.0 / 4                # it is spread


def test_restatement_firefly_weights_tame_an_outlier():
    """A film of 0.5 with one texel of 1e6: without the weights the blurred maximum is the outlier's share, tens of thousands; with them the
    first reduction averages by 1 / (1 + Y) and the maximum falls by orders of magnitude, below twice the film's value."""
    film = np.full((64, 64, 3), 0.5, np.float32)
    film[31, 30] = 1e6
    plain = br.bloom(film, 1, br.params(firefly=0))
    tamed = br.bloom(film, 1, br.params(firefly=1))
    print(f"blurred maximum without the weights {plain.B.max():.1f}, with them {tamed.B.max():.4f}")
    assert plain.B.max() > 1e4 and tamed.B.max() < 1.0 and tamed.B.min() >= 0.5 * (1 - 200 * U)


@pytest.mark.parametrize("firefly", [0, 1])
def test_restatement_constant_film_stays_constant(firefly):
    """A constant film comes back as the constant — B and, with base = 1 - intensity, the output — within ops_on_the_path roundings (three
    more for the composite: its product, its sum, and base + intensity differing from 1 by a rounding of base), at odd shapes and 1 to 8
    levels: the clamped borders lose nothing."""
    for (w, h) in ((1, 1), (7, 5), (33, 17), (130, 10)):
        for L in (1, 3, 8):
            for v in (0.37, 1234.5):
                film = np.full((h, w, 3), v, np.float32) * F32(4)
                ref = br.bloom(film, 4, br.params(levels=L, firefly=firefly, scatter=0.6))
                n = ops_on_the_path(L, bool(firefly))
                vb = float(F32(v))
                assert np.abs(ref.B.astype(np.float64) / vb - 1).max() <= 1.001 * n * U, (w, h, L, v)
                assert np.abs(ref.out.astype(np.float64) / vb - 1).max() <= 1.001 * (n + 3) * U, (w, h, L, v)


def test_restatement_variants_cross_what_they_should():
    """The parameter sets the GPU tests run do reach what they are for: a threshold that cuts part of the film and passes part, through the knee
    and above it; a record that changes the result; scatter 0 and 1 as the two pure ends; and the scratch layout: U_1 .. U_{L-1}, D_L."""
    film, spp = br.film(67, 19, "specials")
    refs = {name: br.bloom(film, spp, br.params(levels=4, **kw), br.record() if rec else None) for name, kw, rec in br.VARIANTS}
    assert np.array_equal(br.bits(refs["record-no-threshold"].out), br.bits(refs["defaults"].out))      # without a threshold no exposure matters
    assert len({br.bits(r.out).tobytes() for r in refs.values()}) == len(refs) - 1
    for name, kw, rec in br.VARIANTS:
        if kw.get("threshold"):
            prm = br.params(**kw)
            cc = np.fmin(br.clean(film, spp), br.CAP)
            p = br.bright_pass(cc, prm, br.record() if rec else None)
            m, pm = cc.max(axis=-1), p.max(axis=-1)
            assert ((pm == 0) & (m > 0)).any() and (pm > 0).any() and (pm <= m).all(), name
    r = refs["defaults"]
    offs, total = br.level_offsets(67, 19, 4)
    assert r.scratch.shape == (total, 4) and not br.bits(r.scratch[:, 3]).any()
    for l in range(1, 5):
        n = r.U[l].shape[0] * r.U[l].shape[1]
        assert np.array_equal(r.scratch[offs[l]:offs[l] + n, :3].reshape(r.U[l].shape), r.U[l])
    assert r.U[4] is r.D[4] and not np.array_equal(r.U[1], r.D[1])
    assert np.array_equal(refs["scatter-0"].U[1], refs["scatter-0"].D[1])           # scatter 0: s0 = 1, the coarser levels add +0
    assert np.array_equal(br.bloom(film, spp, br.params(levels=1)).D[1], r.D[1])    # D_l does not depend on the level count


def test_bloom_cli_argument_errors(pkg, tmp_path):
    """The bloom flags' misuse — a sub-flag without --bloom, an AOV renderer, --gpus 2, values out of range or not numbers: exit status 2 with
    a message naming the flag, before any scene is loaded (no device needed); --help lists the flags."""
    exe = os.path.join(pkg.ffi.ROOT, "toy-cpu-pathtracing_amd", "host", "mi355pt")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.dirname(exe)])
    for args, flag in br.CLI_MISUSE:
        r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=60, cwd=tmp_path)
        assert r.returncode == 2 and flag in r.stderr and "Start build scene" not in r.stdout, (args, r.returncode, r.stderr)
    r = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and all(k in r.stdout for k in ("--bloom]", "--bloom-levels", "--bloom-threshold", "--bloom-knee", "--bloom-scatter", "--bloom-intensity",
                                                             "--bloom-additive", "--bloom-no-firefly"))
    assert not os.listdir(tmp_path)
