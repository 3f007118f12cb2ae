"""CPU-side tests of the robust film (include/mi355pt_robust.h): the ABI surface, the defaults and every refusal of the entry points —
reached without a device —, the coverage of the seeded generator the GPU parity tests run on (asserted, not assumed), properties of the NumPy
restatement (tests/robust_reference.py) and the CLI's argument errors."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import robust_reference as rr  # noqa: E402

F32 = np.float32
E_INVALID = -1


def test_robust_header_symbols_are_exported_and_mirrored(pkg):
    """every function include/mi355pt_robust.h declares is exported, ffi.ROBUST_SYMBOLS lists exactly those, mi355pt.h includes the header
    after the display block and before the variance-guided denoiser's, and the enum and the struct have the header's values and layout"""
    f = pkg.ffi
    lib = ctypes.CDLL(f.LIB_PATH)
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(f.ROOT, "include", "mi355pt_robust.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(mi355pt_[a-z0-9_]+)\s*\(", hdr)))
    assert declared == sorted("mi355pt_" + s for s in f.ROBUST_SYMBOLS) and len(declared) == 5
    for name in declared:
        assert hasattr(lib, name), name
    main = open(os.path.join(f.ROOT, "include", "mi355pt.h")).read()
    includes = re.findall(r'#include "(mi355pt_\w+\.h)"', main)
    assert includes.index("mi355pt_display.h") + 1 == includes.index("mi355pt_robust.h") and includes[-1] == "mi355pt_denoise_var.h"
    assert re.search(r"MI355PT_ROBUST_MEAN = 0, MI355PT_ROBUST_MOM = 1, MI355PT_ROBUST_GMON = 2", hdr)
    assert f.ROBUST_MODE == {"mean": rr.MEAN, "mom": rr.MOM, "gmon": rr.GMON}
    assert ctypes.sizeof(f.RobustParams) == 8 and f.RobustParams.mode.offset == 0 and f.RobustParams.gini_scale.offset == 4
    rs = open(os.path.join(f.ROOT, "bindings", "rust", "mi355pt_sys.rs")).read()
    assert "pub struct RobustParams" in rs and all("pub fn %s(" % n in rs for n in declared)


def test_robust_defaults(pkg):
    p = pkg.Product().robust_params_default()
    assert p.mode == rr.GMON and p.gini_scale == 1.0
    pkg.Product().lib.mi355pt_robust_params_default(None)        # a NULL output is ignored


def _combine_rc(prod, f, buckets=0x10000, k=8, spp=4, w=16, h=16, params="default", out=0x4000000, half=0, trim=0, host=False):
    """the return code of mi355pt_robust_combine(_device) on made-up pointers: every refusal comes before they are touched"""
    p = prod.robust_params_default() if isinstance(params, str) else params
    pp = ctypes.byref(p) if p is not None else None
    vp = ctypes.c_void_p
    if host:
        return prod.lib.mi355pt_robust_combine(vp(buckets), k, spp, w, h, pp, vp(out), vp(half), vp(trim))
    return prod.lib.mi355pt_robust_combine_device(vp(buckets), k, spp, w, h, pp, vp(out), vp(half), vp(trim), None)


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
def test_combine_refusals_come_before_the_device(pkg, host):
    """every refusal the header lists, with pointers that are not memory: a call that touched them, or the device, would not return -1"""
    f = pkg.ffi
    prod = pkg.Product()
    rc = lambda **kw: _combine_rc(prod, f, host=host, **kw)      # noqa: E731
    frame = 16 * 16 * 3 * 4
    assert rc(params=None) == E_INVALID and rc(buckets=0) == E_INVALID and rc(out=0) == E_INVALID
    for k in (0, 1, 2, 3, 5, 6, 12, 24, 33, 64):
        assert rc(k=k) == E_INVALID, k
    assert rc(spp=0) == E_INVALID
    assert rc(w=0) == E_INVALID and rc(h=0) == E_INVALID
    assert rc(w=(1 << 24) + 1, h=1) == E_INVALID and rc(w=1 << 16, h=1 << 16) == E_INVALID and rc(w=1 << 24, h=1 << 24) == E_INVALID
    assert rc(params=f.RobustParams(3, 1.0)) == E_INVALID and rc(params=f.RobustParams(0xFFFFFFFF, 1.0)) == E_INVALID
    for s in (float("nan"), float("inf"), -float("inf"), -1.0, -1e-30):
        assert rc(params=f.RobustParams(rr.GMON, s)) == E_INVALID, s
    base = 0x10000
    assert rc(out=base) == E_INVALID                                   # an output at the first bucket
    assert rc(out=base + 7 * frame) == E_INVALID                       # ... inside the last bucket
    assert rc(out=base + 8 * frame - 4) == E_INVALID
    assert rc(half=base + 3 * frame) == E_INVALID and rc(trim=base + 8 * frame - 1) == E_INVALID
    assert rc(out=base - frame + 4) == E_INVALID                       # ... whose end runs into the first bucket
    assert rc(half=0x4000000) == E_INVALID and rc(trim=0x4000000) == E_INVALID and rc(half=0x5000000, trim=0x5000000) == E_INVALID
    assert rc(half=0x4000000 + frame - 4) == E_INVALID
    msg = prod.lib.mi355pt_last_error
    msg.restype = ctypes.c_char_p
    assert b"robust combine" in msg()


def test_zeroed_params_are_mean_and_accepted_by_the_checks(pkg):
    """a zero-initialised struct is MEAN with scale 0: the parameter checks, which come first, let it through — the call is then refused
    for its frame, so nothing is launched on the made-up pointers"""
    f = pkg.ffi
    prod = pkg.Product()
    prod.lib.mi355pt_last_error.restype = ctypes.c_char_p
    assert _combine_rc(prod, f, params=f.RobustParams(3, 0.0), w=0) == E_INVALID and b"unknown mode" in prod.lib.mi355pt_last_error()
    assert _combine_rc(prod, f, params=f.RobustParams(), w=0) == E_INVALID
    assert b"zero width" in prod.lib.mi355pt_last_error()             # the params are checked first: the zeroed struct passed, the frame did not


def test_render_entry_refusals_come_before_the_device(pkg):
    """mi355pt_render_buckets_device and mi355pt_render_robust: NULL arguments, a bad K, spp not a multiple of K, collect_stats — refused
    on an unbuilt scene, before the scene or the device is looked at"""
    f = pkg.ffi
    prod = pkg.Product()
    sc = prod.new_scene()
    cam = f.make_camera((0, 0, 3), (0, 0, -1), (0, 1, 0), 16, 16)
    lib, vp = prod.lib, ctypes.c_void_p
    rp = prod.robust_params_default()
    buf = vp(0x10000)

    def buckets(prm, k, scene=sc.h, camera=cam, dst=buf):
        return lib.mi355pt_render_buckets_device(scene, ctypes.byref(camera) if camera is not None else None, ctypes.byref(prm) if prm is not None else None, k, dst, None, None)

    def robust(prm, k, params=rp, dst=buf):
        return lib.mi355pt_render_robust(sc.h, ctypes.byref(cam), ctypes.byref(prm), k, ctypes.byref(params) if params is not None else None, dst)
    ok = f.make_params(64)
    for k in (0, 2, 3, 5, 12, 64):
        assert buckets(ok, k) == E_INVALID and robust(ok, k) == E_INVALID, k
    for spp, k in ((20, 8), (63, 4), (16, 32), (0, 4)):
        assert buckets(f.make_params(spp), k) == E_INVALID and robust(f.make_params(spp), k) == E_INVALID, (spp, k)
    for cs in (1, 2):
        assert buckets(f.make_params(64, collect_stats=cs), 16) == E_INVALID and robust(f.make_params(64, collect_stats=cs), 16) == E_INVALID
    assert buckets(ok, 16, scene=None) == E_INVALID and buckets(ok, 16, camera=None) == E_INVALID and buckets(None, 16) == E_INVALID
    assert buckets(ok, 16, dst=None) == E_INVALID and robust(ok, 16, dst=None) == E_INVALID
    assert robust(ok, 16, params=None) == E_INVALID
    assert robust(ok, 16, params=f.RobustParams(7, 1.0)) == E_INVALID and robust(ok, 16, params=f.RobustParams(rr.GMON, float("nan"))) == E_INVALID
    assert buckets(ok, 16) == -3 and robust(ok, 16) == -3              # all of the above passed: MI355PT_E_NOT_BUILT, still without a device


# ---------------- the generator ----------------

@pytest.fixture(scope="module")
def stacks():
    """one stack per set size N at the parity tests' largest frame: K = N buckets (K = 4 for N = 2, whose sets are the even and odd buckets)"""
    out = {}
    for n in rr.SET_SIZES:
        k = max(n, 4)
        s = rr.make_stack(k, 37, 200, seed=100 + n).reshape(k, -1, 3)
        out[n] = [s] if n == k else [s[0::2], s[1::2]]
    return out


@pytest.mark.parametrize("n", rr.SET_SIZES)
def test_generator_reaches_every_branch(stacks, n):
    for s in stacks[n]:
        assert s.shape[0] == n
        d = rr.set_diagnostics(s, 4)
        assert sorted(set(d["t"].tolist())) == list(range(n // 2)), np.bincount(d["t"])      # every trim count 0 .. N/2 - 1 under GMON
        assert d["tie"].mean() >= 0.01 and d["s_zero"].any() and (~d["s_zero"]).any() and d["cleaned"].any()
        assert (np.sort(d["ranks"], axis=0) == np.arange(n)[:, None]).all()                  # the ranks are a permutation
        with np.errstate(all="ignore"):
            assert np.isnan(s).any() and (s == np.inf).any() and (s == -np.inf).any() and (s < 0).any()
    # scales 0.5 and 2 (the parity tests' others) move the trims and still reach both ends
    for scale in (0.5, 2.0):
        t = rr.set_diagnostics(stacks[n][0], 4, scale)["t"]
        assert t.min() == 0 and (n == 2 or t.max() >= (n // 2 - 1 if scale == 2.0 else n // 4 - 1))


# ---------------- properties of the restatement ----------------

def _stack(k, seed=7, h=9, w=31):
    return rr.make_stack(k, h, w, seed)


@pytest.mark.parametrize("k", rr.BUCKET_COUNTS)
def test_mean_is_the_ordered_sum_over_k(k):
    s = _stack(k)
    out, _, trim = rr.combine(s, 4, rr.MEAN)
    m = rr.clean_means(s, 4)
    acc = np.zeros(m.shape[1:], F32)
    for b in range(k):
        acc = (acc + m[b]).astype(F32)
    assert np.array_equal(rr.bits(out), rr.bits(acc / F32(k))) and not trim.any()
    out2, half, trim2 = rr.combine(s, 4, rr.MEAN, pair=True)
    e = np.zeros(m.shape[1:], F32); o = np.zeros(m.shape[1:], F32)
    for b in range(0, k, 2):
        e = (e + m[b]).astype(F32); o = (o + m[b + 1]).astype(F32)
    assert np.array_equal(rr.bits(half), rr.bits(e / F32(k // 2))) and np.array_equal(rr.bits(out2), rr.bits(e / F32(k // 2) + o / F32(k // 2))) and not trim2.any()


@pytest.mark.parametrize("k", rr.BUCKET_COUNTS)
def test_mom_of_identical_buckets_is_the_cleaned_mean(k):
    one = _stack(4)[0]
    s = np.repeat(one[None], k, axis=0)
    out, _, trim = rr.combine(s, 4, rr.MOM)
    # the two middle ranks of K equal buckets: (m + m) / 2 = m exactly (no overflow in the generator's range)
    assert np.array_equal(rr.bits(out), rr.bits(rr.clean_means(one, 4))) and (trim[..., 0] == k // 2 - 1).all()


@pytest.mark.parametrize("k", rr.BUCKET_COUNTS)
@pytest.mark.parametrize("j", [-3, 5])
def test_power_of_two_scaling_commutes(k, j):
    s = _stack(k)
    f = F32(2.0) ** j
    for pair in (False, True):
        a, ah, at = rr.combine(s, 4, rr.GMON, 1.0, pair)
        b, bh, bt = rr.combine((s * f).astype(F32), 4, rr.GMON, 1.0, pair)
        assert np.array_equal(at, bt) and np.array_equal(rr.bits(a * f), rr.bits(b))
        assert not pair or np.array_equal(rr.bits(ah * f), rr.bits(bh))


@pytest.mark.parametrize("k", rr.BUCKET_COUNTS)
def test_a_permutation_of_the_buckets_keeps_every_trim_count(k):
    """t is a function of the multiset of bucket luminances: ties get equal weights in S and adjacent ranks in Q.  The definition takes S
    and Q in bucket order, so on arbitrary values a permutation rounds them differently.  (1) On a stack whose sums are exact in binary32
    (rr.exact_stack) EVERY t is unchanged, in single and pair output (a permutation of the pairs (2i, 2i + 1), which keeps the two sets)
    and under every mode.  (2) On the generator's stack every t is unchanged except where g N / 2 lies within rounding (1e-4) of an
    integer, the step of floor(); those are fewer than 1 in 1000."""
    rng = np.random.default_rng(5)
    s = rr.exact_stack(k, 6000, seed=k)
    base = rr.combine(s, 1, rr.GMON)[2]
    assert len(set(base[..., 0].ravel().tolist())) == k // 2                     # every trim count occurs on this stack too
    for _ in range(3):
        perm = rng.permutation(k)
        assert np.array_equal(rr.combine(s[perm], 1, rr.GMON)[2], base)
        pairs = rng.permutation(k // 2)
        pperm = np.stack([2 * pairs, 2 * pairs + 1], 1).reshape(-1)
        for scale in (0.5, 1.0, 2.0):
            assert np.array_equal(rr.combine(s[pperm], 1, rr.GMON, scale, pair=True)[2], rr.combine(s, 1, rr.GMON, scale, pair=True)[2])
    s = _stack(k, seed=11, h=37, w=200)
    perm = rng.permutation(k)
    m = rr.clean_means(s, 4).reshape(k, -1, 3)
    l = rr.luminance(m)
    g = rr.gini(l, rr.ranks(l))[2]
    x = np.clip(g.astype(np.float64), 0, 1) * (k // 2)
    safe = np.abs(x - np.round(x)) > 1e-4
    t0 = rr.combine(s, 4, rr.GMON)[2][..., 0].reshape(-1)
    t1 = rr.combine(s[perm], 4, rr.GMON)[2][..., 0].reshape(-1)
    assert np.array_equal(t0[safe], t1[safe]) and (t0 != t1).mean() < 1e-3


def test_gmon_removes_the_fireflies_of_the_model():
    """the model of the block's motivation at K = 16: Gamma(8, 1/8) bucket means, probability 0.02 of an added 200, 20 000 pixels.
    GMON's RMSE against the firefly-free expectation 1 is below a tenth of MEAN's (the model gives about 0.1 against 7 - 8)."""
    s = rr.firefly_model(16, 20000, seed=1)
    rmse = {}
    for name, mode in rr.MODES.items():
        out = rr.combine(s, 1, mode)[0][..., 0].astype(np.float64)
        rmse[name] = float(np.sqrt(np.mean((out - 1.0) ** 2)))
    print(rmse)
    assert rmse["gmon"] < 0.1 * rmse["mean"] and rmse["mom"] < 0.1 * rmse["mean"]
    assert rmse["mean"] > 3.0 and rmse["gmon"] < 0.2


# ---------------- the CLI ----------------

def test_robust_cli_argument_errors(pkg, tmp_path):
    """The robust flags' misuse — K outside {4, 8, 16, 32}, --spp not a multiple of K, an AOV or G-buffer renderer, --gpus 2,
    --adaptive-threshold, --half-res, --temporal-frames, a bad mode or scale, a dependent flag without --robust-buckets: exit status 2 with
    a message naming the flag, before any scene is loaded (no device needed); --help lists the flags."""
    exe = os.path.join(pkg.ffi.ROOT, "toy-cpu-pathtracing_amd", "host", "mi355pt")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.dirname(exe)])
    for args, flag in rr.CLI_MISUSE:
        r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=60, cwd=tmp_path)
        assert r.returncode == 2 and flag in r.stderr and "Start build scene" not in r.stdout, (args, r.returncode, r.stderr)
    r = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and all(k in r.stdout for k in ("--robust-buckets", "--robust-mode", "--robust-scale"))
    assert not os.listdir(tmp_path)
