"""TEST INFRASTRUCTURE ONLY.  The NumPy restatement of include/mi355pt_upsample.h (the header's comment is the normative text): with
dtype=np.float32 every operation is rounded on its own, in the order the header states, and the device result must be BIT-EQUAL to it;
np.float64 is there for the property tests.  Also seeded synthetic frames at both resolutions, built from temporal_reference.raycast and
gbuffer_sums (the two-plane step, the plane, a background band) with an emitter patch, zero-albedo pixels and bad film values."""
import os
import sys
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import temporal_reference as tr  # noqa: E402

FLT_MAX = np.finfo(np.float32).max
GUIDES = ("albedo", "shading_normal", "position", "hit")
DEFAULTS = dict(pos_tol=0.01, normal_cos=0.9, emitter_tol=0.25, min_weight=0.01, albedo_eps=0.01)
OTHER = dict(pos_tol=0.5, normal_cos=-1.0, emitter_tol=0.0, min_weight=0.3, albedo_eps=0.25)      # every parameter off its default


def params(**kw):
    """the defaults of mi355pt_upsample_params_default as f32 values, with overrides"""
    d = dict(DEFAULTS); d.update(kw)
    return SimpleNamespace(**{k: np.float32(v) for k, v in d.items()})


def low_camera(cam):
    """mi355pt_upsample_low_camera on a camera of temporal_reference.camera"""
    assert cam.width % 2 == 0 and cam.height % 2 == 0
    return SimpleNamespace(position=list(cam.position), direction=list(cam.direction), up=list(cam.up), width=cam.width // 2, height=cam.height // 2,
                           fov_deg=cam.fov_deg)


def clean(x):
    return np.where((x > 0) & (x <= FLT_MAX), x, 0).astype(x.dtype)


def clip0(x):
    return np.where(x > 0, x, 0).astype(x.dtype)


def footprint(W, H):
    """-> (x0 (1, W), y0 (H, 1), wx, wy as float64 arrays of the same shapes, parent X (1, W), parent Y (H, 1))"""
    x, y = np.arange(W, dtype=np.int64)[None, :], np.arange(H, dtype=np.int64)[:, None]
    X, Y = x >> 1, y >> 1
    xe, ye = (x & 1) == 0, (y & 1) == 0
    return X - xe, Y - ye, np.where(xe, 0.75, 0.25), np.where(ye, 0.75, 0.25), X, Y


def upsample(low_film, low_half, spp, low, spp_albedo_low, full, spp_albedo_full, prm=None, dtype=np.float32, detail=False):
    """mi355pt_upsample: low_film / low_half (h, w, 3) sums (low_half may be None); low / full map guide names to (h, w, 3) / (H, W, 3)
    arrays, albedo missing or None on both sides or on neither.  -> (out_film, out_half or None) in `dtype` (and a dict with detail=True:
    valid (4 masks), fallback, surface, Wt, c, m)"""
    dt = dtype
    prm = prm if prm is not None else params()
    A = lambda v: np.asarray(v, dt)   # noqa: E731
    H, W = full["hit"].shape[:2]
    h, w = H // 2, W // 2
    assert H % 2 == 0 and W % 2 == 0 and np.shape(low_film)[:2] == (h, w) and low["hit"].shape[:2] == (h, w)
    has_half = low_half is not None
    has_albedo = full.get("albedo") is not None
    assert has_albedo == (low.get("albedo") is not None)
    B = A(low_film)
    with np.errstate(all="ignore"):
        if has_half:
            Hf, hs = A(low_half), dt(spp // 2)
            c = [clean(Hf / hs), clean((B - Hf) / hs)]
        else:
            c = [clean(B / dt(spp))]
        hit = A(full["hit"])
        hp = hit[..., 1]
        surface = hp > 0
        Xp = A(full["position"]) / hp[..., None]
        nrm = dt(2) * (A(full["shading_normal"]) / hp[..., None]) - dt(1)
        t, em = hit[..., 0] / hp, hit[..., 2] / hp
        tol = dt(prm.pos_tol) * t
        dot = lambda a, b: (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]   # noqa: E731
        x0, y0, wx, wy, PX, PY = footprint(W, H)
        wx, wy = wx.astype(dt), wy.astype(dt)
        omx, omy = dt(1) - wx, dt(1) - wy
        bw = [omx * omy, wx * omy, omx * wy, wx * wy]
        l_hit, l_pos, l_nrm = A(low["hit"]), A(low["position"]), A(low["shading_normal"])
        if has_albedo:
            l_den = clip0(A(low["albedo"]) / dt(spp_albedo_low)) + dt(prm.albedo_eps)
            re = clip0(A(full["albedo"]) / dt(spp_albedo_full)) + dt(prm.albedo_eps)
        wk, vals, valids = [], [[] for _ in c], []
        for k in range(4):
            qx, qy = x0 + (k & 1) + 0 * y0, y0 + (k >> 1) + 0 * x0
            inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
            ix, iy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
            hq = l_hit[iy, ix, 1]
            e = Xp - l_pos[iy, ix] / hq[..., None]
            pd = np.abs(dot(e, nrm))
            nq = dt(2) * (l_nrm[iy, ix] / hq[..., None]) - dt(1)
            nd = dot(nrm, nq)
            ed = np.abs(em - l_hit[iy, ix, 2] / hq)
            same = (hq > 0) & (pd <= tol) & (nd >= dt(prm.normal_cos)) & (ed <= dt(prm.emitter_tol))
            valid = inside & np.where(surface, same, hq == 0)
            valids.append(valid)
            wk.append(np.where(valid, bw[k], dt(0)).astype(dt))
            for s, cs in enumerate(c):
                v = cs[iy, ix]
                if has_albedo:
                    v = np.where(surface[..., None], v / l_den[iy, ix], v)
                vals[s].append(np.where(valid[..., None], v, dt(0)).astype(dt))
        Wt = ((wk[0] + wk[1]) + wk[2]) + wk[3]
        has = Wt > dt(prm.min_weight)
        w3 = [x[..., None] for x in wk]
        m = []
        for s, cs in enumerate(c):
            v = vals[s]
            i = (((w3[0] * v[0] + w3[1] * v[1]) + w3[2] * v[2]) + w3[3] * v[3]) / Wt[..., None]
            if has_albedo:
                i = np.where(surface[..., None], i * re, i)
            parent = cs[PY + 0 * PX, PX + 0 * PY]
            m.append(np.where(has[..., None], i, parent).astype(dt))
    out = (m[0] + m[1], m[0]) if has_half else (m[0], None)
    if detail:
        return out + (dict(valid=valids, fallback=~has, surface=surface, Wt=Wt, c=c, m=m),)
    return out


def replicate(low):
    """pixel replication: low pixel (X, Y) to its four full pixels"""
    return np.repeat(np.repeat(np.asarray(low), 2, axis=0), 2, axis=1)


# ---------------- seeded synthetic frames ----------------
def guides(cam, scene, rng, spp_g=16, albedo=True):
    """the raw G-buffer sums of one resolution: temporal_reference.gbuffer_sums, an emitter patch (hit.z = hit.y on a disc of the image) and
    an albedo film that varies smoothly in the world-space hit position, with seeded pixels of albedo 0"""
    g, hit = tr.gbuffer_sums(cam, scene, rng, spp_g)
    X, _, _ = tr.raycast(cam, scene)
    P = X + np.asarray(cam.position, np.float64)
    patch = hit & ((P[..., 0] - 0.6) ** 2 + (P[..., 1] + 0.5) ** 2 < 0.3)
    g["hit"][..., 2] = np.where(patch, g["hit"][..., 1], 0.0)
    if albedo:
        a = 0.5 + 0.4 * np.stack([np.sin(3.0 * P[..., 0]), np.cos(2.0 * P[..., 1]), np.sin(P[..., 0] + P[..., 1])], -1)
        a = np.where(hit[..., None], a, 0.0)
        a[rng.random(hit.shape) < 0.05] = 0.0
        g["albedo"] = (a * spp_g).astype(np.float32)
    return g, hit


def synthetic(W, H, scene="step", half=True, albedo=True, spp=4, seed=11, bad=True, spp_g=16):
    """-> (low_film, low_half or None, spp, low guides, full guides, spp_g): the full and the low camera look at the same synthetic scene; the
    low film and half film are HDR noise SUMS with NaN / inf / negative values among them when `bad`"""
    rng = np.random.default_rng([seed, W, H, 1 if scene == "step" else 0])
    cam = tr.camera(width=W, height=H)
    full, _ = guides(cam, scene, rng, spp_g, albedo)
    low, _ = guides(low_camera(cam), scene, rng, spp_g, albedo)
    h, w = H // 2, W // 2
    hf = tr.hdr(rng, (h, w, 3)) * (spp // 2)
    film = hf + tr.hdr(rng, (h, w, 3)) * (spp - spp // 2)
    if bad:
        for buf in (film, hf):
            k = rng.integers(0, buf.size, size=max(1, buf.size // 16))
            buf.reshape(-1)[k] = rng.choice(np.array([np.nan, np.inf, -np.inf, -3.0], np.float32), size=k.size)
    return film, (hf if half else None), spp, low, full, spp_g


def tonemapped_rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))


CLI_MISUSE = [   # argument lists of the mi355pt CLI that must exit 2 with a message naming --half-res, before any scene is loaded
    ["--renderer", "mis", "--half-res", "--width", "63", "--height", "48"],
    ["--renderer", "mis", "--half-res", "--width", "64", "--height", "47"],
    ["--renderer", "normal", "--half-res"],
    ["--renderer", "albedo", "--half-res"],
    ["--renderer", "shading-normal", "--half-res"],
    ["--renderer", "position", "-o", "x.pfm", "--half-res"],
    ["--renderer", "depth", "-o", "x.pfm", "--half-res"],
    ["--renderer", "mis", "--half-res", "--denoise"],
    ["--renderer", "mis", "--spp", "16", "--half-res", "--adaptive-threshold", "0.05"],
    ["--renderer", "mis", "--half-res", "--gpus", "2"],
    ["--renderer", "mis", "--half-res-albedo"],
]
