"""TEST INFRASTRUCTURE ONLY.  The NumPy restatement of include/mi355pt_temporal_rectify.h (the header's comment is the normative text), built
on tests/temporal_reference.py: accumulate(..., detail=True) gives c, "has history", hist and L, which are taken as they are.  With
dtype=np.float32 every operation is rounded on its own, in the order the header states, and the device result must be BIT-EQUAL to it;
np.float64 is there for the property tests."""
from types import SimpleNamespace

import numpy as np

import temporal_reference as tr

DEFAULTS = dict(radius=2, gamma=2.0)


def params(**kw):
    """the defaults of mi355pt_temporal_rectify_params_default, with overrides"""
    d = dict(DEFAULTS); d.update(kw)
    return SimpleNamespace(radius=int(d["radius"]), gamma=np.float32(d["gamma"]))


def window_sum(x, r):
    """(H, W, ...) -> the sum over |dx|, |dy| <= r of the in-frame values (values outside the frame count as 0): row sums dx = -r .. r left to
    right starting from 0, then the row sums dy = -r .. r top to bottom starting from 0"""
    H, W = x.shape[:2]
    pad = np.zeros((H + 2 * r, W + 2 * r) + x.shape[2:], x.dtype)
    pad[r:r + H, r:r + W] = x
    rows = np.zeros((H + 2 * r, W) + x.shape[2:], x.dtype)
    for dx in range(2 * r + 1):
        rows = rows + pad[:, dx:dx + W]
    out = np.zeros_like(x)
    for dy in range(2 * r + 1):
        out = out + rows[dy:dy + H]
    return out


def accumulate(cur, spp, prev=None, view=None, prm=None, rprm=None, dtype=np.float32, detail=False):
    """mi355pt_temporal_accumulate_rectified: the arguments of temporal_reference.accumulate and the rectification's parameters
    -> (out_film, out_half or None, out_length) in `dtype` (and a dict of intermediates with detail=True)"""
    dt = dtype
    rprm = rprm if rprm is not None else params()
    of, oh, L, info = tr.accumulate(cur, spp, prev, view, prm, dtype=dt, detail=True)
    if prev is None:
        return (of, oh, L, info) if detail else (of, oh, L)
    has_half = cur.get("half") is not None
    c, hist, has = info["c"], info["hist"], info["has"]
    r, gamma = int(rprm.radius), dt(rprm.gamma)
    with np.errstate(all="ignore"):
        v = (c[0] + c[1]) * dt(0.5) if has_half else c[0]
        g = (hist[0] + hist[1]) * dt(0.5) if has_half else hist[0]
        member = has[..., None]
        v, g = np.where(member, v, dt(0)).astype(dt), np.where(member, g, dt(0)).astype(dt)
        S1, S2, Sg = window_sum(v, r), window_sum(v * v, r), window_sum(g, r)
        n = window_sum(has.astype(dt), r)[..., None]
        mu = S1 / n
        s2 = S2 / n - mu * mu
        s2 = np.where(s2 > 0, s2, dt(0)).astype(dt)
        se = np.sqrt(s2 / n)
        muh = Sg / n
        lo, hi = mu - gamma * se, mu + gamma * se
        tgt = np.minimum(np.maximum(muh, lo), hi)
        k = np.where(muh > 0, tgt / muh, dt(1)).astype(dt)
        a = (dt(1) / L)[..., None]
        rect = [h * k for h in hist]
        m = [np.where(member, hr + (ci - hr) * a, ci).astype(dt) for hr, ci in zip(rect, c)]
    info = dict(info, m=m, k=k, n=n[..., 0], mu=mu, muh=muh, se=se, rect=rect, v=v, g=g)
    out = (m[0] + m[1], m[0], L) if has_half else (m[0], None, L)
    return out + (info,) if detail else out


CLI_MISUSE = [   # argument lists of the mi355pt CLI that must exit 2 with a message, before any scene is loaded
    ["--renderer", "mis", "--temporal-rectify"],
    ["--renderer", "mis", "--temporal-rectify-radius", "2"],
    ["--renderer", "mis", "--temporal-rectify-gamma", "2"],
    ["--renderer", "mis", "--temporal-frames", "3", "--temporal-rectify-radius", "2"],
    ["--renderer", "mis", "--temporal-frames", "3", "--temporal-rectify-gamma", "2"],
    ["--renderer", "mis", "--temporal-frames", "3", "--temporal-rectify", "--temporal-rectify-radius", "0"],
    ["--renderer", "mis", "--temporal-frames", "3", "--temporal-rectify", "--temporal-rectify-radius", "4"],
    ["--renderer", "mis", "--temporal-frames", "3", "--temporal-rectify", "--temporal-rectify-gamma", "0"],
    ["--renderer", "mis", "--temporal-frames", "3", "--temporal-rectify", "--temporal-rectify-gamma", "-1.5"],
    ["--renderer", "mis", "--temporal-frames", "3", "--temporal-rectify", "--temporal-rectify-gamma", "nan"],
    ["--renderer", "mis", "--temporal-frames", "3", "--temporal-rectify", "--temporal-rectify-gamma", "inf"],
]
