"""TEST INFRASTRUCTURE ONLY.  The NumPy restatement of include/mi355pt_motion.h (the header's comment is the normative text) on top of
tests/temporal_reference.py and tests/temporal_rectify_reference.py: the motion table in float64, and the motion-aware accumulation —
the gather of temporal_reference.accumulate with the header's changes (the pixel's record instead of delta, the carried normal, the id test
of the taps), everything else taken from that module as it is.  The rectified form is temporal_rectify_reference.accumulate over this
gather.  With dtype=np.float32 every operation is rounded on its own, in the order the header states, and the device result must be
BIT-EQUAL to it."""
import contextlib
from types import SimpleNamespace

import numpy as np

import temporal_rectify_reference as rr
import temporal_reference as tr

ENTRY_WORDS = 24          # a 0:9, b 9:12, n 12:21, pad 21:24 — mi355pt_motion_xform as one row of float32


# ---------------- the table ----------------
def mat4(l2w):
    """a local_to_world as SceneHandle.add_instance takes it (row-major 4 x 4 float32: it multiplies column vectors) in float64"""
    return np.asarray(l2w, np.float32).astype(np.float64).reshape(4, 4)


def static_entry(cur_cam, prev_cam):
    e = np.zeros(ENTRY_WORDS, np.float64)
    e[[0, 4, 8, 12, 16, 20]] = 1.0
    e[9:12] = np.asarray(cur_cam.position, np.float64) - np.asarray(prev_cam.position, np.float64)
    return e


def table64(cur_cam, prev_cam, l2w_cur, l2w_prev):
    """mi355pt_motion_table in float64, NOT rounded: (n + 1, 24).  T = l2w_prev l2w_cur^-1;  a = lin(T),  b = a c_cur + trans(T) - c_prev,
    n = (a^-1)^T; a bytewise unmoved instance gets the static entry"""
    cc, cp = np.asarray(cur_cam.position, np.float64), np.asarray(prev_cam.position, np.float64)
    out = [static_entry(cur_cam, prev_cam)]
    for mc, mp in zip(l2w_cur, l2w_prev):
        mc32, mp32 = np.asarray(mc, np.float32).reshape(4, 4), np.asarray(mp, np.float32).reshape(4, 4)
        if mc32.tobytes() == mp32.tobytes():
            out.append(static_entry(cur_cam, prev_cam))
            continue
        T = mat4(mp32) @ np.linalg.inv(mat4(mc32))
        a = T[:3, :3]
        e = np.zeros(ENTRY_WORDS, np.float64)
        e[0:9] = a.reshape(-1)
        e[9:12] = a @ cc + T[:3, 3] - cp
        e[12:21] = np.linalg.inv(a).T.reshape(-1)
        out.append(e)
    return np.stack(out)


def apply_entry(entry, X, dtype=np.float64):
    """X_prev = a X + b in `dtype`, in the header's operation order"""
    dt = dtype
    e, X = np.asarray(entry, dt), np.asarray(X, dt)
    return np.stack([((e[3 * i] * X[..., 0] + e[3 * i + 1] * X[..., 1]) + e[3 * i + 2] * X[..., 2]) + e[9 + i] for i in range(3)], -1)


# ---------------- the accumulation ----------------
def accumulate_motion(cur, spp, prev, view, ids_cur, ids_prev, table, prm=None, dtype=np.float32, detail=False):
    """mi355pt_temporal_accumulate_motion: the arguments of temporal_reference.accumulate plus ids_cur (H, W), ids_prev ((H, W) or None) and
    table (n_entries, 24).  The text of temporal_reference.accumulate with the changes marked MOTION"""
    if prev is None:
        return tr.accumulate(cur, spp, None, None, prm, dtype=dtype, detail=detail)
    dt = dtype
    prm = prm if prm is not None else tr.params()
    A = lambda x: np.asarray(x, dt)   # noqa: E731
    B = A(cur["film"])
    H, W = B.shape[:2]
    has_half = cur.get("half") is not None
    idc = np.asarray(ids_cur, np.uint32)
    tab = np.asarray(table, np.float32).reshape(-1, ENTRY_WORDS)
    M = A(tab[np.minimum(idc, np.uint32(tab.shape[0] - 1))])                  # MOTION: e = min(ids_cur[p], n_entries - 1), (H, W, 24)
    with np.errstate(all="ignore"):
        if has_half:
            Hf, hs = A(cur["half"]), dt(spp // 2)
            c = [tr.clean(Hf / hs), tr.clean((B - Hf) / hs)]
        else:
            c = [tr.clean(B / dt(spp))]
        hit = A(cur["hit"])
        h = hit[..., 1]
        dot = lambda a, b: (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]   # noqa: E731
        X = A(cur["position"]) / h[..., None]
        Xp = np.stack([dot(M[..., 3 * i:3 * i + 3], X) + M[..., 9 + i] for i in range(3)], -1)          # MOTION: a X + b, delta not added
        nrm0 = dt(2) * (A(cur["shading_normal"]) / h[..., None]) - dt(1)
        nrm = np.stack([dot(M[..., 12 + 3 * i:15 + 3 * i], nrm0) for i in range(3)], -1)              # MOTION: n nrm
        t = hit[..., 0] / h
        r = A(view.rows)
        vx, vy, zc = dot(r[0:3], Xp), dot(r[3:6], Xp), -dot(r[6:9], Xp)
        gx = (dt(view.cx) + (vx / zc) * dt(view.sx)) - dt(0.5)
        gy = (dt(view.cy) - (vy / zc) * dt(view.sy)) - dt(0.5)
        ok = (h != 0) & (zc > 0) & (gx >= -1) & (gx < dt(W)) & (gy >= -1) & (gy < dt(H))
        gx, gy = np.where(ok, gx, dt(0)), np.where(ok, gy, dt(0))
        x0f, y0f = np.floor(gx), np.floor(gy)
        wx, wy = gx - x0f, gy - y0f
        x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
        omx, omy = dt(1) - wx, dt(1) - wy
        bw = [omx * omy, wx * omy, omx * wy, wx * wy]
        tol = dt(prm.pos_tol) * t
        p_hit, p_len = A(prev["hit"]), A(prev["length"])
        p_pos, p_nrm, p_film = A(prev["position"]), A(prev["shading_normal"]), A(prev["film"])
        p_half = A(prev["half"]) if has_half else None
        p_ids = np.asarray(ids_prev, np.uint32) if ids_prev is not None else None
        w, ln, fv, gv, valids = [], [], [], [], []
        for k in range(4):
            qx, qy = x0 + (k & 1), y0 + (k >> 1)
            inside = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
            ix, iy = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
            hq, lq = p_hit[iy, ix, 1], p_len[iy, ix]
            e = Xp - p_pos[iy, ix] / hq[..., None]
            pd = np.abs(dot(e, nrm))
            nq = dt(2) * (p_nrm[iy, ix] / hq[..., None]) - dt(1)
            nd = dot(nrm, nq)
            valid = ok & inside & (hq > 0) & (lq > 0) & (pd <= tol) & (nd >= dt(prm.normal_cos))
            if p_ids is not None:
                valid = valid & (p_ids[iy, ix] == idc)                                                # MOTION: the tap shows the pixel's id
            valids.append(valid)
            w.append(np.where(valid, bw[k], dt(0)))
            ln.append(np.where(valid, lq, dt(0)))
            fv.append(np.where(valid[..., None], p_film[iy, ix], dt(0)))
            if has_half:
                gv.append(np.where(valid[..., None], p_half[iy, ix], dt(0)))
        Wt = ((w[0] + w[1]) + w[2]) + w[3]
        has = Wt > dt(prm.min_weight)
        wsum = lambda v, wk=None: (((wk[0] * v[0] + wk[1] * v[1]) + wk[2] * v[2]) + wk[3] * v[3])   # noqa: E731
        Lh = wsum(ln, w) / Wt
        Lc = np.minimum(Lh + dt(1), dt(prm.max_history))
        alpha = (dt(1) / Lc)[..., None]
        L = np.where(has, Lc, dt(1)).astype(dt)
        w3 = [x[..., None] for x in w]
        if has_half:
            hist = [wsum(gv, w3) / Wt[..., None], wsum([f - g for f, g in zip(fv, gv)], w3) / Wt[..., None]]
        else:
            hist = [wsum(fv, w3) / Wt[..., None]]
        m = [np.where(has[..., None], hi + (ci - hi) * alpha, ci).astype(dt) for hi, ci in zip(hist, c)]
    info = dict(m=m, ok=ok, has=has, valid=valids, x0=x0, y0=y0, wx=wx, wy=wy, Wt=Wt, hist=hist, gx=gx, gy=gy, c=c)
    out = (m[0] + m[1], m[0], L) if has_half else (m[0], None, L)
    return out + (info,) if detail else out


@contextlib.contextmanager
def _gather_of(fn):
    """temporal_rectify_reference.accumulate over another gather: it asks its module-level `tr` for accumulate(..., detail=True)"""
    saved = rr.tr
    rr.tr = SimpleNamespace(accumulate=fn)
    try:
        yield
    finally:
        rr.tr = saved


def accumulate_rectified_motion(cur, spp, prev, view, ids_cur, ids_prev, table, prm=None, rprm=None, dtype=np.float32, detail=False):
    """mi355pt_temporal_accumulate_rectified_motion: temporal_rectify_reference.accumulate, whose gather is accumulate_motion"""
    def gather(cur_, spp_, prev_, view_, prm_, dtype=np.float32, detail=False):
        return accumulate_motion(cur_, spp_, prev_, view_, ids_cur, ids_prev, table, prm_, dtype=dtype, detail=detail)
    with _gather_of(gather):
        return rr.accumulate(cur, spp, prev, view, prm, rprm, dtype=dtype, detail=detail)


# ---------------- synthetic ids and tables ----------------
def static_table(view, n_entries):
    """n_entries static records for `view`: a = n = I, b = view.delta"""
    t = np.zeros((n_entries, ENTRY_WORDS), np.float32)
    t[:, [0, 4, 8, 12, 16, 20]] = 1.0
    t[:, 9:12] = np.asarray(view.delta, np.float32)
    return t


def moved_entry(view, shift=(0.15, -0.05, 0.1), yaw=0.03):
    """one record of a rigid motion beside `view`'s delta: a yaw about +y and a shift (n = a for a rotation)"""
    c, s = np.cos(yaw), np.sin(yaw)
    a = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    e = np.zeros(ENTRY_WORDS, np.float32)
    e[0:9] = a.reshape(-1).astype(np.float32)
    e[9:12] = (np.asarray(view.delta, np.float64) + np.asarray(shift)).astype(np.float32)
    e[12:21] = a.reshape(-1).astype(np.float32)
    return e


def synthetic_ids(W, H, seed=11, n_ids=5):
    """(ids_cur, ids_prev): vertical bands of the ids 0 .. n_ids - 1 (some above any small table: the clamp), the previous frame's bands
    shifted by two pixels and with seeded single-pixel disagreements"""
    rng = np.random.default_rng([seed, W, H])
    band = max(1, W // n_ids)
    x = np.arange(W)[None, :] + np.zeros((H, 1), np.int64)
    cur = np.minimum(x // band, n_ids - 1).astype(np.uint32)
    prev = np.minimum((x + 2) // band, n_ids - 1).astype(np.uint32)
    flip = rng.random((H, W)) < 0.05
    prev[flip] = (prev[flip] + 1) % n_ids
    return cur, prev
