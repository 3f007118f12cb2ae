"""TEST INFRASTRUCTURE ONLY.  The NumPy restatement of include/mi355pt_flow.h (the header's comment is the normative text): the per-pixel
motion record from (tri, b, current triangles, marked triangles), and the flow-aware accumulation — the gather of
temporal_reference.accumulate with the header's changes (the pixel's record added to X and to nrm, the id test of the taps), everything
else taken from that module as it is.  The rectified form is temporal_rectify_reference.accumulate over this gather.  With
dtype=np.float32 every operation is rounded on its own, in the order the header states, and the device result must be BIT-EQUAL to it."""
import numpy as np

import motion_reference as mr
import temporal_rectify_reference as rr
import temporal_reference as tr

# mi355pt_flow_pixel and the debug pass's hit record (ffi.FLOW_PIXEL / ffi.FLOW_HIT, restated: this module needs no library)
FLOW_PIXEL = np.dtype([("d", np.float32, 3), ("id", np.uint32), ("dn", np.float32, 3), ("pad", np.uint32)])
FLOW_HIT = np.dtype([("tri", np.uint32), ("b", np.float32, 3)])
assert FLOW_PIXEL.itemsize == 32 and FLOW_HIT.itemsize == 16
FLT_MAX = np.float32(3.402823466e+38)


# ---------------- the record ----------------
def interpolate(b, P, dtype=np.float32):
    """(b0 P0 + b1 P1) + b2 P2 per component, in `dtype`: b (..., 3), P (..., 3 vertices, 3 components)"""
    b, P = np.asarray(b, dtype), np.asarray(P, dtype)
    return (b[..., 0, None] * P[..., 0, :] + b[..., 1, None] * P[..., 1, :]) + b[..., 2, None] * P[..., 2, :]


def facet_normal(P, dtype=np.float32):
    """cross(P1 - P0, P2 - P0) / sqrt(dot) in `dtype`, every operation rounded on its own -> (ng (..., 3), ok (...))"""
    P = np.asarray(P, dtype)
    with np.errstate(all="ignore"):
        e1, e2 = P[..., 1, :] - P[..., 0, :], P[..., 2, :] - P[..., 0, :]
        cx = e1[..., 1] * e2[..., 2] - e1[..., 2] * e2[..., 1]
        cy = e1[..., 2] * e2[..., 0] - e1[..., 0] * e2[..., 2]
        cz = e1[..., 0] * e2[..., 1] - e1[..., 1] * e2[..., 0]
        l2 = (cx * cx + cy * cy) + cz * cz
        ok = (l2 > 0) & (l2 <= FLT_MAX)
        ln = np.sqrt(l2)
        return np.stack([cx / ln, cy / ln, cz / ln], -1), ok


def words(tris):
    """48-byte triangle records as (n, 12) float32 words, whichever 32-bit type the exporter gave them (Product.export_bvh: uint32)"""
    t = np.ascontiguousarray(tris)
    assert t.dtype.itemsize == 4
    return t.view(np.float32).reshape(-1, 12)


def positions(tris):
    """the three vertices of 48-byte triangle records (p0 p1 p2 in words 0 - 8) -> (n, 3, 3) float32"""
    return words(tris)[:, :9].reshape(-1, 3, 3)


def instances(tris):
    """DevTri::instance (word 9) of 48-byte triangle records"""
    return np.ascontiguousarray(words(tris)[:, 9]).view(np.uint32)


def records(hit_mask, tri, b, tris_cur, tris_prev):
    """the flow pass's records for pixels with the hit (tri, b = (b0, b1, b2)); hit_mask False: a miss, all eight words 0.
    tris_cur / tris_prev: the (n, 12) 32-bit words of the current and the marked triangle arrays.  -> array of FLOW_PIXEL, hit_mask's shape"""
    hit_mask = np.asarray(hit_mask, bool)
    tri = np.where(hit_mask, np.asarray(tri, np.int64), 0)
    b = np.asarray(b, np.float32)
    Pc, Pv = positions(tris_cur)[tri], positions(tris_prev)[tri]
    with np.errstate(all="ignore"):
        d = interpolate(b, Pv) - interpolate(b, Pc)
        (nc, okc), (nv, okv) = facet_normal(Pc), facet_normal(Pv)
        dn = np.where((okc & okv)[..., None], nv - nc, np.float32(0))
    out = np.zeros(hit_mask.shape, FLOW_PIXEL)
    out["d"] = np.where(hit_mask[..., None], d, np.float32(0))
    out["dn"] = np.where(hit_mask[..., None], dn, np.float32(0))
    out["id"] = np.where(hit_mask, instances(tris_cur)[tri] + np.uint32(1), np.uint32(0))
    return out


def records_from_hits(hits, ids, tris_cur, tris_prev):
    """records() fed mi355pt_render_flow_debug's hit film (FLOW_HIT) and the id film, which says where a ray hit at all"""
    return records(np.asarray(ids) != 0, hits["tri"], hits["b"], tris_cur, tris_prev)


def zero_records(W, H):
    return np.zeros((H, W), FLOW_PIXEL)


# ---------------- the accumulation ----------------
def accumulate_flow(cur, spp, prev, view, ids_cur, ids_prev, flow, prm=None, dtype=np.float32, detail=False):
    """mi355pt_temporal_accumulate_flow: the arguments of temporal_reference.accumulate plus ids_cur ((H, W) or None without ids_prev),
    ids_prev ((H, W) or None) and flow ((H, W) FLOW_PIXEL).  The text of temporal_reference.accumulate with the changes marked FLOW"""
    if prev is None:
        return tr.accumulate(cur, spp, None, None, prm, dtype=dtype, detail=detail)
    dt = dtype
    prm = prm if prm is not None else tr.params()
    A = lambda x: np.asarray(x, dt)   # noqa: E731
    B = A(cur["film"])
    H, W = B.shape[:2]
    has_half = cur.get("half") is not None
    fl = np.asarray(flow, FLOW_PIXEL).reshape(H, W)
    idc = np.asarray(ids_cur, np.uint32) if ids_cur is not None else None
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
        Xp = X + A(fl["d"])                                                                           # FLOW: X + d, delta not added
        nrm = (dt(2) * (A(cur["shading_normal"]) / h[..., None]) - dt(1)) + A(fl["dn"])               # FLOW: nrm + dn
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
                valid = valid & (p_ids[iy, ix] == idc)                                                # FLOW: the tap shows the pixel's id
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


def accumulate_rectified_flow(cur, spp, prev, view, ids_cur, ids_prev, flow, prm=None, rprm=None, dtype=np.float32, detail=False):
    """mi355pt_temporal_accumulate_rectified_flow: temporal_rectify_reference.accumulate, whose gather is accumulate_flow"""
    def gather(cur_, spp_, prev_, view_, prm_, dtype=np.float32, detail=False):
        return accumulate_flow(cur_, spp_, prev_, view_, ids_cur, ids_prev, flow, prm_, dtype=dtype, detail=detail)
    with mr._gather_of(gather):
        return rr.accumulate(cur, spp, prev, view, prm, rprm, dtype=dtype, detail=detail)


# ---------------- synthetic records ----------------
def zero_delta(view):
    """`view` with delta = 0: what the existing calls must be given to equal the flow calls at all-zero records"""
    from types import SimpleNamespace
    return SimpleNamespace(delta=np.zeros(3, np.float32), rows=np.asarray(view.rows, np.float32), sx=view.sx, sy=view.sy, cx=view.cx, cy=view.cy)


def synthetic_flow(W, H, view, seed=13, big=False):
    """(H, W) records for the synthetic films of temporal_reference.synthetic: the view's own delta (so that the static world reprojects as
    under the existing call) plus, in vertical bands, nothing / a small shift with a small dn / (big) displacements that throw the taps out of
    the frame and behind the previous camera"""
    rng = np.random.default_rng([seed, W, H])
    fl = np.zeros((H, W), FLOW_PIXEL)
    x = np.arange(W)[None, :] + np.zeros((H, 1), np.int64)
    band = (3 * x) // max(W, 1)
    d = np.zeros((H, W, 3), np.float32) + np.asarray(view.delta, np.float32)
    d[band == 1] += np.array([0.15, -0.05, 0.1], np.float32)
    dn = np.zeros((H, W, 3), np.float32)
    dn[band == 1] = (rng.normal(size=(int((band == 1).sum()), 3)) * 0.02).astype(np.float32)
    if big:
        d[band == 2] += np.where(rng.random((int((band == 2).sum()), 1)) < 0.5, np.array([40.0, 0.0, 0.0], np.float32), np.array([0.0, 0.0, 60.0], np.float32))
    fl["d"], fl["dn"] = d, dn
    fl["id"] = (band + 1).astype(np.uint32)
    return fl
