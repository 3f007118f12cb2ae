"""TEST INFRASTRUCTURE ONLY.  The NumPy restatement of include/mi355pt_budget.h (the header's comment is the normative text) on top of
tests/temporal_reference.py, tests/motion_reference.py and tests/flow_reference.py, which it imports and does not edit: the carried point,
the projection and the tap tests are theirs (their accumulate(..., detail=True) on frames whose films are zero), the gathered length Lh
before the + 1, the per-tile minimum, the budget formula, the pair normalise and the length credit are restated here.  With np.float32
every operation is rounded on its own, in the order the header states, and the device result must be BIT-EQUAL to it."""
from types import SimpleNamespace

import numpy as np

import flow_reference as fr
import motion_reference as mr
import temporal_reference as tr

F = np.float32


def budget(base_spp, max_spp, target_history):
    return SimpleNamespace(base_spp=int(base_spp), max_spp=int(max_spp), target_history=F(target_history))


def tiles_of(W, H):
    return (H + 7) // 8, (W + 7) // 8


def gathered_length(cur, prev, view, prm=None, ids_cur=None, ids_prev=None, table=None, flow=None):
    """P of the header, (H, W) float32: Lh where the pixel has history, 0 elsewhere.  The films of the two frames are not read."""
    H, W = np.asarray(cur["hit"]).shape[:2]
    if prev is None:
        return np.zeros((H, W), F)
    assert table is None or flow is None
    prm = prm if prm is not None else tr.params()
    zero = np.zeros((H, W, 3), F)
    c = dict(position=cur["position"], shading_normal=cur["shading_normal"], hit=cur["hit"], film=zero, half=None)
    p = dict(position=prev["position"], shading_normal=prev["shading_normal"], hit=prev["hit"], length=prev["length"], film=zero, half=None)
    if table is not None:
        info = mr.accumulate_motion(c, 1, p, view, ids_cur, ids_prev, table, prm, detail=True)[3]
    elif flow is not None:
        info = fr.accumulate_flow(c, 1, p, view, ids_cur, ids_prev, flow, prm, detail=True)[3]
    else:
        info = tr.accumulate(c, 1, p, view, prm, detail=True)[3]
    one = F(1)
    wx, wy = info["wx"].astype(F), info["wy"].astype(F)
    omx, omy = one - wx, one - wy
    bw = [omx * omy, wx * omy, omx * wy, wx * wy]
    p_len = np.asarray(prev["length"], F)
    w, ln = [], []
    for k in range(4):
        ix, iy = np.clip(info["x0"] + (k & 1), 0, W - 1), np.clip(info["y0"] + (k >> 1), 0, H - 1)
        valid = info["valid"][k]
        w.append(np.where(valid, bw[k], F(0)).astype(F))
        ln.append(np.where(valid, p_len[iy, ix], F(0)).astype(F))
    Wt = ((w[0] + w[1]) + w[2]) + w[3]
    assert np.array_equal(Wt.view(np.uint32), np.asarray(info["Wt"], F).view(np.uint32))          # the same weights as the restatement's
    with np.errstate(all="ignore"):
        Lh = (((w[0] * ln[0] + w[1] * ln[1]) + w[2] * ln[2]) + w[3] * ln[3]) / Wt
    return np.where(info["has"], Lh, F(0)).astype(F)


def spp_of(lmin, b):
    """the formula: base_spp << j, j the smallest integer >= 0 with (lmin + 1) 2^j >= target or base_spp << j == max_spp"""
    lmin = np.asarray(lmin, F)
    out = np.zeros(lmin.shape, np.uint32)
    with np.errstate(all="ignore"):
        reach0 = lmin + F(1)
        for i, r in np.ndenumerate(reach0):
            n = b.base_spp
            while n < b.max_spp and not (r >= b.target_history):
                r = F(r * F(2))
                n <<= 1
            out[i] = n
    return out


def tile_min(P):
    """(tiles_y, tiles_x) float32: the minimum over each tile's in-frame pixels of P, a P that is not > 0 counting as 0"""
    H, W = P.shape
    ty, tx = tiles_of(W, H)
    v = np.full((ty * 8, tx * 8), np.inf, F)
    v[:H, :W] = np.where(P > 0, P, F(0))
    return v.reshape(ty, 8, tx, 8).min(axis=(1, 3))


def probe(cur, prev, view, b, prm=None, ids_cur=None, ids_prev=None, table=None, flow=None):
    """mi355pt_temporal_budget -> (P (H, W) f32, tile_len (tiles_y, tiles_x) f32, tile_spp (tiles_y, tiles_x) u32)"""
    P = gathered_length(cur, prev, view, prm, ids_cur, ids_prev, table, flow)
    lmin = tile_min(P)
    return P, lmin, spp_of(lmin, b)


def expected_out_length(P, max_history):
    """what every accumulation call writes to out_length on the probe's inputs"""
    return np.where(P > 0, np.minimum(P + F(1), F(max_history)), F(1)).astype(F)


def per_pixel(tile_values, W, H):
    return np.repeat(np.repeat(np.asarray(tile_values), 8, axis=0), 8, axis=1)[:H, :W]


def pair_normalize(film, half, tile_spp):
    """both films / (float)(n_t / 2)"""
    H, W = film.shape[:2]
    n = per_pixel(np.asarray(tile_spp, np.uint32) // np.uint32(2), W, H).astype(F)[..., None]
    with np.errstate(all="ignore"):
        return (np.asarray(film, F) / n).astype(F), (np.asarray(half, F) / n).astype(F)


def length_credit(length, tile_spp, base_spp, max_history):
    """length := min(length + (float)(n_t / base_spp - 1), max_history) on the tiles with n_t > base_spp; the others keep their bits"""
    H, W = length.shape
    n = per_pixel(np.asarray(tile_spp, np.uint32), W, H).astype(np.int64)
    credit = (n // base_spp - 1).astype(F)
    with np.errstate(all="ignore"):
        boosted = np.minimum(np.asarray(length, F) + credit, F(max_history)).astype(F)
    return np.where(n > base_spp, boosted, np.asarray(length, F)).astype(F)


def rendered_count(tile_spp, b):
    """the count a tile ends the driver with: the clamped value, raised to the next base_spp << j"""
    c = np.clip(np.asarray(tile_spp, np.int64), b.base_spp, b.max_spp)
    out = np.full(c.shape, b.base_spp, np.int64)
    while (out < c).any():
        out = np.where(out < c, out * 2, out)
    return out.astype(np.uint32)


def driver_levels(tile_spp, b):
    """the passes of the driver's step 5 -> [(level, ascending list of the tiles with clamped tile_spp > level)], the empty list that ends the
    loop included"""
    c = np.clip(np.asarray(tile_spp, np.int64).reshape(-1), b.base_spp, b.max_spp)
    out, level = [], b.base_spp
    while level < b.max_spp:
        tiles = np.flatnonzero(c > level).astype(np.uint32)
        out.append((level, tiles))
        if tiles.size == 0:
            break
        level *= 2
    return out
