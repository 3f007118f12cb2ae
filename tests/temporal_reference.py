"""TEST INFRASTRUCTURE ONLY.  The NumPy restatement of include/mi355pt_temporal.h (the header's comment is the normative text): with
dtype=np.float32 every operation is rounded on its own, in the order the header states, and the device result must be BIT-EQUAL to it;
np.float64 is there for the property tests.  Also the view of a camera pair in double, and seeded synthetic frames whose G-buffer sums are
written analytically (a fronto-parallel plane, a two-plane step, a background band)."""
import math
from types import SimpleNamespace

import numpy as np

FLT_MAX = np.finfo(np.float32).max
FILMS = ("film", "half", "length", "position", "shading_normal", "hit")
DEFAULTS = dict(pos_tol=0.01, normal_cos=0.9, min_weight=0.01, max_history=32.0)


def params(**kw):
    """the defaults of mi355pt_temporal_params_default as f32 values, with overrides"""
    d = dict(DEFAULTS); d.update(kw)
    return SimpleNamespace(**{k: np.float32(v) for k, v in d.items()})


def camera(position=(0.0, 0.0, 0.0), direction=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), width=64, height=48, fov_deg=45.0):
    """a camera as plain data; the fields hold what the f32 fields of mi355pt_camera hold"""
    f32 = lambda v: [float(np.float32(x)) for x in v]   # noqa: E731
    return SimpleNamespace(position=f32(position), direction=f32(direction), up=f32(up), width=width, height=height, fov_deg=float(np.float32(fov_deg)))


def yawed(direction, angle):
    """`direction` turned by `angle` radians about +y"""
    c, s = math.cos(angle), math.sin(angle)
    x, y, z = direction
    return (c * x + s * z, y, -s * x + c * z)


def camera_frame(cam):
    """(s, u, f) of look_to_rh(direction, up) in double: direction and up normalised as set_look_to does"""
    f = np.asarray(cam.direction, np.float64); f = f / np.linalg.norm(f)
    up = np.asarray(cam.up, np.float64); up = up / np.linalg.norm(up)
    s = np.cross(f, up); s = s / np.linalg.norm(s)
    return s, np.cross(s, f), f


def view_from_cameras(cur, prev):
    """mi355pt_temporal_view_from_cameras in double, each entry rounded once to f32"""
    s, u, f = camera_frame(prev)
    w, h = float(cur.width), float(cur.height)
    scale = math.tan(math.radians(prev.fov_deg) / 2.0)
    v = SimpleNamespace()
    v.delta = (np.asarray(cur.position, np.float64) - np.asarray(prev.position, np.float64)).astype(np.float32)
    v.rows = np.concatenate([s, u, -f]).astype(np.float32)
    v.sx, v.sy = np.float32((w / 2.0) / ((w / h) * scale)), np.float32((h / 2.0) / scale)
    v.cx, v.cy = np.float32(w / 2.0), np.float32(h / 2.0)
    return v


def view_entries(v):
    """the 16 entries of a view (this module's or ffi.TemporalView) as a float32 array"""
    return np.array(list(v.delta) + list(v.rows) + [v.sx, v.sy, v.cx, v.cy], np.float32)


def pixel_rays(cam):
    """(H, W, 3) unit render-space directions through the pixel CENTRES, camera.rs:51-65 in double"""
    W, H = cam.width, cam.height
    scale = math.tan(math.radians(cam.fov_deg) / 2.0)
    x = np.arange(W, dtype=np.float64)[None, :] + 0.5
    y = np.arange(H, dtype=np.float64)[:, None] + 0.5
    dx = (2.0 * x / W - 1.0) * (W / H) * scale + 0.0 * y
    dy = (1.0 - 2.0 * y / H) * scale + 0.0 * x
    d = np.stack([dx, dy, -np.ones_like(dx)], -1)
    d = d / np.linalg.norm(d, axis=-1, keepdims=True)
    s, u, f = camera_frame(cam)
    return d[..., 0:1] * s + d[..., 1:2] * u - d[..., 2:3] * f


def project(view, X, dtype=np.float64):
    """render-space points of the current frame -> continuous pixel coordinates (fx, fy) in the previous image and zc, in `dtype`"""
    dt = dtype
    Xp = np.asarray(X, dt) + np.asarray(view.delta, dt)
    r = np.asarray(view.rows, dt)
    v = [(r[3 * i] * Xp[..., 0] + r[3 * i + 1] * Xp[..., 1]) + r[3 * i + 2] * Xp[..., 2] for i in range(3)]
    zc = -v[2]
    with np.errstate(all="ignore"):
        return dt(view.cx) + (v[0] / zc) * dt(view.sx), dt(view.cy) - (v[1] / zc) * dt(view.sy), zc


def clean(x):
    return np.where((x > 0) & (x <= FLT_MAX), x, 0).astype(x.dtype)


def accumulate(cur, spp, prev=None, view=None, prm=None, dtype=np.float32, detail=False):
    """mi355pt_temporal_accumulate: cur / prev map film names to arrays ((H, W, 3); length (H, W)), half may be missing or None.
    -> (out_film, out_half or None, out_length) in `dtype` (and a dict of intermediates with detail=True)"""
    dt = dtype
    prm = prm if prm is not None else params()
    A = lambda x: np.asarray(x, dt)   # noqa: E731
    B = A(cur["film"])
    H, W = B.shape[:2]
    has_half = cur.get("half") is not None
    info = {}
    with np.errstate(all="ignore"):
        if has_half:
            Hf, hs = A(cur["half"]), dt(spp // 2)
            c = [clean(Hf / hs), clean((B - Hf) / hs)]
        else:
            c = [clean(B / dt(spp))]
        m, L = c, np.ones((H, W), dt)
        if prev is not None:
            hit = A(cur["hit"])
            h = hit[..., 1]
            Xp = A(cur["position"]) / h[..., None] + A(view.delta)
            nrm = dt(2) * (A(cur["shading_normal"]) / h[..., None]) - dt(1)
            t = hit[..., 0] / h
            dot = lambda a, b: (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]   # noqa: E731
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
            info = dict(m=m, ok=ok, has=has, valid=valids, x0=x0, y0=y0, wx=wx, wy=wy, Wt=Wt, hist=hist, gx=gx, gy=gy)
    info["c"] = c
    info.setdefault("m", m)
    out = (m[0] + m[1], m[0], L) if has_half else (m[0], None, L)
    return out + (info,) if detail else out


# ---------------- seeded synthetic frames ----------------
PLANE_D, STEP_NEAR, STEP_FAR, STEP_EDGE_X, TOP_Y = 4.0, 4.0, 5.0, -0.2, 1.2


def raycast(cam, scene):
    """Analytic closest hits through the pixel centres, in double.  scene "plane": the plane z = -4 (world) below y = TOP_Y, nothing above
    (the background band); "step": a near plane z = -4 for world x < STEP_EDGE_X in front of a far plane z = -5, the same band.  Both face
    +z.  -> (X render space (H, W, 3), t (H, W), hit mask (H, W))"""
    d = pixel_rays(cam)
    o = np.asarray(cam.position, np.float64)
    with np.errstate(all="ignore"):
        def plane(depth):
            t = (-depth - o[2]) / d[..., 2]
            return t, o + d * t[..., None]
        if scene == "plane":
            t, P = plane(PLANE_D)
            hit = (t > 0) & (P[..., 1] < TOP_Y)
        else:
            tn, Pn = plane(STEP_NEAR)
            tf, Pf = plane(STEP_FAR)
            near = (tn > 0) & (Pn[..., 0] < STEP_EDGE_X)
            t, P = np.where(near, tn, tf), np.where(near[..., None], Pn, Pf)
            hit = (t > 0) & (P[..., 1] < TOP_Y)
    t = np.where(hit, t, 0.0)
    X = np.where(hit[..., None], d * t[..., None], 0.0)
    return X, t, hit


def gbuffer_sums(cam, scene, rng, spp_g=16):
    """the raw G-buffer sums of mi355pt_gbuffer.h for `spp_g` samples of which a seeded 1 .. spp_g hit (all through the pixel centre), f32"""
    X, t, hit = raycast(cam, scene)
    n = np.where(hit, rng.integers(1, spp_g + 1, size=hit.shape), 0).astype(np.float64)
    position = (X * n[..., None]).astype(np.float32)
    normal = (np.array([0.5, 0.5, 1.0]) * n[..., None]).astype(np.float32)             # (0, 0, 1) * 0.5 + 0.5 per hit
    hitf = np.stack([t * n, n, np.zeros_like(n)], -1).astype(np.float32)
    return dict(position=position, shading_normal=normal, hit=hitf), hit


def hdr(rng, shape):
    """positive HDR noise, up to about 100"""
    return (rng.random(shape) ** 4 * 100.0 + 0.01).astype(np.float32)


VIEWS = ("static", "shift3", "move", "outside", "behind")


def camera_pair(name, W, H):
    """(current camera, previous camera) of a synthetic view: "static" lands on exact pixel centres, "shift3" moves the plane z = -4 by
    exactly 3 pixels, "move" is a translation plus a yaw (of the PREVIOUS camera: the rows of the view are no identity), "outside" pushes part of the frame out of the history, "behind" has a previous
    camera that stands close to the planes and looks along them: the left part of the frame lies behind it"""
    base = camera(width=W, height=H)
    px = PLANE_D * 2.0 * math.tan(math.radians(45.0) / 2.0) / H
    if name == "static":
        return base, base
    if name == "shift3":
        return camera(position=(3.0 * px, 0.0, 0.0), width=W, height=H), base
    if name == "move":
        return base, camera(position=(-0.3, -0.1, 0.2), direction=yawed((0.0, 0.0, -1.0), -0.05), width=W, height=H)
    if name == "outside":
        return camera(position=(1.5, -0.8, 0.0), width=W, height=H), base
    if name == "behind":
        return base, camera(position=(-1.0, 0.0, -3.0), direction=(1.0, 0.0, -1.0), width=W, height=H)
    raise ValueError(name)


def synthetic(W, H, view="static", scene="step", half=True, spp=4, seed=7, bad=True):
    """-> (cur, prev, view, spp): the current frame (beauty and half-film SUMS with NaN / inf / negative values when `bad`), the previous
    frame (a finite accumulated pair, lengths 0 .. 40 with zeros among them) and the view between their cameras"""
    rng = np.random.default_rng([seed, W, H, VIEWS.index(view)])
    cam_c, cam_p = camera_pair(view, W, H)
    cur, _ = gbuffer_sums(cam_c, scene, rng)
    prev, _ = gbuffer_sums(cam_p, scene, rng)
    hf = hdr(rng, (H, W, 3)) * (spp // 2)
    film = hf + hdr(rng, (H, W, 3)) * (spp - spp // 2)
    if bad:
        for buf in (film, hf):
            k = rng.integers(0, buf.size, size=max(1, buf.size // 16))
            buf.reshape(-1)[k] = rng.choice(np.array([np.nan, np.inf, -np.inf, -3.0], np.float32), size=k.size)
    cur["film"], cur["half"] = film, (hf if half else None)
    p_half = hdr(rng, (H, W, 3))
    prev["half"] = p_half if half else None
    prev["film"] = p_half + hdr(rng, (H, W, 3)) if half else hdr(rng, (H, W, 3))
    length = rng.integers(0, 41, size=(H, W)).astype(np.float32)
    length[rng.random((H, W)) < 0.1] = 0.0
    prev["length"] = length
    return cur, prev, view_from_cameras(cam_c, cam_p), spp


# ---------------- an exact pixel grid: every projection is exact in binary32 ----------------
def grid_frame(W, H):
    """the G-buffer sums (one hit per pixel) of the plane z = -1 seen by the pinhole camera of grid_view: X = (i + 0.5 - W/2, -(j + 0.5 - H/2), -1)"""
    x = np.arange(W, dtype=np.float64)[None, :] + 0.5 - W / 2.0 + np.zeros((H, 1))
    y = -(np.arange(H, dtype=np.float64)[:, None] + 0.5 - H / 2.0) + np.zeros((1, W))
    X = np.stack([x, y, -np.ones((H, W))], -1)
    t = np.linalg.norm(X, axis=-1)
    one = np.ones((H, W))
    return dict(position=X.astype(np.float32), shading_normal=(np.array([0.5, 0.5, 1.0]) * one[..., None]).astype(np.float32),
                hit=np.stack([t, one, 0 * one], -1).astype(np.float32))


def grid_view(W, H, dx=0.0, dy=0.0):
    """plain data: identity rows, sx = sy = 1, so that pixel (i, j) of grid_frame lands on (i + dx, j + dy) EXACTLY (dx, dy small integers or
    dyadic fractions): the current camera stands dx to the right of and dy below the previous one"""
    return SimpleNamespace(delta=np.array([dx, -dy, 0.0], np.float32), rows=np.eye(3, dtype=np.float32).reshape(-1), sx=np.float32(1), sy=np.float32(1),
                           cx=np.float32(W / 2.0), cy=np.float32(H / 2.0))


# ---------------- rendered frames ----------------
def load_moved(backend, pkg, scene_id, W, H, move=(0.0, 0.0, 0.0), yaw=0.0, tex_size=128):
    """(scene, camera, D65 LUT id) of scenes.load_scene with the camera moved by `move` and turned by `yaw` radians about +y before the build"""
    sc = backend.new_scene()
    cam = pkg.scenes.load_scene(sc, scene_id, W, H, tex_size=tex_size, build=False)
    d65 = sc.add_lut470(pkg.scenes.presets()["cie_illum_d6500"])
    for i in range(3):
        cam.position[i] += move[i]
    if yaw != 0.0:
        d = yawed(tuple(cam.direction), yaw)
        for i in range(3):
            cam.direction[i] = d[i]
    sc.build(cam)
    return sc, cam, d65


CAMERA_PAIRS = {"x": ((0.3, 0.0, 0.0), 0.0), "xyz_yaw": ((0.3, 0.1, -0.2), 0.05)}      # the current camera: the scene's, moved and yawed
GEOMETRY_BARS = dict(median=0.1, share_under_quarter=0.97, interior_share=0.6)


def geometry_frames(gb_cur, gb_prev, cam_cur, cam_prev, spp_g):
    """The frames of the reprojection-geometry check: the previous film is the previous frame's WORLD-space mean hit position, the current
    beauty the current frame's (times spp_g); the previous length is 2^20, so that with max_history = 2^21 the output is the gathered
    history up to 2^-20 of its distance to the current value.  -> (cur, prev, params)"""
    def world(gb, cam):
        with np.errstate(all="ignore"):
            x = gb["position"] / gb["hit"][..., 1:2] + np.array(list(cam.position), np.float32)
        return np.where(gb["hit"][..., 1:2] > 0, x, 0).astype(np.float32)
    cur = dict(gb_cur, film=world(gb_cur, cam_cur) * np.float32(spp_g), half=None)
    prev = dict(gb_prev, film=world(gb_prev, cam_prev), half=None, length=np.full(gb_prev["hit"].shape[:2], 2.0 ** 20, np.float32))
    return cur, prev, params(max_history=2.0 ** 21)


def geometry_figures(out_film, cur, prev, view, prm, cam_cur, spp_g):
    """-> dict(median, share_under_quarter, interior_share, interior, hit): the distance between the gathered history (out_film of
    geometry_frames) and the current world-space position, in pixel footprints t 2 tan(fov / 2) / H, over the INTERIOR pixels: current
    hit.y == spp_g and all four taps valid, each with hit.y == spp_g"""
    _, _, _, info = accumulate(cur, spp_g, prev, view, prm, detail=True)
    H, W = cur["hit"].shape[:2]
    full_prev = prev["hit"][..., 1] == spp_g
    interior = cur["hit"][..., 1] == spp_g
    for k in range(4):
        qx, qy = np.clip(info["x0"] + (k & 1), 0, W - 1), np.clip(info["y0"] + (k >> 1), 0, H - 1)
        interior &= info["valid"][k] & full_prev[qy, qx]
    hit = cur["hit"][..., 1] > 0
    X = cur["position"].astype(np.float64) / spp_g + np.array(list(cam_cur.position), np.float64)
    t = cur["hit"][..., 0].astype(np.float64) / spp_g
    foot = t * 2.0 * math.tan(math.radians(cam_cur.fov_deg) / 2.0) / H
    with np.errstate(all="ignore"):
        d = np.linalg.norm(np.asarray(out_film, np.float64) - X, axis=-1) / foot
    d = d[interior]
    return dict(median=float(np.median(d)), share_under_quarter=float((d < 0.25).mean()), interior_share=float(interior.sum() / hit.sum()),
                interior=int(interior.sum()), hit=int(hit.sum()))


CLI_MISUSE = [   # argument lists of the mi355pt CLI that must exit 2 with a message, before any scene is loaded
    ["--renderer", "mis", "--temporal-frames", "0"],
    ["--renderer", "mis", "--temporal-frames", "3", "--gpus", "2"],
    ["--renderer", "normal", "--temporal-frames", "3"],
    ["--renderer", "albedo", "--temporal-frames", "3"],
    ["--renderer", "shading-normal", "--temporal-frames", "3"],
    ["--renderer", "position", "-o", "x.pfm", "--temporal-frames", "3"],
    ["--renderer", "depth", "-o", "x.pfm", "--temporal-frames", "3"],
    ["--renderer", "mis", "--spp", "16", "--temporal-frames", "3", "--adaptive-threshold", "0.05"],
    ["--renderer", "mis", "--temporal-frames", "3", "--denoise"],
    ["--renderer", "mis", "--camera-step", "0.1,0,0"],
]
