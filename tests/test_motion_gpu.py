"""GPU tests of the object motion vectors (include/mi355pt_motion.h): the ID pass (csrc/pt_kernels_ids.hip) pixel for pixel against a CPU
restatement on the oracle (tests/ids_reference.cpp), and the motion-aware accumulations (the motion kernels of
csrc/pt_kernels_temporal.hip and csrc/pt_kernels_temporal_rectify.hip) against the NumPy restatement of tests/motion_reference.py.  Every
operation of the kernels is a single binary32 operation in the order the header states, so the bar is BIT EQUALITY on every output value;
the outputs start as NaN, so a value the kernels leave out shows.  One line per comparison goes to the file MI355PT_FRAME_LOG names
(profiles/motion_parity.jsonl)."""
import ctypes
import json
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geometry_stress as gs  # noqa: E402
import ids_reference  # noqa: E402
import motion_reference as mr  # noqa: E402
import temporal_rectify_reference as rr  # noqa: E402
import temporal_reference as tr  # noqa: E402
from test_temporal_rectify_gpu import Device, assert_bit_equal, bits, ffi_params, ffi_rectify, ffi_view  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
SIZES = [(64, 48), (50, 37)]                 # the frame of the suite and a ragged one (partial 8 x 8 tiles, partial 64 x 4 blocks)
GUIDE_SPP, FRAME_SPP = 16, 4
HERO = 0                                     # scene 17's hero (tests/test_instance_move.py ORDINARY)
HERO_STEP = ((0.12, 0.0, 0.06), 0.05)        # per frame: a translation and a yaw in radians, applied in world space after the scene's matrix
CAMERA_STEP = (0.1, 0.02, -0.05)


def log_line(rec):
    print(json.dumps(rec))
    if os.environ.get("MI355PT_FRAME_LOG"):
        with open(os.environ["MI355PT_FRAME_LOG"], "a") as f:
            f.write(json.dumps(rec) + "\n")


@pytest.fixture(scope="module")
def dev(product, pkg):
    return MotionDevice(product, pkg)


@pytest.fixture(scope="module")
def reference():
    return ids_reference.IdsReference()


class MotionDevice(Device):
    """tests/test_temporal_rectify_gpu.py's Device plus one call of a motion-aware entry point; the outputs start as NaN"""

    def ids_up(self, ids):
        return self.torch.from_numpy(np.ascontiguousarray(ids, dtype=np.uint32).view(np.int32)).cuda() if ids is not None else None

    def table_up(self, table):
        return self.torch.from_numpy(np.ascontiguousarray(table, dtype=F)).cuda()

    def run_motion_device(self, cur, spp, prev, view, ids_cur, ids_prev, table, prm=None, rprm=None, rectified=False, scratch=None):
        """cur / prev: dicts of device tensors; ids and table: device tensors -> the three output tensors"""
        H, W = cur["film"].shape[:2]
        of, oh, ol = self.outputs(W, H, "half" in cur)
        ptr = lambda d: {k: v.data_ptr() for k, v in d.items()} if d is not None else None   # noqa: E731
        kw = {}
        if rectified:
            scratch = scratch if scratch is not None else self.scratch(W, H)
            kw = dict(rectify_params=ffi_rectify(self.product, rprm), d_scratch_ptr=scratch.data_ptr(), scratch_bytes=scratch.numel())
        self.product.temporal_accumulate_motion_device(ptr(cur), spp, ptr(prev), ffi_view(self.pkg, view), W, H, ffi_params(self.product, prm),
                                                       ids_cur.data_ptr(), ids_prev.data_ptr() if ids_prev is not None else None, table.data_ptr(),
                                                       table.shape[0], of.data_ptr(), oh.data_ptr() if oh is not None else None, ol.data_ptr(), **kw)
        self.torch.cuda.synchronize()
        return of, oh, ol

    def run_motion(self, cur, spp, prev, view, ids_cur, ids_prev, table, prm=None, rprm=None, rectified=False):
        """host frames in, host arrays out"""
        out = self.run_motion_device(self.up(cur), spp, self.up(prev), view, self.ids_up(ids_cur), self.ids_up(ids_prev), self.table_up(table), prm, rprm, rectified)
        return [x.cpu().numpy() if x is not None else None for x in out]

    def render_ids(self, sc, cam, params, into=None):
        """mi355pt_render_ids_device into a device buffer that starts as 0xffffffff -> (H, W) uint32 on the host"""
        t = into if into is not None else self.torch.full((cam.height, cam.width), -1, dtype=self.torch.int32, device="cuda")
        self.product.render_ids_device(sc, cam, params, t.data_ptr())
        self.torch.cuda.synchronize()
        return t.cpu().numpy().view(np.uint32), t


# ---------------- 1. the ID pass against the CPU restatement ----------------
def described(pkg, backend, case, W, H, builder=None):
    """(scene, camera) of scene 3 / 17 or a tests/geometry_stress.py family, built; `builder` on the product only"""
    if case in gs.NAMES:
        sc, cam, _ = gs.build_scene(backend, case, builder=builder, width=W, height=H, build=False)
    else:
        sc = backend.new_scene()
        cam = pkg.scenes.load_scene(sc, int(case), W, H, tex_size=16, build=False)
        if builder:
            sc.set_bvh_builder(builder)
    sc.build(cam)
    return sc, cam


@pytest.fixture(scope="module")
def reference_ids(pkg, reference):
    """the CPU ids per (case, W, H), computed once and left unchanged"""
    cache = {}

    def get(case, W, H):
        if (case, W, H) not in cache:
            sc, cam = described(pkg, reference, case, W, H)
            ids = reference.render_ids(sc, cam, pkg.make_params(1))
            ids.setflags(write=False)
            cache[(case, W, H)] = ids
        return cache[(case, W, H)]
    return get


@pytest.mark.parametrize("builder", ["host", "gpu"])
@pytest.mark.parametrize("case", ["3", "17", "instanced"])
def test_ids_match_the_cpu_restatement(dev, product, pkg, reference_ids, case, builder):
    """Scene 3 (local-triangle mode), scene 17 (several instances) and the `instanced` family, both builders, at 64 x 48, the ragged 50 x 37 and
    1 x 1: every pixel equals the CPU restatement (the same centre ray, the closest hit's primitive + 1, 0 for a miss); the result does not
    depend on spp, seed or sampler; three shards into one buffer equal the unsharded buffer, and one shard alone leaves the other pixels as
    they were."""
    for W, H in SIZES + [(1, 1)]:
        sc, cam = described(pkg, product, case, W, H, builder)
        want = reference_ids(case, W, H)
        got, _ = dev.render_ids(sc, cam, pkg.make_params(1))
        bad = int((got != want).sum())
        log_line({"test": "ids_parity", "case": case, "builder": builder, "size": [W, H], "pixels": int(want.size), "hit": int((want > 0).sum()),
                  "instances_seen": int(np.unique(want[want > 0]).size), "mismatching": bad})
        assert bad == 0, (case, builder, W, H, bad)
        if (W, H) == SIZES[0]:
            assert np.unique(want[want > 0]).size >= 2                                  # more than one instance is in view
        other, _ = dev.render_ids(sc, cam, pkg.make_params(7, "nee", "random", seed=12345))
        assert np.array_equal(other, got)
        if (W, H) == (1, 1):
            continue
        one, buf = dev.render_ids(sc, cam, pkg.make_params(1, shard_index=1, shard_count=3))
        tiles = (np.arange(H)[:, None] // 8) * ((W + 7) // 8) + np.arange(W)[None, :] // 8
        mine = tiles % 3 == 1
        assert np.array_equal(one[mine], want[mine]) and (one[~mine] == 0xffffffff).all()
        for k in (0, 2):
            dev.render_ids(sc, cam, pkg.make_params(1, shard_index=k, shard_count=3), into=buf)
        assert np.array_equal(buf.cpu().numpy().view(np.uint32), want)
    assert np.array_equal(product.render_ids(sc, cam, pkg.make_params(1)), want)       # the host-buffer form, at the last size


# ---------------- scene 17 with a hero that moves ----------------
def step_matrix(k, step=HERO_STEP):
    """the hero's step applied k times: R_y(k yaw) and k t, as a float64 4 x 4"""
    (t, yaw) = step
    c, s = math.cos(k * yaw), math.sin(k * yaw)
    m = np.eye(4)
    m[:3, :3] = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    m[:3, 3] = np.asarray(t, np.float64) * k
    return m


class HeroScene:
    """scene 17 at W x H with its hero marked dynamic, built once; pose(k) moves the hero to its k-th pose on the device"""

    def __init__(self, product, pkg, W, H, backend=None):
        self.product, self.pkg = product, pkg
        self.sc = (backend or product).new_scene()
        self.cam = pkg.scenes.load_scene(self.sc, 17, W, H, tex_size=16, build=False)
        self.d65 = self.sc.add_lut470(pkg.scenes.presets()["cie_illum_d6500"])
        self.sc.set_instance_dynamic(HERO)
        self.sc.build(self.cam)
        self.home = [m.copy() for _, _, m in self.sc.instances]
        self.now = [m.copy() for m in self.home]

    def matrices(self, k):
        out = [m.copy() for m in self.home]
        out[HERO] = (step_matrix(k) @ self.home[HERO].astype(np.float64)).astype(F)
        return out

    def pose(self, k):
        new = self.matrices(k)
        if new[HERO].tobytes() != self.now[HERO].tobytes():
            res = self.sc.move_instances(self.cam, [HERO], [new[HERO]])
            assert res["rebuilt"] == 0, res
        self.now = new
        return new

    def move_camera(self, position):
        for i in range(3):
            self.cam.position[i] = position[i]
        assert self.sc.move_camera(self.cam)["rebuilt"] == 0


def render_frame(dev, hs, seed, spp=FRAME_SPP, half=True):
    """one frame's device films (G-buffer sums at GUIDE_SPP, the half film, the film) and its ids"""
    torch, product, pkg = dev.torch, hs.product, hs.pkg
    H, W = hs.cam.height, hs.cam.width
    f = {k: torch.zeros((H, W, 3), dtype=torch.float32, device="cuda") for k in ("film", "position", "shading_normal", "hit")}
    g = {k: f[k].data_ptr() for k in ("shading_normal", "position", "hit")}
    product.render_gbuffer_accum_device(hs.sc, hs.cam, pkg.make_params(GUIDE_SPP, "mis", "sobol", seed=seed), hs.d65, 0, GUIDE_SPP, g)
    prm = pkg.make_params(spp, "mis", "sobol", seed=seed)
    if half:
        f["half"] = torch.zeros_like(f["film"])
        product.render_accum_device(hs.sc, hs.cam, prm, 0, spp // 2, f["half"].data_ptr())
        torch.cuda.synchronize()
        f["film"].copy_(f["half"])
        product.render_accum_device(hs.sc, hs.cam, prm, spp // 2, spp, f["film"].data_ptr())
    else:
        product.render_accum_device(hs.sc, hs.cam, prm, 0, spp, f["film"].data_ptr())
    _, ids = dev.render_ids(hs.sc, hs.cam, pkg.make_params(1))
    return f, ids


def host(f):
    return {k: v.cpu().numpy() for k, v in f.items()}


def uniform3(ids):
    """pixels whose id is the same over their 3 x 3 neighbourhood (frame edges are not)"""
    H, W = ids.shape
    ok = np.zeros((H, W), bool)
    c = ids[1:-1, 1:-1]
    same = np.ones(c.shape, bool)
    for dy in range(3):
        for dx in range(3):
            same &= ids[dy:dy + H - 2, dx:dx + W - 2] == c
    ok[1:-1, 1:-1] = same
    return ok


def test_ids_follow_an_instance_move(dev, product, pkg):
    """after mi355pt_scene_move_instances (a translation and a yaw of the dynamic hero) the ID buffer equals that of a scene freshly BUILT
    from the updated description, and differs from the buffer before the move"""
    W, H = SIZES[0]
    hs = HeroScene(product, pkg, W, H)
    before, _ = dev.render_ids(hs.sc, hs.cam, pkg.make_params(1))
    new = hs.pose(3)
    after, _ = dev.render_ids(hs.sc, hs.cam, pkg.make_params(1))
    fresh = product.new_scene()
    add = fresh.add_instance
    fresh.add_instance = lambda geom, mat, local_to_world=None: add(geom, mat, new[HERO] if len(fresh.instances) == HERO else local_to_world)
    cam = pkg.scenes.load_scene(fresh, 17, W, H, tex_size=16, build=False)
    fresh.set_instance_dynamic(HERO)
    fresh.build(cam)
    want, _ = dev.render_ids(fresh, cam, pkg.make_params(1))
    log_line({"test": "ids_follow_move", "changed_by_move": int((after != before).sum()), "mismatching": int((after != want).sum())})
    assert np.array_equal(after, want) and (after != before).sum() > 20 and (after == HERO + 1).sum() > 100


# ---------------- 3. / 4. synthetic frames ----------------
def synthetic_case(W, H, view, half, n_entries=3):
    cur, prev, vw, spp = tr.synthetic(W, H, view, "step", half)
    ids_cur, ids_prev = mr.synthetic_ids(W, H)                      # ids 0 .. 4: those above n_entries - 1 are clamped
    table = mr.static_table(vw, n_entries)
    table[1] = mr.moved_entry(vw)
    return cur, prev, vw, spp, ids_cur, ids_prev, table


@pytest.mark.parametrize("half", [True, False], ids=["half", "nohalf"])
@pytest.mark.parametrize("shape", [(64, 48), (70, 50), (1, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_motion_synthetic_parity(dev, shape, half):
    """Seeded synthetic frames (tests/temporal_reference.py synthetic) with a synthetic id map — vertical bands of the ids 0 .. 4, of which 3
    and 4 lie above the table and are clamped to its last entry — and a table of one moved (a yaw and a shift) and two static entries; with
    and without the half film, with and without the previous frame's ids (bands shifted by two pixels and seeded disagreements), the plain
    and the rectified kernels, a static view and a camera move: every output value is bit-equal to tests/motion_reference.py."""
    W, H = shape
    for view in ("static", "move"):
        cur, prev, vw, spp, ids_cur, ids_prev, table = synthetic_case(W, H, view, half)
        dc, dp, di, dq, dt = dev.up(cur), dev.up(prev), dev.ids_up(ids_cur), dev.ids_up(ids_prev), dev.table_up(table)
        for with_prev_ids in (False, True):
            ip, dip = (ids_prev, dq) if with_prev_ids else (None, None)
            tag = f"{W}x{H}_{'half' if half else 'nohalf'}_{view}_{'ids' if with_prev_ids else 'noids'}"
            got = [x.cpu().numpy() if x is not None else None for x in dev.run_motion_device(dc, spp, dp, vw, di, dip, dt)]
            assert_bit_equal(got, mr.accumulate_motion(cur, spp, prev, vw, ids_cur, ip, table), "motion_synthetic_" + tag)
            got = [x.cpu().numpy() if x is not None else None for x in dev.run_motion_device(dc, spp, dp, vw, di, dip, dt, rectified=True)]
            assert_bit_equal(got, mr.accumulate_rectified_motion(cur, spp, prev, vw, ids_cur, ip, table), "motion_rectified_synthetic_" + tag)
        if (W, H) != (1, 1):
            base = tr.accumulate(cur, spp, prev, vw)[0]
            assert not np.array_equal(bits(got[0]), bits(base))                        # the motion and the id test changed something


@pytest.mark.parametrize("half", [True, False], ids=["half", "nohalf"])
def test_static_table_equals_the_existing_call(dev, half):
    """The same device buffers, a table of static entries only, no previous ids: all three outputs of the motion-aware call are bit-equal
    to mi355pt_temporal_accumulate_device's, and the rectified pair likewise — through every view, ids above the table included."""
    W, H = 70, 50
    for view in ("static", "move", "outside", "behind"):
        cur, prev, vw, spp = tr.synthetic(W, H, view, "step", half)
        ids_cur, _ = mr.synthetic_ids(W, H)
        dc, dp, di, dt = dev.up(cur), dev.up(prev), dev.ids_up(ids_cur), dev.table_up(mr.static_table(vw, 3))
        for rectified in (False, True):
            got = dev.run_motion_device(dc, spp, dp, vw, di, None, dt, rectified=rectified)
            want = dev.run_device(dc, spp, dp, vw, rectified=rectified)
            for name, a, b in zip(("film", "half", "length"), got, want):
                assert (a is None) == (b is None)
                if a is not None:
                    a, b = a.cpu().numpy(), b.cpu().numpy()
                    assert not np.isnan(a).any() and np.array_equal(bits(a), bits(b)), (view, rectified, name, int((bits(a) != bits(b)).sum()))
        log_line({"test": "motion_static_table_equals_existing", "view": view, "half": half, "mismatching": 0})


# ---------------- 5. a rendered, moved object ----------------
def hero_geometry(out_film, cur, cam_cur, interior):
    """temporal_reference.geometry_figures' measure — the distance between the gathered history (out_film of geometry frames) and the current
    world-space position in pixel footprints t 2 tan(fov / 2) / H — over the pixels of `interior`"""
    H = cur["hit"].shape[0]
    X = cur["position"].astype(np.float64) / GUIDE_SPP + np.array(list(cam_cur.position), np.float64)
    t = cur["hit"][..., 0].astype(np.float64) / GUIDE_SPP
    foot = t * 2.0 * math.tan(math.radians(cam_cur.fov_deg) / 2.0) / H
    with np.errstate(all="ignore"):
        d = np.linalg.norm(np.asarray(out_film, np.float64) - X, axis=-1) / foot
    d = d[interior]
    return dict(median=float(np.median(d)), share_under_quarter=float((d < 0.25).mean()), interior=int(interior.sum()))


@pytest.mark.parametrize("camera_moves", [False, True], ids=["camera_fixed", "camera_step"])
def test_rendered_moved_object(dev, product, pkg, camera_moves):
    """Scene 17 at 64 x 48 with its hero dynamic, two frames, the hero translated and yawed between them; without and with a camera step as
    well.  The motion-aware accumulation of frame 1 over frame 0 — with the previous ids, plain and rectified — is bit-equal to the
    restatement on the same buffers.  Reprojection error: the frames of temporal_reference.geometry_frames (the previous film holds world
    positions — for the hero's pixels carried to the current pose, so that a correct reprojection gathers the current pixel's own world
    position) over the hero's INTERIOR pixels: id == hero over the 3 x 3 neighbourhood in both frames (in the current frame at the pixel,
    in the previous one at all four taps), full G-buffer coverage.  Held to temporal_reference.GEOMETRY_BARS, the bars
    tests/test_temporal_gpu.py holds camera moves to: median <= 0.1 footprints, >= 0.97 under 0.25, and history on >= 0.6 of them.
    Against the static-world call on the same buffers: pixels that show a static instance are bit-equal between the two calls (no previous
    ids in this comparison: that is the header's statement), and the share of hero interior pixels with history is strictly higher with
    motion."""
    W, H = SIZES[0]
    hs = HeroScene(product, pkg, W, H)
    cam_prev = pkg.ffi.Camera.from_buffer_copy(hs.cam)
    m_prev = hs.pose(0)
    f0, ids0 = render_frame(dev, hs, 0)
    if camera_moves:
        hs.move_camera([cam_prev.position[i] + CAMERA_STEP[i] for i in range(3)])
    m_cur = hs.pose(1)
    f1, ids1 = render_frame(dev, hs, 1)
    cam_cur = hs.cam
    view = product.temporal_view_from_cameras(cam_cur, cam_prev)
    table = product.motion_table(cam_cur, cam_prev, m_cur, m_prev)
    tag = "camera_step" if camera_moves else "camera_fixed"
    assert np.array_equal(bits(table[0]), bits(mr.static_table(view, 1)[0])) and not np.array_equal(table[HERO + 1], table[0])
    assert all(np.array_equal(bits(table[i + 1]), bits(table[0])) for i in range(len(m_cur)) if i != HERO)
    a0 = dev.run_motion_device(f0, FRAME_SPP, None, None, ids0, None, dev.table_up(table))
    geo = ("position", "shading_normal", "hit")
    prev = dict({k: f0[k] for k in geo}, film=a0[0], half=a0[1], length=a0[2])
    h1, hp, i0, i1 = host(f1), host(prev), ids0.cpu().numpy().view(np.uint32), ids1.cpu().numpy().view(np.uint32)
    dt = dev.table_up(table)
    for rectified in (False, True):
        got = [x.cpu().numpy() for x in dev.run_motion_device(f1, FRAME_SPP, prev, view, ids1, ids0, dt, rectified=rectified)]
        fn = mr.accumulate_rectified_motion if rectified else mr.accumulate_motion
        assert_bit_equal(got, fn(h1, FRAME_SPP, hp, view, i1, i0, table), f"motion_rendered_{tag}_{'rectified' if rectified else 'plain'}")

    # the contrast with the static-world call, on the same buffers
    with_motion = mr.accumulate_motion(h1, FRAME_SPP, hp, view, i1, None, table, detail=True)
    got_m = [x.cpu().numpy() for x in dev.run_motion_device(f1, FRAME_SPP, prev, view, ids1, None, dt)]
    got_s = [x.cpu().numpy() for x in dev.run_device(f1, FRAME_SPP, prev, view, rectified=False)]
    assert_bit_equal(got_m, with_motion[:3], f"motion_rendered_{tag}_noids")
    static_pixels = (i1 != HERO + 1)
    for a, b in zip(got_m, got_s):
        assert np.array_equal(bits(a)[static_pixels], bits(b)[static_pixels])
    hero_cur, hero_prev = uniform3(i1) & (i1 == HERO + 1), uniform3(i0) & (i0 == HERO + 1)
    static_info = tr.accumulate(h1, FRAME_SPP, hp, view, detail=True)[3]
    share_m, share_s = float(with_motion[3]["has"][hero_cur].mean()), float(static_info["has"][hero_cur].mean())

    # the reprojection error on the hero's interior
    gb1, gb0 = {k: h1[k] for k in geo}, {k: hp[k] for k in geo}
    cur_g, prev_g, prm = tr.geometry_frames(gb1, gb0, cam_cur, cam_prev, GUIDE_SPP)
    T_inv = mr.mat4(m_cur[HERO]) @ np.linalg.inv(mr.mat4(m_prev[HERO]))                # previous world -> current world, for the hero's points
    carried = (prev_g["film"].astype(np.float64) @ T_inv[:3, :3].T + T_inv[:3, 3]).astype(F)
    prev_g["film"] = np.where((i0 == HERO + 1)[..., None], carried, prev_g["film"]).astype(F)
    out_g = dev.run_motion(cur_g, GUIDE_SPP, prev_g, view, i1, i0, table, prm)
    want_g = mr.accumulate_motion(cur_g, GUIDE_SPP, prev_g, view, i1, i0, table, prm, detail=True)
    assert_bit_equal(out_g, want_g[:3], f"motion_rendered_{tag}_geometry")
    info = want_g[3]
    interior = hero_cur & (gb1["hit"][..., 1] == GUIDE_SPP) & info["has"]
    full_prev = hero_prev & (gb0["hit"][..., 1] == GUIDE_SPP)
    for k in range(4):
        qx, qy = np.clip(info["x0"] + (k & 1), 0, W - 1), np.clip(info["y0"] + (k >> 1), 0, H - 1)
        interior &= info["valid"][k] & full_prev[qy, qx]
    fig = hero_geometry(out_g[0], cur_g, cam_cur, interior)
    candidates = int((hero_cur & (gb1["hit"][..., 1] == GUIDE_SPP)).sum())
    fig["interior_share"] = fig["interior"] / max(candidates, 1)
    log_line(dict({"test": "motion_rendered_geometry", "camera": tag, "hero_interior_candidates": candidates, "history_share_motion": share_m,
                   "history_share_static": share_s}, **fig))
    bars = tr.GEOMETRY_BARS
    assert fig["interior"] > 50 and fig["interior_share"] >= bars["interior_share"], fig
    assert fig["median"] <= bars["median"] and fig["share_under_quarter"] >= bars["share_under_quarter"], fig
    assert share_m > share_s, (share_m, share_s)


# ---------------- 6. convergence under motion ----------------
def test_convergence_under_motion(dev, product, pkg):
    """8 frames of 4 spp with the hero stepping every frame (no half film, the plain kernel, the previous frame's ids), against a 256-spp
    frame of the last pose: over the hero's interior pixels of the last frame (id uniform over 3 x 3) the RMSE of the accumulated frame is
    below that of the last 4-spp frame alone.  The static-world accumulation of the same frames is recorded beside it, not asserted: nobody
    has measured it."""
    torch = dev.torch
    W, H = SIZES[0]
    hs = HeroScene(product, pkg, W, H)
    cam = hs.cam
    view = product.temporal_view_from_cameras(cam, cam)
    acc = {"motion": None, "static": None}
    prev_f, prev_ids, prev_m = None, None, None
    for k in range(8):
        m = hs.pose(k)
        f, ids = render_frame(dev, hs, k, half=False)
        for name in acc:
            if prev_f is None:
                out = dev.run_device(f, FRAME_SPP, None, None, rectified=False)
            else:
                prev = dict({g: prev_f[g] for g in ("position", "shading_normal", "hit")}, film=acc[name][0], length=acc[name][2])
                if name == "motion":
                    table = dev.table_up(product.motion_table(cam, cam, m, prev_m))
                    out = dev.run_motion_device(f, FRAME_SPP, prev, view, ids, prev_ids, table)
                else:
                    out = dev.run_device(f, FRAME_SPP, prev, view, rectified=False)
            acc[name] = out
        prev_f, prev_ids, prev_m = f, ids, m
    ref = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    product.render_accum_device(hs.sc, cam, pkg.make_params(256, "mis", "sobol", seed=1000), 0, 256, ref.data_ptr())
    torch.cuda.synchronize()
    ref = ref.cpu().numpy().astype(np.float64) / 256.0
    i_last = prev_ids.cpu().numpy().view(np.uint32)
    interior = uniform3(i_last) & (i_last == HERO + 1)
    rmse = lambda a: float(np.sqrt(np.mean((a[interior] - ref[interior]) ** 2)))   # noqa: E731
    e_last = rmse(prev_f["film"].cpu().numpy().astype(np.float64) / FRAME_SPP)
    e_motion, e_static = rmse(acc["motion"][0].cpu().numpy().astype(np.float64)), rmse(acc["static"][0].cpu().numpy().astype(np.float64))
    len_motion = float(acc["motion"][2].cpu().numpy()[interior].mean())
    log_line({"test": "motion_convergence", "frames": 8, "spp": FRAME_SPP, "hero_interior": int(interior.sum()), "rmse_last_frame": e_last,
              "rmse_motion": e_motion, "rmse_static_world": e_static, "mean_history_length_motion": len_motion})
    assert interior.sum() > 50
    assert e_motion < e_last, (e_motion, e_last)


# ---------------- 7. determinism, the host forms, the refusals ----------------
def test_motion_is_deterministic_and_host_forms_match(dev, product, pkg):
    """Two calls are bit-equal; the host-buffer forms equal the device forms — plain and rectified, with and without a half film, previous
    ids and a previous frame."""
    W, H = 70, 50
    for half in (True, False):
        cur, prev, vw, spp, ids_cur, ids_prev, table = synthetic_case(W, H, "move", half)
        for p, v, ip in ((prev, vw, ids_prev), (prev, vw, None), (None, None, None)):
            for rectified in (False, True):
                one = dev.run_motion(cur, spp, p, v, ids_cur, ip, table, rectified=rectified)
                two = dev.run_motion(cur, spp, p, v, ids_cur, ip, table, rectified=rectified)
                hostf = product.temporal_accumulate_motion(cur, spp, p, ffi_view(pkg, v), ids_cur, ip, table,
                                                           rectify_params=product.temporal_rectify_params_default() if rectified else None)
                for a, b, c in zip(one, two, hostf):
                    assert (a is None) == (b is None) == (c is None)
                    if a is not None:
                        assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a), bits(c))


def test_motion_refusals_with_real_buffers(dev, product, pkg):
    """What the header refuses beyond its twins, with device buffers: MI355PT_E_INVALID, the outputs and the scratch stay untouched."""
    f = pkg.ffi
    W, H = 70, 50
    cur, prev, vw, spp, ids_cur, ids_prev, table = synthetic_case(W, H, "move", True)
    dc, dp, di, dq, dt = dev.up(cur), dev.up(prev), dev.ids_up(ids_cur), dev.ids_up(ids_prev), dev.table_up(table)
    outs = dev.outputs(W, H, True)
    scratch = dev.scratch(W, H)
    view, good, rgood = ffi_view(pkg, vw), product.temporal_params_default(), product.temporal_rectify_params_default()
    frame = lambda d: f.TemporalFrame(*[{k: v.data_ptr() for k, v in d.items()}.get(k) for k in f.TEMPORAL_FILMS])   # noqa: E731
    fc, fp, o = frame(dc), frame(dp), [x.data_ptr() for x in outs]
    ref = lambda x: ctypes.byref(x) if x is not None else None   # noqa: E731
    lib = product.lib

    def refused(ic, ip, tb, n, out=o, p=good, rp=rgood, sp=scratch.data_ptr(), nbytes=scratch.numel()):
        rc = lib.mi355pt_temporal_accumulate_motion_device(ref(fc), spp, ref(fp), ref(view), W, H, ref(p), ic, ip, tb, n, *out, None)
        assert rc == -1 and b"temporal" in lib.mi355pt_last_error(), rc
        rc = lib.mi355pt_temporal_accumulate_rectified_motion_device(ref(fc), spp, ref(fp), ref(view), W, H, ref(p), ref(rp), sp, nbytes, ic, ip, tb, n, *out, None)
        assert rc == -1 and b"temporal" in lib.mi355pt_last_error(), rc
    ic, ip, tb, n = di.data_ptr(), dq.data_ptr(), dt.data_ptr(), table.shape[0]
    refused(None, ip, tb, n)                                  # no current ids
    refused(ic, ip, None, n)                                  # no table
    refused(ic, ip, tb, 0)                                    # no entries
    refused(ic, ip, tb + 4, n)                                # a table that is not 16-byte aligned
    refused(o[0], ip, tb, n)                                  # the current ids alias an output
    refused(ic, o[2], tb, n)                                  # the previous ids alias an output
    refused(ic, ip, o[1], n)                                  # the table aliases an output
    refused(ic, ip, tb, n, p=f.TemporalParams())              # a refusal of the twin: zeroed parameters
    refused(ic, ip, tb, n, out=[o[0], o[0], o[2]])            # ... two outputs are the same buffer
    rc = lib.mi355pt_temporal_accumulate_rectified_motion_device(ref(fc), spp, ref(fp), ref(view), W, H, ref(good), ref(rgood), ic, scratch.numel(), ic, ip, tb, n, *o, None)
    assert rc == -1                                           # the scratch is the id buffer
    dev.torch.cuda.synchronize()
    assert all(np.isnan(x.cpu().numpy()).all() for x in outs) and bool((scratch == 0x5a).all())
    # the ID pass
    sc, cam = described(pkg, product, "3", 16, 16)
    prm = pkg.make_params(1)
    fn = lib.mi355pt_render_ids_device
    assert fn(sc.h, ctypes.byref(cam), ctypes.byref(prm), None, None, None) == -1
    assert fn(None, ctypes.byref(cam), ctypes.byref(prm), di.data_ptr(), None, None) == -1
    assert fn(sc.h, ctypes.byref(cam), ctypes.byref(pkg.make_params(1, collect_stats=1)), di.data_ptr(), None, None) == -1
    zero = pkg.ffi.Camera.from_buffer_copy(cam); zero.width = 0
    assert fn(sc.h, ctypes.byref(zero), ctypes.byref(prm), di.data_ptr(), None, None) == -1
    unbuilt = product.new_scene()
    pkg.scenes.load_scene(unbuilt, 3, 16, 16, tex_size=16, build=False)
    assert fn(unbuilt.h, ctypes.byref(cam), ctypes.byref(prm), di.data_ptr(), None, None) == -3
    assert np.array_equal(di.cpu().numpy().view(np.uint32), ids_cur)


# ---------------- 8. the CLI ----------------
from test_instance_move_gpu import cli, cli_matrix  # noqa: E402,F401  (the CLI fixture and host/main.cpp's matrix, shared)

CLI_STEPS = {1: ((0.1, 0.0, 0.05), 10.0), 6: ((0.0, 0.02, 0.0), 0.0)}      # instance: (translation, ry_deg) per frame — scene 3's box and a wall


def replay(product, pkg, dev, frames, camera_step, rprm):
    """the calls of `mi355pt --scene 3 --temporal-frames N --instance-step ...` (no half film) through the ABI from the public pieces -> u8"""
    import torch
    W, H = SIZES[0]
    sc = product.new_scene()
    cam = pkg.scenes.load_scene(sc, 3, W, H, build=False)
    d65 = sc.add_lut470(pkg.scenes.presets()["cie_illum_d6500"])
    for i in CLI_STEPS:
        sc.set_instance_dynamic(i)
    sc.build(cam)
    base = np.array(list(cam.position), F)
    now = [m.copy() for _, _, m in sc.instances]
    acc, g, prev_cam, prev_ids, prev_m = None, None, None, None, None
    for k in range(frames):
        pos = base + F(k) * np.asarray(camera_step, F)
        for i in range(3):
            cam.position[i] = pos[i]
        if k > 0 and any(s != 0.0 for s in camera_step):
            sc.build(cam)                                                              # --camera-move rebuild, the default
        prev_m = [m.copy() for m in now]
        if k > 0:
            for i, (t, ry) in CLI_STEPS.items():
                now[i] = cli_matrix(t, ry, (1.0, 1.0, 1.0), now[i])
            assert sc.move_instances(cam, sorted(CLI_STEPS), [now[i] for i in sorted(CLI_STEPS)])["rebuilt"] == 0
        f = {n: torch.zeros((H, W, 3), dtype=torch.float32, device="cuda") for n in ("film", "position", "shading_normal", "hit")}
        gb = {n: f[n].data_ptr() for n in ("shading_normal", "position", "hit")}
        product.render_gbuffer_accum_device(sc, cam, pkg.make_params(GUIDE_SPP, "mis", "sobol", seed=k), d65, 0, GUIDE_SPP, gb)
        product.render_accum_device(sc, cam, pkg.make_params(FRAME_SPP, "mis", "sobol", seed=k), 0, FRAME_SPP, f["film"].data_ptr())
        _, ids = dev.render_ids(sc, cam, pkg.make_params(GUIDE_SPP, "mis", "sobol", seed=k))
        prev, view = None, None
        if acc is not None:
            prev = dict({n: g[n] for n in ("position", "shading_normal", "hit")}, film=acc[0], length=acc[2])
            view = product.temporal_view_from_cameras(cam, prev_cam)
        table = dev.table_up(product.motion_table(cam, prev_cam if prev_cam is not None else cam, now, prev_m))
        acc = dev.run_motion_device(f, FRAME_SPP, prev, view, ids, prev_ids if prev is not None else None, table, None, rprm, rectified=rprm is not None)
        g, prev_cam, prev_ids = f, pkg.ffi.Camera.from_buffer_copy(cam), ids
    rgb = torch.empty_like(acc[0])
    product.film_resolve_device(acc[0].data_ptr(), W * H, 1, rgb.data_ptr())
    torch.cuda.synchronize()
    return product.quantize_u8(rgb.cpu().numpy())


def test_motion_cli(product, pkg, dev, cli, tmp_path):
    """`--temporal-frames 3 --instance-step 1:... --instance-step 6:...` at 64 x 48 — plain, and with --temporal-rectify and a --camera-step —
    writes the picture of the same calls replayed through the ABI, u8-equal, says one line per moved frame on stderr, and differs from the
    picture without the steps; every refusal exits 2 naming --instance-step, and --instance-transform with --temporal-frames stays refused."""
    import subprocess
    from PIL import Image
    exe, env = cli
    W, H = SIZES[0]
    base = [exe, "--scene", "3", "--renderer", "mis", "--sampler", "sobol", "--spp", str(FRAME_SPP), "--width", str(W), "--height", str(H),
            "--denoise-guide-spp", str(GUIDE_SPP)]
    steps = []
    for i, (t, ry) in sorted(CLI_STEPS.items(), reverse=True):                          # (given out of order: the CLI sorts)
        steps += ["--instance-step", "%d:%g,%g,%g" % ((i,) + t) + (":%g" % ry if ry else "")]

    def picture(extra, name):
        path = str(tmp_path / name)
        r = subprocess.run(base + ["--temporal-frames", "3"] + extra + ["-o", path], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        return np.asarray(Image.open(path).convert("RGB")), r.stderr
    still, _ = picture([], "still.png")
    for name, extra, camera_step, rprm in (("plain", [], (0.0, 0.0, 0.0), None),
                                           ("rectified", ["--temporal-rectify", "--camera-step", "0.1,0,0"], (0.1, 0.0, 0.0), rr.params())):
        got, err = picture(steps + extra, name + ".png")
        lines = [ln for ln in err.splitlines() if ln.startswith("instance step, frame ")]
        assert len(lines) == 2 and all("rebuilt=0" in ln for ln in lines), err
        want = replay(product, pkg, dev, 3, camera_step, rprm)
        log_line({"test": "motion_cli", "run": name, "differing_u8": int((got != want).sum()), "differs_from_still": int((got != still).sum())})
        assert got.shape == want.shape and np.array_equal(got, want), (name, int((got != want).sum()))
        assert got.mean() > 10.0 and not np.array_equal(got, still)
    t3 = ["--temporal-frames", "3"]
    for args in (["--instance-step", "1:0.1,0,0"],                                                        # without --temporal-frames
                 t3 + ["--instance-step", "1:0.1,0,0", "--half-res", "--denoise-variance"],             # out of scope here
                 ["--instance-step", "1:0.1,0,0", "--instance-transform", "1:0,0.1,0"],                  # the same id twice over
                 t3 + ["--instance-step", "99:0.1,0,0"],                                                 # a bad id
                 t3 + ["--instance-step", "1:0.1,0"], t3 + ["--instance-step", "x:0,0,0"], t3 + ["--instance-step", "1:0,0,0:30:1,1,1"],
                 t3 + ["--instance-step", "1:0,0,nan"], t3 + ["--instance-step", "1:0,0,0", "--instance-step", "1:1,0,0"]):
        r = subprocess.run(base + args, env=env, capture_output=True, text=True, timeout=120, cwd=tmp_path)
        assert r.returncode == 2 and "--instance-step" in r.stderr, (args, r.returncode, r.stderr)
    r = subprocess.run(base + t3 + ["--instance-transform", "1:0,0,0"], env=env, capture_output=True, text=True, timeout=120, cwd=tmp_path)
    assert r.returncode == 2 and "--temporal-frames" in r.stderr and "--instance-step" not in r.stderr
