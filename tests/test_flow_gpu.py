"""GPU tests of the per-pixel motion vectors (include/mi355pt_flow.h): the mark and its lifecycle, the flow pass (csrc/pt_kernels_flow.hip)
against the NumPy restatement of tests/flow_reference.py fed the kernel's own hits — BIT EQUALITY on every record — and against the
oracle's centre-ray hits (tests/flow_reference.cpp), and the flow-aware accumulations (csrc/pt_kernels_temporal.hip) against the
restatement, bit for bit; then what the records buy on a deforming mesh.  The outputs start as NaN or 0xff, so a value the kernels leave
out shows.  One line per comparison goes to the file MI355PT_FRAME_LOG names (profiles/flow_parity.jsonl)."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_hits_reference  # noqa: E402
import flow_reference as fr  # noqa: E402
import geometry_stress as gs  # noqa: E402
import temporal_rectify_reference as rr  # noqa: E402
import temporal_reference as tr  # noqa: E402
from test_deform import Remeshed, arrays_of, deformed  # noqa: E402
from test_instance_move import DEGRADING_STEP, applied, trs  # noqa: E402
from test_temporal_rectify_gpu import Device, assert_bit_equal, bits, ffi_params, ffi_rectify, ffi_view  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
W, H = 64, 48
GUIDE_SPP, FRAME_SPP = 16, 4
CAMERA_STEP = (0.1, 0.02, -0.05)
# case: (mesh that deforms, instance that moves or None).  Scene 3 is in local-triangle mode while no instance is dynamic, so nothing
# moves there but the camera and the vertices; scene 24's root is a leaf (one triangle)
CASES = {"3": (1, None), "17": (0, 0), "instanced": (0, 2), "24": (0, None)}
# |Xc - oracle position| / max|P|, measured on these scenes after every move of test_records_after_moves (profiles/flow_parity.jsonl,
# "xc_rel_max"): the largest value seen is 1.93e-7 (scenes 3 and 17 after all three moves; a position of 10 units, so 1.6 ulp); the bar is
# twice that
XC_REL_TOL = 3.86e-7


def log_line(rec):
    print(json.dumps(rec))
    if os.environ.get("MI355PT_FRAME_LOG"):
        with open(os.environ["MI355PT_FRAME_LOG"], "a") as f:
            f.write(json.dumps(rec) + "\n")


class FlowDevice(Device):
    """tests/test_temporal_rectify_gpu.py's Device plus the flow pass and one call of a flow-aware entry point; the outputs start as NaN"""

    def ids_up(self, ids):
        return self.torch.from_numpy(np.ascontiguousarray(ids, dtype=np.uint32).view(np.int32)).cuda() if ids is not None else None

    def flow_up(self, flow):
        return self.torch.from_numpy(np.ascontiguousarray(flow, dtype=fr.FLOW_PIXEL).view(np.int32).reshape(flow.shape + (8,))).cuda()

    def run_flow_device(self, cur, spp, prev, view, ids_cur, ids_prev, flow, prm=None, rprm=None, rectified=False):
        """cur / prev: dicts of device tensors; ids and flow: device tensors -> the three output tensors"""
        h, w = cur["film"].shape[:2]
        of, oh, ol = self.outputs(w, h, "half" in cur)
        ptr = lambda d: {k: v.data_ptr() for k, v in d.items()} if d is not None else None   # noqa: E731
        kw = {}
        if rectified:
            scratch = self.scratch(w, h)
            kw = dict(rectify_params=ffi_rectify(self.product, rprm), d_scratch_ptr=scratch.data_ptr(), scratch_bytes=scratch.numel())
        self.product.temporal_accumulate_flow_device(ptr(cur), spp, ptr(prev), ffi_view(self.pkg, view), w, h, ffi_params(self.product, prm),
                                                     ids_cur.data_ptr() if ids_cur is not None else None, ids_prev.data_ptr() if ids_prev is not None else None,
                                                     flow.data_ptr(), of.data_ptr(), oh.data_ptr() if oh is not None else None, ol.data_ptr(), **kw)
        self.torch.cuda.synchronize()
        return of, oh, ol

    def run_flow(self, cur, spp, prev, view, ids_cur, ids_prev, flow, prm=None, rprm=None, rectified=False):
        out = self.run_flow_device(self.up(cur), spp, self.up(prev), view, self.ids_up(ids_cur), self.ids_up(ids_prev), self.flow_up(flow), prm, rprm, rectified)
        return [x.cpu().numpy() if x is not None else None for x in out]

    def render_ids(self, sc, cam, params):
        t = self.torch.full((cam.height, cam.width), -1, dtype=self.torch.int32, device="cuda")
        self.product.render_ids_device(sc, cam, params, t.data_ptr())
        self.torch.cuda.synchronize()
        return t.cpu().numpy().view(np.uint32), t

    def render_flow(self, sc, cam, params, want_ids=True, into=None):
        """mi355pt_render_flow_device into device buffers that start as 0xff bytes -> ((H, W) FLOW_PIXEL, (H, W) uint32 or None, the tensors)"""
        fl, ids = into if into is not None else (self.torch.full((cam.height, cam.width, 8), -1, dtype=self.torch.int32, device="cuda"),
                                                 self.torch.full((cam.height, cam.width), -1, dtype=self.torch.int32, device="cuda") if want_ids else None)
        self.product.render_flow_device(sc, cam, params, fl.data_ptr(), ids.data_ptr() if ids is not None else None)
        self.torch.cuda.synchronize()
        rec = fl.cpu().numpy().view(fr.FLOW_PIXEL).reshape(cam.height, cam.width)
        return rec, (ids.cpu().numpy().view(np.uint32) if ids is not None else None), (fl, ids)


@pytest.fixture(scope="module")
def dev(product, pkg):
    return FlowDevice(product, pkg)


@pytest.fixture(scope="module")
def reference():
    return flow_hits_reference.FlowHitsReference()


def raw(rec):
    return np.ascontiguousarray(rec).view(np.uint32)


def describe(pkg, backend, case, w=W, h=H, builder=None, replace=None, matrices=None):
    """(scene, camera) described, not built.  replace: vertex arrays for some meshes from the start; matrices: {instance: local_to_world}
    from the start (the way to the oracle's scene of a moved state)"""
    be = Remeshed(backend, replace)
    real_new = be.new_scene

    def new_scene():
        sc = real_new()
        add = sc.add_instance
        sc.add_instance = lambda geom, mat, local_to_world=None: add(geom, mat, (matrices or {}).get(len(sc.instances), local_to_world))
        return sc
    be.new_scene = new_scene
    if case in gs.NAMES:
        sc, cam, _ = gs.build_scene(be, case, builder=builder, width=w, height=h, build=False)
    else:
        sc = be.new_scene()
        cam = pkg.scenes.load_scene(sc, int(case), w, h, tex_size=16, build=False)
        if builder:
            sc.set_bvh_builder(builder)
    return sc, cam


def built(pkg, product, case, builder, w=W, h=H):
    sc, cam = describe(pkg, product, case, w, h, builder)
    inst = CASES[case][1]
    if inst is not None:
        sc.set_instance_dynamic(inst)
    sc.build(cam)
    return sc, cam


def move_camera(sc, cam, step=CAMERA_STEP, k=1):
    for i in range(3):
        cam.position[i] = float(F(cam.position[i]) + F(k) * F(step[i]))
    return sc.move_camera(cam)


# ---------------- 1. ids and shards ----------------
# (the GPU builder takes scenes of 8 triangles and more: scene 24's single triangle is built on the host only)
CASE_BUILDERS = [(c, b) for c in CASES for b in ("host", "gpu") if not (c == "24" and b == "gpu")]


@pytest.mark.parametrize("case,builder", CASE_BUILDERS)
def test_flow_ids_match_the_id_pass(dev, product, pkg, case, builder):
    """Every case and both builders at 64 x 48, the ragged 50 x 37 and 1 x 1, after a mark and a camera move: the record's id and d_ids
    equal mi355pt_render_ids_device pixel for pixel; a miss is eight zero words; without d_ids the records are the same; the result does not
    depend on spp, seed or sampler; shard 1 of 3 leaves every other pixel's bytes as they were, and the three shards make the unsharded
    buffers; the host-buffer form gives the same records."""
    for w, h in [(W, H), (50, 37), (1, 1)]:
        sc, cam = built(pkg, product, case, builder, w, h)
        product.scene_flow_mark(sc)
        assert move_camera(sc, cam)["rebuilt"] == 0 and product.scene_flow_marked(sc)
        want, _ = dev.render_ids(sc, cam, pkg.make_params(1))
        rec, ids, _ = dev.render_flow(sc, cam, pkg.make_params(1))
        bad = int((rec["id"] != want).sum() + (ids != want).sum())
        log_line({"test": "flow_ids", "case": case, "builder": builder, "size": [w, h], "hit": int((want > 0).sum()), "mismatching": bad})
        assert bad == 0 and not rec["pad"].any()
        assert not raw(rec[want == 0]).any()
        if (w, h) == (W, H):
            assert (want > 0).sum() > 50 and np.abs(rec["d"][want > 0]).max() > 0.01       # the camera's share is in d
        alone, none, _ = dev.render_flow(sc, cam, pkg.make_params(1), want_ids=False)
        other, _, _ = dev.render_flow(sc, cam, pkg.make_params(7, "nee", "random", seed=12345))
        assert none is None and np.array_equal(raw(alone), raw(rec)) and np.array_equal(raw(other), raw(rec))
        if (w, h) == (1, 1):
            continue
        one, one_ids, buf = dev.render_flow(sc, cam, pkg.make_params(1, shard_index=1, shard_count=3))
        tiles = (np.arange(h)[:, None] // 8) * ((w + 7) // 8) + np.arange(w)[None, :] // 8
        mine = tiles % 3 == 1
        assert np.array_equal(raw(one[mine]), raw(rec[mine])) and (raw(one[~mine]) == 0xffffffff).all()
        assert np.array_equal(one_ids[mine], want[mine]) and (one_ids[~mine] == 0xffffffff).all()
        for k in (0, 2):
            full, full_ids, _ = dev.render_flow(sc, cam, pkg.make_params(1, shard_index=k, shard_count=3), into=buf)
        assert np.array_equal(raw(full), raw(rec)) and np.array_equal(full_ids, want)
    hostf, host_ids = product.render_flow(sc, cam, pkg.make_params(1))                  # the host-buffer form, at the last size
    assert np.array_equal(raw(hostf), raw(rec)) and np.array_equal(host_ids, want)


# ---------------- 2. records after every kind of move ----------------
def check_records(dev, product, pkg, reference, sc, cam, case, builder, tag, marked_tris, replace, matrices):
    """the debug pass after a move: records bit-equal to the restatement fed the kernel's own hits, the mark's array unchanged by the move,
    the hits the oracle's, Xc near the oracle's position -> the figures"""
    flow, ids, hits = product.render_flow_debug(sc, cam, pkg.make_params(1))
    assert product.scene_flow_marked(sc)
    _, tris_cur, _ = product.export_bvh(sc)
    tris_prev = product.scene_export_flow_mark(sc)
    assert np.array_equal(raw(tris_prev), raw(marked_tris))                              # the moves left the mark alone
    want = fr.records_from_hits(hits, ids, tris_cur, tris_prev)
    bad = int((raw(flow) != raw(want)).sum())
    plain, plain_ids, _ = dev.render_flow(sc, cam, pkg.make_params(1))
    assert np.array_equal(raw(plain), raw(flow)) and np.array_equal(plain_ids, ids)      # the production kernel writes the debug twin's records
    assert np.array_equal(ids, dev.render_ids(sc, cam, pkg.make_params(1))[0])
    assert not raw(hits[ids == 0]).any()
    # the oracle's scene of the moved state, described from the start
    osc, ocam = describe(pkg, reference, case, replace=replace, matrices=matrices)
    for i in range(3):
        ocam.position[i] = cam.position[i]
    osc.build(ocam)
    o_ids, o_tri, o_pos = reference.render_flow_hits(osc, ocam, pkg.make_params(1))
    tri_ids = product.scene_export_triangle_ids(sc)[hits["tri"]]
    hit = ids != 0
    wrong = int((o_ids != ids).sum() + ((tri_ids[..., 0] + 1 != o_ids) & hit).sum() + ((tri_ids[..., 1] != o_tri) & hit).sum())
    Pc = fr.positions(tris_cur)
    xc = fr.interpolate(hits["b"], Pc[hits["tri"]])
    scale = float(np.abs(Pc).max())
    xc_rel = float(np.abs(xc.astype(np.float64) - o_pos.astype(np.float64))[hit].max() / scale) if hit.any() else 0.0
    moved = int((np.abs(flow["d"]).max(axis=-1) > 0).sum())
    log_line({"test": "flow_records", "case": case, "builder": builder, "move": tag, "hit": int(hit.sum()), "moved_pixels": moved,
              "mismatching_words": bad, "hits_differing_from_oracle": wrong, "xc_rel_max": xc_rel, "xc_scale": scale})
    assert bad == 0, (case, builder, tag, bad)
    assert wrong == 0, (case, builder, tag, wrong)
    assert xc_rel <= XC_REL_TOL, (case, builder, tag, xc_rel)
    return flow, ids, moved


@pytest.mark.parametrize("case,builder", CASE_BUILDERS)
def test_records_after_moves(dev, product, pkg, reference, case, builder):
    """Mark, then a camera move / an instance move / a deformation / all three (a fresh mark before each): the flow pass is refused without a
    mark; mark and no move gives all-zero d and dn; the mark survives each in-place move; after each, every record is bit-equal to
    tests/flow_reference.py fed the debug hits, the exported current triangles and the exported mark; the debug hit's (instance, triangle)
    equals the oracle's (primitive, triangle) for a scene described in the moved state, and Xc is within XC_REL_TOL x max|P| of its hit
    position."""
    geom, inst = CASES[case]
    sc, cam = built(pkg, product, case, builder)
    assert not product.scene_flow_marked(sc)
    with pytest.raises(RuntimeError, match="code -1.*no mark"):
        product.render_flow(sc, cam, pkg.make_params(1))
    with pytest.raises(RuntimeError, match="code -1.*no mark"):
        product.scene_export_flow_mark(sc)
    product.scene_flow_mark(sc)
    assert product.scene_flow_marked(sc)
    still, still_ids, _ = dev.render_flow(sc, cam, pkg.make_params(1))
    assert not raw(still["d"]).any() and not raw(still["dn"]).any() and (still_ids > 0).sum() > 50     # +0 exactly: the arrays are bytewise equal
    assert np.array_equal(still_ids, dev.render_ids(sc, cam, pkg.make_params(1))[0])
    home = sc.instances[inst][2].copy() if inst is not None else None
    replace, matrices, seen = None, None, {}

    def mark():
        product.scene_flow_mark(sc)
        return product.export_bvh(sc)[1]

    marked = mark()
    assert move_camera(sc, cam)["rebuilt"] == 0
    seen["camera"] = check_records(dev, product, pkg, reference, sc, cam, case, builder, "camera", marked, replace, matrices)[2]
    if inst is not None:
        marked = mark()
        matrices = {inst: applied(trs((0.12, 0.0, 0.06), 0.05, (1.0, 1.0, 1.0)), home)}
        assert sc.move_instances(cam, [inst], [matrices[inst]])["rebuilt"] == 0
        seen["instance"] = check_records(dev, product, pkg, reference, sc, cam, case, builder, "instance", marked, replace, matrices)[2]
    marked = mark()
    replace = {geom: deformed(sc.meshes[geom])}
    assert sc.deform_meshes(cam, replace)["rebuilt"] == 0
    flow, ids, seen["deform"] = check_records(dev, product, pkg, reference, sc, cam, case, builder, "deform", marked, replace, matrices)
    if case != "24":
        assert np.abs(flow["dn"]).max() > 1e-4                                           # a deformation turns facets
    marked = mark()
    assert move_camera(sc, cam, k=1)["rebuilt"] == 0
    if inst is not None:
        matrices = {inst: applied(trs((-0.05, 0.03, 0.1), -0.08, (1.0, 1.0, 1.0)), matrices[inst])}
        assert sc.move_instances(cam, [inst], [matrices[inst]])["rebuilt"] == 0
    replace = {geom: deformed(sc.meshes[geom], seed=4, amp=0.02)}
    assert sc.deform_meshes(cam, replace)["rebuilt"] == 0
    seen["all"] = check_records(dev, product, pkg, reference, sc, cam, case, builder, "all", marked, replace, matrices)[2]
    assert all(v > 0 for v in seen.values()), seen


# ---------------- 3. what drops the mark ----------------
def test_mark_is_dropped_by_builds_and_fallbacks(dev, product, pkg):
    """mi355pt_scene_build drops the mark, and so does each move that fell back to a build: a deformation that changes the degenerate set, a
    deformation and an instance move above rebuild_above.  After a drop the flow pass is refused until the next mark, which serves the
    new tree."""
    prm = pkg.make_params(1)
    sc, cam = built(pkg, product, "17", "host")
    product.scene_flow_mark(sc)
    sc.build(cam)
    assert not product.scene_flow_marked(sc)
    with pytest.raises(RuntimeError, match="code -1.*no mark"):
        product.render_flow(sc, cam, prm)
    # rebuild_above, through a deformation and through an instance move
    product.scene_flow_mark(sc)
    pos, nrm, tan = arrays_of(sc.meshes[0])
    ext = float((pos.max(axis=0) - pos.min(axis=0)).max())
    scattered = ((pos + np.random.default_rng(3).uniform(-0.3 * ext, 0.3 * ext, pos.shape)).astype(F), nrm, tan)
    res = sc.deform_meshes(cam, {0: scattered}, rebuild_above=1.0 + 1e-6)
    assert res["rebuilt"] == 1 and res["reason"] == "sah_degraded" and not product.scene_flow_marked(sc)
    sc2, cam2 = built(pkg, product, "17", "host")
    product.scene_flow_mark(sc2)
    far = applied(trs(DEGRADING_STEP, 0.0, (1.0, 1.0, 1.0)), sc2.instances[0][2])      # (tests/test_instance_move.py: the pose whose refit costs more than the build)
    res = sc2.move_instances(cam2, [0], [far], rebuild_above=1.0)
    log_line({"test": "flow_mark_dropped", "by": "instance_move_rebuild_above", "rebuilt": int(res["rebuilt"]), "reason": res["reason"]})
    assert res["rebuilt"] == 1 and not product.scene_flow_marked(sc2)
    # the degenerate set
    sc3, cam3 = describe(pkg, product, "soup1025", builder="host")
    sc3.build(cam3)
    product.scene_flow_mark(sc3)
    p3, n3, t3 = arrays_of(sc3.meshes[0])
    idx = np.asarray(sc3.meshes[0]["idx"], np.uint32).reshape(-1, 3)
    flat = p3.copy(); flat[idx[17]] = flat[idx[17, 0]]
    res = sc3.deform_meshes(cam3, {0: (flat, n3, t3)})
    assert res["rebuilt"] == 1 and res["reason"] == "degenerate_set_changed" and not product.scene_flow_marked(sc3)
    product.scene_flow_mark(sc3)                                                         # ... and the next mark serves the new tree
    rec, ids, _ = dev.render_flow(sc3, cam3, prm)
    assert product.scene_flow_marked(sc3) and not raw(rec["d"]).any()
    # the refusals that need a device: a scene built over several devices is not marked; another current device; with real buffers, a
    # misaligned record buffer and the record buffer given as the id buffer too, both leaving the buffers as they were
    torch = dev.torch
    if torch.cuda.device_count() >= 2:
        with torch.cuda.device(1):
            with pytest.raises(RuntimeError, match="code -2.*current HIP device"):
                product.scene_flow_mark(sc3)
    s4, cam4 = describe(pkg, product, "3")
    product.build_multi(s4, cam4, [0, 0])
    with pytest.raises(RuntimeError, match="code -1.*mi355pt_scene_build_multi"):
        product.scene_flow_mark(s4)
    assert not product.scene_flow_marked(s4)
    buf = torch.full((cam3.height * cam3.width * 8 + 4,), -1, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="code -1.*16-byte aligned"):
        product.render_flow_device(sc3, cam3, prm, buf.data_ptr() + 4)
    with pytest.raises(RuntimeError, match="code -1.*must not be the id buffer"):
        product.render_flow_device(sc3, cam3, prm, buf.data_ptr(), buf.data_ptr())
    torch.cuda.synchronize()
    assert bool((buf == -1).all())
    log_line({"test": "flow_mark_dropped", "by": ["scene_build", "deform_rebuild_above", "instance_move_rebuild_above", "degenerate_set_changed"], "ok": True})


# ---------------- 4. the accumulations against the restatement ----------------
def synthetic_case(w, h, view, half, big):
    cur, prev, vw, spp = tr.synthetic(w, h, view, "step", half)
    flow = fr.synthetic_flow(w, h, vw, big=big)
    ids_cur = flow["id"].copy()
    ids_prev = np.roll(ids_cur, 2, axis=1)
    flip = np.random.default_rng([5, w, h]).random((h, w)) < 0.05
    ids_prev[flip] += 1
    return cur, prev, vw, spp, ids_cur, ids_prev, flow


@pytest.mark.parametrize("half", [True, False], ids=["half", "nohalf"])
@pytest.mark.parametrize("shape", [(64, 48), (70, 50), (1, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_flow_synthetic_parity(dev, shape, half):
    """Seeded synthetic frames (tests/temporal_reference.py synthetic) with synthetic records — three vertical bands: the view's delta alone,
    a shift with a dn, and displacements of 40 and 60 units that throw the taps out of the frame and behind the previous camera — with and
    without the half film, with and without the previous frame's ids, the plain and the rectified kernels, through the static view, a
    camera move, and the views with part of the frame outside the history and behind the previous camera: every output value is bit-equal
    to tests/flow_reference.py."""
    w, h = shape
    for view in ("static", "move", "outside", "behind"):
        cur, prev, vw, spp, ids_cur, ids_prev, flow = synthetic_case(w, h, view, half, big=True)
        dc, dp, di, dq, df = dev.up(cur), dev.up(prev), dev.ids_up(ids_cur), dev.ids_up(ids_prev), dev.flow_up(flow)
        for with_ids in (False, True):
            ic, ip, dic, dip = (ids_cur, ids_prev, di, dq) if with_ids else (None, None, None, None)
            tag = f"{w}x{h}_{'half' if half else 'nohalf'}_{view}_{'ids' if with_ids else 'noids'}"
            got = [x.cpu().numpy() if x is not None else None for x in dev.run_flow_device(dc, spp, dp, vw, dic, dip, df)]
            want = fr.accumulate_flow(cur, spp, prev, vw, ic, ip, flow, detail=True)
            assert_bit_equal(got, want[:3], "flow_synthetic_" + tag)
            got = [x.cpu().numpy() if x is not None else None for x in dev.run_flow_device(dc, spp, dp, vw, dic, dip, df, rectified=True)]
            assert_bit_equal(got, fr.accumulate_rectified_flow(cur, spp, prev, vw, ic, ip, flow), "flow_rectified_synthetic_" + tag)
        if (w, h) != (1, 1) and view == "move":
            band = (3 * np.arange(w)[None, :] // w + np.zeros((h, 1), np.int64)) == 2
            info = fr.accumulate_flow(cur, spp, prev, vw, None, None, flow, detail=True)[3]
            assert not info["ok"][band].all() and info["has"][~band].any()              # the big displacements did leave the frame / the front
            assert not np.array_equal(bits(got[0]), bits(tr.accumulate(cur, spp, prev, vw)[0]))


@pytest.mark.parametrize("half", [True, False], ids=["half", "nohalf"])
def test_zero_records_equal_the_existing_call(dev, half):
    """The same device buffers, all-zero records, no ids: all three outputs of the flow-aware call are bit-equal to
    mi355pt_temporal_accumulate_device's at delta = 0 — whatever delta the view given to the flow call holds, which it does not read —,
    and the rectified pair likewise, through every view."""
    w, h = 70, 50
    for view in ("static", "move", "outside", "behind"):
        cur, prev, vw, spp = tr.synthetic(w, h, view, "step", half)
        dc, dp, df = dev.up(cur), dev.up(prev), dev.flow_up(fr.zero_records(w, h))
        for rectified in (False, True):
            got = dev.run_flow_device(dc, spp, dp, vw, None, None, df, rectified=rectified)
            want = dev.run_device(dc, spp, dp, fr.zero_delta(vw), rectified=rectified)
            for name, a, b in zip(("film", "half", "length"), got, want):
                assert (a is None) == (b is None)
                if a is not None:
                    a, b = a.cpu().numpy(), b.cpu().numpy()
                    assert not np.isnan(a).any() and np.array_equal(bits(a), bits(b)), (view, rectified, name, int((bits(a) != bits(b)).sum()))
        log_line({"test": "flow_zero_records_equal_existing", "view": view, "half": half, "mismatching": 0})


def test_flow_is_deterministic_and_host_forms_match(dev, product, pkg):
    """Two calls are bit-equal; the host-buffer forms equal the device forms — plain and rectified, with and without a half film, previous
    ids and a previous frame; the flow pass twice gives the same bytes."""
    w, h = 70, 50
    for half in (True, False):
        cur, prev, vw, spp, ids_cur, ids_prev, flow = synthetic_case(w, h, "move", half, big=True)
        for p, v, ic, ip in ((prev, vw, ids_cur, ids_prev), (prev, vw, None, None), (None, None, ids_cur, None)):
            for rectified in (False, True):
                one = dev.run_flow(cur, spp, p, v, ic, ip, flow, rectified=rectified)
                two = dev.run_flow(cur, spp, p, v, ic, ip, flow, rectified=rectified)
                hostf = product.temporal_accumulate_flow(cur, spp, p, ffi_view(pkg, v), ic, ip, flow,
                                                         rectify_params=product.temporal_rectify_params_default() if rectified else None)
                for a, b, c in zip(one, two, hostf):
                    assert (a is None) == (b is None) == (c is None)
                    if a is not None:
                        assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a), bits(c))
    sc, cam = built(pkg, product, "17", "host")
    product.scene_flow_mark(sc)
    assert sc.deform_meshes(cam, {0: deformed(sc.meshes[0])})["rebuilt"] == 0
    a, ia, _ = dev.render_flow(sc, cam, pkg.make_params(1))
    b, ib, _ = dev.render_flow(sc, cam, pkg.make_params(1))
    assert np.array_equal(raw(a), raw(b)) and np.array_equal(ia, ib)


# ---------------- 5. rendered frames ----------------
HERO = 0


class HeroScene:
    """scene 17 at W x H with its hero dynamic, built once; the hero's mesh as described is kept for the wave"""

    def __init__(self, product, pkg):
        self.product, self.pkg = product, pkg
        self.sc, self.cam = describe(pkg, product, "17")
        self.d65 = self.sc.add_lut470(pkg.scenes.presets()["cie_illum_d6500"])
        self.sc.set_instance_dynamic(HERO)
        self.sc.build(self.cam)
        self.home = self.sc.instances[HERO][2].copy()
        self.mesh = self.sc.meshes[HERO]
        self.pos0, self.nrm0, _ = arrays_of(self.mesh)
        self.idx = np.asarray(self.mesh["idx"], np.uint32).reshape(-1, 3)


def waved(pos, amp, wavelength, phase):
    """host/main.cpp waved_positions: y += amp sin(2 pi x / wavelength + phase) in double (libm's sin), rounded to float32"""
    out = np.array(pos, F)
    a, lam = float(F(amp)), float(F(wavelength))
    for v in range(out.shape[0]):
        out[v, 1] = F(float(pos[v, 1]) + a * math.sin(2.0 * 3.14159265358979323846 * float(pos[v, 0]) / lam + phase))
    return out


def area_normals(pos, idx, old):
    """host/renderer.hpp area_weighted_normals: float32 edges and cross products, summed per vertex in double in index order"""
    p = np.asarray(pos, F)
    a, b = p[idx[:, 1]] - p[idx[:, 0]], p[idx[:, 2]] - p[idx[:, 0]]
    n = np.stack([a[:, 1] * b[:, 2] - b[:, 1] * a[:, 2], a[:, 2] * b[:, 0] - b[:, 2] * a[:, 0], a[:, 0] * b[:, 1] - b[:, 0] * a[:, 1]], -1).astype(F)
    acc = np.zeros(p.shape, np.float64)
    np.add.at(acc, idx.reshape(-1), np.repeat(n.astype(np.float64), 3, axis=0))
    ln = np.sqrt(acc[:, 0] * acc[:, 0] + acc[:, 1] * acc[:, 1] + acc[:, 2] * acc[:, 2])
    out = np.array(old, F)
    ok = ln > 0.0
    out[ok] = (acc[ok] / ln[ok, None]).astype(F)
    return out


def render_frame(dev, hs, sc, cam, seed, spp=FRAME_SPP):
    """one frame's device films (G-buffer sums at GUIDE_SPP, the film; no half film)"""
    torch, product, pkg = dev.torch, hs.product, hs.pkg
    f = {k: torch.zeros((H, W, 3), dtype=torch.float32, device="cuda") for k in ("film", "position", "shading_normal", "hit")}
    g = {k: f[k].data_ptr() for k in ("shading_normal", "position", "hit")}
    product.render_gbuffer_accum_device(sc, cam, pkg.make_params(GUIDE_SPP, "mis", "sobol", seed=seed), hs.d65, 0, GUIDE_SPP, g)
    product.render_accum_device(sc, cam, pkg.make_params(spp, "mis", "sobol", seed=seed), 0, spp, f["film"].data_ptr())
    torch.cuda.synchronize()
    return f


def host(f):
    return {k: v.cpu().numpy() for k, v in f.items()}


def uniform3(ids):
    h, w = ids.shape
    ok = np.zeros((h, w), bool)
    c = ids[1:-1, 1:-1]
    same = np.ones(c.shape, bool)
    for dy in range(3):
        for dx in range(3):
            same &= ids[dy:dy + h - 2, dx:dx + w - 2] == c
    ok[1:-1, 1:-1] = same
    return ok


def test_against_the_rigid_twin(dev, product, pkg):
    """Scene 17, the hero translated between two frames: the pixels with history under the flow call are those under the motion-table call
    on the hero's interior (id uniform over 3 x 3), and the films agree there within a tolerance measured here: the table form computes
    a X + b with a = I (exact) and b = the translation rounded once to f32; the flow form interpolates both triangles and subtracts, an
    error of 13 x 2^-24 x max|P| in d (tests/test_flow.py) — about 1e-5 of a scene of 10 units, 1e-4 of a pixel footprint, which moves the
    bilinear weights by as much: the films (values up to a few units) are held to 1e-3 absolute, ten times that."""
    hs = HeroScene(product, pkg)
    sc, cam = hs.sc, hs.cam
    f0 = render_frame(dev, hs, sc, cam, 0)
    ids0, t0 = dev.render_ids(sc, cam, pkg.make_params(1))
    product.scene_flow_mark(sc)
    m1 = applied(trs((0.12, 0.0, 0.06), 0.0, (1.0, 1.0, 1.0)), hs.home)
    assert sc.move_instances(cam, [HERO], [m1])["rebuilt"] == 0
    f1 = render_frame(dev, hs, sc, cam, 1)
    flow, ids1, (tf, ti) = dev.render_flow(sc, cam, pkg.make_params(1))
    view = product.temporal_view_from_cameras(cam, cam)
    now = [m.copy() for _, _, m in sc.instances]; before = [m.copy() for m in now]
    now[HERO], before[HERO] = m1, hs.home
    table = dev.torch.from_numpy(product.motion_table(cam, cam, now, before)).cuda()
    a0 = dev.run_device(f0, FRAME_SPP, None, None, rectified=False)
    prev = dict({k: f0[k] for k in ("position", "shading_normal", "hit")}, film=a0[0], length=a0[2])
    got_f = dev.run_flow_device(f1, FRAME_SPP, prev, view, ti, t0, tf)
    of, oh, ol = dev.outputs(W, H, False)
    ptr = lambda d: {k: v.data_ptr() for k, v in d.items()}   # noqa: E731
    product.temporal_accumulate_motion_device(ptr(f1), FRAME_SPP, ptr(prev), view, W, H, product.temporal_params_default(), ti.data_ptr(), t0.data_ptr(),
                                              table.data_ptr(), table.shape[0], of.data_ptr(), None, ol.data_ptr())
    dev.torch.cuda.synchronize()
    film_f, len_f, film_m, len_m = got_f[0].cpu().numpy(), got_f[2].cpu().numpy(), of.cpu().numpy(), ol.cpu().numpy()
    interior = uniform3(ids1) & (ids1 == HERO + 1)
    has_f, has_m = len_f > 1.0, len_m > 1.0
    differ = int((has_f != has_m)[interior].sum())
    both = interior & has_f & has_m
    dmax = float(np.abs(film_f - film_m)[both].max())
    log_line({"test": "flow_vs_motion_table", "hero_interior": int(interior.sum()), "with_history_flow": int(has_f[interior].sum()),
              "with_history_table": int(has_m[interior].sum()), "history_differs": differ, "film_max_abs_diff": dmax, "tolerance": 1e-3})
    assert interior.sum() > 100 and has_m[interior].mean() > 0.8
    assert differ == 0 and dmax <= 1e-3, (differ, dmax)


# amplitude and wavelength as shares of the hero mesh's extent along its local x, phase step per frame.  Sized so that a vertex moves by up to
# 0.08 x 0.96 x 2.5 (the hero's scale) x 2 sin(0.75) = 0.26 world units per frame, four times what the plane test allows at the hero's
# distance (pos_tol 0.01 x t, t = 6.5): the static-world call then loses the history wherever the surface faces the motion
WAVE = (0.08, 2.0, 1.5)


def test_what_it_buys_on_a_waving_mesh(dev, product, pkg):
    """Scene 17 at 64 x 48, the hero under the CLI's wave with an advancing phase, 8 frames of 4 spp, flow-aware accumulation with the
    previous ids against the static-world call on the same frames.
      history   the share of hero interior pixels (id uniform over 3 x 3) with history in the last frame exceeds the static-world call's;
      geometry  frames of temporal_reference.geometry_frames for the last pair: the previous film holds world positions, for the hero's
                pixels carried to the current pose by the ANALYTIC wave (local y + a sin(k x + phase_cur) - a sin(k x + phase_prev), through
                the hero's matrix), so a correct reprojection gathers the current pixel's own world position; over the hero's interior the
                distance is held to the bars camera moves have: median <= 0.1 pixel footprints, >= 0.97 under 0.25;
      noise     the hero's RMSE against a 256-spp frame of the last pose is below the last frame's alone."""
    torch = dev.torch
    hs = HeroScene(product, pkg)
    sc, cam = hs.sc, hs.cam
    ext = float(np.ptp(hs.pos0[:, 0]))
    amp, lam, step = float(F(WAVE[0] * ext)), float(F(WAVE[1] * ext)), WAVE[2]
    view = product.temporal_view_from_cameras(cam, cam)
    acc = {"flow": None, "static": None}
    prev_f = prev_ids = None
    frames = 8
    for k in range(frames):
        if k > 0:
            product.scene_flow_mark(sc)
        pos = waved(hs.pos0, amp, lam, k * float(F(step)))
        assert sc.deform_meshes(cam, {HERO: (pos, area_normals(pos, hs.idx, hs.nrm0), None)})["rebuilt"] == 0
        f = render_frame(dev, hs, sc, cam, k)
        if k > 0:
            flow, ids, (tf, ti) = dev.render_flow(sc, cam, pkg.make_params(1))
        else:
            ids, ti = dev.render_ids(sc, cam, pkg.make_params(1))
        for name in acc:
            if prev_f is None:
                out = dev.run_device(f, FRAME_SPP, None, None, rectified=False)
            else:
                prev = dict({g: prev_f[g] for g in ("position", "shading_normal", "hit")}, film=acc[name][0], length=acc[name][2])
                out = dev.run_flow_device(f, FRAME_SPP, prev, view, ti, prev_ids, tf) if name == "flow" else dev.run_device(f, FRAME_SPP, prev, view, rectified=False)
            acc[name] = out
        last_prev_f, last_prev_ids = prev_f, (prev_ids.cpu().numpy().view(np.uint32) if prev_ids is not None else None)
        prev_f, prev_ids = f, ti
    i_last = ids
    interior = uniform3(i_last) & (i_last == HERO + 1)
    share_flow = float((acc["flow"][2].cpu().numpy() > 1.0)[interior].mean())
    share_static = float((acc["static"][2].cpu().numpy() > 1.0)[interior].mean())

    # geometry: the last pair
    geo = ("position", "shading_normal", "hit")
    h1, h0 = host(prev_f), host(last_prev_f)
    cur_g, prev_g, prm = tr.geometry_frames({k: h1[k] for k in geo}, {k: h0[k] for k in geo}, cam, cam, GUIDE_SPP)
    M = hs.home.astype(np.float64)
    Minv = np.linalg.inv(M)
    world_prev = prev_g["film"].astype(np.float64)
    local = world_prev @ Minv[:3, :3].T + Minv[:3, 3]
    kx = 2.0 * math.pi * local[..., 0] / float(F(lam))
    ph1, ph0 = (frames - 1) * float(F(step)), (frames - 2) * float(F(step))
    # the wave displaces y by a function of the ORIGINAL x, which the wave leaves alone: the same vertex is at y0 + a sin(kx + phase)
    local[..., 1] += float(F(amp)) * (np.sin(kx + ph1) - np.sin(kx + ph0))
    carried = (local @ M[:3, :3].T + M[:3, 3]).astype(F)
    prev_g["film"] = np.where((last_prev_ids == HERO + 1)[..., None], carried, prev_g["film"]).astype(F)
    out_g = dev.run_flow(cur_g, GUIDE_SPP, prev_g, view, i_last, last_prev_ids, flow, prm)
    want_g = fr.accumulate_flow(cur_g, GUIDE_SPP, prev_g, view, i_last, last_prev_ids, flow, prm, detail=True)
    assert_bit_equal(out_g, want_g[:3], "flow_wave_geometry")
    info = want_g[3]
    inner = interior & (h1["hit"][..., 1] == GUIDE_SPP) & info["has"]
    full_prev = uniform3(last_prev_ids) & (last_prev_ids == HERO + 1) & (h0["hit"][..., 1] == GUIDE_SPP)
    for k in range(4):
        qx, qy = np.clip(info["x0"] + (k & 1), 0, W - 1), np.clip(info["y0"] + (k >> 1), 0, H - 1)
        inner &= info["valid"][k] & full_prev[qy, qx]
    X = cur_g["position"].astype(np.float64) / GUIDE_SPP + np.array(list(cam.position), np.float64)
    t = cur_g["hit"][..., 0].astype(np.float64) / GUIDE_SPP
    foot = t * 2.0 * math.tan(math.radians(cam.fov_deg) / 2.0) / H
    with np.errstate(all="ignore"):
        dist = (np.linalg.norm(np.asarray(out_g[0], np.float64) - X, axis=-1) / foot)[inner]
    median, under = float(np.median(dist)), float((dist < 0.25).mean())

    ref = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    product.render_accum_device(sc, cam, pkg.make_params(256, "mis", "sobol", seed=1000), 0, 256, ref.data_ptr())
    torch.cuda.synchronize()
    ref = ref.cpu().numpy().astype(np.float64) / 256.0
    rmse = lambda a: float(np.sqrt(np.mean((a[interior] - ref[interior]) ** 2)))   # noqa: E731
    e_last = rmse(prev_f["film"].cpu().numpy().astype(np.float64) / FRAME_SPP)
    e_flow, e_static = rmse(acc["flow"][0].cpu().numpy().astype(np.float64)), rmse(acc["static"][0].cpu().numpy().astype(np.float64))
    log_line({"test": "flow_wave", "frames": frames, "spp": FRAME_SPP, "wave": list(WAVE), "hero_interior": int(interior.sum()), "geometry_interior": int(inner.sum()),
              "history_share_flow": share_flow, "history_share_static": share_static, "median_footprints": median, "share_under_quarter": under,
              "rmse_last_frame": e_last, "rmse_flow": e_flow, "rmse_static_world": e_static,
              "mean_history_length_flow": float(acc["flow"][2].cpu().numpy()[interior].mean())})
    bars = tr.GEOMETRY_BARS
    assert interior.sum() > 100 and inner.sum() > 50
    assert share_flow > share_static, (share_flow, share_static)
    assert median <= bars["median"] and under >= bars["share_under_quarter"], (median, under)
    assert e_flow < e_last, (e_flow, e_last)


# ---------------- 6. the CLI ----------------
from test_instance_move_gpu import cli, cli_matrix  # noqa: E402,F401  (the CLI fixture and host/main.cpp's matrix, shared)

CLI_STEP = (1, (0.1, 0.0, 0.05), 10.0)        # scene 3's box: translation and ry_deg per frame
CLI_WAVE = (0, 0.05, 0.7, 0.4)                # scene 3's hero: amp, wavelength, phase step
CLI_CAMERA = (0.1, 0.0, 0.0)


def replay(product, pkg, dev, frames, rprm):
    """the calls of `mi355pt --scene 3 --temporal-frames N --flow --camera-step --instance-step --mesh-wave` (no half film) through the ABI -> u8"""
    torch = dev.torch
    sc = Remeshed(product).new_scene()
    cam = pkg.scenes.load_scene(sc, 3, W, H, build=False)
    d65 = sc.add_lut470(pkg.scenes.presets()["cie_illum_d6500"])
    inst, t, ry = CLI_STEP
    geom, amp, lam, step = CLI_WAVE
    sc.set_instance_dynamic(inst)
    sc.build(cam)
    base = np.array(list(cam.position), F)
    now = sc.instances[inst][2].copy()
    pos0, nrm0, _ = arrays_of(sc.meshes[geom])
    idx = np.asarray(sc.meshes[geom]["idx"], np.uint32).reshape(-1, 3)
    nrm_now = nrm0
    acc = g = prev_cam = prev_ids = None
    for k in range(frames):
        if k > 0:
            product.scene_flow_mark(sc)
            p = base + F(k) * np.asarray(CLI_CAMERA, F)
            for i in range(3):
                cam.position[i] = p[i]
            assert sc.move_camera(cam)["rebuilt"] == 0
            now = cli_matrix(t, ry, (1.0, 1.0, 1.0), now)
            assert sc.move_instances(cam, [inst], [now])["rebuilt"] == 0
        pos = waved(pos0, amp, lam, float(k) * float(F(step)))
        nrm_now = area_normals(pos, idx, nrm_now)
        assert sc.deform_meshes(cam, {geom: (pos, nrm_now, None)})["rebuilt"] == 0
        assert k == 0 or product.scene_flow_marked(sc)
        f = {n: torch.zeros((H, W, 3), dtype=torch.float32, device="cuda") for n in ("film", "position", "shading_normal", "hit")}
        gb = {n: f[n].data_ptr() for n in ("shading_normal", "position", "hit")}
        product.render_gbuffer_accum_device(sc, cam, pkg.make_params(GUIDE_SPP, "mis", "sobol", seed=k), d65, 0, GUIDE_SPP, gb)
        product.render_accum_device(sc, cam, pkg.make_params(FRAME_SPP, "mis", "sobol", seed=k), 0, FRAME_SPP, f["film"].data_ptr())
        prev = view = None
        if k == 0:
            _, ti = dev.render_ids(sc, cam, pkg.make_params(1))
            tf = torch.zeros((H, W, 8), dtype=torch.int32, device="cuda")
        else:
            _, _, (tf, ti) = dev.render_flow(sc, cam, pkg.make_params(1))
            prev = dict({n: g[n] for n in ("position", "shading_normal", "hit")}, film=acc[0], length=acc[2])
            view = product.temporal_view_from_cameras(cam, prev_cam)
        acc = dev.run_flow_device(f, FRAME_SPP, prev, view, ti, prev_ids if prev is not None else None, tf, None, rprm, rectified=rprm is not None)
        g, prev_cam, prev_ids = f, pkg.ffi.Camera.from_buffer_copy(cam), ti
    rgb = torch.empty_like(acc[0])
    product.film_resolve_device(acc[0].data_ptr(), W * H, 1, rgb.data_ptr())
    torch.cuda.synchronize()
    return product.quantize_u8(rgb.cpu().numpy())


def test_flow_cli(product, pkg, dev, cli, tmp_path):
    """`--temporal-frames 3 --flow` with a --camera-step, an --instance-step and a --mesh-wave at 64 x 48 — plain and with
    --temporal-rectify — writes the picture of the same calls replayed through the ABI, u8-equal, with one line per move and frame on stderr
    and none about a restart; with --instance-rebuild-above 1e-6 every frame's deformation rebuilds and the accumulation restarts, one line
    each; --flow without --temporal-frames and with --half-res exit 2 naming the flag; without --flow every old refusal stays."""
    from PIL import Image
    exe, env = cli
    base = [exe, "--scene", "3", "--renderer", "mis", "--sampler", "sobol", "--spp", str(FRAME_SPP), "--width", str(W), "--height", str(H),
            "--denoise-guide-spp", str(GUIDE_SPP)]
    inst, t, ry = CLI_STEP
    moves = ["--camera-step", "%g,%g,%g" % CLI_CAMERA, "--instance-step", "%d:%g,%g,%g:%g" % ((inst,) + t + (ry,)), "--mesh-wave", "%d:%g,%g,%g" % CLI_WAVE]

    def picture(extra, name):
        path = str(tmp_path / name)
        r = subprocess.run(base + ["--temporal-frames", "3"] + extra + ["-o", path], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        return np.asarray(Image.open(path).convert("RGB")), r.stderr
    still, _ = picture(["--flow"], "still.png")
    for name, extra, rprm in (("plain", [], None), ("rectified", ["--temporal-rectify"], rr.params())):
        got, err = picture(["--flow"] + moves + extra, name + ".png")
        lines = err.splitlines()
        assert sum(ln.startswith("mesh deform, frame ") and "rebuilt=0" in ln for ln in lines) == 3, err
        assert sum(ln.startswith("instance step, frame ") and "rebuilt=0" in ln for ln in lines) == 2, err
        assert sum(ln.startswith("camera move, frame ") and "rebuilt=0" in ln for ln in lines) == 2, err
        assert not any(ln.startswith("flow, frame ") for ln in lines), err
        want = replay(product, pkg, dev, 3, rprm)
        log_line({"test": "flow_cli", "run": name, "differing_u8": int((got != want).sum()), "differs_from_still": int((got != still).sum())})
        assert got.shape == want.shape and np.array_equal(got, want), (name, int((got != want).sum()))
        assert got.mean() > 10.0 and not np.array_equal(got, still)
    _, err = picture(["--flow", "--mesh-wave", "%d:%g,%g,%g" % CLI_WAVE, "--instance-rebuild-above", "1e-6"], "restart.png")
    assert sum(ln.startswith("flow, frame ") and "restarts" in ln for ln in err.splitlines()) == 2, err
    t3 = ["--temporal-frames", "3"]
    for args, flag in ((["--flow"], "--flow"), (t3 + ["--flow", "--half-res", "--denoise-variance"], "--flow"),
                       (t3 + ["--mesh-wave", "0:0.05,0.7"], "--temporal-frames"), (t3 + ["--instance-transform", "1:0,0,0"], "--temporal-frames"),
                       (t3 + ["--flow", "--instance-transform", "1:0,0,0"], "--temporal-frames"), (["--instance-step", "1:0.1,0,0"], "--instance-step")):
        r = subprocess.run(base + args, env=env, capture_output=True, text=True, timeout=120, cwd=tmp_path)
        assert r.returncode == 2 and flag in r.stderr, (args, r.returncode, r.stderr)
