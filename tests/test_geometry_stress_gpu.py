"""GPU tests on the adversarial geometry of tests/geometry_stress.py: the tree each builder exports against the triangles it was built
from, closest and any hits through both trees and against the oracle, the production cooperative traversal ray by ray (the G-buffer pass
at 1 spp against its CPU restatement) under both builders and all three lowering modes, and the camera candidate lists against the
traversal.  Figures go to the file MI355PT_FRAME_LOG names (profiles/geometry_stress.jsonl)."""
import json
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gbuffer_reference  # noqa: E402
import geometry_stress as gs  # noqa: E402
from test_camera_candidates_gpu import CAP, bits, item_rects  # noqa: E402

pytestmark = pytest.mark.gpu

FILMS = gbuffer_reference.FILMS
W, H = gs.W, gs.H
BUILDERS = ("host", "gpu")
LOWERINGS = ("auto", "no_local_tris", "general")
PER_SAMPLE_MIN = 0.9995          # share within 1e-3 |c| + 1e-4   (tests/test_gbuffer_gpu.py)
TIGHT_MIN = 0.997                # share within 1e-5 max(1, t)
# SAH cost of the GPU builder's tree over the host sweep's, spatial families: 1 + twice the largest excess of the first recorded run
# (profiles/geometry_stress.jsonl, "test": "sah_ratio"), at least 0.10.  32 bins against an exact sweep is the only legitimate excess.
# That run: 0.9909 (slivers64) ... 1.0083 (line64); twice 0.0083 is below the floor, so the floor holds.
SAH_MARGIN = 0.10


def log_line(line):
    print(line)
    if os.environ.get("MI355PT_FRAME_LOG"):
        with open(os.environ["MI355PT_FRAME_LOG"], "a") as f:
            f.write(json.dumps(line) + "\n")


def info_of(product, sc):
    return dict(re.findall(r"(\w+)=(\S+)", product.scene_info(sc)))


@pytest.fixture(scope="module")
def ref():
    return gbuffer_reference.GbufferReference()


@pytest.fixture(scope="module")
def cpu(ref, pkg):
    """family -> the CPU side, made once and left unchanged: the scene (fast walker; equal to the faithful one bit for bit on every family,
    tests/test_geometry_stress.py), its G-buffer films and hit classes at 256 x 192 and 1 spp, and 20 000 camera-like plus 20 000
    incoherent secondary rays from its hit points with its closest hits"""
    cache = {}

    def get(name):
        if name in cache:
            return cache[name]
        fam = gs.family(name)
        sc, cam, d65 = gs.build_scene(ref, name)
        ref.set_faithful(sc, False)
        films, cls = ref.render_gbuffer_accum(sc, cam, pkg.make_params(1, "mis", "sobol"), d65, want_classes=True)
        o, d = gs.camera_like_rays(20000, 1)
        t, inst, tri, n = sc.probe_intersect(o, d)
        ok = t > 0
        rng = np.random.default_rng(5)
        pick = np.nonzero(ok)[0][rng.integers(0, int(ok.sum()), 20000)]
        p = o[pick] + d[pick] * t[pick, None]
        d2 = rng.normal(size=p.shape).astype(np.float32)
        d2 /= np.linalg.norm(d2, axis=1, keepdims=True)
        flip = np.sum(d2 * n[pick], 1) * np.sum(-d[pick] * n[pick], 1) < 0      # keep them on the side the ray came from
        d2[flip] *= -1
        o2 = (p + d2 * np.float32(1e-3 * fam.scale)).astype(np.float32)
        rays_o, rays_d = np.concatenate([o, o2]), np.concatenate([d, d2])
        hits = sc.probe_intersect(rays_o, rays_d)
        cache[name] = dict(scene=sc, films=films, cls=cls, rays=(rays_o, rays_d), hits=hits)
        return cache[name]
    return get


@pytest.fixture(scope="module")
def gpu(product):
    """(family, builder) -> (scene, camera, d65) with the default lowering, built once"""
    cache = {}

    def get(name, builder):
        if (name, builder) not in cache:
            cache[name, builder] = gs.build_scene(product, name, builder=builder)
        return cache[name, builder]
    return get


def exported(product, gpu, name, builder):
    sc = gpu(name, builder)[0]
    nodes, tris, root = product.export_bvh(sc)
    return sc, nodes, tris, root


# ------------------------------------------------------------------------------------------------------------------ builder structure
@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("name", gs.NAMES)
def test_exported_tree_is_a_tree_over_its_triangles(product, gpu, name, builder):
    """The leaves partition the triangles, hold at most 4 each and lie no deeper than 22; every stored child box EQUALS the min / max of the
    vertices below it (the GPU builder's boxes are min / max merges of the input boxes, the host builder's unions of them: neither may
    be larger); the exported triangles are the input triangles; scene_info reports what the tree holds; a second GPU build is the
    same tree byte for byte."""
    fam = gs.family(name)
    sc, nodes, tris, root = exported(product, gpu, name, builder)
    out = gs.validate_bvh(nodes, tris, root, input_tris=fam.render32(), equal_boxes=True)
    info = info_of(product, sc)
    assert info["builder"] == builder
    need, cap = map(int, info["stack_need"].split("/"))
    assert int(info["tris"]) == out["tris"] == fam.n_tris and int(info["depth"]) == out["depth"] and int(info["nodes"]) == out["nodes"] == nodes.shape[0]
    assert need < cap == 24
    again = product.probe_bvh_collapse_nodes(nodes, root, tris.shape[0])
    assert again["max_stack4"] == need and again["nodes4"] == int(info["nodes4"])
    log_line({"test": "structure", "family": name, "builder": builder, **{k: out[k] for k in ("tris", "nodes", "leaves", "depth", "max_leaf")},
              "stack_need": need, "sah": round(out["sah"], 4)})
    if builder == "gpu":
        sc2, _, _ = gs.build_scene(product, name, builder="gpu")
        nodes2, tris2, root2 = product.export_bvh(sc2)
        assert root2 == root and np.array_equal(nodes2, nodes) and np.array_equal(tris2, tris)


@pytest.mark.parametrize("name", gs.NAMES)
def test_sah_cost_of_the_gpu_tree_against_the_host_sweep(product, gpu, name):
    cost = {}
    for builder in BUILDERS:
        _, nodes, tris, root = exported(product, gpu, name, builder)
        cost[builder] = gs.validate_bvh(nodes, tris, root)["sah"]
    ratio = cost["gpu"] / cost["host"]
    log_line({"test": "sah_ratio", "family": name, "host": round(cost["host"], 4), "gpu": round(cost["gpu"], 4), "ratio": round(ratio, 4),
              "asserted": gs.family(name).spatial})
    if gs.family(name).spatial:
        assert ratio <= 1.0 + SAH_MARGIN, ratio


# ------------------------------------------------------------------------------------------------------------------ hits through both trees
@pytest.mark.parametrize("name", gs.NAMES)
def test_hits_through_both_trees_and_the_oracle(product, gpu, cpu, name):
    """20 000 camera-like and 20 000 incoherent secondary rays (from the oracle's hit points) through mi355pt_probe_intersect /
    mi355pt_probe_occluded: the host-built and the GPU-built tree give the same hit / miss answers, bit-equal t on >= 0.9999 of the rays
    and the same any-hit answers; on the tie-free families both find the oracle's triangle on >= 0.9999 of the rays, with t within
    2.5e-7 relative on those."""
    fam = gs.family(name)
    c = cpu(name)
    o, d = c["rays"]
    tc, ic, trc, _ = c["hits"]
    res = {b: gpu(name, b)[0].probe_intersect(o, d) for b in BUILDERS}
    th, tg = res["host"][0], res["gpu"][0]
    rng = np.random.default_rng(7)
    tm = (np.where(th > 0, th, fam.scale) * rng.uniform(0.3, 1.7, th.shape[0])).astype(np.float32)
    occ = {b: gpu(name, b)[0].probe_occluded(o, d, tm) for b in BUILDERS}
    line = {"test": "probe_hits", "family": name, "hit_share": round(float((th > 0).mean()), 4), "t_bit_equal_host_gpu": round(float((th == tg).mean()), 6),
            "occluded_share": round(float(occ["host"].mean()), 4), "occluded_differ": int((occ["host"] != occ["gpu"]).sum())}
    for b in BUILDERS:
        t, inst, tri, _ = res[b]
        both = (t > 0) & (tc > 0) & (inst == ic) & (tri == trc)
        same = both | ((t <= 0) & (tc <= 0))
        rel = np.abs(t[both] - tc[both]) / np.abs(tc[both])
        line[f"{b}_same_triangle_as_oracle"] = round(float(same.mean()), 6)
        line[f"{b}_t_rel_max_vs_oracle"] = float(f"{rel.max():.3e}")
        line[f"{b}_t_bit_equal_oracle"] = round(float((t[both] == tc[both]).mean()), 6)
    log_line(line)
    assert (th > 0).sum() >= 200                                            # (the planar grid's secondary rays leave the plane: nearly all miss)
    assert np.array_equal(th > 0, tg > 0)
    assert (th == tg).mean() >= 0.9999
    assert np.array_equal(occ["host"], occ["gpu"]) and 0 < occ["host"].sum() < occ["host"].size
    if fam.tie_free:
        for b in BUILDERS:
            assert line[f"{b}_same_triangle_as_oracle"] >= 0.9999, b
            assert line[f"{b}_t_rel_max_vs_oracle"] <= 2.5e-7, b


# ------------------------------------------------------------------------------------------------------------------ the production traversal
def gpu_gbuffer(product, pkg, scene):
    import torch
    sc, cam, d65 = scene
    buf = torch.zeros((4, H, W, 3), dtype=torch.float32, device="cuda")
    product.render_gbuffer_accum_device(sc, cam, pkg.make_params(1, "mis", "sobol"), d65, 0, 1, {k: buf[i].data_ptr() for i, k in enumerate(FILMS)})
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    return {k: host[i] for i, k in enumerate(FILMS)}


@pytest.mark.parametrize("lowering", LOWERINGS)
@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("name", gs.NAMES)
def test_cooperative_traversal_ray_by_ray(product, pkg, gpu, cpu, name, builder, lowering):
    """trace_closest_coop over the padded 4-wide tree, one pixel = one camera ray (the G-buffer pass, 256 x 192 at 1 spp, Sobol), against
    tests/gbuffer_reference.cpp exactly as tests/test_gbuffer_gpu.py::test_gbuffer_parity_with_the_cpu_restatement compares them: the NaN
    patterns are equal; where both sides hit the same class shading_normal and hit.yz are bit-equal; position and hit.x meet the two
    per-sample caps over ALL pixels (a pixel whose classes differ counts as left out)."""
    scene = gpu(name, builder) if lowering == "auto" else gs.build_scene(product, name, builder=builder, lowering=lowering)
    local = "tri_space=local" in product.scene_info(scene[0])
    assert not (local and lowering != "auto")
    g = gpu_gbuffer(product, pkg, scene)
    c, cls = cpu(name)["films"], cpu(name)["cls"]
    for k in FILMS:
        assert np.array_equal(np.isnan(g[k]), np.isnan(c[k])), k
    g_class = np.where(g["hit"][..., 1] == 0, 2, np.where(g["hit"][..., 2] == 1, 1, 0))
    c_class = np.argmax(cls, axis=2)
    same = g_class == c_class
    t = c["hit"][..., 0]
    line = {"test": "gbuffer", "family": name, "builder": builder, "lowering": lowering, "tri_space": "local" if local else "render",
            "same_class": round(float(same.mean()), 6), "hit_share": round(float((c_class == 0).mean()), 4),
            "normal_differs": int((g["shading_normal"][same].view(np.uint32) != c["shading_normal"][same].view(np.uint32)).any(axis=-1).sum())}
    shares = {}
    for film, gv, cv in (("position", g["position"], c["position"]), ("hit_x", g["hit"][..., :1], c["hit"][..., :1])):
        dev = np.abs(gv - cv)
        close = (np.all(dev <= 1e-3 * np.abs(cv) + 1e-4, axis=2) & same).mean()
        tight = (np.all(dev <= 1e-5 * np.maximum(1.0, t)[..., None], axis=2) & same).mean()
        shares[film] = (close, tight)
        line.update({f"{film}_close": round(float(close), 6), f"{film}_tight": round(float(tight), 6), f"{film}_max_dev": float(f"{dev.max():.3e}"),
                     f"{film}_bit_equal": round(float(np.all(gv == cv, axis=2).mean()), 6)})
    log_line(line)
    assert np.array_equal(g["shading_normal"][same].view(np.uint32), c["shading_normal"][same].view(np.uint32))
    assert np.array_equal(g["hit"][..., 1:][same].view(np.uint32), c["hit"][..., 1:][same].view(np.uint32))
    for film, (close, tight) in shares.items():
        assert close >= PER_SAMPLE_MIN, (film, close)
        assert tight >= TIGHT_MIN, (film, tight)


@pytest.mark.parametrize("name", gs.NAMES)
def test_cooperative_traversal_does_not_depend_on_the_builder(product, pkg, gpu, name):
    a, b = gpu_gbuffer(product, pkg, gpu(name, "host")), gpu_gbuffer(product, pkg, gpu(name, "gpu"))
    share = float((a["hit"][..., 0].view(np.uint32) == b["hit"][..., 0].view(np.uint32)).mean())
    log_line({"test": "gbuffer_host_vs_gpu_tree", "family": name, "hit_x_bit_equal": round(share, 6)})
    assert share >= 0.9999, share


def test_node_visits_per_ray_at_three_scales_are_recorded(product, pkg, gpu):
    """The cost of the relative box pad (2^-22 x the largest coordinate, against the absolute RAY_EPS): nodes_closest per closest ray of
    the production traversal (the instrumented kernel, collect_stats = 2) on the same soup at scale 1, 1e3 and 1e-3, 256 x 192 at 4 spp.
    Recorded (MI355PT_FRAME_LOG), not asserted; what is asserted is that every run traced the frame's samples."""
    import torch
    for name in ("soup1025", "soup1025_x1e3", "soup1025_x1e-3"):
        for builder in BUILDERS:
            sc, cam, _ = gpu(name, builder)
            st = pkg.ffi.Stats()
            film = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
            product.render_accum_device(sc, cam, pkg.make_params(4, "mis", "sobol", collect_stats=2), 0, 4, film.data_ptr(), None, stats=st)
            torch.cuda.synchronize()
            assert st.samples == W * H * 4 and st.closest_rays >= st.samples
            log_line({"test": "node_visits", "family": name, "builder": builder, "closest_rays": int(st.closest_rays),
                      "nodes_closest_per_ray": round(st.nodes_closest / st.closest_rays, 3), "tris_closest_per_ray": round(st.tris_closest / st.closest_rays, 3)})


# ------------------------------------------------------------------------------------------------------------------ candidate lists
LIST_W, LIST_H, LIST_SPP, LIST_SHARDS = 1920, 1080, 64, 4001
CENTRAL = (67 * ((LIST_W + 7) // 8) + 120) % LIST_SHARDS             # the shard that holds the frame's central tile
LIST_CASES = {"soup1025_x1e3": CENTRAL, "slivers64": 0, "instanced": CENTRAL}    # family: shard index (the slivers all cross in the central tile)


def list_rects(name):
    return item_rects(LIST_W, LIST_H, LIST_SPP, LIST_CASES[name], LIST_SHARDS)


@pytest.mark.parametrize("name", list(LIST_CASES))
def test_candidate_lists_against_the_traversal(product, pkg, monkeypatch, name):
    """A sparse shard of the 1920 x 1080 frame at 64 spp under MIS, a constant environment light added: with MI355PT_NO_CAMERA_LISTS set and
    unset the per-sample log (L, lambda, pdf) and the film are bit-equal, and the case has a work item whose list holds 3 or more
    triangles within the kernels' cap."""
    sc, cam, _ = gs.build_scene(product, name, env_light=True, width=LIST_W, height=LIST_H)
    counts, over, _ = sc.debug_camera_candidates(cam, list_rects(name), cap=CAP)
    log_line({"test": "camera_lists", "family": name, "work_items": int(counts.size), "within_cap": int((~over).sum()),
              "longest_within_cap": int(counts[~over].max(initial=0)), "overflow": int(over.sum())})
    assert (counts[~over] >= 3).any()
    prm = pkg.make_params(LIST_SPP, "mis", "sobol", shard_index=LIST_CASES[name], shard_count=LIST_SHARDS)
    monkeypatch.setenv("MI355PT_NO_CAMERA_LISTS", "1")
    want = product.render_sample_log(sc, cam, prm, 0, LIST_SPP, want_accum=True)
    monkeypatch.delenv("MI355PT_NO_CAMERA_LISTS")
    got = product.render_sample_log(sc, cam, prm, 0, LIST_SPP, want_accum=True)
    assert float(np.nansum(want[3])) > 0.0
    for what, a, b in zip(("L", "lambda", "pdf", "film"), want, got):
        assert np.array_equal(bits(a), bits(b)), f"{what}: {int((bits(a) != bits(b)).sum())} values differ"


def test_candidate_list_cases_include_an_overflow(product):
    """across the three cases at least one work item has more candidates than the cap (the fallback to the traversal runs beside the lists)"""
    overflow = 0
    for name in LIST_CASES:
        sc, cam, _ = gs.build_scene(product, name, env_light=True, width=LIST_W, height=LIST_H, build=False)
        overflow += int(sc.debug_camera_candidates(cam, list_rects(name), cap=CAP)[1].sum())
    assert overflow >= 1
