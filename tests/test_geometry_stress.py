"""CPU tests on the adversarial geometry of tests/geometry_stress.py: the oracle (the other half of every GPU comparison) against a float64
brute force, its fast walker against its faithful one, the BVH2 -> BVH4 collapse on this geometry, the render-space vertices the GPU tests
expect against what the host lowering makes, and the tree validator against trees with known defects.  No GPU involved.  Figures go to
the file MI355PT_FRAME_LOG names (profiles/geometry_stress.jsonl)."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gbuffer_reference  # noqa: E402
import geometry_stress as gs  # noqa: E402

FILMS = gbuffer_reference.FILMS
# |t - t64| / t of the oracle's G-buffer restatement, 256 x 192 at 1 spp: 4 x the largest per-family maximum of profiles/geometry_stress.jsonl
# ("test": "oracle_vs_float64"), rounded up to one digit: 4 x 5.199e-6 (soup1025) = 2.08e-5.  soup1025_far has its own figure by the same
# rule, 4 x 8.666e-3 = 3.47e-2: its positions are rounded at the magnitude of its world coordinates (2000, one ulp = 1.2e-4), the ray drawn
# through such a position is off by that much sideways, and along a ray that grazes a triangle at 1 degree a sideways 1.2e-4 is 7e-3 of t.
# The same pixels give |position| against t within 9.2e-5 ("position_vs_t_max"): the distance itself is not what deviates.
T_REL_BOUND = 3e-5
T_REL_BOUND_FAR = 4e-2


def t_rel_bound(name):
    return T_REL_BOUND_FAR if name == "soup1025_far" else T_REL_BOUND


def log_line(line):
    print(line)
    if os.environ.get("MI355PT_FRAME_LOG"):
        with open(os.environ["MI355PT_FRAME_LOG"], "a") as f:
            f.write(json.dumps(line) + "\n")


@pytest.fixture(scope="module")
def ref():
    return gbuffer_reference.GbufferReference()


@pytest.fixture(scope="module")
def restated(ref, pkg):
    """family -> {"fast": films, "faithful": films} of the G-buffer restatement, 256 x 192 at 1 spp with Sobol, rendered once"""
    cache = {}

    def get(name):
        if name not in cache:
            sc, cam, d65 = gs.build_scene(ref, name)
            out = {}
            for mode, faithful in (("faithful", True), ("fast", False)):
                ref.set_faithful(sc, faithful)
                out[mode] = ref.render_gbuffer_accum(sc, cam, pkg.make_params(1, "mis", "sobol"), d65)
            cache[name] = out
        return cache[name]
    return get


@pytest.mark.parametrize("name", gs.NAMES)
def test_oracle_hits_agree_with_a_float64_brute_force(restated, name):
    """Every hit pixel of the restatement against Moeller-Trumbore in float64 over ALL triangles, along the ray from the camera through the
    reported position: the nearest float64 hit exists and |t - t64| / t stays below T_REL_BOUND.

    The ray is known only as well as the position is: a float32 sum of vertices weighted in the mesh's local space, off by a few roundings
    at the magnitude of the largest coordinate (2000 where the world is far from the origin).  Where such a ray passes a triangle's edge
    within delta = 32 * 2^-24 * (largest |coordinate| + |position|) the float64 answer depends on less than the input holds; there the
    check is two-sided instead: (a) a triangle that the ray hits or passes within delta lies at the reported t (the hit is real), and
    (b) no triangle that the ray hits even when every triangle is shrunk by delta lies in front of it (nothing certain was missed).
    Away from edges that IS the nearest exact hit; the pixels where it is not are counted ("edge_pixels").
    Tie-free families: the nearest and second-nearest exact t differ on every pixel."""
    fam = gs.family(name)
    c = restated(name)["fast"]
    hit = c["hit"][..., 1] == 1.0
    assert hit.sum() >= 300, hit.sum()
    p = c["position"][hit].astype(np.float64)
    t = c["hit"][..., 0][hit].astype(np.float64)
    dist = np.linalg.norm(p, axis=1)
    tris = fam.render64()
    coord = max(float(np.abs(fam.world64()).max()), max(float(np.abs(m).max()) for m in fam.meshes))
    delta = 32.0 * 2.0 ** -24 * (coord + float(dist.max()))
    t1, t2, rel, t_certain = gs.brute_force64(tris, p / dist[:, None], t, delta / gs.min_altitude(tris))
    assert np.isfinite(rel).all(), f"{int((~np.isfinite(rel)).sum())} hit pixels have no float64 hit"
    rel_exact = np.where(np.isfinite(t1), np.abs(t - t1) / t, np.inf)
    in_front = np.maximum((t - t_certain) / t, 0.0)                  # how far in front of the reported hit a certain one lies
    both = np.isfinite(t2)
    gap = (t2[both] - t1[both]) / t1[both]
    log_line({"test": "oracle_vs_float64", "family": name, "tris": fam.n_tris, "hit_pixels": int(hit.sum()), "t_rel_max": float(f"{rel.max():.3e}"),
              "missed_in_front_max": float(f"{in_front.max():.3e}"), "edge_pixels": int((rel_exact > rel).sum()), "delta": float(f"{delta:.3e}"),
              "position_vs_t_max": float(f"{(np.abs(dist - t) / t).max():.3e}"), "smallest_t_gap": float(f"{gap.min():.3e}") if gap.size else None})
    if fam.tie_free:
        assert gap.size == 0 or gap.min() > 0.0, "two triangles tie exactly in t along a camera ray"
    assert rel.max() < t_rel_bound(name), float(rel.max())
    assert in_front.max() < t_rel_bound(name), float(in_front.max())


@pytest.mark.parametrize("name", gs.NAMES)
def test_fast_walker_equals_faithful_walker_on_this_geometry(restated, name):
    both = restated(name)
    for k in FILMS:
        assert np.isfinite(both["fast"][k]).all(), k
        assert np.array_equal(both["fast"][k].view(np.uint32), both["faithful"][k].view(np.uint32)), k


@pytest.mark.parametrize("name", gs.NAMES)
def test_bvh_collapse_on_this_geometry(product, name):
    """mi355pt_probe_bvh_collapse (host only): the sweep-SAH BVH2 over the family's render-space triangles and its 4-wide collapse reach the
    same leaves for 4000 rays - camera rays, incoherent rays, rays with one and with two zero direction components, rays lying exactly in
    the planes that hold the triangles of `grid` and `cubes` - and the collapsed tree fits the 24-entry stack."""
    rays = gs.collapse_rays(name, 4000)
    assert rays.shape == (4000, 6) and np.isfinite(rays).all()
    d = rays[:, 3:]
    assert ((d == 0).sum(axis=1) == 1).sum() > 300 and ((d == 0).sum(axis=1) == 2).sum() > 300
    info, mismatch = product.probe_bvh_collapse(gs.family(name).render32(), rays)
    log_line({"test": "collapse", "family": name, **info, "mismatch": mismatch})
    assert mismatch == 0
    assert info["max_stack4"] < 24 and info["depth2"] <= gs.MAX_BUILD_DEPTH


@pytest.mark.parametrize("name", gs.NAMES)
def test_expected_render_space_vertices_are_the_host_lowering(product, name):
    """Family.render32 (what the GPU tests hold the exported triangles against) is, as a multiset, what the host lowering makes of the
    described scene (mi355pt_scene_debug_camera_candidates returns the lowered triangles; host only)."""
    sc, cam, _ = gs.build_scene(product, name, build=False)
    _, _, _, tris = sc.debug_camera_candidates(cam, np.array([[0, 0, 7, 7]], np.uint32), want_tris=True)
    assert tris.shape[0] == gs.family(name).n_tris
    assert gs.same_multiset(tris.reshape(-1, 9), gs.family(name).render32().reshape(-1, 9))


def test_families_are_what_they_claim():
    """the properties the families exist for, on the float32 data the builders get: box centres (the builders' centroids) without extent
    where promised, the sizes around the 1024-triangle workgroup of k_bin, finite coordinates, at least 8 triangles"""
    for name in gs.NAMES:
        v = gs.family(name).render32()
        assert np.isfinite(v).all() and v.shape[0] >= 8 and v.shape[0] == gs.family(name).n_tris, name
        assert v.shape[0] <= 2049, name
    assert [gs.family(f"soup{n}").n_tris for n in (8, 9, 1023, 1024, 1025, 2049)] == [8, 9, 1023, 1024, 1025, 2049]

    def centres(name):
        v = gs.family(name).render32()
        return (np.float32(0.5) * (v.min(axis=1) + v.max(axis=1))).astype(np.float32)
    ext = lambda name: np.ptp(centres(name), axis=0)
    assert ext("grid16")[2] == 0.0 and np.all(ext("grid16")[:2] > 1.0) and gs.family("grid16").n_tris == 512
    assert ext("line64")[0] > 1.0 and np.all(ext("line64")[1:] == 0.0)
    assert np.all(ext("coincident9") == 0.0) and np.all(ext("coincident64") == 0.0)
    c3 = centres("soup256_x3")
    assert np.array_equal(c3[:256], c3[256:512]) and np.array_equal(c3[:256], c3[512:])
    s = gs.family("slivers64").render64()
    e = np.linalg.norm(s[:, 1] - s[:, 0], axis=1)
    assert np.allclose(e, 3.0, atol=1e-5) and np.allclose(gs.min_altitude(s), 2e-3, rtol=0.01)
    assert np.abs(gs.family("soup1025_x1e3").render32()).max() > 3e3 and np.abs(gs.family("soup1025_x1e-3").render32()).max() < 6e-3
    assert np.abs(gs.family("soup1025_far").render32()).max() < 6.0 and np.abs(gs.family("soup1025_far").world64()).min() > 490.0


# ------------------------------------------------------------------------------------------------------------- the validator's own test
@pytest.fixture(scope="module")
def small_tree():
    tris = gs.family("soup9").meshes[0]
    more = np.concatenate([tris, gs.family("soup8").meshes[0], gs.family("line64").meshes[0][:6]])      # 23 triangles: leaves of 2 and 3
    return more, gs.median_tree(more)


def test_validator_accepts_a_sound_tree(small_tree):
    tris, (nodes, recs, root) = small_tree
    out = gs.validate_bvh(nodes, recs, root, input_tris=tris, equal_boxes=True)
    assert out["tris"] == 23 and out["leaves"] == 8 and out["nodes"] == 7 and out["depth"] == 3 and out["max_leaf"] == 3
    # the cost by hand for the root alone: its two child boxes are stored in it
    f = nodes.view(np.float32)
    assert out["sah"] > gs.COST_TRAVERSE and np.isfinite(out["sah"])
    # an oversized box is not an error of enclosure, but it is one of equality, and it costs
    fat = nodes.copy(); fat.view(np.float32)[root, 2] = np.nextafter(f[root, 2], np.float32(np.inf))
    assert gs.validate_bvh(fat, recs, root, input_tris=tris)["sah"] > out["sah"]
    with pytest.raises(AssertionError, match="is larger than"):
        gs.validate_bvh(fat, recs, root, input_tris=tris, equal_boxes=True)


def test_validator_rejects_a_box_shrunk_by_one_ulp(small_tree):
    tris, (nodes, recs, root) = small_tree
    for word, towards in ((2, -np.inf), (0, np.inf), (7, -np.inf), (9, np.inf)):       # hi0.x, lo0.x, hi1.y, lo1.z of the root
        bad = nodes.copy()
        bad.view(np.float32)[root, word] = np.nextafter(nodes.view(np.float32)[root, word], np.float32(towards))
        with pytest.raises(AssertionError, match="does not enclose"):
            gs.validate_bvh(bad, recs, root, input_tris=tris)


def test_validator_rejects_a_dropped_triangle_index(small_tree):
    tris, (nodes, recs, root) = small_tree
    links = nodes[:, 12:14].view(np.int32)
    n, s = next((n, s) for n in range(nodes.shape[0]) for s in (0, 1) if links[n, s] < 0 and gs._leaf(links[n, s])[1] == 3)
    bad = nodes.copy()
    bad[n, 12 + s] = nodes[n, 12 + s] - 1                                # the leaf keeps its first two triangles
    with pytest.raises(AssertionError, match="in no reachable leaf"):
        gs.validate_bvh(bad, recs, root)


def test_validator_rejects_a_leaf_range_referenced_twice(small_tree):
    tris, (nodes, recs, root) = small_tree
    links = nodes[:, 12:14].view(np.int32)
    n = next(n for n in range(nodes.shape[0]) if links[n, 0] < 0 and links[n, 1] < 0)
    bad = nodes.copy()
    bad[n, 13] = nodes[n, 12]                                            # both links of a node name its first leaf ...
    for w in (0, 4, 8, 2, 6, 10):                                        # ... with that leaf's box: every box still encloses, only the partition is wrong
        bad[n, w + 1] = nodes[n, w]
    with pytest.raises(AssertionError, match="more than one leaf"):
        gs.validate_bvh(bad, recs, root)
    twice = nodes.copy(); twice[n, 13] = root                            # and a node reached twice (a cycle would never end otherwise)
    with pytest.raises(AssertionError, match="reached twice"):
        gs.validate_bvh(twice, recs, root)


def test_validator_rejects_other_triangles_and_deep_or_fat_leaves(small_tree):
    tris, (nodes, recs, root) = small_tree
    other = tris.copy(); other[5, 1, 2] = np.nextafter(other[5, 1, 2], np.float32(np.inf))
    with pytest.raises(AssertionError, match="not the input triangles"):
        gs.validate_bvh(nodes, recs, root, input_tris=other)
    with pytest.raises(AssertionError, match="not the input triangles"):
        gs.validate_bvh(nodes, recs, root, input_tris=np.concatenate([tris[:22], tris[:1]]))          # same rows, other multiplicities
    # a chain of 24 nodes, one triangle per leaf: deeper than the builders may go
    chain = gs.family("soup1023").meshes[0][:25]
    lo, hi = chain.min(axis=1), chain.max(axis=1)
    recs2 = np.zeros((25, 12), np.uint32); recs2[:, :9] = chain.reshape(-1, 9).view(np.uint32)
    cn = np.zeros((24, 16), np.uint32); cf = cn.view(np.float32)
    for i in range(24):
        rest_lo, rest_hi = lo[i + 1:].min(axis=0), hi[i + 1:].max(axis=0)
        cf[i, 0:12:4], cf[i, 2:12:4] = lo[i], hi[i]
        cf[i, 1:12:4], cf[i, 3:12:4] = rest_lo, rest_hi
        cn[i, 12] = 0x80000000 | (i << 3)
        cn[i, 13] = i + 1 if i < 23 else 0x80000000 | (24 << 3)
    with pytest.raises(AssertionError, match="depth"):
        gs.validate_bvh(cn, recs2, 0)
    # a leaf of five triangles
    five = np.zeros((1, 16), np.uint32); ff = five.view(np.float32)
    ff[0, 0:12:4], ff[0, 2:12:4] = lo[:5].min(axis=0), hi[:5].max(axis=0)
    ff[0, 1:12:4], ff[0, 3:12:4] = lo[5:8].min(axis=0), hi[5:8].max(axis=0)
    five[0, 12] = 0x80000000 | (0 << 3) | 4
    five[0, 13] = 0x80000000 | (5 << 3) | 2
    with pytest.raises(AssertionError, match="leaf of 5"):
        gs.validate_bvh(five, recs2[:8], 0)
