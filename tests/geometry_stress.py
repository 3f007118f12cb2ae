"""TEST INFRASTRUCTURE ONLY.  Adversarial geometry for the BVH builders and the primary-ray traversals: seeded mesh families, one scene
builder that describes a family identically to any backend (the product, the oracle, the G-buffer restatement), a float64 brute force,
and a validator for the tree mi355pt_scene_export_bvh returns.  Nothing here is designed to make a kernel fault: every family is a valid
scene of finite coordinates with at least 8 non-degenerate triangles.  tests/test_geometry_stress.py and tests/test_geometry_stress_gpu.py
use it."""
import importlib

import numpy as np

pkg = importlib.import_module("toy-cpu-pathtracing_amd")
ffi = pkg.ffi
F = np.float32
W, H = 256, 192
MAX_LEAF_TRIS, MAX_BUILD_DEPTH = 4, 22          # csrc/layout.hpp
COST_TRAVERSE, COST_TRI = 1.0, 0.8              # csrc/bvh_builder.cpp, shared by both builders
IDENTITY = np.eye(4, dtype=F)


class Family:
    """meshes: [(n, 3, 3) float32 LOCAL triangles]; instances: [(mesh index, (4, 4) float32 local_to_world)]; the camera sits at `offset`
    (which the generator has already added to the geometry) and looks down -z.  tie_free: no two triangles tie exactly in t along a camera
    ray (checked by tests/test_geometry_stress.py); spatial: the centroids have extent, so binned SAH has something to bin; scale: the
    size of the scene relative to the unit soup (lengths such as a ray offset scale with it); planes: (axis, world coordinate) of planes
    that hold triangles exactly, for rays lying inside them."""

    def __init__(self, name, meshes, instances=None, offset=(0.0, 0.0, 0.0), tie_free=True, spatial=True, scale=1.0, planes=()):
        self.name, self.meshes = name, [np.ascontiguousarray(m, dtype=F) for m in meshes]
        self.instances = instances if instances is not None else [(0, IDENTITY)]
        self.offset = np.asarray(offset, dtype=F)
        self.tie_free, self.spatial, self.scale, self.planes = tie_free, spatial, float(scale), tuple(planes)

    @property
    def n_tris(self):
        return sum(self.meshes[m].shape[0] for m, _ in self.instances)

    def world64(self):
        """(n, 3, 3) float64: the float32 description carried to world space without rounding, instance after instance"""
        out = []
        for m, l2w in self.instances:
            p = self.meshes[m].astype(np.float64)
            M = np.asarray(l2w, dtype=F).astype(np.float64)
            out.append(p @ M[:3, :3].T + M[:3, 3])
        return np.concatenate(out)

    def render64(self):
        return self.world64() - self.offset.astype(np.float64)

    def render32(self):
        """(n, 3, 3) float32: the render-space vertices as csrc/scene_lower.cpp computes them, operation for operation (world_to_render *
        local_to_world, then glam's transform_point3 order: ((m.x * p.x + m.y * p.y) + m.z * p.z) + m.w), uncontracted float32"""
        w2r = np.eye(4, dtype=F); w2r[:3, 3] = -self.offset
        out = []
        for m, l2w in self.instances:
            a, b = w2r, np.asarray(l2w, dtype=F)
            l2r = np.zeros((4, 4), F)
            for c in range(4):
                for r in range(4):
                    s = F(a[r, 0] * b[0, c]); s = F(s + F(a[r, 1] * b[1, c])); s = F(s + F(a[r, 2] * b[2, c])); s = F(s + F(a[r, 3] * b[3, c]))
                    l2r[r, c] = s
            p = self.meshes[m]
            q = np.zeros(p.shape, F)
            for r in range(3):
                v = (l2r[r, 0] * p[..., 0]).astype(F)
                v = (v + (l2r[r, 1] * p[..., 1]).astype(F)).astype(F)
                v = (v + (l2r[r, 2] * p[..., 2]).astype(F)).astype(F)
                q[..., r] = (v + l2r[r, 3]).astype(F)
            out.append(q)
        return np.concatenate(out)


# ---------------------------------------------------------------------------------------------------------------- generators
def _soup(n, seed=None, sigma=0.15):
    rng = np.random.default_rng(1000 + n if seed is None else seed)
    c = np.stack([rng.uniform(-1.0, 1.0, n), rng.uniform(-0.75, 0.75, n), rng.uniform(-4.0, -2.0, n)], 1)
    return (c[:, None, :] + rng.normal(0.0, sigma, (n, 3, 3))).astype(F)


def _grid(k, seed=7):
    """a jittered planar grid at z = -3: (k + 1)^2 shared corners moved in x and y only, two triangles per cell"""
    rng = np.random.default_rng(seed)
    xs, ys = np.meshgrid(np.linspace(-1.0, 1.0, k + 1), np.linspace(-0.75, 0.75, k + 1), indexing="xy")
    cell = 2.0 / k
    p = np.stack([xs + rng.uniform(-0.3, 0.3, xs.shape) * cell, ys + rng.uniform(-0.3, 0.3, xs.shape) * cell * 0.75, np.full(xs.shape, -3.0)], -1)
    tris = []
    for j in range(k):
        for i in range(k):
            a, b, c, d = p[j, i], p[j, i + 1], p[j + 1, i + 1], p[j + 1, i]
            tris += [(a, b, c), (a, c, d)]
    return np.array(tris, F)


def _dyadic(a, bits=10):
    return np.round(np.asarray(a, np.float64) * (1 << bits)) / (1 << bits)


def _line(n, seed=11):
    """triangles whose BOX CENTRES (the builders' centroids, 0.5 * (lo + hi)) lie on the line y = 0.125, z = -3 exactly: the y and z
    offsets of the vertices are dyadic and symmetric about the line, so both sums are exact in float32"""
    rng = np.random.default_rng(seed)
    tris = []
    for i in range(n):
        x = -1.0 + 2.0 * (i + 0.5) / n
        hy, hz = _dyadic(rng.uniform(0.05, 0.3)), _dyadic(rng.uniform(0.05, 0.3))
        my, mz = _dyadic(rng.uniform(-1, 1) * hy), _dyadic(rng.uniform(-1, 1) * hz)
        dy, dz = np.array([-hy, hy, my]), np.array([mz, -hz, hz])
        dx = rng.uniform(-0.05, 0.05, 3)
        tris.append(np.stack([x + dx, 0.125 + dy, -3.0 + dz], 1))
    return np.array(tris, F)


def _coincident(n):
    """n different triangles with ONE box centre, exactly: a triangle whose box is symmetric about the origin, its axes permuted and its
    size stepped in dyadic factors, around a dyadic centre.  The copies lie in different planes (the triangle's plane misses the centre)."""
    base = np.array([[-1.0, -1.0, -0.5], [1.0, -0.25, 0.5], [0.375, 1.0, 0.125]])
    perms = [(0, 1, 2), (1, 2, 0), (2, 0, 1), (0, 2, 1), (2, 1, 0), (1, 0, 2)]
    centre = np.array([0.125, -0.0625, -3.0])
    tris = []
    for i in range(n):
        v = base[:, perms[i % 6]] * (1 if (i // 6) % 2 == 0 else -1)
        k = (i * (64 // n) + 8) / 256.0                       # sizes 0.03 .. 0.28: every product is a multiple of 2^-11
        tris.append(centre + k * v)
    t = np.array(tris, F)
    assert np.array_equal(t.astype(np.float64), np.array(tris))      # nothing was rounded
    return t


def _slivers(n, seed=5):
    """triangles 3 long and 2e-3 wide, fanned around the view axis, each at its own depth and tilt"""
    rng = np.random.default_rng(seed)
    tris = []
    for i in range(n):
        th = np.pi * (i + rng.uniform(0.2, 0.8)) / n
        u = np.array([np.cos(th), np.sin(th), rng.uniform(-0.1, 0.1)]); u /= np.linalg.norm(u)
        w = np.array([-np.sin(th), np.cos(th), 0.0])
        c = np.array([rng.uniform(-0.02, 0.02), rng.uniform(-0.02, 0.02), -3.0 - 0.02 * i])
        tris.append([c - 1.5 * u, c + 1.5 * u, c - 1.5 * u + 2e-3 * w])
    return np.array(tris, F)


def _clusters(seed=13):
    """one 1e3-sized background pair behind 1024 triangles of size 1e-2 in four clumps"""
    rng = np.random.default_rng(seed)
    a = 500.0
    bg = [[(-a, -a, -6.0), (a, -a, -6.0), (a, a, -6.5)], [(-a, -a, -6.0), (a, a, -6.5), (-a, a, -6.5)]]
    small = []
    for cx, cy, cz in ((-0.5, -0.3, -2.5), (0.45, 0.25, -3.0), (0.1, -0.35, -3.5), (-0.3, 0.4, -2.2)):
        c = np.array([cx, cy, cz]) + rng.normal(0.0, 0.05, (256, 3))
        small.append(c[:, None, :] + rng.normal(0.0, 1e-2, (256, 3, 3)))
    return np.concatenate([np.array(bg), np.concatenate(small)]).astype(F)


CUBE_LO = {"x": (-0.5, 0.0, 0.5), "y": (-0.5, 0.0, 0.5), "z": (-2.3, -2.8, -3.3)}
CUBE_SIZE = 0.3


def _cubes():
    """27 axis-aligned cuboids on a 3 x 3 x 3 lattice; the planes x = 0 and y = 0 hold faces AND the camera"""
    tris = []
    for x in CUBE_LO["x"]:
        for y in CUBE_LO["y"]:
            for z in CUBE_LO["z"]:
                m = pkg.assets._cuboid((x, y, z), (x + CUBE_SIZE, y + CUBE_SIZE, z + CUBE_SIZE))
                tris.append(m["pos"][m["idx"].reshape(-1, 3)])
    return np.concatenate(tris).astype(F)


def _trs(t, axis, deg, s):
    axis = np.asarray(axis, np.float64); axis /= np.linalg.norm(axis)
    a = np.deg2rad(deg)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)
    M = np.eye(4); M[:3, :3] = R @ np.diag(s); M[:3, 3] = t
    return M.astype(F)


def _instanced():
    mesh = _soup(256).astype(np.float64) + np.array([0.0, 0.0, 3.0])        # centred on its own origin
    inst = [(0, _trs((-0.6, -0.35, -3.0), (0, 1, 0), 30.0, (0.45, 0.3, 0.25))),
            (0, _trs((0.6, -0.35, -3.2), (1, 0, 0), 75.0, (0.3, 0.5, 0.2))),
            (0, _trs((0.0, 0.0, -4.0), (1, 1, 1), 120.0, (0.5, 0.45, 0.4))),
            (0, _trs((-0.55, 0.4, -2.6), (0, 0, 1), 200.0, (0.2, 0.35, 0.3))),
            (0, _trs((0.55, 0.4, -2.8), (1, 2, 3), 310.0, (0.4, 0.2, 0.35)))]
    return [mesh.astype(F)], inst


FAR = (1000.0, -2000.0, 500.0)
_CACHE = {}


def _make(name):
    if name.startswith("soup") and name[4:].isdigit():
        return Family(name, [_soup(int(name[4:]))])
    if name == "soup1025_x1e3":
        return Family(name, [(_soup(1025) * F(1e3)).astype(F)], scale=1e3)
    if name == "soup1025_x1e-3":
        return Family(name, [(_soup(1025) * F(1e-3)).astype(F)], scale=1e-3)
    if name == "soup1025_far":
        return Family(name, [(_soup(1025) + np.asarray(FAR, F)).astype(F)], offset=FAR)
    if name == "grid16":
        return Family(name, [_grid(16)], planes=((2, -3.0),))
    if name == "line64":
        return Family(name, [_line(64)])
    if name in ("coincident9", "coincident64"):
        return Family(name, [_coincident(int(name[10:]))], tie_free=False, spatial=False)
    if name == "soup256_x3":
        return Family(name, [_soup(256)], instances=[(0, IDENTITY)] * 3, tie_free=False, spatial=False)
    if name == "slivers64":
        return Family(name, [_slivers(64)])
    if name == "clusters":
        return Family(name, [_clusters()])
    if name == "cubes27":
        return Family(name, [_cubes()], planes=((0, 0.0), (1, 0.0), (0, CUBE_SIZE), (2, -2.5)))
    if name == "instanced":
        meshes, inst = _instanced()
        return Family(name, meshes, instances=inst)
    raise KeyError(name)


NAMES = ["soup8", "soup9", "soup1023", "soup1024", "soup1025", "soup2049", "soup1025_x1e3", "soup1025_x1e-3", "soup1025_far", "grid16", "line64",
         "coincident9", "coincident64", "soup256_x3", "slivers64", "clusters", "cubes27", "instanced"]


def family(name):
    if name not in _CACHE:
        _CACHE[name] = _make(name)
    return _CACHE[name]


# ---------------------------------------------------------------------------------------------------------------- the scene builder
def _mesh_dict(tris):
    t64 = tris.astype(np.float64)
    n = np.cross(t64[:, 1] - t64[:, 0], t64[:, 2] - t64[:, 0])
    ln = np.linalg.norm(n, axis=1, keepdims=True)
    assert np.all(ln > 0.0), "a generator made a degenerate triangle"
    n = (n / ln).astype(F)
    return dict(pos=tris.reshape(-1, 3), nrm=np.repeat(n, 3, axis=0), uv=None, idx=np.arange(tris.shape[0] * 3, dtype=np.uint32))


def camera(name, width=W, height=H):
    return ffi.make_camera(tuple(float(v) for v in family(name).offset), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), width, height)


def build_scene(backend, name, builder=None, lowering=None, env_light=False, width=W, height=H, build=True):
    """(scene, camera, D65 LUT id) of family `name`, described identically to whichever backend: unshared vertices with facet normals, one
    constant-0.7 Lambert material.  builder ("host" | "gpu" | "auto") and lowering ("auto" | "no_local_tris" | "general") exist on the
    product only; env_light adds a constant environment light (the path kernels then have something to carry)."""
    fam = family(name)
    sc = backend.new_scene()
    sc.set_rgb2spec(pkg.scenes.srgb_table())
    if builder is not None:
        sc.set_bvh_builder(builder)
    if lowering is not None:
        sc.debug_set_lowering(lowering)
    d = ffi.MaterialDesc(); d.type = ffi.MAT_LAMBERT; d.color = ffi.Spectrum.constant(0.7); d.normal_tex = ffi.NONE
    mat = sc.add_material(d)
    geoms = [sc.add_mesh(_mesh_dict(m)) for m in fam.meshes]
    for m, l2w in fam.instances:
        sc.add_instance(geoms[m], mat, l2w)
    d65 = sc.add_lut470(pkg.scenes.presets()["cie_illum_d6500"])
    if env_light:
        sc.add_environment_light(1.0, np.ones((8, 16, 3), dtype=F), d65)
    cam = camera(name, width, height)
    if build:
        sc.build(cam)
    return sc, cam, d65


# ---------------------------------------------------------------------------------------------------------------- rays
def camera_like_rays(n, seed):
    """render-space rays from the camera into its field of view"""
    rng = np.random.default_rng(seed)
    d = np.stack([rng.uniform(-0.5, 0.5, n), rng.uniform(-0.38, 0.38, n), -np.ones(n)], 1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.zeros((n, 3), F), d.astype(F)


def collapse_rays(name, n=4000, seed=3):
    """(n, 6) render-space origin + direction: camera rays, rays from inside the geometry's bounds in random directions, rays whose
    direction has exactly one and exactly two zero components (parallel to a coordinate plane / to an axis), and rays lying exactly in
    the family's planes (origin on the plane, no direction component across it)"""
    fam = family(name)
    rng = np.random.default_rng(seed)
    v = fam.render32().reshape(-1, 3).astype(np.float64)
    lo, hi = np.percentile(v, 1, axis=0), np.percentile(v, 99, axis=0)
    q = n // 5
    o_cam, d_cam = camera_like_rays(q, seed)
    rays = [np.concatenate([o_cam, d_cam], 1)]
    o = rng.uniform(lo - 0.1 * (hi - lo), hi + 0.1 * (hi - lo), (n - q, 3))
    d = rng.normal(size=(n - q, 3))
    kind = np.arange(n - q) % 4                  # 0: general, 1: one zero component, 2: two zero components, 3: in a plane of the family
    for i in range(n - q):
        if kind[i] == 1:
            d[i, rng.integers(3)] = 0.0
        elif kind[i] == 2:
            keep = rng.integers(3); s = np.sign(d[i, keep]) or 1.0
            d[i] = 0.0; d[i, keep] = s
        elif kind[i] == 3 and fam.planes:
            axis, w = fam.planes[rng.integers(len(fam.planes))]
            o[i, axis] = np.float64(F(w) - fam.offset[axis]); d[i, axis] = 0.0
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays.append(np.concatenate([o, d], 1))
    return np.concatenate(rays).astype(F)


# ---------------------------------------------------------------------------------------------------------------- float64 brute force
def brute_force64(tris64, dirs, t_ref, slack, chunk=4096):
    """Moeller-Trumbore in float64 for rays that all start at the origin (the camera in render space): every ray against every triangle.
    slack: per-triangle uncertainty of the barycentric bounds (the ray is known only so well).  t_ref: the distance to judge, per ray.
    Returns per ray
      t1, t2     the nearest and second-nearest exact hit (inf = none),
      rel        min over the triangles the ray hits or passes within the slack of |t_ref - t| / t_ref (inf: no such triangle),
      t_certain  the nearest hit that stays one with every triangle shrunk by the slack."""
    p0, e1, e2 = tris64[:, 0], tris64[:, 1] - tris64[:, 0], tris64[:, 2] - tris64[:, 0]
    tvec = -p0
    qvec = np.cross(tvec, e1)
    A_det, A_u, A_v = np.cross(e2, e1), np.cross(e2, tvec), qvec          # d . A = the triple products with the ray direction
    t_num = np.einsum("ij,ij->i", e2, qvec)
    s = np.asarray(slack, np.float64)
    d = np.asarray(dirs, np.float64)
    n = d.shape[0]
    t1, t2, rel, t_certain = (np.full(n, np.inf) for _ in range(4))
    for b in range(0, n, chunk):
        dd = d[b:b + chunk]
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1.0 / (dd @ A_det.T)
            u, v, t = (dd @ A_u.T) * inv, (dd @ A_v.T) * inv, t_num[None, :] * inv
        w = 1.0 - u - v
        front = np.isfinite(inv) & (t > 0.0)
        lowest = np.minimum(np.minimum(u, v), w)
        exact = np.where(front & (lowest >= 0.0), t, np.inf)
        part = np.partition(exact, 1, axis=1)[:, :2] if exact.shape[1] > 1 else np.concatenate([exact, np.full_like(exact, np.inf)], 1)
        t1[b:b + chunk], t2[b:b + chunk] = part[:, 0], part[:, 1]
        near = front & (lowest >= -s)
        r = np.where(near, np.abs(t - t_ref[b:b + chunk, None]) / t_ref[b:b + chunk, None], np.inf)
        rel[b:b + chunk] = r.min(axis=1)
        t_certain[b:b + chunk] = np.where(front & (lowest >= s), t, np.inf).min(axis=1)
    return t1, t2, rel, t_certain


def min_altitude(tris64):
    e = np.stack([tris64[:, 1] - tris64[:, 0], tris64[:, 2] - tris64[:, 1], tris64[:, 0] - tris64[:, 2]], 1)
    area2 = np.linalg.norm(np.cross(e[:, 0], -e[:, 2]), axis=1)
    return area2 / np.linalg.norm(e, axis=2).max(axis=1)


# ---------------------------------------------------------------------------------------------------------------- the tree validator
def _leaf(link):
    c = int(link) & 0xFFFFFFFF
    return (c & 0x7FFFFFFF) >> 3, (c & 7) + 1


def tri_vertices(tris_words):
    return np.ascontiguousarray(np.asarray(tris_words, np.uint32).reshape(-1, 12)[:, :9]).view(F).reshape(-1, 3, 3)


def same_multiset(a, b):
    """two (m, 9) float32 arrays hold the same rows with the same multiplicities, compared as bit patterns"""
    a = np.ascontiguousarray(a, dtype=F).reshape(-1, 9).view(np.uint32); b = np.ascontiguousarray(b, dtype=F).reshape(-1, 9).view(np.uint32)
    if a.shape != b.shape:
        return False
    return np.array_equal(a[np.lexsort(a.T[::-1])], b[np.lexsort(b.T[::-1])])


def validate_bvh(nodes, tris, root, input_tris=None, equal_boxes=False):
    """The structure of an exported BVH2 (include/mi355pt_debug.h: 64-byte node records holding both child boxes, 48-byte leaf-ordered
    triangle records), checked against the triangles it was built from.  Raises AssertionError when
      1. the leaf ranges reachable from the root do not partition [0, m) (an index missing, or reached twice; a node reached twice),
      2. a leaf holds more than MAX_LEAF_TRIS triangles,
      3. a leaf lies deeper than MAX_BUILD_DEPTH (the root node is depth 0),
      4. a stored child box does not enclose the exact min / max of the vertices below that child (compared as values),
      5. equal_boxes: a stored child box differs from that exact box,
      6. input_tris given: the exported triangles are not the input triangles as a multiset of 9-float rows.
    Returns {"depth", "leaves", "nodes", "tris", "max_leaf", "sah"}: sah is the tree's cost with the builders' constants over the STORED
    boxes, (sum over nodes of 1.0 * A(node) + sum over leaves of 0.8 * count * A(leaf)) / A(root)."""
    words = np.ascontiguousarray(np.asarray(nodes, np.uint32).reshape(-1, 16))
    f, links = words.view(F), words[:, 12:14].view(np.int32)
    n = words.shape[0]
    v = tri_vertices(tris)
    m = v.shape[0]
    tlo, thi = v.min(axis=1), v.max(axis=1)
    seen_tri, seen_node = np.zeros(m, np.int64), np.zeros(n, bool)
    out = {"depth": 0, "leaves": 0, "nodes": 0, "tris": m, "max_leaf": 0}
    cost = [0.0]

    def area(lo, hi):
        e = np.maximum(hi.astype(np.float64) - lo.astype(np.float64), 0.0)
        return 2.0 * (e[0] * e[1] + e[1] * e[2] + e[2] * e[0])

    def visit(link, depth, stored):
        """-> exact (lo, hi) of the vertices below `link`; stored: the (lo, hi) its parent holds for it (None at the root)"""
        if link < 0:
            first, count = _leaf(link)
            assert count <= MAX_LEAF_TRIS, f"leaf of {count} triangles"
            assert first + count <= m, f"leaf range [{first}, {first + count}) leaves the {m} triangles"
            assert depth <= MAX_BUILD_DEPTH, f"leaf at depth {depth}"
            seen_tri[first:first + count] += 1
            out["depth"] = max(out["depth"], depth); out["leaves"] += 1; out["max_leaf"] = max(out["max_leaf"], count)
            if stored is not None:
                cost[0] += COST_TRI * count * area(*stored)
            return tlo[first:first + count].min(axis=0), thi[first:first + count].max(axis=0)
        assert 0 <= link < n, f"link {link} outside the {n} nodes"
        assert not seen_node[link], f"node {link} is reached twice"
        assert depth < MAX_BUILD_DEPTH, f"node at depth {depth}"
        seen_node[link] = True; out["nodes"] += 1
        boxes = []
        for s in (0, 1):
            st = (np.array([f[link, s], f[link, 4 + s], f[link, 8 + s]]), np.array([f[link, 2 + s], f[link, 6 + s], f[link, 10 + s]]))
            lo, hi = visit(int(links[link, s]), depth + 1, st)
            assert np.all(st[0] <= lo) and np.all(st[1] >= hi), f"node {link} child {s}: stored box {st} does not enclose {lo, hi}"
            if equal_boxes:
                assert np.all(st[0] == lo) and np.all(st[1] == hi), f"node {link} child {s}: stored box {st} is larger than {lo, hi}"
            boxes.append(st)
        mine = stored if stored is not None else (np.minimum(boxes[0][0], boxes[1][0]), np.maximum(boxes[0][1], boxes[1][1]))
        cost[0] += COST_TRAVERSE * area(*mine)
        if stored is None:
            out["root_area"] = area(*mine)
        return np.minimum(boxes[0][0], boxes[1][0]), np.maximum(boxes[0][1], boxes[1][1])

    assert root >= 0, "the root is a leaf link"
    visit(int(root), 0, None)
    missing, twice = np.nonzero(seen_tri == 0)[0], np.nonzero(seen_tri > 1)[0]
    assert twice.size == 0, f"{twice.size} triangle indices are in more than one leaf, the first {twice[:4]}"
    assert missing.size == 0, f"{missing.size} triangle indices are in no reachable leaf, the first {missing[:4]}"
    if input_tris is not None:
        assert same_multiset(v.reshape(-1, 9), np.asarray(input_tris, F).reshape(-1, 9)), "the exported triangles are not the input triangles"
    out["sah"] = cost[0] / out.pop("root_area")
    return out


def median_tree(tris):
    """A small BVH2 in the exported layout, built in NumPy (object-median splits on the widest axis of the box centres, leaves of at most
    MAX_LEAF_TRIS): the validator's own test subject.  -> nodes (n, 16) uint32, triangle records (m, 12) uint32, root"""
    tris = np.ascontiguousarray(tris, dtype=F)
    lo, hi = tris.min(axis=1), tris.max(axis=1)
    c = (F(0.5) * (lo + hi)).astype(F)
    nodes, order = [], []

    def build(ids):
        if len(ids) <= MAX_LEAF_TRIS:
            first = len(order); order.extend(ids)
            return np.int32(np.uint32(0x80000000 | (first << 3) | (len(ids) - 1)).view(np.int32)), lo[ids].min(axis=0), hi[ids].max(axis=0)
        axis = int(np.argmax(c[ids].max(axis=0) - c[ids].min(axis=0)))
        ids = sorted(ids, key=lambda i: (c[i, axis], i))
        me = len(nodes); nodes.append(None)
        kids = [build(ids[:len(ids) // 2]), build(ids[len(ids) // 2:])]
        rec = np.zeros(16, np.uint32); fr = rec.view(F)
        for s, (link, blo, bhi) in enumerate(kids):
            fr[s], fr[4 + s], fr[8 + s] = blo; fr[2 + s], fr[6 + s], fr[10 + s] = bhi
            rec[12 + s] = np.int32(link).view(np.uint32)
        nodes[me] = rec
        return np.int32(me), np.minimum(kids[0][1], kids[1][1]), np.maximum(kids[0][2], kids[1][2])

    root, _, _ = build(list(range(tris.shape[0])))
    recs = np.zeros((len(order), 12), np.uint32)
    recs[:, :9] = tris[order].reshape(-1, 9).view(np.uint32)
    return np.array(nodes, np.uint32), recs, int(root)
