"""The camera-ray candidate lists (csrc/camera_candidates.hpp) without a GPU.

tests/camera_candidates_check.cpp runs the header's walk on seeded synthetic 4-wide trees (unused slots as point boxes at FLT_MAX, boxes
that contain the apex, straddle a side plane or lie behind the camera, rectangles at the frame's corners, the cap reached exactly and
exceeded by one) and compares every list with a brute-force loop of the kernels' watertight triangle test over rays through the
rectangle's corners, edges and interior; it is built a second time with -fsanitize=address,undefined and run as its own executable.

The lowered scene 3 goes through mi355pt_scene_debug_camera_candidates (the lowering runs without a device) at 1920 x 1080: the pyramid of
every 2x2 block of the eight tiles through the frame centre and of eight tiles on the hero's silhouette, against a brute-force float64
ray / triangle test over ALL of the scene's triangles."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("rects", "rays", "hits", "longest", "behind_lists", "unused_slots")


def build_checker(tmp_path_factory, name, extra):
    exe = str(tmp_path_factory.mktemp(name) / "camera_candidates_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror"] + extra +
                   ["-I", os.path.join(ROOT, "toy-cpu-pathtracing_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "camera_candidates_check.cpp")], check=True)

    def run(seed, n_tris, w, h, *camera):
        """camera: nothing, or the seven optional arguments (direction, up, fov in degrees)"""
        r = subprocess.run([exe, str(seed), str(n_tris), str(w), str(h)] + [repr(float(v)) for v in camera], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        tag, *vals = r.stdout.split()
        assert tag == "ok", r.stdout
        return dict(zip(FIELDS, map(int, vals)))
    return run


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return build_checker(tmp_path_factory, "camera_candidates", [])


@pytest.fixture(scope="module")
def checker_sanitized(tmp_path_factory):
    return build_checker(tmp_path_factory, "camera_candidates_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


# (seed parity picks render-space or shifted "local" vertices: DevScene::tri_shift)
@pytest.mark.parametrize("seed,n_tris,w,h", [(1, 600, 1920, 1080), (2, 600, 1920, 1080), (3, 300, 64, 48), (4, 300, 9, 8), (5, 40, 16, 16), (6, 1500, 4096, 4096)])
def test_every_triangle_a_camera_ray_hits_is_in_its_rectangles_list(checker, seed, n_tris, w, h):
    r = checker(seed, n_tris, w, h)
    assert r["rects"] == 50 and r["rays"] > 5000
    assert r["hits"] > 100                      # the brute force found something to compare
    assert r["unused_slots"] > 0                # nodes with fewer than four children were walked
    assert r["behind_lists"] > 0                # boxes behind the camera were culled by the fifth plane alone
    assert 0 < r["longest"] < n_tris            # and the lists are lists, not the scene


def test_the_walk_is_clean_under_address_and_undefined_behaviour_sanitizers(checker_sanitized):
    r = checker_sanitized(7, 300, 1920, 1080)
    assert r["hits"] > 100
    r = checker_sanitized(8, 200, 9, 8)
    assert r["rays"] > 1000


# ---- the lowered scene 3 through the debug entry point ----
W, H = 1920, 1080


@pytest.fixture(scope="module")
def scene3(pkg):
    prod = pkg.Product()
    sc = prod.new_scene()
    cam = pkg.scenes.load_scene(sc, 3, W, H, tex_size=128, build=False)
    counts, over, idx, tris = sc.debug_camera_candidates(cam, np.zeros((0, 4), np.uint32), cap=16, want_tris=True)
    tris = tris.astype(np.float64)
    tris.setflags(write=False)
    return sc, cam, tris


def camera_dirs(cam, fx, fy):
    """regen_path's direction through continuous pixel coordinates (float64: the brute force is the geometry, not the kernel's rounding)"""
    f = np.array(list(cam.direction), np.float64); f /= np.linalg.norm(f)
    up = np.array(list(cam.up), np.float64); up /= np.linalg.norm(up)
    s = np.cross(f, up); s /= np.linalg.norm(s)
    u = np.cross(s, f)
    t = np.tan(np.radians(cam.fov_deg) / 2.0)
    dx = (2.0 * fx / cam.width - 1.0) * (cam.width / cam.height) * t
    dy = (1.0 - 2.0 * fy / cam.height) * t
    d = s[None, :] * dx[:, None] + u[None, :] * dy[:, None] + f[None, :]
    return d / np.linalg.norm(d, axis=1)[:, None]


def brute_force_hits(tris, dirs):
    """(n_rays, n_tris) bool: the ray from the origin along dirs[r] crosses triangle t (Moeller-Trumbore in float64, edges included)"""
    p0, e1, e2 = tris[:, 0], tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]
    out = np.zeros((dirs.shape[0], tris.shape[0]), bool)
    for r, d in enumerate(dirs):
        pv = np.cross(d[None, :], e2)
        det = np.einsum("ij,ij->i", e1, pv)
        ok = np.abs(det) > 0.0
        inv = np.where(ok, 1.0 / np.where(ok, det, 1.0), 0.0)
        tv = -p0
        bu = np.einsum("ij,ij->i", tv, pv) * inv
        qv = np.cross(tv, e1)
        bv = (qv @ d) * inv
        t = np.einsum("ij,ij->i", e2, qv) * inv
        out[r] = ok & (bu >= 0.0) & (bv >= 0.0) & (bu + bv <= 1.0) & (t > 0.0)
    return out


def block_rays(x0, y0, bs=2):
    """continuous pixel coordinates of rays through a bs x bs block: its corners, its edges and its interior (pixel corners and centres)"""
    g = np.linspace(0.0, float(bs), 2 * bs + 1)
    fx, fy = np.meshgrid(x0 + g, y0 + g)
    return fx.ravel(), fy.ravel()


def check_tiles(sc, cam, tris, tiles):
    rects = np.array([(tx * 8 + bx, ty * 8 + by, tx * 8 + bx + 1, ty * 8 + by + 1) for tx, ty in tiles for by in range(0, 8, 2) for bx in range(0, 8, 2)], np.uint32)
    counts, over, idx = sc.debug_camera_candidates(cam, rects, cap=4096)
    assert not over.any()
    n_hit_pairs = 0
    for r, (x0, y0, _, _) in enumerate(rects):
        fx, fy = block_rays(float(x0), float(y0))
        hit = brute_force_hits(tris, camera_dirs(cam, fx, fy)).any(axis=0)
        listed = np.zeros(tris.shape[0], bool)
        listed[idx[r, :counts[r]]] = True
        assert len(set(idx[r, :counts[r]].tolist())) == counts[r]
        missing = np.flatnonzero(hit & ~listed)
        assert missing.size == 0, f"block at ({x0}, {y0}): triangles {missing[:8]} are hit but not in the list of {counts[r]}"
        n_hit_pairs += int(hit.sum())
    return counts, n_hit_pairs


def test_scene3_blocks_of_the_eight_tiles_through_the_frame_centre(scene3):
    sc, cam, tris = scene3
    tiles = [(W // 16 - 4 + i, H // 16) for i in range(8)]
    counts, n = check_tiles(sc, cam, tris, tiles)
    assert n >= len(tiles) * 16                  # every block's rays hit something (the room is closed)
    assert counts.min() >= 1


def test_scene3_blocks_of_tiles_on_the_heros_silhouette(scene3):
    sc, cam, tris = scene3
    # a tile is on the silhouette when the closest hits of its corner and centre rays lie on both the hero (small triangles) and the room
    # (large ones): scan the tile row through the frame centre and the row a quarter of the frame above it
    area = 0.5 * np.linalg.norm(np.cross(tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]), axis=1)
    small = area < 0.25 * np.median(np.sort(area)[-16:])         # (the room's dozen walls are the largest triangles by far)
    found = []
    for ty in (H // 16, H // 16 - H // 64, H // 16 + H // 64):
        for tx in range(W // 16 - 40, W // 16 + 40):
            fx = np.array([tx * 8 + 0.5, tx * 8 + 7.5, tx * 8 + 0.5, tx * 8 + 7.5, tx * 8 + 4.0])
            fy = np.array([ty * 8 + 0.5, ty * 8 + 0.5, ty * 8 + 7.5, ty * 8 + 7.5, ty * 8 + 4.0])
            d = camera_dirs(cam, fx, fy)
            hit = brute_force_hits(tris, d)
            # closest hit per ray: the distance along the ray of each crossed triangle's plane
            n = np.cross(tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0])
            t = np.einsum("ij,ij->i", tris[:, 0], n)[None, :] / np.where(hit, d @ n.T, 1.0)
            first = np.where(hit, t, np.inf).argmin(axis=1)
            kinds = small[first]
            if kinds.any() and not kinds.all():
                found.append((tx, ty))
        if len(found) >= 8:
            break
    assert len(found) >= 8, found
    counts, n = check_tiles(sc, cam, tris, found[:8])
    assert counts.max() >= 3
