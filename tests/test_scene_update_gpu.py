"""The three in-place updates of a built scene as ONE chain through the device step they share (csrc/scene_update.cpp):
camera move, instance move, deformation, camera move, instance move on scene 3, either builder, the default and the general lowering.
The per-kind tests (tests/test_rebase_gpu.py, test_instance_move_gpu.py, test_deform_gpu.py) hold each update and each PAIR of kinds to
the host's pinned lowering; the chain holds what the kinds share across calls — the buffers the first call of a kind allocates, the
once-per-build sah_built, the cached light records a camera move starts from, the once-per-build index uploads."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import linear_rmse_u8  # noqa: E402
from test_deform import BOX, EMITTER3, Remeshed, deformed  # noqa: E402
from test_deform_gpu import DEFORM_LAUNCHES  # noqa: E402
from test_instance_move import applied, describe, trs  # noqa: E402
from test_instance_move_gpu import MOVE_LAUNCHES, Redescribed  # noqa: E402
from test_rebase import moved  # noqa: E402
from test_rebase_gpu import STEP, heights_of  # noqa: E402

pytestmark = pytest.mark.gpu
CAMERA_LAUNCHES = 2           # positions, the 4-wide tree; + one per node height (include/mi355pt_rebase.h states it)
BOX_I, EMITTER_I = BOX[1], EMITTER3[1]       # one mesh per instance in scene 3: the geom id is the instance id


def bits(x):
    return np.float32(x).tobytes()


@pytest.mark.parametrize("case", ["3", "3:general"])
@pytest.mark.parametrize("builder", ["host", "gpu"])
def test_chain_of_all_three_updates(product, pkg, case, builder):
    """after every link every device array has the digest of the host's pinned lowering of the description as it then stands, the launch
    count is the header's formula for that kind, and sah_built is, bit for bit, what the first instance move found; the film at 1 spp is
    that of a scene DESCRIBED at the final state and built fresh — bit-equal where the two scenes' device digests are equal, else within
    linear_rmse_u8 2e-3, the bar of tests/test_instance_move_gpu.py test_moved_scene_against_a_fresh_build between two trees"""
    dynamic = [BOX_I, EMITTER_I]
    sc, cam = describe(pkg, Remeshed(product), case, dynamic=dynamic, builder=builder)
    sc.build(cam)
    assert f"builder={builder}" in product.scene_info(sc) and "tri_space=render" in product.scene_info(sc)
    nodes, _, root = product.export_bvh(sc)
    heights = heights_of(nodes, root)
    cams = [moved(pkg, cam, STEP, times=k) for k in (1, 2)]
    emitter_1 = applied(trs(), sc.instances[EMITTER_I][2])
    final = {BOX_I: applied(trs((-0.2, 0.1, 0.3), -0.3), sc.instances[BOX_I][2]), EMITTER_I: applied(trs((0.1, 0.0, -0.2), 0.2, (0.9, 1.0, 1.1)), emitter_1)}
    new = {g: deformed(sc.meshes[g]) for g in (BOX_I, EMITTER_I)}
    links = [("camera", lambda: sc.move_camera(cams[0]), cams[0]),
             ("instances", lambda: sc.move_instances(cam_now, [EMITTER_I], [emitter_1]), cams[0]),
             ("deform", lambda: sc.deform_meshes(cam_now, new), cams[0]),
             ("camera", lambda: sc.move_camera(cams[1]), cams[1]),
             ("instances", lambda: sc.move_instances(cam_now, sorted(final), [final[i] for i in sorted(final)]), cams[1])]
    launches = {"camera": CAMERA_LAUNCHES, "instances": MOVE_LAUNCHES, "deform": DEFORM_LAUNCHES}
    cam_now, sah_built = cam, None
    for k, (kind, call, cam_after) in enumerate(links):
        res = call()
        cam_now = cam_after
        assert res["rebuilt"] == 0 and res["reason"] == "rebased", (k, kind, res)
        assert res["launches"] == heights + launches[kind], (k, kind, res)
        got, want = sc.debug_device_digest(), sc.debug_pinned_digest(cam_now)
        assert got == want, (k, kind, [n for n in want[0] if got[0][n] != want[0][n]])
        if kind != "camera":
            sah_built = sah_built or res["sah_built"]
            assert sah_built > 1.0 and bits(res["sah_built"]) == bits(sah_built) and res["sah_after"] > 1.0, (k, kind, res)
    fresh, _ = describe(pkg, Remeshed(Redescribed(product, final), new), case, dynamic=dynamic, builder=builder)
    fresh.build(cam_now)
    da, db = sc.debug_device_digest()[0], fresh.debug_device_digest()[0]
    for name in ("instances", "lights", "light_tris", "light_uvs", "materials", "texels", "rgb2spec"):     # tree-order-free arrays: the same description
        assert da[name] == db[name], name
    prm = pkg.make_params(1, "mis", "sobol")
    img_a, img_b = product.render(sc, cam_now, prm), product.render(fresh, cam_now, prm)
    rmse = linear_rmse_u8(product.quantize_u8(img_a), product.quantize_u8(img_b))
    print(f"chain {case} {builder}: heights={heights} device_digests_equal={da == db} film_bit_equal={np.array_equal(img_a, img_b)} linear_rmse_u8={rmse:.3e}")
    assert img_a.mean() > 0.0
    if da == db:
        assert np.array_equal(img_a, img_b)
    else:
        assert rmse <= 2e-3, rmse
