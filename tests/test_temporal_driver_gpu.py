"""The first-frame rule of the one driver behind the mi355pt_temporal_accumulate* entry points (csrc/api_temporal.cpp): without a previous
frame every device form — rectified or not, whatever carries the hits back — is the plain first-frame instance of temporal_kernel, and a scratch stays
as it is.  The forms with a previous frame are held to the restatements by tests/test_temporal_gpu.py, test_temporal_rectify_gpu.py,
test_motion_gpu.py and test_flow_gpu.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_reference as fr  # noqa: E402
import motion_reference as mr  # noqa: E402
import temporal_reference as tr  # noqa: E402
from test_temporal_rectify_gpu import Device, bits, ffi_params, ffi_rectify  # noqa: E402

pytestmark = pytest.mark.gpu
N_ENTRIES = 3


@pytest.fixture(scope="module")
def dev(product, pkg):
    return Device(product, pkg)


@pytest.mark.parametrize("half", [True, False], ids=["half", "nohalf"])
@pytest.mark.parametrize("shape", [(70, 50), (1, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_first_frame_is_the_plain_kernel_in_every_device_form(dev, shape, half):
    """prev and view NULL, valid ids and a valid table or valid records, ids_prev NULL: all three outputs of each of the six _device forms
    are bit-equal to mi355pt_temporal_accumulate_device's on the same device buffers (70 x 50: a ragged last block in both directions), and
    the rectified forms leave their scratch, pre-filled with the byte 0x5a, unchanged."""
    w, h = shape
    torch, product = dev.torch, dev.product
    cur, _, vw, spp = tr.synthetic(w, h, "move", "step", half)
    dc = dev.up(cur)
    want = [x.cpu().numpy() if x is not None else None for x in dev.run_device(dc, spp, None, None, rectified=False)]
    assert not any(np.isnan(x).any() for x in want if x is not None)

    ids = torch.from_numpy(np.ascontiguousarray(mr.synthetic_ids(w, h)[0], dtype=np.uint32).view(np.int32)).cuda()      # 0 .. 4: some beyond the table
    table = torch.from_numpy(mr.static_table(vw, N_ENTRIES)).cuda()
    records = np.ascontiguousarray(fr.synthetic_flow(w, h, vw, big=True), dtype=fr.FLOW_PIXEL)
    flow = torch.from_numpy(records.view(np.int32).reshape(h, w, 8)).cuda()
    ptrs = {k: v.data_ptr() for k, v in dc.items()}
    prm, rprm = ffi_params(product, None), ffi_rectify(product, None)

    for carry in ("none", "table", "flow"):
        for rectified in (False, True):
            if carry == "none" and not rectified:
                continue                                           # the call `want` came from
            of, oh, ol = dev.outputs(w, h, half)
            scratch = dev.scratch(w, h)
            outs = (of.data_ptr(), oh.data_ptr() if oh is not None else None, ol.data_ptr())
            rect = dict(rectify_params=rprm, d_scratch_ptr=scratch.data_ptr(), scratch_bytes=scratch.numel()) if rectified else {}
            head = (ptrs, spp, None, None, w, h, prm)
            if carry == "none":
                product.temporal_accumulate_rectified_device(*head, rprm, scratch.data_ptr(), scratch.numel(), *outs)
            elif carry == "table":
                product.temporal_accumulate_motion_device(*head, ids.data_ptr(), None, table.data_ptr(), N_ENTRIES, *outs, **rect)
            else:
                product.temporal_accumulate_flow_device(*head, ids.data_ptr(), None, flow.data_ptr(), *outs, **rect)
            torch.cuda.synchronize()
            for name, g, wv in zip(("film", "half", "length"), (of, oh, ol), want):
                assert (g is None) == (wv is None), (carry, rectified, name)
                if g is not None:
                    g = g.cpu().numpy()
                    assert np.array_equal(bits(g), bits(wv)), (carry, rectified, name, int((bits(g) != bits(wv)).sum()))
            assert bool((scratch == 0x5a).all()), (carry, rectified, "the scratch was written")
