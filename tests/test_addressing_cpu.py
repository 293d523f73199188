"""The general sequence's unit bound (include/vpcc_recon.h, vpcc_frame_validate): a frame whose general-sequence unit count —
virtual blocks x ceil(R^2 / 256) for R >= 16, by either kernel's formula — is above 2^31 is refused with VPCC_ERR_UNSUPPORTED,
because the kernels count units and groups in 32 bits.  Validation reads descriptors and patch tables, never a plane sample
(validate_frame checks plane pointers, sizes and strides only), so small buffers stand behind the 32768 x 32768 canvases
declared here.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

from tmc2rs import _abi

SIDE = 32768
UNIT_BOUND = 1 << 31


def _validate(desc):
    return _abi.load_library().vpcc_frame_validate(C.byref(desc))


def _patch(u0, v0, su, sv):
    p = np.zeros((), dtype=_abi.PATCH_DTYPE)
    p["u0"], p["v0"], p["size_u0"], p["size_v0"] = u0, v0, su, sv
    p["lod_x"] = p["lod_y"] = 1
    p["normal_axis"], p["tangent_axis"], p["bitangent_axis"] = 0, 2, 1
    return p


def _frame_desc(R, patches, precision=4):
    """A SIDE x SIDE canvas with occupancy precision 4, two maps and an attribute: every plane pointer is a 16-element
    buffer (never read), every declared size covers the canvas."""
    keep = [np.zeros(16, np.uint16), np.ascontiguousarray(np.array(patches, dtype=_abi.PATCH_DTYPE))]
    buf = keep[0].ctypes.data
    d = _abi.FrameDesc()
    d.width = d.height = SIDE
    d.occupancy_resolution, d.occupancy_precision = R, precision
    d.map_count, d.absolute_d1, d.attribute_count = 2, 1, 1
    d.occupancy.y, d.occupancy.width, d.occupancy.height = buf, SIDE // precision, SIDE // precision
    d.occupancy.stride = d.occupancy.width
    for m in range(2):
        G, A = d.geometry[m], d.attribute[m]
        G.y, G.width, G.height, G.stride, G.cstride = buf, SIDE, SIDE, SIDE, SIDE // 2
        A.y, A.u, A.v, A.width, A.height, A.stride, A.cstride = buf, buf, buf, SIDE, SIDE, SIDE, SIDE // 2
    d.patches, d.patch_count = keep[1].ctypes.data, len(keep[1])
    return d, keep


def _units(R, n_vblocks):
    return n_vblocks * -(-(R * R) // 256)


def _full_canvas_patches(R, n_vblocks):
    """Overlapping full-canvas patches, then one partial patch, of n_vblocks virtual blocks in all."""
    b = SIDE // R
    full, rest = divmod(n_vblocks, b * b)
    patches = [_patch(0, 0, b, b)] * full
    if rest >= b:
        patches.append(_patch(0, 0, b, rest // b))
    if rest % b:
        patches.append(_patch(0, 0, rest % b, 1))
    assert sum(int(p["size_u0"]) * int(p["size_v0"]) for p in patches) == n_vblocks
    return patches


@pytest.mark.parametrize("R", [32, 64, 128, 256, 512, 32768])
def test_unit_bound_on_each_side(R):
    at_bound = UNIT_BOUND // _units(R, 1)                     # virtual blocks with exactly 2^31 units
    assert _units(R, at_bound) == UNIT_BOUND
    d, keep = _frame_desc(R, _full_canvas_patches(R, at_bound))
    assert _validate(d) == _abi.VPCC_OK
    d, keep = _frame_desc(R, _full_canvas_patches(R, at_bound + 1))
    assert _validate(d) == _abi.VPCC_ERR_UNSUPPORTED


def test_unit_count_that_wraps_32_bits_is_refused():
    """R = 32768: one block per canvas; 1024 overlapping one-block patches are 2^32 units — 0 in 32 bits."""
    R = SIDE
    d, keep = _frame_desc(R, [_patch(0, 0, 1, 1)] * 1024, precision=1)
    assert _units(R, 1024) == 1 << 32
    assert _validate(d) == _abi.VPCC_ERR_UNSUPPORTED


def test_r16_frames_up_to_the_virtual_block_limit_are_accepted():
    """R = 16, the production stream: a unit per virtual block, so the unit bound never binds before the virtual-block
    limit (2^31 - 1) does."""
    d, keep = _frame_desc(16, _full_canvas_patches(16, (1 << 31) - 1))
    assert _validate(d) == _abi.VPCC_OK
    d, keep = _frame_desc(16, _full_canvas_patches(16, 1 << 31))
    assert _validate(d) == _abi.VPCC_ERR_INVALID_ARG           # the virtual-block limit, as before


@pytest.mark.parametrize("R", [1, 8, 15])
def test_small_blocks_pack_into_units(R):
    """R < 16: several virtual blocks share a unit — never more units than virtual blocks."""
    b = min(SIDE // R, 65535)
    n = ((1 << 31) - 1) // (b * b) * (b * b)
    d, keep = _frame_desc(R, _full_canvas_patches(R, n), precision=1)
    assert _validate(d) == _abi.VPCC_OK
