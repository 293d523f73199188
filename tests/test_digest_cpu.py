"""The frame digest's host implementation (vpcc_digest_points / vpcc_digest_frame_planes) against its numpy restatement —
no GPU needed."""
import numpy as np
import pytest

import cases
import digest_ref
import oracle_binding as ob
from tmc2rs import recon


def _padded(rng, h, w, hi, pad):
    """An (h, w) u16/u8 plane; with pad > 0 a view into wider rows (stride above the width)."""
    dtype = np.uint8 if hi <= 256 else np.uint16
    full = rng.randint(0, hi, size=(h, w + pad)).astype(dtype)
    return full[:, :w] if pad else full


def _random_frame(seed, W, H, prec, maps, attr, pad):
    rng = np.random.RandomState(seed)
    oh, ow = (H + prec - 1) // prec, (W + prec - 1) // prec
    return {"width": W, "height": H, "occupancy_resolution": 16, "occupancy_precision": prec, "map_count": maps,
            "absolute_d1": 1, "attribute_count": 1 if attr else 0, "flags": 0, "patches": cases._tiny_frame([], np.ones((1, 1)))["patches"],
            "occupancy": _padded(rng, oh, ow, 256, pad),
            "geometry": [_padded(rng, H, W, 1024, pad) for _ in range(maps)],
            "attribute": [(_padded(rng, H, W, 1024, pad), _padded(rng, H // 2, W // 2, 1024, pad + 3),
                           _padded(rng, H // 2, W // 2, 1024, pad + 3)) for _ in range(maps)] if attr else []}


@pytest.mark.parametrize("name", sorted(cases.PARITY_CASES))
def test_parity_case_digests(name):
    f = cases.PARITY_CASES[name]()
    assert recon.digest_planes(f) == digest_ref.digest_planes(f)
    st, r = ob.reconstruct(f)
    assert st == 0
    xyz, rgb = ob.xyz_array(r), ob.rgb_array(r)
    assert recon.digest_points(xyz, rgb) == digest_ref.digest_points(xyz, rgb)
    assert recon.digest_points(xyz) == digest_ref.digest_points(xyz)


@pytest.mark.parametrize("W,H", [(33, 17), (64, 30), (47, 9), (1, 1), (130, 66)])
@pytest.mark.parametrize("prec", [1, 2, 3, 4, 5, 6, 7, 8])
def test_random_frames(W, H, prec):
    for maps in (1, 2):
        for attr in (False, True):
            for pad in (0, 5):
                f = _random_frame(W * 1000 + H * 10 + prec + 97 * maps + 31 * attr + pad, W, H, prec, maps, attr, pad)
                assert recon.digest_planes(f) == digest_ref.digest_planes(f), (maps, attr, pad)


@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 5, 7, 8, 9, 1000, 4099])
def test_points(n):
    rng = np.random.RandomState(n)
    xyz = rng.randint(0, 65536, size=(n, 3)).astype(np.uint16)
    rgb = rng.randint(0, 256, size=(n, 3)).astype(np.uint8)
    assert recon.digest_points(xyz, rgb) == digest_ref.digest_points(xyz, rgb)
    assert recon.digest_points(xyz, None) == digest_ref.digest_points(xyz, None)
    if n:
        assert recon.digest_points(xyz, None) != recon.digest_points(xyz, rgb)


def test_empty_frame_is_its_head():
    assert recon.digest_points(np.zeros((0, 3), np.uint16)) == int(digest_ref.mix64(np.uint64(digest_ref.G)))
    assert recon.digest_points(np.zeros((0, 3), np.uint16), np.zeros((0, 3), np.uint8)) == recon.digest_points(np.zeros((0, 3), np.uint16))


def test_every_flipped_byte_changes_the_digest():
    rng = np.random.RandomState(3)
    xyz = rng.randint(0, 65536, size=(37, 3)).astype(np.uint16)
    rgb = rng.randint(0, 256, size=(37, 3)).astype(np.uint8)
    base = recon.digest_points(xyz, rgb)
    for arr in (xyz, rgb):
        raw = arr.view(np.uint8).reshape(-1)
        for i in range(raw.size):
            raw[i] ^= 1
            assert recon.digest_points(xyz, rgb) != base, i
            raw[i] ^= 1
    assert recon.digest_points(xyz, rgb) == base
    f = cases.PARITY_CASES["small0"]()
    pb = recon.digest_planes(f)
    for plane in (f["occupancy"], f["geometry"][1], f["attribute"][0][2]):
        plane.reshape(-1)[plane.size // 2] ^= 1
        assert recon.digest_planes(f) != pb
        plane.reshape(-1)[plane.size // 2] ^= 1
    assert recon.digest_planes(f) == pb


def test_swapped_points_change_the_digest():
    rng = np.random.RandomState(4)
    xyz = rng.randint(0, 65536, size=(50, 3)).astype(np.uint16)
    rgb = rng.randint(0, 256, size=(50, 3)).astype(np.uint8)
    base = recon.digest_points(xyz, rgb)
    for i, j in [(0, 1), (3, 40), (48, 49)]:
        x2, c2 = xyz.copy(), rgb.copy()
        x2[[i, j]], c2[[i, j]] = x2[[j, i]], c2[[j, i]]
        assert recon.digest_points(x2, c2) != base
        assert recon.digest_points(x2, rgb) != base


def test_stride_padding_is_not_hashed():
    f = _random_frame(11, 33, 17, 4, 2, True, 6)
    d = recon.digest_planes(f)
    f["geometry"][0].base[:, 33:] ^= 0x55                   # the padding behind each row
    assert recon.digest_planes(f) == d
