"""Semi-planar (P010 / P016) video decoder surfaces on the host side — descriptor validation, the plane digest's extended
definition, the synthetic surfaces and the Decoder's video-format switch.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

import cases
import digest_ref
import surface_ref
from tmc2rs import _abi, recon, synth


def _surface(name="medium0", **kw):
    kw.setdefault("junk_seed", 7)
    return synth.to_semiplanar(cases.PARITY_CASES[name](), **kw)


def _desc(frame):
    return _abi.host_frame_desc(frame)


def _validate(desc):
    return _abi.load_library().vpcc_frame_validate(C.byref(desc))


@pytest.mark.parametrize("name", sorted(cases.PARITY_CASES))
def test_validate_accepts_interleaved_and_shifted(name):
    f = _surface(name)
    d, keep = _desc(f)
    if f.get("attribute_count", 1):
        assert d.flags & _abi.VPCC_FRAME_UV_INTERLEAVED and not d.attribute[0].v
    assert (d.flags >> 8) & 15 == 6 and (d.flags >> 12) & 15 == 6
    assert _validate(d) == _abi.VPCC_OK


def test_validate_rejects_bad_surface_descriptors():
    f = _surface()
    d, keep = _desc(f)
    assert _validate(d) == _abi.VPCC_OK
    W = d.width
    # a V plane under the flag
    d2, k2 = _desc(f)
    d2.attribute[1].v = d2.attribute[1].u
    assert _validate(d2) == _abi.VPCC_ERR_INVALID_ARG
    # an interleaved row shorter than the U,V pairs of a row
    d2, k2 = _desc(f)
    d2.attribute[0].cstride = 2 * (W // 2) - 1
    assert _validate(d2) == _abi.VPCC_ERR_INVALID_ARG
    d2.attribute[0].cstride = W // 2                     # (enough for a planar chroma row, not for an interleaved one)
    assert _validate(d2) == _abi.VPCC_ERR_INVALID_ARG
    d2.attribute[0].cstride = 2 * (W // 2)
    assert _validate(d2) == _abi.VPCC_OK
    # shifts above 8
    for bits in (_abi.VPCC_FRAME_GEO_SHIFT(9), _abi.VPCC_FRAME_ATTR_SHIFT(9), _abi.VPCC_FRAME_GEO_SHIFT(15)):
        d2, k2 = _desc(f)
        d2.flags = (d2.flags & ~0xFF00) | bits
        assert _validate(d2) == _abi.VPCC_ERR_INVALID_ARG
    d2, k2 = _desc(f)
    d2.flags = (d2.flags & ~0xFF00) | _abi.VPCC_FRAME_GEO_SHIFT(8) | _abi.VPCC_FRAME_ATTR_SHIFT(0)
    assert _validate(d2) == _abi.VPCC_OK
    # a missing UV plane
    d2, k2 = _desc(f)
    d2.attribute[0].u = None
    assert _validate(d2) == _abi.VPCC_ERR_SHORT_VIDEO
    # the same descriptors without the flag are planar ones with a missing V plane, as before
    d2, k2 = _desc(f)
    d2.flags &= ~_abi.VPCC_FRAME_UV_INTERLEAVED
    assert _validate(d2) == _abi.VPCC_ERR_SHORT_VIDEO


@pytest.mark.parametrize("name", sorted(cases.PARITY_CASES))
def test_planar_frames_validate_as_before(name):
    f = cases.PARITY_CASES[name]()
    d, keep = _desc(f)
    assert d.flags == 0 and _validate(d) == _abi.VPCC_OK


@pytest.mark.parametrize("name", ["medium0", "small2_wide", "strided_planes", "single_map_extension", "no_attribute",
                                  "block8_ragged", "wide_samples"])
@pytest.mark.parametrize("shifts", [(6, 6), (0, 4), (8, 2)])
def test_surface_digest_matches_its_definition(name, shifts):
    f = _surface(name, geo_shift=shifts[0], attr_shift=shifts[1])
    got = recon.digest_planes(f)
    assert got == surface_ref.digest_planes(f)
    planar = cases.PARITY_CASES[name]()
    if f.get("attribute_count", 1) or shifts[0]:
        assert got != digest_ref.digest_planes(planar)
    # one junk bit below the shift changes it: the digest is of the planes as delivered
    if shifts[1] and f.get("attribute_count", 1):
        g = dict(f)
        y, uv = g["attribute"][0]
        uv2 = uv.copy()
        uv2[0, 1] ^= 1                                   # (V of the first pair)
        g["attribute"] = [(y, uv2)] + list(g["attribute"][1:])
        assert recon.digest_planes(g) != got
        assert recon.digest_planes(g) == surface_ref.digest_planes(g)
    if shifts[0]:
        g = dict(f)
        geo = g["geometry"][0].copy()
        geo[0, 0] ^= 1
        g["geometry"] = [geo] + list(g["geometry"][1:])
        assert recon.digest_planes(g) != got


def test_surface_digest_rejects_a_v_plane():
    f = _surface()
    d, keep = _desc(f)
    d.attribute[0].v = d.attribute[0].u
    out = C.c_uint64(0)
    assert _abi.load_library().vpcc_digest_frame_planes(C.byref(d), C.byref(out)) == _abi.VPCC_ERR_INVALID_ARG


@pytest.mark.parametrize("name", sorted(cases.PARITY_CASES))
def test_to_semiplanar_round_trips(name):
    f = cases.PARITY_CASES[name]()
    s = synth.to_semiplanar(f, shift=6, junk_seed=11)
    W, H = f["width"], f["height"]
    for g in s["geometry"]:
        assert g.dtype == np.uint16 and g.shape == (H, W) and g.strides[0] % 256 == 0
    for y, uv in s["attribute"]:
        assert uv.shape == (H // 2, 2 * (W // 2)) and uv.strides[0] % 256 == 0
        # the UV plane does not follow the luma plane directly
        assert uv.ctypes.data != y.ctypes.data + H * y.strides[0]
    back = synth.from_semiplanar(s)
    if f["attribute"] and int(np.max([np.max(p) for a in f["attribute"] for p in a])) >= 1024:
        return                                           # (16-bit samples: cut to 10 bits by the shift)
    for a, b in zip(f["geometry"], back["geometry"]):
        assert np.array_equal(np.asarray(a), b)
    for la, lb in zip(f["attribute"], back["attribute"]):
        for a, b in zip(la, lb):
            assert np.array_equal(np.asarray(a), b)
    assert "geo_shift" not in back and back["flags"] == f["flags"]


def test_to_semiplanar_junk_is_below_the_shift():
    f = cases.medium_frame(0)
    a = synth.to_semiplanar(f, shift=6)
    b = synth.to_semiplanar(f, shift=6, junk_seed=3)
    assert np.all((a["geometry"][0] & 63) == 0)
    assert np.any((b["geometry"][0] & 63) != 0)
    assert np.array_equal(a["geometry"][0] >> 6, b["geometry"][0] >> 6)
    assert np.array_equal(a["attribute"][1][1] >> 6, b["attribute"][1][1] >> 6)


def test_p010_rewrite_of_a_planar_raw_file(tmp_path):
    f = cases.medium_frame(1)
    W, H = f["width"], f["height"]
    src, dst = tmp_path / "a.yuv", tmp_path / "a.p010"
    with open(src, "wb") as o:
        for (y, u, v) in f["attribute"]:
            for p in (y, u, v):
                o.write(np.ascontiguousarray(p, dtype="<u2").tobytes())
    synth.yuv420p10le_to_p010le(src, dst, W, H, junk_seed=5)
    assert dst.stat().st_size == src.stat().st_size
    data = np.fromfile(dst, dtype="<u2")
    per = W * H * 3 // 2
    for k, (y, u, v) in enumerate(f["attribute"]):
        fr = data[k * per:(k + 1) * per]
        assert np.array_equal(fr[:W * H].reshape(H, W) >> 6, y)
        uv = fr[W * H:].reshape(H // 2, W)
        assert np.array_equal(uv[:, 0::2] >> 6, u) and np.array_equal(uv[:, 1::2] >> 6, v)


def test_decoder_set_video_format_is_host_only(tmp_path):
    """On a container-opened decoder, and for an unknown format: VPCC_ERR_INVALID_ARG — before anything touches a GPU."""
    lib = _abi.load_library()
    h = C.c_void_p()
    dev = (C.c_int * 1)(0)
    assert lib.vpcc_decoder_open(str(tmp_path / "x.vpccgof").encode(), dev, 1, C.byref(h)) == 0
    try:
        assert lib.vpcc_decoder_set_video_format(h, _abi.VPCC_VIDEO_P010LE) == _abi.VPCC_ERR_INVALID_ARG
        assert lib.vpcc_decoder_set_video_format(h, _abi.VPCC_VIDEO_YUV420P10LE) == _abi.VPCC_ERR_INVALID_ARG
    finally:
        lib.vpcc_decoder_close(h)
    h = C.c_void_p()
    paths = [str(tmp_path / n).encode() for n in ("s.bin", "occ.yuv", "geo.yuv", "attr.yuv")]
    assert lib.vpcc_decoder_open_v3c(*paths, 4, dev, 1, C.byref(h)) == 0
    try:
        assert lib.vpcc_decoder_set_video_format(h, 2) == _abi.VPCC_ERR_INVALID_ARG
        assert lib.vpcc_decoder_set_video_format(h, -1) == _abi.VPCC_ERR_INVALID_ARG
        assert lib.vpcc_decoder_set_video_format(h, _abi.VPCC_VIDEO_P010LE) == _abi.VPCC_OK
        assert lib.vpcc_decoder_set_video_format(h, _abi.VPCC_VIDEO_YUV420P10LE) == _abi.VPCC_OK
    finally:
        lib.vpcc_decoder_close(h)
    assert lib.vpcc_decoder_set_video_format(None, 0) == _abi.VPCC_ERR_INVALID_ARG
    with pytest.raises(recon.VpccError) as e:
        recon.Decoder(tmp_path / "x.vpccgof", video_format="p010le")
    assert e.value.status == _abi.VPCC_ERR_INVALID_ARG
