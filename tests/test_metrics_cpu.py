"""Cloud metrics without a GPU: the CPU restatement (metrics_ref) against an exhaustive search, the PSNR helper on hand-computed
sums, the ctypes mirror of the new structs, and the argument checks that need no device."""
import ctypes as C
import math

import numpy as np
import pytest

import metrics_ref
from tmc2rs import _abi, recon


def _clouds(seed, n, m, span):
    rng = np.random.RandomState(seed)
    a = rng.randint(0, span, size=(n, 3)).astype(np.uint16)
    b = rng.randint(0, span, size=(m, 3)).astype(np.uint16)
    b[: m // 4] = b[m // 4: 2 * (m // 4)]               # duplicate positions in the target
    return a, b


@pytest.mark.parametrize("seed,n,m,span", [(1, 300, 200, 8), (2, 500, 50, 4), (3, 200, 400, 64), (4, 100, 7, 2),
                                            (5, 50, 300, 65536)])
def test_restatement_equals_exhaustive_search(seed, n, m, span):
    a, b = _clouds(seed, n, m, span)
    idx, d2 = metrics_ref.nearest(a, b)
    bidx, bd2 = metrics_ref.nearest_brute(a, b)
    assert np.array_equal(d2, bd2)
    assert np.array_equal(idx, bidx)


def test_ties_go_to_the_smallest_index():
    # the source point (10, 10, 10) has six targets at d² = 1 and duplicates of them; index 3 is the first of them
    t = np.array([[20, 20, 20], [10, 10, 12], [0, 0, 0], [10, 11, 10], [9, 10, 10], [10, 10, 11], [10, 11, 10], [11, 10, 10]],
                 np.uint16)
    s = np.array([[10, 10, 10], [10, 11, 10], [10, 10, 13]], np.uint16)
    idx, d2 = metrics_ref.nearest(s, t)
    assert list(idx) == [3, 3, 1] and list(d2) == [1, 0, 1]
    # more equidistant candidates than the k-d tree is asked for
    ring = np.array([[5 + dx, 5 + dy, 5 + dz] for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)
                     if abs(dx) + abs(dy) + abs(dz) == 2], np.uint16)[::-1]
    idx, d2 = metrics_ref.nearest(np.array([[5, 5, 5]], np.uint16), np.concatenate([ring, ring]))
    assert idx[0] == 0 and d2[0] == 2


def test_direction_sums_by_hand():
    s_xyz = np.array([[0, 0, 0], [5, 0, 0]], np.uint16)
    t_xyz = np.array([[1, 0, 0], [5, 0, 2]], np.uint16)
    s_rgb = np.array([[10, 20, 30], [0, 0, 0]], np.uint8)
    t_rgb = np.array([[12, 20, 27], [255, 0, 1]], np.uint8)
    d = metrics_ref.direction(s_xyz, s_rgb, t_xyz, t_rgb)
    assert d["geo_sse"] == 1 + 4 and d["geo_max"] == 4
    assert d["rgb_sse"] == [4 + 255 ** 2, 0, 9 + 1]
    y0 = 0.2126 * -2 + 0.7152 * 0 + 0.0722 * 3
    y1 = 0.2126 * -255 + 0.7152 * 0 + 0.0722 * -1
    assert d["ycc_sse"][0] == y0 * y0 + y1 * y1
    # duplicate positions with different colours: the first index supplies the colour
    t_xyz2 = np.array([[0, 0, 0], [0, 0, 0]], np.uint16)
    d = metrics_ref.direction(s_xyz[:1], s_rgb[:1], t_xyz2, np.array([[10, 20, 31], [10, 20, 30]], np.uint8))
    assert d["rgb_sse"] == [0, 0, 1]


def test_empty_sides():
    e = np.zeros((0, 3), np.uint16)
    a = np.array([[1, 2, 3]], np.uint16)
    d = metrics_ref.direction(a, None, e, None)
    assert d["n_tgt"] == 0 and d["geo_sse"] == 0 and d["geo_max"] == 0
    idx, d2 = metrics_ref.nearest(a, e)
    assert idx[0] == 0xFFFFFFFF and d2[0] == np.iinfo(np.uint64).max


def _dir(n_src, n_tgt, sse, mx=0, rgb=(0, 0, 0), ycc=(0.0, 0.0, 0.0), colour=True):
    return {"n_src": n_src, "n_tgt": n_tgt, "has_color": colour, "geo_sse": sse, "geo_max": mx, "rgb_sse": list(rgb),
            "ycc_sse": list(ycc)}


def test_psnr_helper():
    ab = _dir(100, 50, 300, 9, rgb=(100, 0, 400), ycc=(50.0, 0.0, 0.0))
    ba = _dir(50, 100, 200, 16, rgb=(50, 0, 100), ycc=(100.0, 0.0, 0.0))
    p = recon.psnr(ab, ba, 1023)
    assert p["d1_mse"] == 4.0                            # max(300 / 100, 200 / 50)
    assert p["d1_psnr"] == pytest.approx(10 * math.log10(3 * 1023 ** 2 / 4.0))
    assert p["hausdorff2"] == 16
    assert p["rgb_mse"] == [1.0, 0.0, 4.0]
    assert p["rgb_psnr"][0] == pytest.approx(10 * math.log10(255 ** 2))
    assert p["rgb_psnr"][1] == math.inf
    assert p["ycc_mse"][0] == 2.0
    # identical clouds: +inf; a direction without terms: NaN
    z = recon.psnr(_dir(10, 10, 0), _dir(10, 10, 0), 1023)
    assert z["d1_psnr"] == math.inf and z["ycc_psnr"] == [math.inf] * 3
    e = recon.psnr(_dir(10, 0, 0), _dir(0, 10, 0), 1023)
    assert math.isnan(e["d1_mse"]) and math.isnan(e["d1_psnr"])
    nc = recon.psnr(_dir(10, 10, 5, colour=False), _dir(10, 10, 5), 255)
    assert nc["d1_mse"] == 0.5 and all(math.isnan(v) for v in nc["rgb_psnr"] + nc["ycc_psnr"])


def test_struct_layout_of_the_metrics():
    assert C.sizeof(_abi.Cloud) == 24
    assert C.sizeof(_abi.CloudErrors) == 80
    assert _abi.CloudErrors.geo_sse.offset == 16 and _abi.CloudErrors.rgb_sse.offset == 32
    assert _abi.CloudErrors.ycc_sse.offset == 56


def test_null_arguments_are_refused_without_a_device():
    lib = _abi.load_library()
    cl = _abi.Cloud()
    err = (_abi.CloudErrors * 1)()
    assert lib.vpcc_cloud_errors_compute(None, C.byref(cl), C.byref(cl), 1, _abi.VPCC_MEM_HOST, err, err) == _abi.VPCC_ERR_INVALID_ARG
    assert lib.vpcc_cloud_nearest(None, C.byref(cl), C.byref(cl), _abi.VPCC_MEM_HOST, None, None) == _abi.VPCC_ERR_INVALID_ARG
    assert lib.vpcc_gof_cloud_errors(None, 0, 1, C.byref(cl), _abi.VPCC_MEM_HOST, err, err) == _abi.VPCC_ERR_INVALID_ARG


def test_perturbation_is_seeded():
    rng = np.random.RandomState(0)
    xyz = rng.randint(0, 1024, size=(1000, 3)).astype(np.uint16)
    rgb = rng.randint(0, 256, size=(1000, 3)).astype(np.uint8)
    a, b = metrics_ref.perturb(xyz, rgb, 7), metrics_ref.perturb(xyz, rgb, 7)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert 980 <= len(a[0]) <= 1020
