"""Cloud metrics on the GPU (vpcc_cloud_errors_compute, vpcc_cloud_nearest, vpcc_gof_cloud_errors: vpcc_metrics.hip) against the
CPU restatement (metrics_ref): integer sums, geo_max and the per-point correspondence exactly, the YCbCr sums to 1e-10."""
import ctypes as C

import numpy as np
import pytest

import metrics_ref
import oracle_binding as ob
from tmc2rs import _abi, recon, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = recon.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def longdress():
    st, r = ob.reconstruct(synth.longdress_frame(3))
    assert st == 0
    xyz, rgb = ob.xyz_array(r), ob.rgb_array(r)
    pxyz, prgb = metrics_ref.perturb(xyz, rgb, 0x3E7)
    return xyz, rgb, pxyz, prgb


def _same_direction(got, ref):
    for k in ("n_src", "n_tgt", "has_color", "geo_sse", "geo_max", "rgb_sse"):
        assert got[k] == ref[k], (k, got[k], ref[k])
    for g, r in zip(got["ycc_sse"], ref["ycc_sse"]):
        assert g == pytest.approx(r, rel=1e-10, abs=0)


def _same_pair(got, ref):
    _same_direction(got["ab"], ref["ab"])
    _same_direction(got["ba"], ref["ba"])


def _same_nearest(ctx, s, t):
    idx, d2 = ctx.cloud_nearest(s, t)
    ridx, rd2 = metrics_ref.nearest(s, t)
    assert np.array_equal(d2, rd2)
    assert np.array_equal(idx, ridx)


def _device(xyz, rgb=None):
    import torch
    x = torch.from_numpy(np.ascontiguousarray(xyz, np.uint16).view(np.int16)).cuda()
    return (x, None if rgb is None else torch.from_numpy(np.ascontiguousarray(rgb, np.uint8)).cuda())


def test_identical_clouds(ctx, longdress):
    xyz, rgb = longdress[0], longdress[1]
    got = ctx.cloud_errors((xyz, rgb), (xyz, rgb), peak=1023)
    _same_pair(got, metrics_ref.pair(xyz, rgb, xyz, rgb))
    assert got["ab"]["geo_sse"] == 0 and got["ab"]["geo_max"] == 0 and got["d1_psnr"] == float("inf")
    idx, d2 = ctx.cloud_nearest(xyz, xyz)
    assert not d2.any()
    # each index is the first point at the same position (reconstructed frames repeat positions across patches)
    key = (xyz[:, 0].astype(np.int64) << 32) | (xyz[:, 1].astype(np.int64) << 16) | xyz[:, 2]
    _, first, inv = np.unique(key, return_index=True, return_inverse=True)
    assert np.array_equal(idx, first[inv])


def test_longdress_against_a_perturbation(ctx, longdress):
    xyz, rgb, pxyz, prgb = longdress
    got = ctx.cloud_errors((xyz, rgb), (pxyz, prgb), peak=1023)
    _same_pair(got, metrics_ref.pair(xyz, rgb, pxyz, prgb))
    assert got["ab"]["geo_sse"] > 0 and got["ba"]["geo_max"] > 0
    _same_nearest(ctx, xyz, pxyz)
    _same_nearest(ctx, pxyz, xyz)


def test_ties_and_duplicates(ctx):
    t = np.array([[20, 20, 20], [10, 10, 12], [0, 0, 0], [10, 11, 10], [9, 10, 10], [10, 10, 11], [10, 11, 10], [11, 10, 10]],
                 np.uint16)
    s = np.array([[10, 10, 10], [10, 11, 10], [10, 10, 13]], np.uint16)
    idx, d2 = ctx.cloud_nearest(s, t)
    assert list(idx) == [3, 3, 1] and list(d2) == [1, 0, 1]
    rng = np.random.RandomState(11)
    for span, n, m in ((4, 3000, 2000), (16, 5000, 800), (3, 200, 5000)):
        a = rng.randint(0, span, size=(n, 3)).astype(np.uint16)
        b = rng.randint(0, span, size=(m, 3)).astype(np.uint16)
        _same_nearest(ctx, a, b)
        ca = rng.randint(0, 256, size=(n, 3)).astype(np.uint8)
        cb = rng.randint(0, 256, size=(m, 3)).astype(np.uint8)
        _same_pair(ctx.cloud_errors((a, ca), (b, cb)), metrics_ref.pair(a, ca, b, cb))


def test_far_outliers_and_the_whole_range(ctx):
    rng = np.random.RandomState(5)
    cluster = (1000 + rng.randint(-40, 41, size=(20000, 3))).astype(np.uint16)
    src = np.concatenate([np.array([[0, 0, 0], [65535, 65535, 65535], [0, 65535, 1000], [1000, 1000, 1000]], np.uint16),
                          rng.randint(0, 65536, size=(500, 3)).astype(np.uint16)])
    _same_nearest(ctx, src, cluster)
    _same_pair(ctx.cloud_errors(src, cluster), metrics_ref.pair(src, None, cluster, None))
    sparse_a = rng.randint(0, 65536, size=(30000, 3)).astype(np.uint16)
    sparse_b = rng.randint(0, 65536, size=(20000, 3)).astype(np.uint16)
    _same_nearest(ctx, sparse_a, sparse_b)
    got = ctx.cloud_errors(sparse_a, sparse_b)
    _same_pair(got, metrics_ref.pair(sparse_a, None, sparse_b, None))
    assert got["ab"]["geo_max"] > 2 ** 32 // 4096           # large distances stay exact
    corners = np.array([[0, 0, 0], [65535, 65535, 65535]], np.uint16)
    got = ctx.cloud_errors(corners[:1], corners[1:])
    assert got["ab"]["geo_max"] == 3 * 65535 ** 2 and got["ab"]["geo_sse"] == 3 * 65535 ** 2


def _batch(rng):
    pairs = []
    for n, m in ((5000, 7000), (0, 300), (400, 0), (1, 1), (20000, 3000), (0, 0), (3, 50000)):
        a = rng.randint(0, 512, size=(n, 3)).astype(np.uint16)
        b = rng.randint(0, 512, size=(m, 3)).astype(np.uint16)
        ca = rng.randint(0, 256, size=(n, 3)).astype(np.uint8)
        cb = rng.randint(0, 256, size=(m, 3)).astype(np.uint8)
        pairs.append(((a, ca), (b, cb)))
    pairs.append(((pairs[0][0][0], None), pairs[0][1]))     # one side without colours
    return pairs


def test_batch_of_mixed_sizes_and_empty_sides(ctx):
    pairs = _batch(np.random.RandomState(21))
    got = ctx.cloud_errors([p[0] for p in pairs], [p[1] for p in pairs], peak=511)
    for g, (a, b) in zip(got, pairs):
        _same_pair(g, metrics_ref.pair(a[0], a[1], b[0], b[1]))
    assert got[1]["ab"]["n_src"] == 0 and got[2]["ab"]["n_tgt"] == 0
    assert np.isnan(got[2]["d1_psnr"]) and not got[-1]["ab"]["has_color"]
    idx, d2 = ctx.cloud_nearest(pairs[2][0][0], pairs[2][1][0])
    assert (idx == 0xFFFFFFFF).all() and (d2 == np.iinfo(np.uint64).max).all()


def test_host_and_device_memory_agree(ctx, longdress):
    xyz, rgb, pxyz, prgb = longdress
    host = ctx.cloud_errors((xyz, rgb), (pxyz, prgb))
    dev = ctx.cloud_errors(_device(xyz, rgb), _device(pxyz, prgb))
    assert dev == host
    idx, d2 = ctx.cloud_nearest(_device(xyz), _device(pxyz))
    hidx, hd2 = ctx.cloud_nearest(xyz, pxyz)
    assert np.array_equal(idx.cpu().numpy(), hidx.astype(np.int64))
    assert np.array_equal(d2.cpu().numpy().view(np.uint64), hd2)


def test_forced_chunking_equals_one_pass(ctx, monkeypatch):
    pairs = _batch(np.random.RandomState(33))
    a, b = [p[0] for p in pairs], [p[1] for p in pairs]
    one = ctx.cloud_errors(a, b)
    monkeypatch.setenv("VPCC_METRICS_SCRATCH_LIMIT_MB", "1")      # about one pair per chunk
    assert ctx.cloud_errors(a, b) == one                            # the doubles bit for bit


def test_two_runs_give_identical_doubles(ctx, longdress):
    xyz, rgb, pxyz, prgb = longdress
    r1 = ctx.cloud_errors((xyz, rgb), (pxyz, prgb))
    r2 = ctx.cloud_errors((xyz, rgb), (pxyz, prgb))
    assert r1 == r2
    assert [np.float64(v).tobytes() for v in r1["ab"]["ycc_sse"]] == [np.float64(v).tobytes() for v in r2["ab"]["ycc_sse"]]


def test_gof_cloud_errors_after_reconstruct_and_smooth(ctx):
    frames = [synth.longdress_frame(i) for i in range(3)]
    g = ctx.gof(frames, flags=_abi.VPCC_GOF_WANT_PATCH_INDEX)
    with pytest.raises(recon.VpccError) as e:
        g.cloud_errors([np.zeros((1, 3), np.uint16)] * 3)
    assert e.value.status == _abi.VPCC_ERR_STATE
    g.reconstruct()
    outs = [g.download(i) for i in range(3)]
    refs = [metrics_ref.perturb(o["xyz"], o["rgb"], 100 + i) for i, o in enumerate(outs)]
    got = g.cloud_errors(refs, peak=1023)
    want = ctx.cloud_errors([(o["xyz"], o["rgb"]) for o in outs], refs, peak=1023)
    assert got == want
    _same_pair(got[1], metrics_ref.pair(outs[1]["xyz"], outs[1]["rgb"], refs[1][0], refs[1][1]))
    # the unsmoothed outputs as the reference of the smoothed ones: behind the smoothing, on the device
    g.smooth(10, grid_size=8, threshold=4)
    smoothed = [g.download(i) for i in range(3)]
    got = g.cloud_errors([(o["xyz"], o["rgb"]) for o in outs], first=0, count=3, peak=1023)
    want = ctx.cloud_errors([(o["xyz"], o["rgb"]) for o in smoothed], [(o["xyz"], o["rgb"]) for o in outs], peak=1023)
    assert got == want
    assert any(r["ab"]["geo_sse"] > 0 for r in got)                 # the smoothing moved points
    assert g.cloud_errors(refs[1:2], first=1, count=1) == [ctx.cloud_errors((smoothed[1]["xyz"], smoothed[1]["rgb"]), refs[1])]
    g.close()


def test_refusals(ctx):
    lib = _abi.load_library()
    big = _abi.Cloud()
    big.xyz, big.n = 1, 1431655766                 # never read: refused before any device work
    small = _abi.Cloud()
    err = (_abi.CloudErrors * 1)()
    st = lib.vpcc_cloud_errors_compute(ctx.h, C.byref(big), C.byref(small), 1, _abi.VPCC_MEM_DEVICE, err, err)
    assert st == _abi.VPCC_ERR_UNSUPPORTED
    assert lib.vpcc_cloud_nearest(ctx.h, C.byref(big), C.byref(small), _abi.VPCC_MEM_DEVICE, None, None) == _abi.VPCC_ERR_UNSUPPORTED
    bad = _abi.Cloud()
    bad.n = 5                                       # points without positions
    assert lib.vpcc_cloud_errors_compute(ctx.h, C.byref(bad), C.byref(small), 1, _abi.VPCC_MEM_HOST, err, err) == \
        _abi.VPCC_ERR_INVALID_ARG


def test_owlii_pair(ctx):
    st, r = ob.reconstruct(synth.owlii_frame(2))
    assert st == 0
    xyz, rgb = ob.xyz_array(r), ob.rgb_array(r)
    assert len(xyz) > 1_800_000
    pxyz, prgb = metrics_ref.perturb(xyz, rgb, 0x0111)
    _same_pair(ctx.cloud_errors((xyz, rgb), (pxyz, prgb), peak=2047), metrics_ref.pair(xyz, rgb, pxyz, prgb))
