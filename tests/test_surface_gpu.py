"""Reconstruction straight from P010 / P016 semi-planar video decoder surfaces (include/vpcc_recon.h,
VPCC_FRAME_UV_INTERLEAVED, VPCC_FRAME_GEO_SHIFT / _ATTR_SHIFT): every result is compared bit for bit with the CPU oracle on the
PLANAR original of the same frame — the samples the surfaces stand for (synth.from_semiplanar) — in host memory and as
borrowed device planes, on the tile kernel and on both kernels of the general sequence."""
import ctypes as C
import os

import numpy as np
import pytest
import torch  # noqa: F401  (before the library is loaded below: torch's bundled HIP runtime must come up first, as it does
              #  when conftest counts devices, or torch finds no GPU once the library's runtime holds the device)

import cases
import oracle_binding as ob
import surface_ref
from tmc2rs import _abi, recon, synth

pytestmark = pytest.mark.gpu

# A library without the feature ignores the layout bits of a frame without attributes and would run its kernels on shifted
# samples: refuse on the host, before any context exists.
assert hasattr(_abi.load_library(), "vpcc_decoder_set_video_format"), "the library predates semi-planar surfaces"

PROFILE = _abi.VPCC_GOF_PROFILE | _abi.VPCC_GOF_WANT_PATCH_INDEX
TILE = ["k_plan_tiles", "k_recon_tiles"]


@pytest.fixture(scope="module")
def ctx():
    c = recon.Context(0)
    yield c
    c.close()


_refs = {}


def _ref(frame):
    """The oracle on the planar original of a (semi-planar or planar) frame."""
    planar = synth.from_semiplanar(frame)
    key = id(frame)
    if key not in _refs:
        st, r = ob.reconstruct(planar)
        assert st == 0
        _refs[key] = (frame, r)                      # (keeps the frame alive: the id stays its own)
    return _refs[key][1]


def _check(res, ref, colour=True):
    assert res["n"] == ref["n"]
    assert np.array_equal(res["xyz"], ob.xyz_array(ref)), "integer geometry must be bit-exact"
    if colour:
        assert np.array_equal(res["rgb"], ob.rgb_array(ref)), "8-bit colour must be bit-exact"
    if "patch_index" in res:
        assert np.array_equal(res["patch_index"].astype(np.uint64), ref["partition"])


def _check_gof(g, frames):
    counts = g.point_counts()
    for i, f in enumerate(frames):
        ref = _ref(f)
        assert int(counts[i]) == ref["n"]
        assert g.frame_status(i) == _abi.VPCC_OK
        _check(g.download(i, want_patch_index=True), ref, colour=f.get("attribute_count", 1) > 0)


def _gof(ctx, frames, memory, flags=PROFILE, keep=None):
    if memory == "host":
        return ctx.gof(frames, flags=flags)
    dev = [recon.DeviceFrame(f) for f in frames]
    if keep is not None:
        keep.extend(dev)
    g = ctx.gof(None, memory=_abi.VPCC_MEM_DEVICE, descs=[d.desc for d in dev], flags=flags)
    g._device_frames = dev                           # (the borrowed planes live as long as the gof)
    return g


PATHS = ["default", "force_general", "general_any"]


def _run(ctx, frames, memory, path, monkeypatch):
    flags = PROFILE | (_abi.VPCC_GOF_FORCE_GENERAL if path != "default" else 0)
    if path == "general_any":
        os.environ["VPCC_GENERAL_ANY_FRAME"] = "1"   # read by every launch: set around the gof's creation and launches
    try:
        g = _gof(ctx, frames, memory, flags)
        g.reconstruct()
        names = [k for k, _ in g.kernel_times()]
    finally:
        os.environ.pop("VPCC_GENERAL_ANY_FRAME", None)
    if path == "force_general":
        assert names[0] == "k_block_owner" and names[1] in ("k_general_blocks", "k_general")
    if path == "general_any":
        assert names == ["k_block_owner", "k_general"]
    _check_gof(g, frames)
    g.close()
    return names


_surfaces = {}


def _surface_case(name):
    if name not in _surfaces:
        _surfaces[name] = synth.to_semiplanar(cases.PARITY_CASES[name](), shift=6, junk_seed=0x5F0 + len(_surfaces))
    return _surfaces[name]


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("memory", ["host", "device"])
@pytest.mark.parametrize("name", sorted(cases.PARITY_CASES))
def test_parity_cases_as_p016(ctx, monkeypatch, name, memory, path):
    _run(ctx, [_surface_case(name)], memory, path, monkeypatch)


@pytest.fixture(scope="module")
def sweep():
    return [synth.to_semiplanar(f, shift=6, junk_seed=0x5EE9 + i) for i, f in enumerate(cases.random_sweep_frames())]


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("memory", ["host", "device"])
def test_random_sweep_as_p016(ctx, monkeypatch, sweep, memory, path):
    names = _run(ctx, sweep, memory, path, monkeypatch)
    if path == "default":
        assert names == TILE


def _medium_surfaces(n=3, **kw):
    kw.setdefault("junk_seed", 91)
    return [synth.to_semiplanar(cases.medium_frame(i), **kw) for i in range(n)]


@pytest.mark.parametrize("memory", ["host", "device"])
def test_aligned_surfaces_take_the_tile_kernel_misaligned_ones_the_general_sequence(ctx, monkeypatch, memory):
    frames = _medium_surfaces()
    g = _gof(ctx, frames, memory)
    g.reconstruct()
    assert [k for k, _ in g.kernel_times()] == TILE
    _check_gof(g, frames)
    g.close()
    # UV rows of 2 * width + 4 bytes: cstride % 4 == 2 — no 8-byte pair loads; the luma rows are misaligned the same way
    frames = _medium_surfaces(pitch_align=4, extra_pitch=4)
    assert frames[0]["attribute"][0][1].strides[0] // 2 % 4 == 2
    g = _gof(ctx, frames, memory)
    g.reconstruct()
    assert [k for k, _ in g.kernel_times()] == ["k_block_owner", "k_general_blocks"]
    _check_gof(g, frames)
    g.close()
    # ... and only the UV plane misaligned (a luma pitch the tile kernel takes)
    frames = _medium_surfaces()
    for f in frames:
        f["attribute"] = [(y, np.concatenate([uv, np.zeros((uv.shape[0], 2), np.uint16)], axis=1)[:, :uv.shape[1]])
                          for y, uv in f["attribute"]]
    assert frames[0]["attribute"][0][1].strides[0] // 2 % 4 == 2
    g = _gof(ctx, frames, memory)
    g.reconstruct()
    assert [k for k, _ in g.kernel_times()] == ["k_block_owner", "k_general_blocks"]
    _check_gof(g, frames)
    g.close()


def _shifted_planar(frame, gs, ash, junk_seed):
    """Planar chroma, shifted samples (no interleaving): the layout bits without VPCC_FRAME_UV_INTERLEAVED."""
    f = dict(frame)
    f["geometry"] = [synth._msb(g, gs, junk_seed, 1 + m) for m, g in enumerate(frame["geometry"])]
    f["attribute"] = [tuple(synth._msb(p, ash, junk_seed, 10 + 3 * m + c) for c, p in enumerate(a))
                      for m, a in enumerate(frame["attribute"])]
    f["geo_shift"], f["attr_shift"] = gs, ash
    return f


SHIFTS = [(0, 0), (0, 4), (4, 0), (6, 6), (4, 8), (8, 6), (8, 8)]


@pytest.mark.parametrize("path", ["default", "force_general", "general_any"])
@pytest.mark.parametrize("interleaved", [True, False])
@pytest.mark.parametrize("shifts", SHIFTS)
def test_sample_shifts(ctx, monkeypatch, shifts, interleaved, path):
    """Surface sample = (value << s) | junk, geometry and attribute shifts apart; the oracle's planar frame holds
    surface >> s — for s = 8 values cut to 8 bits, and wide_samples' 16-bit values cut to 16 - s bits."""
    gs, ash = shifts
    base = [cases.medium_frame(5), cases.PARITY_CASES["wide_samples"](), cases.PARITY_CASES["single_map_extension"](),
            cases.PARITY_CASES["relative_d1"]()]
    if interleaved:
        frames = [synth.to_semiplanar(f, geo_shift=gs, attr_shift=ash, junk_seed=300 + k) for k, f in enumerate(base)]
    else:
        frames = [_shifted_planar(f, gs, ash, 300 + k) for k, f in enumerate(base)]
    for memory in ("host", "device"):
        for f in frames:
            _run(ctx, [f], memory, path, monkeypatch)
    # the attribute-less frame: geometry shift alone
    f = cases.PARITY_CASES["no_attribute"]()
    s = synth.to_semiplanar(f, geo_shift=gs, attr_shift=ash, junk_seed=9) if interleaved else _shifted_planar(f, gs, ash, 9)
    _run(ctx, [s], "device", path, monkeypatch)


def test_copy_planes(ctx):
    frames = _medium_surfaces(4)
    dev = [recon.DeviceFrame(f) for f in frames]
    g = ctx.gof(None, memory=_abi.VPCC_MEM_DEVICE, descs=[d.desc for d in dev], flags=PROFILE | _abi.VPCC_GOF_COPY_PLANES)
    del dev                                          # (copied at creation: the gof needs them no longer)
    g.reconstruct()
    assert [k for k, _ in g.kernel_times()] == TILE
    _check_gof(g, frames)
    assert list(g.plane_digests()) == [surface_ref.digest_planes(f) for f in frames]
    g.close()


def _packed_pinned(ctx, frames):
    """The frames' buffers copied back to back (256-byte aligned) into ONE page-locked host region, as a decoder's frame pool
    lies — frames of the same buffers, pointing into it — and the region (unpinned by the caller)."""
    roots = []
    for f in frames:
        d, keep = _abi.host_frame_desc(f)
        roots.append(recon.DeviceFrame._roots_of(keep[:-1]))
    total = sum((r.nbytes + 255) // 256 * 256 for rs in roots for r in rs)
    raw = np.zeros(total + 256, np.uint8)
    off0 = (-raw.ctypes.data) % 256
    arena = raw[off0:off0 + total]
    lib = _abi.load_library()
    assert lib.vpcc_host_pin(ctx.h, arena.ctypes.data, arena.nbytes) == 0
    where = {}
    at = 0
    for rs in roots:
        for r in rs:
            arena[at:at + r.nbytes] = r.view(np.uint8).reshape(-1)
            where[id(r)] = (r, at)
            at += (r.nbytes + 255) // 256 * 256

    def moved(a):
        r = recon._root(a)
        src, at = where[id(r)]
        off = a.ctypes.data - r.ctypes.data
        return np.ndarray(a.shape, a.dtype, buffer=arena, offset=at + off, strides=a.strides)
    out = []
    for f in frames:
        g = dict(f)
        g["occupancy"] = moved(np.asarray(f["occupancy"]))
        g["geometry"] = [moved(np.asarray(x)) for x in f["geometry"]]
        g["attribute"] = [tuple(moved(np.asarray(p)) for p in a) for a in f["attribute"]]
        out.append(g)
    return out, arena, raw


@pytest.mark.parametrize("route", ["extent", "pull", "copies"])
def test_page_locked_host_surfaces(ctx, monkeypatch, route):
    """Page-locked P016 host surfaces through every ingest route: whole stretches of the pinned region (tight rows), the pull
    kernel (VPCC_NO_EXTENT_INGEST), per-plane copies (pitched rows)."""
    if route != "extent":
        monkeypatch.setenv("VPCC_NO_EXTENT_INGEST", "1")
    src = [cases.medium_frame(10 + i) for i in range(8)]
    surfaces = [synth.to_semiplanar(f, junk_seed=40 + i, pitch_align=2 if route != "copies" else 256) for i, f in enumerate(src)]
    frames, arena, raw = _packed_pinned(ctx, surfaces)
    lib = _abi.load_library()
    try:
        g = ctx.gof(frames, flags=PROFILE | _abi.VPCC_GOF_ASYNC_UPLOAD)
        g.reconstruct()
        assert [k for k, _ in g.kernel_times()] == TILE
        _check_gof(g, frames)
        assert list(g.plane_digests()) == [surface_ref.digest_planes(f) for f in frames]
        g.close()
    finally:
        lib.vpcc_host_unpin(ctx.h, arena.ctypes.data)


@pytest.mark.parametrize("memory", ["host", "device"])
def test_full_size_frames(ctx, monkeypatch, memory):
    frames = [synth.to_semiplanar(synth.longdress_frame(0), junk_seed=1), synth.to_semiplanar(synth.owlii_frame(0), junk_seed=2)]
    for f in frames:
        g = _gof(ctx, [f], memory)
        g.reconstruct()
        assert [k for k, _ in g.kernel_times()] == TILE
        _check_gof(g, [f])
        g.close()


def test_gof_of_mixed_layouts_is_refused(ctx):
    planar = cases.medium_frame(0)
    cases_ = [[synth.to_semiplanar(planar), planar],
              [planar, synth.to_semiplanar(planar)],
              [synth.to_semiplanar(planar, shift=6), synth.to_semiplanar(planar, shift=4)],
              [synth.to_semiplanar(planar, geo_shift=6, attr_shift=6), synth.to_semiplanar(planar, geo_shift=6, attr_shift=5)],
              [planar, _shifted_planar(planar, 6, 6, None)]]
    for frames in cases_:
        with pytest.raises(recon.VpccError) as e:
            ctx.gof(frames)
        assert e.value.status == _abi.VPCC_ERR_UNSUPPORTED
    # the one-frame entry point validates the same way
    d, keep = _abi.host_frame_desc(synth.to_semiplanar(planar))
    d.flags |= _abi.VPCC_FRAME_GEO_SHIFT(9) & 0xF00
    with pytest.raises(recon.VpccError):
        ctx.gof(None, descs=[d])


def test_borrowed_p016_pool_refilled_between_launches(ctx):
    """Two slots of a P016 device pool, refilled on the launch stream between launches — full, empty, the other frame, full:
    every launch against the oracle on the planes as they are then."""
    import torch
    bases = [synth.longdress_frame(5), cases.medium_frame(6)]
    others = [synth.longdress_frame(6), cases.medium_frame(7)]
    states = []
    for b, o in zip(bases, others):
        full = synth.to_semiplanar(b, junk_seed=61)
        empty = dict(full)
        empty["occupancy"] = np.zeros_like(b["occupancy"])
        other = synth.to_semiplanar(o, junk_seed=62)
        other["patches"] = b["patches"]                # (the gof's patch table is read once, at creation)
        states.append({"F": full, "E": empty, "O": other})
    slots = [recon.DeviceFrame(s["F"]) for s in states]
    staged = [{k: sl.stage(v) for k, v in s.items()} for sl, s in zip(slots, states)]
    torch.cuda.synchronize()
    g = ctx.gof(None, memory=_abi.VPCC_MEM_DEVICE, descs=[s.desc for s in slots], flags=PROFILE)
    stream = torch.cuda.Stream(device=torch.device("cuda:0"))
    for step in ("F", "E", "O", "F", "O", "E"):
        for sl, st in zip(slots, staged):
            sl.fill(st[step], stream)
        g.reconstruct(stream=stream.cuda_stream)
        assert [k for k, _ in g.kernel_times()] == ["k_plan_tiles", "k_recon_tiles"]
        _check_gof(g, [s[step] for s in states])
        assert list(g.plane_digests()) == [surface_ref.digest_planes(s[step]) for s in states]
    g.close()


def test_smoothing_after_a_semi_planar_launch(ctx):
    params = dict(grid_size=8, threshold=2, color_grid_size=8, color_threshold_smoothing=10, color_threshold_difference=60)
    frames = [synth.to_semiplanar(cases.overlapping_3d_frame(i), junk_seed=70 + i) for i in range(3)]
    g = _gof(ctx, frames, "device")
    g.reconstruct()
    before = [g.download(i, want_patch_index=True) for i in range(len(frames))]
    for f, b in zip(frames, before):
        _check(b, _ref(f))
    g.smooth(10, **params)
    for i, b in enumerate(before):
        after = g.download(i)
        exp_xyz = ob.spec_smooth_geometry(b["xyz"], b["patch_index"], 10, params["grid_size"], params["threshold"])
        exp_rgb = ob.spec_smooth_color(exp_xyz, b["rgb"], b["patch_index"], 10, params["color_grid_size"],
                                       params["color_threshold_smoothing"], params["color_threshold_difference"])
        assert np.array_equal(after["xyz"], exp_xyz) and np.array_equal(after["rgb"], exp_rgb)
    g.close()


@pytest.mark.parametrize("memory", ["host", "device"])
def test_plane_digests_of_surfaces(ctx, memory):
    frames = [_surface_case(n) for n in ("small0", "no_attribute", "single_map_extension", "block8_ragged", "medium0",
                                         "strided_planes")]
    g = _gof(ctx, frames, memory, flags=0)
    want = [surface_ref.digest_planes(f) for f in frames]
    assert want == [recon.digest_planes(f) for f in frames]
    assert list(g.plane_digests()) == want
    g.reconstruct()
    assert list(g.plane_digests()) == want
    g.close()


def _decoder_frames(paths, verify=None, video_format=None):
    d = recon.Decoder(paths["bin"], occupancy_yuv=paths["occ"], geometry_yuv=paths["geo"], attribute_yuv=paths["attr"],
                      verify=verify, video_format=video_format)
    d.start()
    frames = list(d)
    err = d.error()
    stats = d.verify_stats()
    d.close()
    return frames, err, stats


def test_decoder_reads_p010le_raw_video(tmp_path):
    """The V3C fixture of test_decoder_gpu.py with its geometry and attribute raw files rewritten as P010LE (junk in the low
    bits): the same frames, in order, as the planar run and the oracle; verified mode passes every check on every frame."""
    import v3c_writer as W
    gofs = [[cases.medium_frame(i) for i in range(3)], [cases.medium_frame(40 + i, occupancy_values="random") for i in range(2)]]
    paths = W.write_sequence(tmp_path, gofs)
    w, h = gofs[0][0]["width"], gofs[0][0]["height"]
    p010 = dict(paths)
    for k in ("geo", "attr"):
        p010[k] = str(tmp_path / f"{k}.p010")
        synth.yuv420p10le_to_p010le(paths[k], p010[k], w, h, junk_seed=17)
    planar, err, _ = _decoder_frames(paths)
    assert err == ""
    got, err, _ = _decoder_frames(p010, video_format="p010le")
    assert err == ""
    expected = [f for g in gofs for f in g]
    assert len(got) == len(planar) == len(expected)
    for a, b, f in zip(got, planar, expected):
        st, ref = ob.reconstruct(f)
        assert st == 0 and a["n"] == b["n"] == ref["n"]
        assert np.array_equal(a["xyz"], ob.xyz_array(ref)) and np.array_equal(a["rgb"], ob.rgb_array(ref))
        assert np.array_equal(a["xyz"], b["xyz"]) and np.array_equal(a["rgb"], b["rgb"])
    got_v, err, stats = _decoder_frames(p010, verify="all", video_format="p010le")
    assert err == ""
    assert [(a["n"], a["xyz"].tobytes(), a["rgb"].tobytes()) for a in got_v] == \
        [(a["n"], a["xyz"].tobytes(), a["rgb"].tobytes()) for a in got]
    n = len(expected)
    assert stats["ingest_frames"] == stats["reconstruct_frames"] == stats["delivery_frames"] == n
    # the planar files read as P010LE are other samples: the format switch really is in force
    wrong, err, _ = _decoder_frames(paths, video_format="p010le")
    assert [(a["n"], a["xyz"].tobytes()) for a in wrong] != [(a["n"], a["xyz"].tobytes()) for a in planar]


def test_decoder_video_format_after_start_is_a_state_error(tmp_path):
    import v3c_writer as W
    paths = W.write_sequence(tmp_path, [[cases.medium_frame(0)]])
    d = recon.Decoder(paths["bin"], occupancy_yuv=paths["occ"], geometry_yuv=paths["geo"], attribute_yuv=paths["attr"])
    d.start()
    assert d.lib.vpcc_decoder_set_video_format(d.h, _abi.VPCC_VIDEO_P010LE) == _abi.VPCC_ERR_STATE
    assert len(list(d)) == 1
    d.close()
