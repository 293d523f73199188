"""Plane addressing at the 32-bit limits: borrowed device planes with row pitches up to where the kernels'
index arithmetic runs out, compared bit for bit with the CPU oracle on tight host copies.

  a. the tile kernel at the largest strides tile_planes_aligned admits (byte offsets just under 2^32), and one stride up;
  b. k_general_blocks at its stride limit of 65536 elements (24-bit row products), and k_general one stride up;
  c. k_general with plane element indices past 2^32 — each plane kind alone, then all at once, at the canvas's foot and
     mid-canvas — through a gof launch, vpcc_reconstruct_frame, VPCC_GOF_COPY_PLANES and a relaunch over refilled planes;
  d. vpcc_upsample_occupancy over an occupancy plane whose indices pass 2^32;
  e. the device plane digests of every gof here against the host digests of the tight copies.

Every case checks that it is not vacuous: some occupied pixel the oracle turns into a point reads a sample past the
boundary under test, in every plane kind under test."""
import ctypes as C

import numpy as np
import pytest

import cases
import oracle_binding as ob
from tmc2rs import _abi, recon

pytestmark = pytest.mark.gpu

GIB = 1 << 30
LIM = 1 << 32
SENTINEL = 0xA5                                  # every byte of an atlas outside the planes' windows
FLAGS = _abi.VPCC_GOF_PROFILE | _abi.VPCC_GOF_WANT_PATCH_INDEX
SHIFT = 6                                        # P016: samples MSB-aligned
KINDS = ("occ", "geo0", "geo1", "luma", "chroma")


@pytest.fixture(scope="module")
def ctx():
    c = recon.Context(0)
    yield c
    c.close()


def _need(nbytes):
    import torch
    free, _ = torch.cuda.mem_get_info(0)
    if free < nbytes:
        pytest.skip(f"needs {nbytes / GIB:.1f} GiB of free device memory, {free / GIB:.1f} GiB free")


def _release():
    import torch
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------- frames
def _patch(u0, v0, su, sv, view=0, orient=0, u1=3, v1=5, d1=17):
    return cases._patch(u0, v0, su, sv, view=view, orient=orient, u1=u1, v1=v1, d1=d1)


def _planes(H, W, prec, seed):
    """Random planes: occupancy 70 % set (values 1-255), depths, colours."""
    rng = np.random.RandomState(seed)
    occ = (rng.randint(1, 256, size=(H // prec, W // prec)) * (rng.rand(H // prec, W // prec) < 0.7)).astype(np.uint8)
    g0 = rng.randint(0, 800, size=(H, W)).astype(np.uint16)
    g1 = (g0 + 4 * rng.randint(0, 4, size=(H, W))).astype(np.uint16)
    attr = [tuple(rng.randint(64, 941, size=s).astype(np.uint16) for s in ((H, W), (H // 2, W // 2), (H // 2, W // 2)))
            for _ in range(2)]
    return {"occupancy": occ, "geometry": [g0, g1], "attribute": attr}


def _frame(H, W, R, prec, patches, seed, map_count=2, absolute_d1=1):
    f = {"width": W, "height": H, "occupancy_resolution": R, "occupancy_precision": prec, "map_count": map_count,
         "absolute_d1": absolute_d1, "attribute_count": 1, "flags": 0, "seed": seed,
         "patches": np.array(patches, dtype=_abi.PATCH_DTYPE)}
    f.update(_planes(H, W, prec, seed))
    f["geometry"] = f["geometry"][:map_count]
    f["attribute"] = f["attribute"][:map_count]
    assert recon.validate_frame(f) == 0
    return f


def _with_planes(f, seed):
    """f's patch table over other random planes (the relaunch)."""
    g = dict(f)
    g.update(_planes(f["height"], f["width"], f["occupancy_precision"], seed))
    g["geometry"] = g["geometry"][:f["map_count"]]
    g["attribute"] = g["attribute"][:f["map_count"]]
    return g


def _rows_patches(rows, R, W, views=(0, 1, 2, 3, 4, 5)):
    """Default and Swap patches whose blocks cover canvas rows [rows[0], rows[1]) (in pixels) — across a boundary row."""
    v0, v1 = rows[0] // R, -(-rows[1] // R)
    bw = W // R
    out, k = [], 0
    for u in range(0, bw - 1, 3):
        sv = v1 - v0
        if k % 2:                                  # Swap: the canvas extent is (size_v0, size_u0)
            out.append(_patch(u, v0, sv, 2, view=views[k % len(views)], orient=1, u1=k, d1=11 * k))
        else:
            out.append(_patch(u, v0, 2, sv, view=views[k % len(views)], orient=0, v1=k, d1=7 * k))
        k += 1
    return out


def _exotic_patches(v_shift):
    """cases.exotic_frame's orientations (rotated, mirrored), moved down by v_shift blocks."""
    out = []
    for p in cases.exotic_frame()["patches"]:
        q = p.copy()
        q["v0"] = int(q["v0"]) + v_shift
        out.append(q)
    return out


def _as_p016(f):
    """The frame as P016 surfaces' samples: geometry and attributes << SHIFT, chroma one interleaved plane."""
    g = dict(f)
    g["geometry"] = [(x.astype(np.uint16) << SHIFT) for x in f["geometry"]]
    attr = []
    for (y, u, v) in f["attribute"]:
        uv = np.empty((u.shape[0], 2 * u.shape[1]), np.uint16)
        uv[:, 0::2], uv[:, 1::2] = u << SHIFT, v << SHIFT
        attr.append((y << SHIFT, uv))
    g["attribute"] = attr
    g["geo_shift"] = g["attr_shift"] = SHIFT
    g["flags"] = int(f.get("flags", 0)) | _abi.VPCC_FRAME_UV_INTERLEAVED
    return g


# ------------------------------------------------------------------------------------------------------------- atlas
class Atlas:
    """One device allocation holding planes as column windows that share one large row pitch (`pitch` bytes).  Occupancy
    lives in the same buffer as bytes; chroma of a frame uses every `chroma_rows`-th row (cstride = chroma_rows x pitch in
    elements, so that chroma indices grow as fast as luma indices).  An occupancy window with a step of half the pitch
    (`occ_half`: the strides of cases a and b, where every plane kind has the same stride in elements) takes one column
    range in each half of a row.

    The buffer is filled with SENTINEL first.  For the wrap cases it is at least 2^33 bytes plus one pitch long: a plane
    index that wraps modulo 2^32 — on a library that forms it in 32 bits — then still addresses a byte inside the
    allocation (byte offsets below 2^33 for 16-bit planes, below 2^32 for occupancy): such a build reads wrong samples
    and cannot fault."""

    def __init__(self, pitch, nbytes, occ_half=False):
        import torch
        self.dev = torch.device("cuda:0")
        self.pitch, self.occ_half = pitch, occ_half
        self.buf = torch.full((nbytes,), SENTINEL, dtype=torch.uint8, device=self.dev)
        self.base = self.buf.data_ptr()
        assert self.base % 256 == 0
        self.col = 0
        self.half = pitch // 2

    def window(self, rows, width_bytes, step):
        """A new column window of `rows` rows, `step` bytes apart; returns its byte offset."""
        col = self.col
        self.col = -(-(col + width_bytes) // 64) * 64
        assert self.col <= (self.half if self.occ_half else self.pitch)
        assert col + (rows - 1) * step + width_bytes <= self.buf.numel()
        return col

    def view(self, off, rows, width_bytes, step):
        return self.buf.as_strided((rows, width_bytes), (step, 1), off)

    def close(self):
        del self.buf


def _u8(a):
    return np.ascontiguousarray(a).view(np.uint8)


class DeviceFrames:
    """Borrowed device planes of a list of frames: the plane kinds in `kinds` in the atlas, every other plane a tight tensor
    of its own; `descs` describe them.  `fill(frames, stream)` writes other planes of the same shapes into the same places."""

    def __init__(self, atlas, frames, kinds):
        import torch
        self.atlas, self.kinds = atlas, set(kinds)
        self.places = []                     # per frame: [(kind, key, offset or tensor, rows, width_bytes, step, elems_per_row)]
        self.descs, self._keep, self._tight = [], [], []
        P = atlas.pitch
        for f in frames:
            d, keep = _abi.host_frame_desc(f)
            self._keep.append(keep)
            uv = bool(int(d.flags) & _abi.VPCC_FRAME_UV_INTERLEAVED)
            pl = []

            def put(kind, key, arr, step_rows=1, step=None):
                a = _u8(arr)
                rows, wb = a.shape
                if kind in self.kinds:
                    st = step if step is not None else step_rows * P
                    off = atlas.window(rows, wb, st)
                    pl.append((key, off, rows, wb, st))
                    return atlas.base + off, st
                t = torch.from_numpy(a.reshape(-1).copy()).to(atlas.dev)
                self._tight.append(t)
                pl.append((key, t, rows, wb, wb))
                return t.data_ptr(), wb

            occ_step = atlas.half if atlas.occ_half else P
            ptr, st = put("occ", "occ", f["occupancy"], step=occ_step)
            d.occupancy.y, d.occupancy.stride = ptr, st
            for m in range(f["map_count"]):
                ptr, st = put(f"geo{m}", ("geo", m), f["geometry"][m])
                d.geometry[m].y, d.geometry[m].stride = ptr, st // 2
                a = f["attribute"][m]
                ptr, st = put("luma", ("y", m), a[0])
                d.attribute[m].y, d.attribute[m].stride = ptr, st // 2
                crow = 1 if atlas.occ_half else 2                       # chroma on every other row (wrap cases)
                ptr, st = put("chroma", ("u", m), a[1], step_rows=crow)
                d.attribute[m].u, d.attribute[m].cstride = ptr, st // 2
                if not uv:
                    ptr, st2 = put("chroma", ("v", m), a[2], step_rows=crow)
                    assert st2 == st
                    d.attribute[m].v = ptr
            self.places.append(pl)
            self.descs.append(d)
        self.fill(frames)
        torch.cuda.synchronize()

    @staticmethod
    def _arrays(f):
        out = {"occ": f["occupancy"]}
        for m in range(f["map_count"]):
            out[("geo", m)] = f["geometry"][m]
            a = f["attribute"][m]
            out[("y", m)], out[("u", m)] = a[0], a[1]
            if len(a) == 3:
                out[("v", m)] = a[2]
        return out

    def fill(self, frames, stream=None):
        """Writes the frames' planes into their places (on `stream`, enqueued only, when given)."""
        import torch
        staged = [{k: torch.from_numpy(_u8(a)).to(self.atlas.dev) for k, a in self._arrays(f).items()} for f in frames]
        torch.cuda.synchronize()
        self._staged = staged                    # alive until the copies are done
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
            for pl, st in zip(self.places, staged):
                for key, where, rows, wb, step in pl:
                    src = st[key]
                    if isinstance(where, int):
                        self.atlas.view(where, rows, wb, step).copy_(src, non_blocking=True)
                    else:
                        where.copy_(src.reshape(-1), non_blocking=True)

    def element_index_past(self, frames, refs):
        """Per plane kind in the atlas: the number of points the oracle made whose pixel's element index in a plane of that
        kind (row x stride + column, chroma (row / 2) x cstride + column / 2, x 2 interleaved) is >= 2^32."""
        out = {k: 0 for k in self.kinds}
        for d, f, ref in zip(self.descs, frames, refs):
            p2p = ref["point_to_pixel"].astype(np.uint64)
            if not len(p2p):
                continue
            x, y, layer = p2p[:, 0], p2p[:, 1], p2p[:, 2]
            prec = np.uint64(f["occupancy_precision"])
            uv = 1 if int(d.flags) & _abi.VPCC_FRAME_UV_INTERLEAVED else 0
            if "occ" in self.kinds:
                out["occ"] += int(np.count_nonzero((y // prec) * np.uint64(d.occupancy.stride) + x // prec >= LIM))
            for m in range(f["map_count"]):
                if f"geo{m}" in self.kinds:
                    out[f"geo{m}"] += int(np.count_nonzero(y * np.uint64(d.geometry[m].stride) + x >= LIM))
                on = layer == m if f["map_count"] > 1 else np.ones(len(x), bool)
                if "luma" in self.kinds:
                    out["luma"] += int(np.count_nonzero(on & (y * np.uint64(d.attribute[m].stride) + x >= LIM)))
                if "chroma" in self.kinds:
                    c = (y >> np.uint64(1)) * np.uint64(d.attribute[m].cstride) + ((x >> np.uint64(1)) << np.uint64(uv))
                    out["chroma"] += int(np.count_nonzero(on & (c >= LIM)))
        return out

    def close(self):
        self._tight.clear()
        self._staged = None


# ------------------------------------------------------------------------------------------------------------- checks
def _refs(frames):
    out = []
    for f in frames:
        st, ref = ob.reconstruct(f)
        assert st == 0
        out.append(ref)
    return out


def _check_points(res, ref, tag):
    assert res["n"] == ref["n"], (tag, res["n"], ref["n"])
    xyz, rgb = ob.xyz_array(ref), ob.rgb_array(ref)
    bad = int(np.count_nonzero(np.any(res["xyz"] != xyz, axis=1))) if len(xyz) else 0
    assert bad == 0, f"{tag}: {bad} of {ref['n']} positions differ from the oracle"
    bad = int(np.count_nonzero(np.any(res["rgb"] != rgb, axis=1))) if len(rgb) else 0
    assert bad == 0, f"{tag}: {bad} of {ref['n']} colours differ from the oracle"
    assert np.array_equal(res["patch_index"].astype(np.uint64), ref["partition"]), f"{tag}: patch index"


def _n_blocks(f):
    return (f["width"] // f["occupancy_resolution"]) * (f["height"] // f["occupancy_resolution"])


def _check_gof(g, frames, refs, kernels, tag, host_frames):
    g.sync()
    counts = g.point_counts()
    names = [n for n, _ in g.kernel_times()]
    assert names == kernels, (tag, names)
    for i, (f, ref) in enumerate(zip(frames, refs)):
        t = f"{tag} frame {i} (R {f['occupancy_resolution']}, precision {f['occupancy_precision']})"
        assert int(counts[i]) == ref["n"], (t, int(counts[i]), ref["n"])
        assert g.frame_status(i) == _abi.VPCC_OK, t
        _check_points(g.download(i, want_patch_index=True), ref, t)
        b2p, _ = g.block_to_patch(i, _n_blocks(f))
        assert np.array_equal(b2p.astype(np.uint64), ref["block_to_patch"]), f"{t}: block_to_patch"
    # e. the device plane digests over the borrowed planes = the host digests of the tight copies
    want = np.array([recon.digest_planes(h) for h in host_frames], dtype=np.uint64)
    assert np.array_equal(g.plane_digests(), want), f"{tag}: plane digests"


def _capacity(refs):
    return max(r["n"] for r in refs) + 16


def _reconstruct_frame_device(ctx, desc, cap):
    """vpcc_reconstruct_frame over a VPCC_MEM_DEVICE descriptor."""
    xyz = np.zeros(cap, dtype=_abi.POINT3_DTYPE)
    rgb = np.zeros(cap, dtype=_abi.COLOR3_DTYPE)
    pidx = np.zeros(cap, dtype=np.uint16)
    n = C.c_size_t(0)
    st = ctx.lib.vpcc_reconstruct_frame(ctx.h, C.byref(desc), _abi.VPCC_MEM_DEVICE, xyz.ctypes.data, rgb.ctypes.data,
                                        pidx.ctypes.data, cap, C.byref(n))
    ctx._check(st, "vpcc_reconstruct_frame")
    k = n.value
    return {"n": k, "xyz": recon._xyz(xyz[:k]), "rgb": recon._rgb(rgb[:k]), "patch_index": pidx[:k].copy()}


def _general_kernels(block_units):
    return ["k_block_owner", "k_general_blocks" if block_units else "k_general"]


# ------------------------------------------------------------------------------------------------------------- a, b
W_AB = 256
H_AB = 32768


def _tile_frames(seed):
    """R = 16, precision 1 / 2 / 4, Default and Swap patches: blocks at the top, the middle and the foot of the canvas."""
    frames = []
    for k, prec in enumerate((1, 2, 4)):
        patches = []
        for rows in ((0, 48), (16352, 16400), (32720, 32768)):
            patches += _rows_patches(rows, 16, W_AB)
        frames.append(_frame(H_AB, W_AB, 16, prec, patches, seed + k, map_count=2, absolute_d1=k % 2))
    return frames


def _bytes_at_foot(dev, refs):
    """Oracle points whose u16 byte offset (row x pitch + 2 x column) lies in the top 1 % below 2^32: the tile kernel's
    offsets there are just under its limit."""
    n = 0
    for d, ref in zip(dev.descs, refs):
        p = ref["point_to_pixel"].astype(np.uint64)
        n += int(np.count_nonzero(p[:, 1] * np.uint64(2 * d.geometry[0].stride) + 2 * p[:, 0] >= np.uint64(LIM * 99 // 100)))
    return n


STRIDE_CASES = [(65532, "tiles", True), (65532, "tiles", False), (65536, "general_blocks", True), (65540, "general", True)]


@pytest.mark.parametrize("layout", ["planar", "p016"])
@pytest.mark.parametrize("stride,expect,lds", STRIDE_CASES, ids=["tiles-lds", "tiles-global", "blocks", "general"])
def test_strides_at_the_tile_and_block_limits(ctx, monkeypatch, layout, stride, expect, lds):
    """a. every plane kind at a stride of `stride` elements (occupancy: `stride` bytes; 65532: the largest tile_planes_aligned
    admits, byte offsets just under 2^32); b. 65536: k_general_blocks' limit, 65540: k_general."""
    if not lds:
        monkeypatch.setenv("VPCC_NO_LDS_PLANNING", "1")
    pitch = 2 * stride
    nbytes = H_AB * pitch
    _need(nbytes + GIB)
    planar = _tile_frames(0xA11 + stride)
    frames = planar if layout == "planar" else [_as_p016(f) for f in planar]
    refs = _refs(planar)
    atlas = Atlas(pitch, nbytes, occ_half=True)
    dev = DeviceFrames(atlas, frames, KINDS)
    try:
        assert _bytes_at_foot(dev, refs) > 0
        for d in dev.descs:
            assert d.geometry[0].stride == stride and d.occupancy.stride == stride and d.attribute[0].cstride == stride
        g = ctx.gof(None, capacity=_capacity(refs), flags=FLAGS, memory=_abi.VPCC_MEM_DEVICE, descs=dev.descs)
        g.reconstruct()
        if expect == "tiles":
            kernels = ["k_plan_tiles" if lds else "k_plan_cover+items", "k_recon_tiles"]
        else:
            kernels = _general_kernels(expect == "general_blocks")
        _check_gof(g, planar, refs, kernels, f"{layout} stride {stride}", frames)
        g.close()
    finally:
        dev.close()
        atlas.close()
        del dev, atlas
        _release()


# ------------------------------------------------------------------------------------------------------------- c, d, e
W_C = 256


def _wrap_frames(H, occ_row, u16_row, seed):
    """Frames of R = 16 (Default / Swap), 8, 32 and of the exotic orientations, with patches across `occ_row` (where the
    occupancy index passes 2^32 at precision 1) and `u16_row` (where the 16-bit planes' indices do), and at the top.
    map_count 1 and 2, absolute_d1 0 and 1."""
    def rows_around(r, R):
        lo = max(0, (r // R - 2) * R)
        return (lo, min(H, lo + 4 * R))

    frames = []
    for k, (R, prec, maps, absolute) in enumerate(((16, 1, 2, 1), (8, 1, 1, 1), (32, 1, 2, 0), (16, 2, 2, 1))):
        patches = _rows_patches((0, 2 * R), R, W_C)
        for r in (occ_row, u16_row):
            if r is not None:
                patches += _rows_patches(rows_around(r, R), R, W_C)
        frames.append(_frame(H, W_C, R, prec, patches, seed + k, map_count=maps, absolute_d1=absolute))
    # the exotic orientations (R = 16, blocks inside a 4 x 4 square) across each boundary row
    ex = []
    for r in (occ_row, u16_row):
        if r is not None:
            ex += _exotic_patches(max(0, r // 16 - 3))
    frames.append(_frame(H, W_C, 16, 1, ex, seed + 9, map_count=2, absolute_d1=1))
    return frames


# (H, pitch in bytes): the foot of a 32768-row canvas, the 16-bit planes pass 2^32 in their last rows and occupancy mid-canvas;
# and a 4096-row canvas whose occupancy passes 2^32 in row 2048 (its 16-bit planes stay below)
CANVAS = {"foot": (32768, 262400), "mid": (4096, (1 << 21) + 128)}
WRAP_CASES = [("foot", ("occ",)), ("foot", ("geo0",)), ("foot", ("geo1",)), ("foot", ("luma",)), ("foot", ("chroma",)),
              ("foot", ("chroma+p016",)), ("foot", KINDS), ("foot", KINDS + ("p016",)), ("mid", KINDS)]


def _wrap_setup(canvas, kinds, seed):
    H, pitch = CANVAS[canvas]
    nbytes = max(H * pitch, LIM * 2 + pitch) + pitch
    occ_row = LIM // pitch
    u16_row = 2 * LIM // pitch if 2 * LIM // pitch < H else None
    planar = _wrap_frames(H, occ_row, u16_row, seed)
    p016 = any("p016" in k for k in kinds)
    kinds = tuple(k.replace("+p016", "") for k in kinds if k != "p016")
    return H, pitch, nbytes, planar, ([_as_p016(f) for f in planar] if p016 else planar), kinds


@pytest.mark.parametrize("canvas,kinds", WRAP_CASES, ids=[f"{c}-{'+'.join(k)}" for c, k in WRAP_CASES])
def test_plane_indices_past_32_bits(ctx, canvas, kinds):
    """c. k_general reads planes whose element indices pass 2^32, through every route that borrows them."""
    import torch
    H, pitch, nbytes, planar, frames, kinds = _wrap_setup(canvas, kinds, 0xC0 + len(kinds))
    _need(nbytes + 2 * GIB)
    refs = _refs(planar)
    atlas = Atlas(pitch, nbytes)
    dev = DeviceFrames(atlas, frames, kinds)
    try:
        past = dev.element_index_past(frames, refs)
        crossing = [k for k in kinds if not (canvas == "mid" and k != "occ")]
        for k in crossing:
            assert past[k] > 0, (k, past)
        other_planar = [_with_planes(f, 0x5EED + i) for i, f in enumerate(planar)]
        other = [_as_p016(f) for f in other_planar] if frames is not planar else other_planar
        other_refs = _refs(other_planar)
        # 1. a gof launch (on its own stream)
        g = ctx.gof(None, capacity=max(_capacity(refs), _capacity(other_refs)), flags=FLAGS, memory=_abi.VPCC_MEM_DEVICE,
                    descs=dev.descs)
        s = torch.cuda.Stream()
        g.reconstruct(stream=s.cuda_stream)
        _check_gof(g, planar, refs, _general_kernels(False), "launch", frames)
        # 4. a second launch after the windows are refilled on the launch stream
        dev.fill(other, stream=s)
        g.reconstruct(stream=s.cuda_stream)
        s.synchronize()
        _check_gof(g, other_planar, other_refs, _general_kernels(False), "relaunch", other)
        g.close()
        dev.fill(frames)
        torch.cuda.synchronize()
        # 2. vpcc_reconstruct_frame over each descriptor
        for i, (d, ref) in enumerate(zip(dev.descs, refs)):
            _check_points(_reconstruct_frame_device(ctx, d, ref["n"] + 16), ref, f"vpcc_reconstruct_frame {i}")
        # 3. VPCC_GOF_COPY_PLANES: the copies are tight — R = 16 Default/Swap frames take the tile kernel.  (Not with chroma in
        # the atlas: a copied chroma plane keeps its source stride, vpcc_gof_create — gigabytes per plane here.)
        for i, (d, f, ref) in enumerate(zip(dev.descs, planar, refs) if "chroma" not in kinds else ()):
            g = ctx.gof(None, capacity=ref["n"] + 16, flags=FLAGS | _abi.VPCC_GOF_COPY_PLANES,
                        memory=_abi.VPCC_MEM_DEVICE, descs=[d])
            g.reconstruct()
            simple, R = i != len(planar) - 1, f["occupancy_resolution"]
            # (k_general_blocks is chosen by the caller's strides, above its 65536 here: the copies' k_general is 32-bit)
            kernels = ["k_plan_tiles", "k_recon_tiles"] if R == 16 and simple else _general_kernels(False)
            _check_gof(g, [f], [ref], kernels, f"copied planes {i}", [frames[i]])
            g.close()
    finally:
        dev.close()
        atlas.close()
        del dev, atlas
        _release()


def test_upsample_occupancy_past_32_bits(ctx):
    """d. vpcc_upsample_occupancy over a VPCC_MEM_DEVICE occupancy plane whose indices pass 2^32 (precision 1 and 2)."""
    H, pitch = CANVAS["foot"]
    nbytes = max(H * pitch, LIM * 2 + pitch) + pitch
    _need(nbytes + GIB)
    atlas = Atlas(pitch, nbytes)
    try:
        for prec in (1, 2):
            f = _frame(H, W_C, 16, prec, _rows_patches((0, 32), 16, W_C), 0xD0 + prec)
            dev = DeviceFrames(atlas, [f], ("occ",))
            d = dev.descs[0]
            assert (H // prec - 1) * d.occupancy.stride + (W_C // prec - 1) >= LIM
            out = np.zeros((H, W_C), np.uint8)
            ctx._check(ctx.lib.vpcc_upsample_occupancy(ctx.h, C.byref(d), _abi.VPCC_MEM_DEVICE, out.ctypes.data),
                       "vpcc_upsample_occupancy")
            want = np.repeat(np.repeat(f["occupancy"], prec, axis=0), prec, axis=1)
            bad = np.argwhere(out != want)
            assert len(bad) == 0, f"precision {prec}: {len(bad)} samples differ, first at (y, x) = {tuple(bad[0])}"
            dev.close()
    finally:
        atlas.close()
        del atlas
        _release()
