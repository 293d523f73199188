"""Frame digests on the device (vpcc_gof_output_digests / vpcc_gof_plane_digests: k_digest_outputs, k_digest_planes) against
the numpy restatement of the definition, over the CPU oracle's output and the frames' host planes."""
import numpy as np
import pytest

import cases
import digest_ref
import oracle_binding as ob
from tmc2rs import _abi, recon

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = recon.Context(0)
    yield c
    c.close()


def _ref_digest(f):
    st, r = ob.reconstruct(f)
    assert st == 0
    return digest_ref.digest_points(ob.xyz_array(r), ob.rgb_array(r) if f.get("attribute_count", 1) else None)


def _planes(f):
    return [f["occupancy"]] + list(f["geometry"][:f.get("map_count", 2)]) + [p for a in f["attribute"] for p in a] \
        if f.get("attribute_count", 1) else [f["occupancy"]] + list(f["geometry"][:f.get("map_count", 2)])


class DevicePlanes:
    """A frame's planes in device memory (torch is only the allocator), tight, and a VPCC_MEM_DEVICE descriptor over them."""

    def __init__(self, f):
        import torch
        self.f = f
        arrs = [np.ascontiguousarray(a) for a in _planes(f)]
        self.t = [torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to("cuda:0") for a in arrs]
        torch.cuda.synchronize()
        self.desc, self._keep = _abi.host_frame_desc(f)
        ptr = iter([t.data_ptr() for t in self.t])
        d = self.desc
        d.occupancy.y, d.occupancy.stride = next(ptr), arrs[0].shape[1]
        maps = f.get("map_count", 2)
        for m in range(maps):
            d.geometry[m].y, d.geometry[m].stride = next(ptr), arrs[1 + m].shape[1]
        if f.get("attribute_count", 1):
            for m in range(maps):
                d.attribute[m].y, d.attribute[m].u, d.attribute[m].v = next(ptr), next(ptr), next(ptr)
                d.attribute[m].stride = arrs[1 + maps + 3 * m].shape[1]
                d.attribute[m].cstride = arrs[2 + maps + 3 * m].shape[1]

    def refill(self, other):
        """The planes of `other` (same shapes) into the same device memory."""
        import torch
        for t, a in zip(self.t, _planes(other)):
            t.copy_(torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0"))
        torch.cuda.synchronize()


def _other_planes(base, seed):
    rng = np.random.RandomState(seed)
    f = dict(base)
    occ = base["occupancy"]
    f["occupancy"] = (rng.randint(1, 256, size=occ.shape) * (rng.rand(*occ.shape) < 0.7)).astype(np.uint8)
    g0 = rng.randint(0, 800, size=base["geometry"][0].shape).astype(np.uint16)
    f["geometry"] = [g0, (g0 + 4 * rng.randint(0, 4, size=g0.shape)).astype(np.uint16)][:len(base["geometry"])]
    f["attribute"] = [tuple(rng.randint(64, 941, size=p.shape).astype(np.uint16) for p in a) for a in base["attribute"]]
    return f


FLAG_SETS = {"tile": 0, "general": _abi.VPCC_GOF_FORCE_GENERAL, "patch_index": _abi.VPCC_GOF_WANT_PATCH_INDEX}


@pytest.mark.parametrize("flags", sorted(FLAG_SETS))
@pytest.mark.parametrize("name", sorted(cases.PARITY_CASES))
def test_output_digests_equal_the_oracle(ctx, name, flags):
    f = cases.PARITY_CASES[name]()
    other = cases.PARITY_CASES["small0"]()
    frames = [f, other, f]
    refs = [_ref_digest(x) for x in frames]
    g = ctx.gof(frames, flags=FLAG_SETS[flags])
    g.reconstruct(1, 2)                                       # a launch of several frames, not all of the gof
    assert list(g.output_digests(1, 2)) == refs[1:]
    g.reconstruct()
    assert list(g.output_digests()) == refs
    g.close()


def test_output_digests_follow_refilled_borrowed_planes(ctx):
    base = cases.medium_frame(0)
    slots = [DevicePlanes(base), DevicePlanes(cases.medium_frame(0))]
    for flags in (0, _abi.VPCC_GOF_FORCE_GENERAL):
        g = ctx.gof(None, memory=_abi.VPCC_MEM_DEVICE, descs=[s.desc for s in slots], flags=flags)
        g.reconstruct()
        assert list(g.output_digests()) == [_ref_digest(base)] * 2
        other = _other_planes(base, 7 + flags)
        slots[1].refill(other)
        g.reconstruct()
        assert list(g.output_digests()) == [_ref_digest(base), _ref_digest(other)]
        assert g.plane_digests()[1] == digest_ref.digest_planes(other)
        slots[1].refill(base)
        g.close()


def test_output_digests_need_a_launch(ctx):
    g = ctx.gof([cases.PARITY_CASES["small0"]()])
    with pytest.raises(recon.VpccError):
        g.output_digests()
    g.close()


@pytest.mark.parametrize("switch", [None, "VPCC_NO_EXTENT_INGEST", "VPCC_NO_PULL_INGEST"])
def test_plane_digests_of_host_planes(ctx, monkeypatch, switch):
    if switch == "VPCC_NO_PULL_INGEST":
        monkeypatch.setenv("VPCC_NO_EXTENT_INGEST", "1")
    if switch:
        monkeypatch.setenv(switch, "1")
    frames = [cases.PARITY_CASES[n]() for n in sorted(cases.PARITY_CASES)]
    g = ctx.gof(frames, flags=_abi.VPCC_GOF_ASYNC_UPLOAD)
    assert list(g.plane_digests()) == [digest_ref.digest_planes(f) for f in frames]
    g.reconstruct()
    assert list(g.plane_digests(2, 3)) == [digest_ref.digest_planes(f) for f in frames[2:5]]
    g.close()


@pytest.mark.parametrize("copy", [False, True])
def test_plane_digests_of_device_planes(ctx, copy):
    names = ["small0", "no_attribute", "single_map_extension", "block8_ragged", "medium0"]
    frames = [cases.PARITY_CASES[n]() for n in names]
    slots = [DevicePlanes(f) for f in frames]
    g = ctx.gof(None, memory=_abi.VPCC_MEM_DEVICE, descs=[s.desc for s in slots],
                flags=_abi.VPCC_GOF_COPY_PLANES if copy else 0)
    want = [digest_ref.digest_planes(f) for f in frames]
    assert list(g.plane_digests()) == want
    g.reconstruct()
    assert list(g.output_digests()) == [_ref_digest(f) for f in frames]
    assert list(g.plane_digests()) == want
    g.close()
