"""Relaunching a gof over borrowed planes that change between launches (vpcc_recon.h, vpcc_gof_block_to_patch: a gof that
borrows the caller's device planes may be launched again after new frames have been decoded into them).  Every launch
plans from the occupancy as it is THEN; nothing of an earlier launch — point counts, ticket counters, look-back words,
the tile map, error flags, smoothing scratch, a recycled arena — may show through.  Each frame slot cycles through
occupancy states (full, empty, sparse, another frame's planes, over capacity), refilled on the launch stream without
any host synchronisation, and every launched frame is compared bit for bit with the CPU oracle on "the gof's patch
table over the planes the slot held at that launch"."""
import ctypes as C

import numpy as np
import pytest

import cases
import oracle_binding as ob
from tmc2rs import _abi, recon, synth

pytestmark = pytest.mark.gpu

FLAGS = _abi.VPCC_GOF_PROFILE | _abi.VPCC_GOF_WANT_PATCH_INDEX

# full, empty, sparse, other: every one of the twelve transitions between two different states, in one circuit
CIRCUIT = "FEFSFOESEOSOF"


@pytest.fixture(scope="module")
def ctx():
    c = recon.Context(0)
    yield c
    c.close()


def _hip():
    hip = C.CDLL("libamdhip64.so.7")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return hip


def _device_count(g, frame):
    """The frame's device-side point counter (vpcc_gof_device_outputs), read after the gof's kernels are over."""
    g.sync()
    out = np.zeros(1, np.uint32)
    assert _hip().hipMemcpy(out.ctypes.data, g.device_outputs(frame)[3], 4, 2) == 0     # hipMemcpyDeviceToHost
    return int(out[0])


def _with_planes(base, planes):
    """base's patch table over the planes of `planes` (the gof's patch table is read once, at creation)."""
    f = dict(base)
    f["occupancy"], f["geometry"], f["attribute"] = planes["occupancy"], planes["geometry"], planes["attribute"]
    return f


def _empty(base):
    f = dict(base)
    f["occupancy"] = np.zeros_like(base["occupancy"])
    return f


def _samples_per_block(f):
    R, prec = f["occupancy_resolution"], f["occupancy_precision"]
    return R // prec if R >= prec else 1


def _sparse(base):
    """One occupied block: the last canvas block the patch table owns, every occupancy sample of it set."""
    b2p = ob.block_to_patch(base)[1]
    cb = int(np.flatnonzero(b2p)[-1])
    bw = base["width"] // base["occupancy_resolution"]
    s = _samples_per_block(base)
    f = _empty(base)
    f["occupancy"][(cb // bw) * s:(cb // bw + 1) * s, (cb % bw) * s:(cb % bw + 1) * s] = 1
    return f


def _random_planes(base, seed):
    """Other planes of the same shapes: random occupancy (70 % of the samples, values 1-255), depths and colours."""
    rng = np.random.RandomState(seed)
    occ = base["occupancy"]
    g0 = rng.randint(0, 800, size=base["geometry"][0].shape).astype(np.uint16)
    f = dict(base)
    f["occupancy"] = (rng.randint(1, 256, size=occ.shape) * (rng.rand(*occ.shape) < 0.7)).astype(np.uint8)
    f["geometry"] = [g0, (g0 + 4 * rng.randint(0, 4, size=g0.shape)).astype(np.uint16)]
    f["attribute"] = [tuple(rng.randint(64, 941, size=p.shape).astype(np.uint16) for p in a) for a in base["attribute"]]
    return f


class Slot:
    """Device planes of one frame that a gof borrows (torch is only the allocator), and the states they are refilled with."""

    def __init__(self, base, other_planes):
        import torch
        self.dev = torch.device("cuda:0")
        self.base = base
        self.states = {"F": base, "E": _empty(base), "S": _sparse(base), "O": _with_planes(base, other_planes)}
        self.refs = {}
        self.staged = {k: self._stage(f) for k, f in self.states.items()}       # uploaded once, before any launch
        torch.cuda.synchronize()
        self.desc, self._keep = _abi.host_frame_desc(base)
        self.planes = [torch.empty_like(t) for t in self.staged["F"]]
        ptr = iter([p.data_ptr() for p in self.planes])
        d = self.desc
        d.occupancy.y = next(ptr)
        d.occupancy.stride = d.occupancy.width
        for m in range(base["map_count"]):
            d.geometry[m].y = next(ptr)
        for m in range(len(base["attribute"])):
            d.attribute[m].y, d.attribute[m].u, d.attribute[m].v = next(ptr), next(ptr), next(ptr)

    def _stage(self, f):
        import torch
        arrs = [f["occupancy"]] + list(f["geometry"][:f["map_count"]]) + [p for a in f["attribute"] for p in a]
        return [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(self.dev) for a in arrs]

    def ref(self, state):
        if state not in self.refs:
            st, r = ob.reconstruct(self.states[state])
            assert st == 0
            self.refs[state] = r
        return self.refs[state]

    def fill(self, state, stream):
        """Refills the planes on `stream` (enqueued only: no synchronisation with the host)."""
        import torch
        with torch.cuda.stream(stream):
            for p, t in zip(self.planes, self.staged[state]):
                p.copy_(t, non_blocking=True)


def _check(res, ref):
    assert res["n"] == ref["n"]
    assert np.array_equal(res["xyz"], ob.xyz_array(ref)), "integer geometry must be bit-exact"
    assert np.array_equal(res["rgb"], ob.rgb_array(ref)), "8-bit colour must be bit-exact"
    assert np.array_equal(res["patch_index"].astype(np.uint64), ref["partition"])


def _n_blocks(f):
    return (f["width"] // f["occupancy_resolution"]) * (f["height"] // f["occupancy_resolution"])


def _check_frame(g, i, base, ref, capacity, tile, counts=None, b2p=True):
    """Everything the gof reports of frame i against the oracle's reconstruction `ref`."""
    counts = g.point_counts() if counts is None else counts
    assert int(counts[i]) == ref["n"], (i, int(counts[i]), ref["n"])
    assert _device_count(g, i) == ref["n"]
    if ref["n"] > capacity:
        assert g.frame_status(i) == _abi.VPCC_ERR_CAPACITY
        with pytest.raises(recon.VpccError) as e:
            g.download(i, want_patch_index=True)
        assert e.value.status == _abi.VPCC_ERR_CAPACITY
    else:
        assert g.frame_status(i) == _abi.VPCC_OK
        _check(g.download(i, want_patch_index=True), ref)
    if b2p:
        m, items = g.block_to_patch(i, _n_blocks(base))
        assert np.array_equal(m.astype(np.uint64), ref["block_to_patch"])
        assert items == (int(np.count_nonzero(ref["block_to_patch"])) if tile else 0)


def _many_patches_frame():
    """2 049 patches, one more than k_plan_tiles' LDS takes: the tile path plans it in global memory by itself."""
    small = cases.medium_frame(7)
    f = dict(small)
    f["patches"] = np.concatenate([small["patches"]] * (2049 // len(small["patches"]) + 1))[:2049]
    return f


# name -> (environment, frames and the planes of their "other" state, kernels of a launch)
PATHS = {
    "tile_lds": ({}, lambda: [(synth.longdress_frame(1), synth.longdress_frame(2)),
                              (synth.longdress_frame(3), synth.longdress_frame(4))],
                 ["k_plan_tiles", "k_recon_tiles"]),
    "tile_global": ({"VPCC_NO_LDS_PLANNING": "1"}, lambda: [(synth.longdress_frame(1), synth.longdress_frame(2)),
                                                           (cases.medium_frame(1), cases.medium_frame(2))],
                    ["k_plan_cover+items", "k_recon_tiles"]),
    "tile_beyond_lds": ({}, lambda: [(_many_patches_frame(), cases.medium_frame(8)), (cases.medium_frame(3), cases.medium_frame(4))],
                        ["k_plan_cover+items", "k_recon_tiles"]),
    # R = 32 (several chunks per virtual block): the units of k_general_blocks
    "general_blocks": ({}, lambda: [(cases.block32_frame(), synth.make_frame(128, 96, 1, 32, seed=79, max_side=2, cover_target=0.9)),
                                    (synth.make_frame(128, 96, 1, 32, seed=80, max_side=3, cover_target=0.8), None)],
                       ["k_block_owner", "k_general_blocks"]),
    # R = 8 takes k_general by itself; the environment sends the exotic orientations' and the R = 32 frame there too
    "general_any": ({"VPCC_GENERAL_ANY_FRAME": "1"}, lambda: [(cases.exotic_frame(), None), (cases.block8_frame(), None),
                                                             (cases.block32_frame(), None)],
                    ["k_block_owner", "k_general"]),
}


def _slots(pairs, seed=1):
    return [Slot(base, other if other is not None else _random_planes(base, seed + k)) for k, (base, other) in enumerate(pairs)]


def _capacity_between(slot):
    """A capacity between the counts of the full and the other state: the larger one does not fit."""
    a, b = sorted((slot.ref("F")["n"], slot.ref("O")["n"]))
    assert b - a >= 2, (a, b)
    return (a + b) // 2


@pytest.mark.parametrize("path", sorted(PATHS))
def test_every_launch_follows_the_planes(ctx, monkeypatch, path):
    """Two or three frame slots cycle through full (F), empty (E), sparse (S) and other (O) planes — slot 0 along a circuit
    that makes every transition once, slot 1 along it backwards, slot 2 from another start — with a launch after each
    refill.  The capacity lies between the counts of F and O of slot 0, so one of them reports VPCC_ERR_CAPACITY with its
    true count, and the launch after it must download cleanly.  Points, colours, patch indices, counts (host and device), status and block_to_patch against
    the oracle after every launch; the kernels of every launch are those of the path."""
    import torch
    env, make, kernels = PATHS[path]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    slots = _slots(make())
    capacity = _capacity_between(slots[0])
    tile = kernels[-1] == "k_recon_tiles"
    g = ctx.gof(None, capacity=capacity, memory=_abi.VPCC_MEM_DEVICE, descs=[s.desc for s in slots], flags=FLAGS)
    stream = torch.cuda.Stream(device=torch.device("cuda:0"))
    c = CIRCUIT[:-1]                                    # (a closed circuit: its rotations and its reverse are circuits too)
    orders = [CIRCUIT, CIRCUIT[::-1], c[4:] + c[:4] + c[4]][:len(slots)]
    seen = set()
    for step in range(len(CIRCUIT)):
        states = [o[step] for o in orders]
        for s, st in zip(slots, states):
            s.fill(st, stream)
        g.reconstruct(stream=stream.cuda_stream)
        assert [k for k, _ in g.kernel_times()] == kernels
        counts = g.point_counts()
        for i, (s, st) in enumerate(zip(slots, states)):
            ref = s.ref(st)
            seen.add(ref["n"] > capacity)
            _check_frame(g, i, s.base, ref, capacity, tile, counts)
    assert seen == {True, False}
    g.close()


@pytest.mark.parametrize("path", ["tile", "general"])
def test_unchanged_neighbours_and_sub_ranges(ctx, path):
    """Ten frames (nine or more: the general sequence takes its eight-lane shape), of which only some change state between
    launches, over full and sub-range launches; a frame is emptied inside a sub-range.  Frames of a launch's range against
    the oracle on their planes of then; a frame outside it keeps the results of the last launch that covered it
    (vpcc_gof_reconstruct) — even when its planes have been refilled since."""
    import torch
    n = 10
    if path == "tile":
        pairs = [(cases.medium_frame(20 + i, occupancy_values="random" if i % 3 == 0 else "one"), None) for i in range(n)]
    else:
        pairs = [(synth.make_frame(72, 40, 2, 8, seed=300 + i, max_side=3, cover_target=0.7), None) for i in range(n)]
    slots = _slots(pairs, seed=50)
    g = ctx.gof(None, capacity=1 << 20, memory=_abi.VPCC_MEM_DEVICE, descs=[s.desc for s in slots], flags=FLAGS)
    stream = torch.cuda.Stream(device=torch.device("cuda:0"))
    state = ["F"] * n
    for s in slots:
        s.fill("F", stream)
    covered = [None] * n                               # the state each frame had at the last launch that covered it
    plan = [  # (refills {frame: state}, first, count)
        ({}, 0, n),
        ({2: "E", 5: "O"}, 0, n),
        ({2: "F", 3: "E", 7: "S"}, 1, 5),             # 7 refilled outside the range: it keeps its results of launch 2
        ({3: "F", 4: "E"}, 3, 6),                     # overlaps the previous range; 4 emptied inside it
        ({4: "O", 0: "E", 9: "S"}, 0, 4),
        ({1: "E", 2: "S"}, 0, n),
        ({1: "F", 5: "E", 6: "E"}, 5, 5),
        ({5: "F"}, 2, 8),
    ]
    tile = path == "tile"
    for refills, first, count in plan:
        for i, st in refills.items():
            slots[i].fill(st, stream)
            state[i] = st
        g.reconstruct(first=first, count=count, stream=stream.cuda_stream)
        for i in range(first, first + count):
            covered[i] = state[i]
        counts = g.point_counts()
        for i in range(n):
            if covered[i] is None:                     # never launched: the header promises nothing of it
                continue
            # block_to_patch plans again from the planes as they are now (tile path): asked of in-range frames only
            _check_frame(g, i, slots[i].base, slots[i].ref(covered[i]), 1 << 20, tile, counts, b2p=first <= i < first + count)
    g.close()


@pytest.mark.parametrize("path", ["tile_lds", "tile_global", "general"])
def test_block_to_patch_query_between_refill_and_launch(ctx, monkeypatch, path):
    """Slots refilled (and the refill complete), then vpcc_gof_block_to_patch, then downloads — all before the next launch:
    the query re-plans from the new planes on the tile path with planning in LDS (with the other paths it returns the last
    launch's map) and must not touch the last launch's results — a frame just emptied still downloads the previous
    launch's points.  The next launch follows the new planes."""
    import torch
    if path == "tile_global":
        monkeypatch.setenv("VPCC_NO_LDS_PLANNING", "1")
    pairs = ([(synth.longdress_frame(5), synth.longdress_frame(6)), (cases.medium_frame(9), None)] if path != "general"
             else [(cases.block8_frame(), None), (cases.block32_frame(), None)])
    slots = _slots(pairs, seed=70)
    g = ctx.gof(None, capacity=1 << 21, memory=_abi.VPCC_MEM_DEVICE, descs=[s.desc for s in slots], flags=FLAGS)
    tile = path != "general"
    stream = torch.cuda.Stream(device=torch.device("cuda:0"))
    prev = ["F", "O"]
    for s, st in zip(slots, prev):
        s.fill(st, stream)
    g.reconstruct(stream=stream.cuda_stream)
    for nxt in (["E", "S"], ["O", "E"], ["F", "F"]):
        for s, st in zip(slots, nxt):
            s.fill(st, stream)
        stream.synchronize()                           # (the query runs on the library's own stream: the refill must be there)
        for i, s in enumerate(slots):
            m, items = g.block_to_patch(i, _n_blocks(s.base))
            planned = s.ref(nxt[i] if path == "tile_lds" else prev[i])
            assert np.array_equal(m.astype(np.uint64), planned["block_to_patch"])
            assert items == (int(np.count_nonzero(planned["block_to_patch"])) if tile else 0)
        counts = g.point_counts()
        for i, s in enumerate(slots):                  # the previous launch's results, untouched by the query
            assert int(counts[i]) == s.ref(prev[i])["n"]
            assert _device_count(g, i) == s.ref(prev[i])["n"]
            _check(g.download(i, want_patch_index=True), s.ref(prev[i]))
        g.reconstruct(stream=stream.cuda_stream)
        for i, s in enumerate(slots):
            _check_frame(g, i, s.base, s.ref(nxt[i]), 1 << 21, tile)
        prev = nxt
    g.close()


def test_smoothing_after_relaunches(ctx):
    """vpcc_gof_smooth reads each frame's point count on the device: after launches that emptied a frame (zero points) or
    refilled it, the smoothed result is the specification's (oracle/vpcc_smoothing_spec.c) on the oracle's reconstruction
    of the frame's planes of then."""
    import torch
    params = dict(grid_size=8, threshold=1, color_grid_size=8, color_threshold_smoothing=5, color_threshold_difference=200)
    pairs = [(cases.overlapping_3d_frame(i), None) for i in range(3)]
    slots = _slots(pairs, seed=90)
    g = ctx.gof(None, capacity=1 << 20, memory=_abi.VPCC_MEM_DEVICE, descs=[s.desc for s in slots], flags=FLAGS)
    stream = torch.cuda.Stream(device=torch.device("cuda:0"))
    moved = False
    for states in (["F", "F", "F"], ["E", "F", "S"], ["F", "E", "F"], ["S", "E", "E"], ["F", "F", "F"]):
        for s, st in zip(slots, states):
            s.fill(st, stream)
        g.reconstruct(stream=stream.cuda_stream)
        g.smooth(10, stream=stream.cuda_stream, **params)
        counts = g.point_counts()
        for i, (s, st) in enumerate(zip(slots, states)):
            ref = s.ref(st)
            assert int(counts[i]) == ref["n"]
            after = g.download(i, want_patch_index=True)
            xyz, part = ob.xyz_array(ref), ref["partition"].astype(np.uint16)
            exp_xyz = ob.spec_smooth_geometry(xyz, part, 10, 8, 1)
            exp_rgb = ob.spec_smooth_color(exp_xyz, ob.rgb_array(ref), part, 10, 8, 5, 200)
            assert after["n"] == ref["n"]
            assert np.array_equal(after["xyz"], exp_xyz), (states, i)
            assert np.array_equal(after["rgb"], exp_rgb), (states, i)
            moved = moved or bool(np.any(exp_xyz != xyz))
    assert moved                                        # the case really exercises the filter
    g.close()


@pytest.mark.parametrize("general", [False, True])
def test_recycled_arena(general):
    """A gof's arena (control words, counts, descriptors) goes to the context's cache when it is destroyed, and the next
    gof of the same layout takes it; its launch generation starts at 1 again, so only the clearing of the control words at
    creation keeps the old owner's ticket and look-back words (tagged with generations 1, 2 ... of ITS launches) from
    being taken for the new gof's.  Gof A is launched once, or three times, on one stream and destroyed; gof B — same
    layout, the arena from the cache (its device counters lie where A's did) — is launched once on ANOTHER stream, its
    slots starting full, then starting empty."""
    import torch
    c = recon.Context(0)                                # a context of its own: its arena cache holds A's arena alone
    flags = FLAGS | (_abi.VPCC_GOF_FORCE_GENERAL if general else 0)
    kernels = ["k_block_owner", "k_general_blocks"] if general else ["k_plan_tiles", "k_recon_tiles"]
    slots = _slots([(cases.medium_frame(40 + i), None) for i in range(3)], seed=110)
    descs = [s.desc for s in slots]
    dev = torch.device("cuda:0")
    sa, sb = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    for a_launches in (1, 3):
        for b_start in ("F", "E"):
            a = c.gof(None, capacity=1 << 20, memory=_abi.VPCC_MEM_DEVICE, descs=descs, flags=flags)
            a_counters = [a.device_outputs(i)[3] for i in range(3)]
            for k in range(a_launches):
                for s, st in zip(slots, "FOS"[k:] + "FOS"[:k]):
                    s.fill(st, sa)
                a.reconstruct(stream=sa.cuda_stream)
            assert [k for k, _ in a.kernel_times()] == kernels
            a.sync()
            a.close()
            states = ["F", "O", "S"] if b_start == "F" else ["E", "E", "F"]
            for s, st in zip(slots, states):
                s.fill(st, sb)
            b = c.gof(None, capacity=1 << 20, memory=_abi.VPCC_MEM_DEVICE, descs=descs, flags=flags)
            assert [b.device_outputs(i)[3] for i in range(3)] == a_counters          # A's arena, from the cache
            b.reconstruct(stream=sb.cuda_stream)
            assert [k for k, _ in b.kernel_times()] == kernels
            counts = b.point_counts()
            for i, (s, st) in enumerate(zip(slots, states)):
                _check_frame(b, i, s.base, s.ref(st), 1 << 20, not general, counts)
            b.close()
    c.close()
