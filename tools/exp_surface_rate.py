#!/usr/bin/env python3
"""Reconstruction rate on planar device planes against the SAME frames as P016 device surfaces (include/vpcc_recon.h,
VPCC_FRAME_UV_INTERLEAVED + VPCC_FRAME_GEO_SHIFT(6) / _ATTR_SHIFT(6)).

A 128-frame S-longdress launch (32 distinct frames, four times, as bench.py) in two forms, both borrowed by the library
(VPCC_MEM_DEVICE) from memory of the context's pool, eight frames per allocation, frames 0-7 in home 0, 8-15 in home 1, ...
(vpcc_ctx_pool_alloc, as bench.py's fresh_gof leg places them):
  planar   tight yuv420p10le planes;
  p016     synth.to_semiplanar(shift=6, junk low bits): 256-byte row pitch, the UV plane a buffer of its own.
Each round times `--launches` back-to-back launches of each form with HIP events on the context's stream, the forms
alternating within the process after a warm-up; reported: median ms per launch over the rounds, and the per-kernel means of
the profiled launches (VPCC_GOF_PROFILE).  --general: the same with VPCC_GOF_FORCE_GENERAL (k_block_owner + k_general_blocks).
Also printed: the bytes of the conversion pass a caller would otherwise need (P016 -> planar: read and write every geometry and
attribute sample once) and, timed, a naive converter built from torch elementwise operations (this tool only).
Usage: tools/exp_surface_rate.py [--rounds 7] [--launches 20] [--no-general] [--no-convert]   (one JSON line per figure)"""
import argparse, ctypes as C, json, os, sys
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tmc2-rs_amd"))
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--launches", type=int, default=20)
ap.add_argument("--frames", type=int, default=32, help="distinct frames (x4 per launch)")
ap.add_argument("--no-general", action="store_true")
ap.add_argument("--no-convert", action="store_true")
args = ap.parse_args()

import torch
if torch.cuda.device_count() == 0:
    sys.exit("exp_surface_rate.py measures the GPU: no GPU here")

from tmc2rs import _abi, recon, synth

hip = C.CDLL("libamdhip64.so.7")
hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]

distinct = [synth.longdress_frame(i) for i in range(args.frames)]
surfaces = [synth.to_semiplanar(f, shift=6, junk_seed=0x5F + i, pitch_align=256, uv_separate=True) for i, f in enumerate(distinct)]
ctx = recon.Context(0)
ctx.reserve(16)
held, keeps = [], []


def place(frames):
    """FrameDesc[len(frames) * 4] over device copies of the frames' buffers, in the pool's homes."""
    batch = frames * 4
    arr = (_abi.FrameDesc * len(batch))()
    for r0 in range(0, len(batch), 8):
        run = batch[r0:r0 + 8]
        descs = [_abi.host_frame_desc(f) for f in run]
        roots = [recon.DeviceFrame._roots_of(k[:-1]) for _, k in descs]
        total = sum((r.nbytes + 255) // 256 * 256 for rs in roots for r in rs)
        base = ctx.pool_alloc((r0 // 8) % 2, total)
        held.append(base)
        at = base
        for j, ((d, keep), rs) in enumerate(zip(descs, roots)):
            where = []
            for r in rs:
                assert hip.hipMemcpy(at, r.ctypes.data, r.nbytes, 1) == 0
                where.append((r.ctypes.data, r.nbytes, at))
                at += (r.nbytes + 255) // 256 * 256

            def remap(p):
                for lo, n, dev in where:
                    if lo <= p < lo + n:
                        return dev + (p - lo)
                raise ValueError(p)
            d.occupancy.y = remap(d.occupancy.y)
            for m in range(2):
                for img in (d.geometry[m], d.attribute[m]):
                    for name in ("y", "u", "v"):
                        if getattr(img, name):
                            setattr(img, name, remap(getattr(img, name)))
            keeps.append(keep)                       # (the patch tables stay on the host: alive until the gofs are made)
            arr[r0 + j] = d
    return arr


forms = {"planar": place(distinct), "p016": place(surfaces)}
ext = torch.cuda.ExternalStream(ctx.stream(), device=torch.device("cuda", 0))


def run(general):
    flags = _abi.VPCC_GOF_PROFILE | (_abi.VPCC_GOF_FORCE_GENERAL if general else 0)
    gofs = {k: ctx.gof(None, capacity=1_000_000, flags=flags, memory=_abi.VPCC_MEM_DEVICE, descs=arr) for k, arr in forms.items()}
    counts, digests = {}, {}
    for k, g in gofs.items():
        g.reconstruct()
        counts[k] = g.point_counts().copy()
        digests[k] = list(g.output_digests())
    assert np.array_equal(counts["planar"], counts["p016"]) and digests["planar"] == digests["p016"], "the two forms differ"
    for _ in range(2):                                   # warm-up: clocks up, code objects loaded
        for g in gofs.values():
            for _ in range(args.launches):
                g.reconstruct()
            g.sync()
    ms = {k: [] for k in gofs}
    for r in range(args.rounds):
        for k in (list(gofs) if r % 2 == 0 else list(gofs)[::-1]):
            g = gofs[k]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(ext)
            for _ in range(args.launches):
                g.reconstruct()
            e1.record(ext)
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / args.launches)
    kern = {k: g.kernel_time_means(args.rounds * args.launches)[0] for k, g in gofs.items()}
    med = {k: float(np.median(v)) for k, v in ms.items()}
    main = "k_general_blocks" if general else "k_recon_tiles"
    print(json.dumps({"path": "general" if general else "tiles", "frames_per_launch": len(forms["planar"]),
                      "points_per_launch": int(counts["planar"].sum()),
                      "ms_per_launch_median": {k: round(v, 4) for k, v in med.items()},
                      "ms_per_launch_all": {k: [round(x, 4) for x in v] for k, v in ms.items()},
                      "kernel_ms_mean": {k: {n: round(t, 4) for n, t in v.items()} for k, v in kern.items()},
                      "p016_vs_planar": round(med["p016"] / med["planar"] - 1.0, 4),
                      "p016_vs_planar_" + main: round(kern["p016"][main] / kern["planar"][main] - 1.0, 4)}), flush=True)
    for g in gofs.values():
        g.close()


run(False)
if not args.no_general:
    run(True)

if not args.no_convert:
    # The pass this feature makes unnecessary: P016 surfaces -> tight yuv420p10le planes, every geometry and attribute sample
    # read once and written once.
    f = distinct[0]
    W, H = f["width"], f["height"]
    per_frame = 2 * (2 * W * H * 2) + 2 * (W * H * 2 + 2 * (W // 2) * (H // 2) * 2)     # geometry + attribute samples, bytes
    n = 4 * len(distinct)
    dev = torch.device("cuda", 0)
    s = surfaces[0]
    # (as int16: torch's uint16 support is limited; a logical shift is an arithmetic one masked)
    src = [torch.from_numpy(np.ascontiguousarray(g).view(np.int16)).to(dev) for g in s["geometry"]] + \
          [torch.from_numpy(np.ascontiguousarray(p).view(np.int16)).to(dev) for a in s["attribute"] for p in a]

    def convert():
        out = []
        for t in src[:2]:
            out.append((t >> 6) & 0x3FF)
        for k in range(2):
            y, uv = src[2 + 2 * k], src[3 + 2 * k]
            out += [(y >> 6) & 0x3FF, ((uv[:, 0::2] >> 6) & 0x3FF).contiguous(), ((uv[:, 1::2] >> 6) & 0x3FF).contiguous()]
        return out
    for _ in range(3):
        convert()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        convert()
    e1.record()
    e1.synchronize()
    conv_ms = e0.elapsed_time(e1)
    print(json.dumps({"conversion_pass": "P016 surfaces -> planar yuv420p10le, per 128-frame launch",
                      "bytes_read": per_frame * n, "bytes_written": per_frame * n, "bytes_total": 2 * per_frame * n,
                      "naive_torch_converter_ms_per_launch": round(conv_ms, 3),
                      "note": "the converter is torch elementwise operations in this tool, timed on one frame's surfaces "
                              "converted 128 times; the library reads the surfaces in place and runs no such pass"}), flush=True)

for p in held:
    ctx.pool_free(p)
ctx.close()
