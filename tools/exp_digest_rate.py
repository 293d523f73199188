#!/usr/bin/env python3
"""Rate of the frame-digest kernels and of the verified Decoder (include/vpcc_recon.h, "frame digests").

  1. k_digest_outputs / k_digest_planes over a 128-frame S-longdress gof (32 distinct frames, four times): each call of
     Gof.output_digests() / plane_digests() = memset + kernel + push of the slots + synchronisation; the mean wall time of a
     call is reported with the kernels' bytes and GB/s (an upper bound of the kernel time: run it under
     `rocprofv3 --kernel-trace --stats -- python tools/exp_digest_rate.py --kernels` for the kernels alone).
  2. frames/s of tmc2rs::Decoder on the 17-GOF stream (17 x 32 S-longdress frames) with verification off, each check alone
     and all three, alternated round by round.
Usage: tools/exp_digest_rate.py [--kernels] [--rounds 2] [--reps 20]   (one JSON line per figure)"""
import argparse, json, os, sys, tempfile, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tmc2-rs_amd"))
import numpy as np
from tmc2rs import container, recon, synth

ap = argparse.ArgumentParser()
ap.add_argument("--kernels", action="store_true", help="the kernels only (no Decoder streams)")
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--reps", type=int, default=20)
args = ap.parse_args()

frames = [synth.longdress_frame(i) for i in range(32)]
ctx = recon.Context(0)
g = ctx.gof(frames * 4)
g.reconstruct()
counts = g.point_counts()
out_bytes = int(9 * counts.sum())
plane_bytes = 0
for f in frames * 4:
    W, H = f["width"], f["height"]
    plane_bytes += f["occupancy"].size + 2 * 2 * W * H + 2 * (2 * W * H + 2 * 2 * (W // 2) * (H // 2))
for name, call, nbytes in (("k_digest_outputs", g.output_digests, out_bytes), ("k_digest_planes", g.plane_digests, plane_bytes)):
    call()                                                  # warm
    t0 = time.perf_counter()
    for _ in range(args.reps):
        call()
    ms = (time.perf_counter() - t0) / args.reps * 1e3
    print(json.dumps({"kernel": name, "frames": 128, "gbytes": round(nbytes / 1e9, 3), "call_ms": round(ms, 3),
                      "gbps_upper_bound_of_call": round(nbytes / ms / 1e6, 1), "copy_rate_gbps": 6300}), flush=True)
g.close()
ctx.close()
if args.kernels:
    sys.exit(0)

d = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
path = os.path.join(d, "stream.vpccgof")
try:
    container.write_container(path, [frames] * 17)
    modes = ["off", "ingest", "reconstruct", "delivery", "all"]
    rates = {m: [] for m in modes}
    for r in range(args.rounds):
        for m in modes:
            dec = recon.Decoder(path, verify=0 if m == "off" else m)
            dec.start()
            nf, npts, sec = dec.drain()
            vs = dec.verify_stats()
            dec.close()
            assert nf == 17 * 32, (m, nf)
            rates[m].append(nf / sec)
            print(json.dumps({"decoder": m, "round": r, "frames": nf, "frames_per_s": round(nf / sec, 1),
                              "verify_host_s": round(vs["host_seconds"], 3), "verify_kernel_s": round(vs["kernel_seconds"], 4)}), flush=True)
    print(json.dumps({"decoder_frames_per_s_median": {m: round(float(np.median(v)), 1) for m, v in rates.items()}}), flush=True)
finally:
    if os.path.exists(path):
        os.remove(path)
    os.rmdir(d)
