#!/usr/bin/env python3
"""Rate of the cloud metrics (include/vpcc_recon.h, "cloud metrics") and what they say about the smoothing.

  1. ms per frame pair, both directions, timed by HIP events on the context's stream around Context.cloud_errors over device
     clouds (borrowed: no staging in the window): an S-longdress frame (~800 k points) against a seeded perturbation of it, and
     an S-owlii frame (~2 M points) likewise.  `compulsory_gbps` = the bytes every direction must read at least — positions and
     colours of both clouds, once as source and once as target: 2 x 9 x (n_a + n_b) — over that time, and its share of the
     measured HBM copy rate (6.3 TB/s).  The search re-reads cells many times over; this is a floor, not the traffic.
  2. The same pair on one host core with scipy's cKDTree (build + query, both directions, k = 1, workers = 1), in the same run.
  3. D1 and colour PSNR between the unsmoothed and the smoothed outputs of the 128 S-longdress frames of a gof
     (vpcc_gof_cloud_errors, bench.py's smoothing parameters) — a figure about the library's own smoothing, not a quality claim.
Usage: tools/exp_metrics_rate.py [--reps 10] [--frames 128]   (one JSON line per figure)"""
import argparse, json, os, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tmc2-rs_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np
import torch
import metrics_ref
from tmc2rs import _abi, recon, synth

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--frames", type=int, default=128)
args = ap.parse_args()

HBM_GBPS = 6300.0
ctx = recon.Context(0)
ext = torch.cuda.ExternalStream(ctx.stream(), device=torch.device("cuda", 0))


def device_cloud(xyz, rgb):
    return (torch.from_numpy(np.ascontiguousarray(xyz, np.uint16).view(np.int16)).cuda(),
            torch.from_numpy(np.ascontiguousarray(rgb, np.uint8)).cuda())


def one_pair(name, make, index, peak):
    g = ctx.gof([make(index)], capacity=2_400_000)
    g.reconstruct()
    out = g.download(0)
    g.close()
    xyz, rgb = out["xyz"], out["rgb"]
    pxyz, prgb = metrics_ref.perturb(xyz, rgb, 0x3E7)
    a, b = device_cloud(xyz, rgb), device_cloud(pxyz, prgb)
    res = ctx.cloud_errors(a, b, peak=peak)                        # warm (scratch allocated, code loaded)
    ms = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(ext)
        ctx.cloud_errors(a, b)
        e1.record(ext)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    nbytes = 2 * 9 * (len(xyz) + len(pxyz))
    med = float(np.median(ms))
    # the CPU baseline: one host core
    from scipy.spatial import cKDTree
    t0 = time.perf_counter()
    ta, tb = cKDTree(xyz.astype(np.float64)), cKDTree(pxyz.astype(np.float64))
    tb.query(xyz.astype(np.float64), k=1, workers=1)
    ta.query(pxyz.astype(np.float64), k=1, workers=1)
    ckd_ms = (time.perf_counter() - t0) * 1e3
    print(json.dumps({"figure": "pair", "workload": name, "n_a": int(len(xyz)), "n_b": int(len(pxyz)), "reps": args.reps,
                      "ms_per_pair_median": round(med, 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3),
                      "compulsory_gbytes": round(nbytes / 1e9, 4), "compulsory_gbps": round(nbytes / med / 1e6, 1),
                      "share_of_hbm_copy_rate": round(nbytes / med / 1e6 / HBM_GBPS, 5),
                      "ckdtree_one_core_ms": round(ckd_ms, 1), "speedup_vs_ckdtree": round(ckd_ms / med, 1),
                      "d1_psnr": round(res["d1_psnr"], 4), "hausdorff2": res["hausdorff2"]}), flush=True)


one_pair("S-longdress", synth.longdress_frame, 3, 1023)
one_pair("S-owlii", synth.owlii_frame, 2, 2047)

# 3. unsmoothed vs smoothed, 128 frames of a gof
frames = [synth.longdress_frame(i) for i in range(args.frames)]
g = ctx.gof(frames, capacity=1_000_000, flags=_abi.VPCC_GOF_WANT_PATCH_INDEX)
g.reconstruct()
before = [g.download(i) for i in range(args.frames)]
g.smooth(10, grid_size=8, threshold=4, color_grid_size=8, color_threshold_smoothing=10, color_threshold_difference=100)
refs = [(o["xyz"], o["rgb"]) for o in before]
t0 = time.perf_counter()
res = g.cloud_errors(refs, peak=1023)
wall = time.perf_counter() - t0


def stats(v):
    v = np.asarray(v, np.float64)
    return {"min": round(float(v.min()), 3), "mean": round(float(v.mean()), 3), "max": round(float(v.max()), 3)}


print(json.dumps({"figure": "smoothing", "frames": args.frames, "points": int(sum(len(o["xyz"]) for o in before)),
                  "call_s_incl_host_staging": round(wall, 3),
                  "d1_psnr": stats([r["d1_psnr"] for r in res]), "d1_mse": stats([r["d1_mse"] for r in res]),
                  "hausdorff2_max": max(r["hausdorff2"] for r in res),
                  "ycc_psnr": [stats([r["ycc_psnr"][c] for r in res]) for c in range(3)],
                  "frames_moved": int(sum(r["ab"]["geo_sse"] > 0 for r in res))}), flush=True)
g.close()
ctx.close()
