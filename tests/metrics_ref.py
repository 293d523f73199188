"""CPU restatement of the cloud metrics of include/vpcc_recon.h ("cloud metrics"): the nearest neighbour of every source point
in a target cloud (exact integer d²; ties to the smallest target index) and the sums of one direction S->T.

scipy.spatial.cKDTree finds the nearest distance; the tie rule is applied on top of it (the k nearest candidates, or every point
within that distance when all k tie).  Without scipy the restatement falls back to an exhaustive search in blocks (exact, slow
on large clouds)."""
import numpy as np

try:
    from scipy.spatial import cKDTree
except ImportError:                     # pragma: no cover - scipy is part of the test image
    cKDTree = None

_K = 8


def _d2(src, tgt, idx):
    d = src.astype(np.int64) - tgt[idx].astype(np.int64)
    return (d * d).sum(axis=-1).astype(np.uint64)


def nearest_brute(src, tgt, block=1024):
    """Exhaustive search: (index uint32, d² uint64) of every source point; the smallest index among equal d²."""
    src = np.asarray(src, np.int64).reshape(-1, 3)
    tgt = np.asarray(tgt, np.int64).reshape(-1, 3)
    n = src.shape[0]
    idx = np.full(n, 0xFFFFFFFF, np.uint32)
    d2 = np.full(n, np.iinfo(np.uint64).max, np.uint64)
    if not len(tgt):
        return idx, d2
    for b in range(0, n, block):
        d = src[b:b + block, None, :] - tgt[None, :, :]
        dd = (d * d).sum(axis=-1)
        k = dd.argmin(axis=1)                          # argmin: the FIRST index of the minimum
        idx[b:b + block] = k
        d2[b:b + block] = dd[np.arange(len(k)), k]
    return idx, d2


def nearest(src, tgt):
    """(index uint32, d² uint64) of every point of src in tgt, by the library's rule."""
    src = np.asarray(src, np.int64).reshape(-1, 3)
    tgt = np.asarray(tgt, np.int64).reshape(-1, 3)
    n, m = src.shape[0], tgt.shape[0]
    if cKDTree is None or m == 0 or n == 0:
        return nearest_brute(src, tgt)
    tree = cKDTree(tgt.astype(np.float64))
    k = min(_K, m)
    _, cand = tree.query(src.astype(np.float64), k=k)
    cand = cand.reshape(n, k)
    cd2 = _d2(src[:, None, :], tgt, cand)               # exact: the k nearest (their order among equal distances is arbitrary)
    best = cd2.min(axis=1)
    masked = np.where(cd2 == best[:, None], cand, np.iinfo(np.int64).max)
    idx = masked.min(axis=1)
    # where all k candidates tie, more points may lie at the same distance: every one of them, from the ball
    more = np.nonzero(cd2[:, k - 1] == best)[0] if k < m else np.zeros(0, np.int64)
    for i in more:
        r = float(np.sqrt(float(best[i])))
        ball = np.asarray(tree.query_ball_point(src[i].astype(np.float64), r * (1 + 1e-12) + 1e-9), np.int64)
        bd = _d2(src[i][None, :], tgt, ball)
        idx[i] = ball[bd == best[i]].min()
    return idx.astype(np.uint32), best.astype(np.uint64)


def ycc_terms(drgb):
    """dY, dCb, dCr of per-point colour differences (float64, left to right as the header writes them)."""
    dR, dG, dB = (drgb[:, c].astype(np.float64) for c in range(3))
    y = 0.2126 * dR + 0.7152 * dG + 0.0722 * dB
    cb = -0.1146 * dR - 0.3854 * dG + 0.5 * dB
    cr = 0.5 * dR - 0.4542 * dG - 0.0458 * dB
    return y, cb, cr


def direction(s_xyz, s_rgb, t_xyz, t_rgb, nn=None):
    """The sums of one direction S->T, as the dict of tmc2rs.recon.Context.cloud_errors (nn: precomputed nearest())."""
    s_xyz = np.asarray(s_xyz).reshape(-1, 3)
    t_xyz = np.asarray(t_xyz).reshape(-1, 3)
    n, m = len(s_xyz), len(t_xyz)
    colour = s_rgb is not None and t_rgb is not None
    out = {"n_src": n, "n_tgt": m, "has_color": colour, "geo_sse": 0, "geo_max": 0, "rgb_sse": [0, 0, 0],
           "ycc_sse": [0.0, 0.0, 0.0]}
    if n == 0 or m == 0:
        return out
    idx, d2 = nearest(s_xyz, t_xyz) if nn is None else nn
    out["geo_sse"] = int(d2.sum(dtype=np.uint64))
    out["geo_max"] = int(d2.max())
    if colour:
        drgb = np.asarray(s_rgb).reshape(-1, 3).astype(np.int64) - np.asarray(t_rgb).reshape(-1, 3)[idx].astype(np.int64)
        out["rgb_sse"] = [int((drgb[:, c] ** 2).sum()) for c in range(3)]
        out["ycc_sse"] = [float((t * t).sum()) for t in ycc_terms(drgb)]
    return out


def pair(a_xyz, a_rgb, b_xyz, b_rgb):
    """{"ab": A->B, "ba": B->A}."""
    return {"ab": direction(a_xyz, a_rgb, b_xyz, b_rgb), "ba": direction(b_xyz, b_rgb, a_xyz, a_rgb)}


def perturb(xyz, rgb, seed, jitter_share=0.3, drop=0.05, add=0.05, colour_noise=6):
    """A seeded perturbation of a cloud: jitter of ±1..2 on a subset, `drop` of the points removed, `add` new points near
    existing ones, colour noise of ±colour_noise."""
    rng = np.random.RandomState(seed)
    xyz = np.asarray(xyz, np.int64).reshape(-1, 3)
    rgb = np.asarray(rgb, np.int64).reshape(-1, 3)
    n = len(xyz)
    out = xyz.copy()
    j = rng.rand(n) < jitter_share
    out[j] += rng.randint(-2, 3, size=(int(j.sum()), 3))
    col = rgb + rng.randint(-colour_noise, colour_noise + 1, size=rgb.shape)
    keep = rng.rand(n) >= drop
    out, col = out[keep], col[keep]
    k = int(add * n)
    src = rng.randint(0, n, size=k)
    new = xyz[src] + rng.randint(-3, 4, size=(k, 3))
    newc = rgb[src] + rng.randint(-20, 21, size=(k, 3))
    out = np.concatenate([out, new])
    col = np.concatenate([col, newc])
    return np.clip(out, 0, 65535).astype(np.uint16), np.clip(col, 0, 255).astype(np.uint8)
