"""numpy restatement of the frame digest (include/vpcc_recon.h, "frame digests")."""
import numpy as np

G = 0x9E3779B97F4A7C15
MASK = (1 << 64) - 1


def mix64(z):
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = z ^ (z >> np.uint64(30))
        z = z * np.uint64(0xBF58476D1CE4E5B9)
        z = z ^ (z >> np.uint64(27))
        z = z * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def row_sum(data, p, y):
    """Σ_k mix64(q_k ^ (((p << 56) | (y << 32) | k) * G)) over the bytes of one row."""
    b = np.frombuffer(np.ascontiguousarray(data).tobytes(), dtype=np.uint8)
    if len(b) == 0:
        return 0
    q = np.concatenate([b, np.zeros((-len(b)) % 8, np.uint8)]).view("<u8").astype(np.uint64)
    k = np.arange(len(q), dtype=np.uint64)
    with np.errstate(over="ignore"):
        pos = (np.uint64((p << 56) | (y << 32)) | k) * np.uint64(G)
        return int(mix64(q ^ pos).sum(dtype=np.uint64))


def digest(head, rows):
    """rows: iterable of (p, y, row bytes)."""
    return (int(mix64(np.uint64(head & MASK) ^ np.uint64(G))) + sum(row_sum(r, p, y) for p, y, r in rows)) & MASK


def digest_points(xyz, rgb=None):
    xyz = np.ascontiguousarray(xyz, dtype=np.uint16).reshape(-1, 3)
    rows = [(0, 0, xyz)] + ([(1, 0, np.ascontiguousarray(rgb, dtype=np.uint8).reshape(-1, 3))] if rgb is not None else [])
    return digest(len(xyz), rows)


def digest_planes(frame):
    W, H = int(frame["width"]), int(frame["height"])
    occ = np.asarray(frame["occupancy"], dtype=np.uint8)
    rows = [(0, y, occ[y]) for y in range(occ.shape[0])]
    for m in range(int(frame.get("map_count", 2))):
        geo = np.asarray(frame["geometry"][m], dtype=np.uint16)
        rows += [(1 + m, y, geo[y, :W].astype("<u2")) for y in range(H)]
        if int(frame.get("attribute_count", 1)):
            for c, plane in enumerate(frame["attribute"][m]):
                plane = np.asarray(plane, dtype=np.uint16)
                w, h = (W, H) if c == 0 else (W // 2, H // 2)
                rows += [(3 + 3 * m + c, y, plane[y, :w].astype("<u2")) for y in range(h)]
    return digest((W << 32) | H, rows)
