"""numpy restatement of the plane digest of a semi-planar frame (include/vpcc_recon.h, "frame digests", with
VPCC_FRAME_UV_INTERLEAVED): map m's chroma is one row set p = 4 + 3m of height/2 rows of 4 * (width/2) bytes, the interleaved U,V
pairs as stored; samples are hashed before any shift."""
import numpy as np

import digest_ref


def digest_planes(frame):
    W, H = int(frame["width"]), int(frame["height"])
    occ = np.asarray(frame["occupancy"], dtype=np.uint8)
    rows = [(0, y, occ[y]) for y in range(occ.shape[0])]
    for m in range(int(frame.get("map_count", 2))):
        geo = np.asarray(frame["geometry"][m], dtype=np.uint16)
        rows += [(1 + m, y, geo[y, :W].astype("<u2")) for y in range(H)]
        if int(frame.get("attribute_count", 1)):
            luma, uv = (np.asarray(p, dtype=np.uint16) for p in frame["attribute"][m])
            rows += [(3 + 3 * m, y, luma[y, :W].astype("<u2")) for y in range(H)]
            rows += [(4 + 3 * m, y, uv[y, :2 * (W // 2)].astype("<u2")) for y in range(H // 2)]
    return digest_ref.digest((W << 32) | H, rows)
