#!/usr/bin/env python
"""Write tests/golden/g20_pil_resize_edges.npz from Pillow itself: Image.fromarray(...).resize((w, h), Image.BILINEAR) on the edge
cases of tests/pil_resize_oracle.py (FRAME_EDGE_CASES, PLANE_EDGE_CASES, PLANE_SPECIAL_CASES, AXIS_SWEEP).  The named cases store the
sha256 of their regenerated input and Pillow's output; the sweep stores only the sha256 of Pillow's output bytes per entry (uint8
[entries, 32]) next to its geometry, and the oracle supplies the element-level diagnosis.  g17 is not touched.

    python tools/gen_golden_pil_resize_edges.py [--out tests/golden/g20_pil_resize_edges.npz]
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]


def main():
    import PIL
    from PIL import Image
    import pil_resize_oracle as R

    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "g20_pil_resize_edges.npz"))
    args = ap.parse_args()

    def pil(a, dst):
        return np.array(Image.fromarray(a).resize((dst[1], dst[0]), Image.BILINEAR))

    def pil_planes(x, dst):
        return np.stack([np.stack([pil(p, dst) for p in item]) for item in x])

    out = {"pillow_version": np.array(PIL.__version__)}
    for name, (n, src, dst, seed) in R.FRAME_EDGE_CASES.items():
        frames = R.make_frames(n, src, seed)
        res = np.stack([pil(f, dst) for f in frames])
        assert res.shape == (n, dst[0], dst[1], 3) and res.dtype == np.uint8
        out["frame_%s_sha" % name] = np.array(R.digest(frames))
        out["frame_%s_u8" % name] = res
    for name, (n, c, src, dst, seed) in R.PLANE_EDGE_CASES.items():
        x = R.make_planes(n, c, src, seed)
        res = pil_planes(x, dst)
        assert res.shape == (n, c, dst[0], dst[1]) and res.dtype == np.float32
        out["plane_%s_sha" % name] = np.array(R.digest(x))
        out["plane_%s_f32" % name] = res
    for name, (src, dst, seed) in R.PLANE_SPECIAL_CASES.items():
        x = R.make_special(src, seed)
        res = pil_planes(x, dst)
        assert res.shape == (1, 2, dst[0], dst[1]) and res.dtype == np.float32
        out["special_%s_sha" % name] = np.array(R.digest(x))
        out["special_%s_f32" % name] = res
    geom, d8, df = [], [], []
    for i, (O, src, dst) in enumerate(R.AXIS_SWEEP):
        frame, plane = R.sweep_inputs(i)
        geom.append(src + dst)
        d8.append(R.digest_bytes(pil(frame[0], dst)))
        df.append(R.digest_bytes(pil(plane, dst)))
    out["sweep_geometry"] = np.array(geom, np.int32)          # (H, W, h, w) per entry: pins the table the digests belong to
    out["sweep_u8_sha"] = np.stack(d8)
    out["sweep_f32_sha"] = np.stack(df)
    np.savez_compressed(args.out, **out)
    print("wrote %s (%d bytes, Pillow %s, %d sweep entries)" % (args.out, os.path.getsize(args.out), PIL.__version__, len(geom)))


if __name__ == "__main__":
    main()
