#!/usr/bin/env python
"""Write tests/golden/g17_pil_resize.npz from Pillow itself: Image.fromarray(...).resize((w, h), Image.BILINEAR) on the 8-bit RGB
frames and the float32 ("F") flow planes of tests/pil_resize_oracle.py's case table.  transforms.Resize makes that same call for a PIL
image (torchvision's documented behaviour; torchvision is not needed here).  The normalised float output of one case is made with
torch's CPU operators.  Inputs are not stored: the tests regenerate them from the seeds and check their sha256 against the fixture.

    python tools/gen_golden_pil_resize.py [--out tests/golden/g17_pil_resize.npz]
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
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "g17_pil_resize.npz"))
    args = ap.parse_args()

    out = {"pillow_version": np.array(PIL.__version__)}
    for name, (n, src, dst, seed) in R.FRAME_CASES.items():
        frames = R.make_frames(n, src, seed)
        res = np.stack([np.array(Image.fromarray(f).resize((dst[1], dst[0]), Image.BILINEAR)) for f in frames])
        assert res.shape == (n, dst[0], dst[1], 3) and res.dtype == np.uint8
        out["frame_%s_sha" % name] = np.array(R.digest(frames))
        out["frame_%s_u8" % name] = res
        if name == R.NORM_CASE:
            out["frame_%s_norm" % name] = R.normalise(res, R.IMAGENET_MEAN, R.IMAGENET_STD)
    for name, (B, src, dst, seed) in R.FLOW_CASES.items():
        flow = R.make_flow(B, src, seed)
        res = np.stack([np.stack([np.array(Image.fromarray(flow[b, c]).resize((dst[1], dst[0]), Image.BILINEAR)) for c in range(2)])
                        for b in range(B)])
        assert res.shape == (B, 2, dst[0], dst[1]) and res.dtype == np.float32
        out["flow_%s_sha" % name] = np.array(R.digest(flow))
        out["flow_%s_f32" % name] = res
    np.savez_compressed(args.out, **out)
    print("wrote %s (%d bytes, Pillow %s)" % (args.out, os.path.getsize(args.out), PIL.__version__))


if __name__ == "__main__":
    main()
