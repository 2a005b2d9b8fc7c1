"""Generate tests/golden/g22_inference_eval.npz from the REFERENCE's own inference.py functions, on the CPU.

Runs only where the reference tree is available (default ../reference, or PWC_REFERENCE) and Pillow is installed; the tests read the
fixture.  Recipe as tools/gen_golden_kitti_score.py: process-local module stubs, no reference file is edited -- ``torchvision`` and
``torchvision.transforms`` become empty modules and the repository root supplies the ``correlation_cuda`` shim that the reference's
``models`` package imports.

Per case of tests/inference_eval_cases.py (inputs are made there from seeds; only results are stored) and per sample the
reference's own ``resize_flow``, ``compute_epe`` and ``compute_fl`` run on float32 inputs, and ``save_flow`` runs with
``Image.fromarray`` replaced for that one call by a function that keeps the array it is handed (the real one raises TypeError for a
uint16 [H,W,3] array, so the reference never gets to write a file).  Stored per case:
  flow        [B,2,H,W] float32  resize_flow's result   (cases over inference_eval_cases.SMALL elements: flow_digest, sha256)
  enc         [B,H,W,3] uint16   save_flow's array      (likewise enc_digest)
  epe, fl     [B] float64        compute_epe / compute_fl
  n_valid, n_outlier [B] int64   the counts behind fl
The generator ASSERTS what the tests rely on: tests/pil_resize_oracle.resize_flow equals the reference's resize_flow bit for bit,
the outlier count implied by compute_fl equals the count of the reference-style predicate on the float32 maps, and every case has
outliers and non-outliers among its valid pixels (except the one-pixel case).

    python tools/gen_golden_inference_eval.py [out.npz]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden_proxy_loss import REF, REPO, _stub  # noqa: E402

sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import inference_eval_cases as C  # noqa: E402
import inference_eval_oracle as O  # noqa: E402
import pil_resize_oracle as R  # noqa: E402


def _import_reference():
    tv = _stub("torchvision")
    tv.transforms = _stub("torchvision.transforms")
    for m in [k for k in sys.modules if k == "models" or k.startswith("models.")]:
        del sys.modules[m]                 # the reference's script imports its own `models` package
    sys.path.insert(0, REF)
    import inference as ri                 # noqa: E402  (the reference's script)
    sys.path.remove(REF)
    return ri


def _saved_array(ri, flow_hw2):
    """The array the reference's save_flow hands to Image.fromarray."""
    kept = []

    class _Sink:
        def save(self, path):
            pass

    def fromarray(a, *args, **kw):
        kept.append(np.array(a))
        return _Sink()
    real = ri.Image.fromarray
    ri.Image.fromarray = fromarray
    try:
        ri.save_flow(flow_hw2, os.devnull, "000000_10.png")
    finally:
        ri.Image.fromarray = real
    assert len(kept) == 1 and kept[0].dtype == np.uint16
    return kept[0]


def main(out_path):
    ri = _import_reference()
    arrays = {}
    for name, (B, hw, HW, seed) in C.CASES.items():
        flow = C.make_flow(name)
        pred = np.stack([ri.resize_flow(flow[b].copy(), HW).transpose(2, 0, 1) for b in range(B)])
        assert pred.dtype == np.float32 and pred.shape == (B, 2) + HW
        assert np.array_equal(pred.view(np.int32), R.resize_flow(flow, HW).view(np.int32)), name
        gt, valid = C.make_gt(name, pred)
        enc = np.stack([_saved_array(ri, np.ascontiguousarray(pred[b].transpose(1, 2, 0))) for b in range(B)])
        epe_map, mag = O.epe_maps(pred, gt)
        rows = {k: [] for k in ("epe", "fl", "nv", "no")}
        for b in range(B):
            p = np.ascontiguousarray(pred[b].transpose(1, 2, 0))
            e, f = ri.compute_epe(p, gt[b], valid[b]), ri.compute_fl(p, gt[b], valid[b])
            nv = int(valid[b].sum())
            no = int(round(f * nv / 100.0))
            assert no == int((O.outliers_reference(epe_map[b], mag[b]) & valid[b]).sum()), (name, b)
            if nv > 1:
                assert 0 < no < nv, (name, b, no, nv)
            for k, v in zip(rows, (e, f, nv, no)):
                rows[k].append(v)
        if flow.size and pred.size <= C.SMALL:
            arrays[name + "/flow"] = pred
            arrays[name + "/enc"] = enc
        else:
            arrays[name + "/flow_digest"] = R.digest_bytes(pred)
            arrays[name + "/enc_digest"] = R.digest_bytes(enc)
        arrays[name + "/epe"] = np.array(rows["epe"], np.float64)
        arrays[name + "/fl"] = np.array(rows["fl"], np.float64)
        arrays[name + "/n_valid"] = np.array(rows["nv"], np.int64)
        arrays[name + "/n_outlier"] = np.array(rows["no"], np.int64)
        rel = int((O.relative_ruled(mag) & valid).sum())
        print("%-12s epe %s fl %s valid %s outliers %s relative-ruled %d" % (name, np.round(rows["epe"], 4), np.round(rows["fl"], 2),
                                                                           rows["nv"], rows["no"], rel))
    np.savez_compressed(out_path, **arrays)
    print("wrote %s (%d bytes)" % (out_path, os.path.getsize(out_path)))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "tests", "golden", "g22_inference_eval.npz"))
