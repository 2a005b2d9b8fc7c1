"""Flow-comparison report on the device: the reference's ``compare_flows`` and ``print_flow_stats`` (onnx_pth_compare.py:133-201,
:225-230) for two float32 flow fields, in one launch pair (csrc/pwc_flow_compare.hip, ops.flow_compare).

    cmp = compare_flows(flow_a, flow_b)            # [n,2,H,W] device tensors; a is the reference side ("pth")
    per_sample, batch = cmp.to_host()              # the only download: (n + 1) x 44 doubles
    print("\\n".join(format_report(batch, (H, W, 2), (H, W, 2))))

``FlowComparer`` keeps workspace, record and map for one shape, so ``run`` only launches and can sit inside ``torch.cuda.graph``
beside the forwards it compares; ``compare_models`` runs two networks on one input and compares their flow2 on the device.

The numerics contract is the kernel's (include/pwc_hip.h): difference and endpoint error in float32 exactly as the reference forms
them, so maxima, threshold counts and agreement percentages equal the reference's bit for bit; every sum in float64, which the
reference's float32 sums approach to 2e-7 relative on the g18 fixture.  Out of scope (cv2- or onnx-defined, not pinned here): the script's HSV
``flow_to_color``, the ``cv2.addWeighted`` overlay, the ``putText`` canvas, ONNX export and runtime.  ``flowviz.flow_to_color`` remains
the package's colour rendering.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import ops

DEFAULT_TAUS = (0.25, 0.5, 1.0, 2.0)
METRIC_FIELDS = (("L2 diff", ops.FC_L2), ("MAE", ops.FC_MAE), ("Max abs diff", ops.FC_MAX_ABS), ("Relative L2 diff", ops.FC_REL_L2),
                 ("Relative MAE", ops.FC_REL_MAE), ("Pearson corr", ops.FC_PEARSON), ("Cosine similarity", ops.FC_COSINE),
                 ("EPE mean", ops.FC_EPE_MEAN), ("EPE max", ops.FC_EPE_MAX))
STAT_FIELDS = {"a": (("min", ops.FC_MIN_A), ("max", ops.FC_MAX_A), ("mean", ops.FC_MEAN_A), ("std", ops.FC_STD_A)),
               "b": (("min", ops.FC_MIN_B), ("max", ops.FC_MAX_B), ("mean", ops.FC_MEAN_B), ("std", ops.FC_STD_B))}
METRIC_KEYS = tuple(k for k, _ in METRIC_FIELDS) + ("agreements", "stats")


def agreement_key(tau: float) -> str:
    """The reference's key of one threshold: f"agree@{tau}" of the Python float (0.25 -> "agree@0.25", 1.0 -> "agree@1.0")."""
    return f"agree@{float(tau)}"


def record_to_dict(row: Sequence[float], taus: Sequence[float]) -> Dict:
    """One row of the device record (host floats) -> the reference's dict plus "stats"."""
    m = {k: float(row[i]) for k, i in METRIC_FIELDS}
    m["agreements"] = {agreement_key(t): float(row[ops.FC_AGREE0 + k]) for k, t in enumerate(taus)}
    m["stats"] = {f: {k: float(row[i]) for k, i in fields} for f, fields in STAT_FIELDS.items()}
    return m


class FlowComparison:
    """The device record of one comparison: float64 [n + 1, ops.FLOW_COMPARE_FIELDS] (row n is the batch), the thresholds it was made
    with, the compared shape and, when asked for, the float32 [n,H,W] EPE map.  Nothing is downloaded until to_host()."""

    def __init__(self, record: torch.Tensor, taus: Sequence[float], shape: Tuple[int, ...], epe_map: Optional[torch.Tensor] = None):
        self.record, self.taus, self.shape, self.epe_map = record, tuple(float(t) for t in taus), tuple(shape), epe_map

    def to_host(self) -> Tuple[List[Dict], Dict]:
        """One download -> (one dict per sample, the batch dict), each with exactly the reference's keys plus "stats"."""
        rows = self.record.cpu().tolist()
        return [record_to_dict(r, self.taus) for r in rows[:-1]], record_to_dict(rows[-1], self.taus)


class FlowComparer:
    """Workspace, record and optional EPE map for flows [n,2,H,W] on `device`, allocated once: run(a, b) only launches (no
    allocation, no synchronisation), so it is safe inside torch.cuda.graph.  The returned FlowComparison shares these buffers: read
    it before the next run, or clone its record."""

    def __init__(self, n: int, H: int, W: int, device, taus: Sequence[float] = DEFAULT_TAUS, epe_map: bool = False):
        self.shape = (int(n), 2, int(H), int(W))
        self.device = torch.device(device)
        self.taus = ops.flow_compare_taus(taus)
        if self.device.type != "cuda":
            raise ops.PwcHipError("FlowComparer is on %s: the HIP path needs a device and has no CPU fallback" % self.device)
        nbytes = ops.flow_compare_workspace_bytes(n, H, W)
        self.workspace = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=self.device)
        self.record = torch.empty((n + 1, ops.FLOW_COMPARE_FIELDS), dtype=torch.float64, device=self.device)
        self.epe_map = torch.empty((n, H, W), dtype=torch.float32, device=self.device) if epe_map else None

    def run(self, a: torch.Tensor, b: torch.Tensor) -> FlowComparison:
        if tuple(a.shape) != self.shape or tuple(b.shape) != self.shape:
            raise ValueError("FlowComparer was built for %s, got %s and %s" % (self.shape, tuple(a.shape), tuple(b.shape)))
        ops.flow_compare(a, b, self.taus, epe_map=self.epe_map, workspace=self.workspace, out=self.record)
        return FlowComparison(self.record, self.taus, self.shape, self.epe_map)


def compare_flows(a: torch.Tensor, b: torch.Tensor, taus: Sequence[float] = DEFAULT_TAUS, epe_map: bool = False) -> FlowComparison:
    """Compare the float32 device flows a (the reference side) and b, [n,2,H,W]; see the module docstring."""
    if a.dim() != 4:
        raise ValueError("a must be [n,2,H,W], got %s" % (tuple(a.shape),))
    n, _, H, W = a.shape
    m = torch.empty((n, H, W), dtype=torch.float32, device=a.device) if epe_map and a.is_cuda else None
    rec = ops.flow_compare(a, b, taus, epe_map=m)
    return FlowComparison(rec, ops.flow_compare_taus(taus), a.shape, m)


def _flow2(net, x: torch.Tensor) -> torch.Tensor:
    out = net(x)
    return out[0] if isinstance(out, (tuple, list)) else out


def compare_models(net_a, net_b, x: torch.Tensor, taus: Sequence[float] = DEFAULT_TAUS, epe_map: bool = False) -> FlowComparison:
    """Run two PWCDCNets (for example precision="fp32" and "fp16-strict") on the same [B,6,H,W] device input and compare their flow2
    on the device, in the current stream; net_a is the reference side.  Only the record is ever downloaded (by to_host())."""
    with torch.no_grad():
        fa = _flow2(net_a, x)
        if getattr(net_a, "borrow_output", False):
            fa = fa.clone()                      # a borrowed buffer may be the next forward's
        fb = _flow2(net_b, x)
    return compare_flows(fa.float() if fa.dtype != torch.float32 else fa, fb.float() if fb.dtype != torch.float32 else fb, taus, epe_map)


def format_report(metrics: Dict, shape_a, shape_b, drawn: bool = False) -> List[str]:
    """The reference's lines for one metrics dict (its own or to_host()'s).  Default: what compare_flows prints
    (onnx_pth_compare.py:177-188); drawn=True: the lines it draws beside the report image (:324-337).  Host only."""
    if drawn:
        return [f"flow_pth shape : {tuple(shape_a)}",
                f"flow_onnx shape: {tuple(shape_b)}",
                "",
                f"L2 diff           : {metrics['L2 diff']:.6f}",
                f"MAE               : {metrics['MAE']:.6f}",
                f"Max abs diff      : {metrics['Max abs diff']:.6f}",
                f"Relative L2 diff  : {metrics['Relative L2 diff']:.6f}",
                f"Relative MAE      : {metrics['Relative MAE']:.6f}",
                f"Pearson corr      : {metrics['Pearson corr']:.6f}",
                f"Cosine similarity : {metrics['Cosine similarity']:.6f}",
                f"EPE mean          : {metrics['EPE mean']:.6f}",
                f"EPE max           : {metrics['EPE max']:.6f}"]
    lines = [f"L2 diff           : {metrics['L2 diff']}",
             f"MAE               : {metrics['MAE']}",
             f"Max abs diff      : {metrics['Max abs diff']}",
             f"Relative L2 diff  : {metrics['Relative L2 diff']}",
             f"Relative MAE      : {metrics['Relative MAE']}",
             f"Pearson corr      : {metrics['Pearson corr']}",
             f"Cosine similarity : {metrics['Cosine similarity']}",
             f"EPE mean          : {metrics['EPE mean']}",
             f"EPE max           : {metrics['EPE max']}"]
    for key, agree in metrics["agreements"].items():
        tau = float(key.split("@", 1)[1])
        lines.append(f"Agreement @ EPE<={tau:4.2f} : {agree:6.2f}%")
    return lines


def format_stats(name: str, shape, stats: Dict) -> List[str]:
    """print_flow_stats' lines (onnx_pth_compare.py:226-230) for one field's {"min", "max", "mean", "std"}.  Host only."""
    return [f"[{name}] shape={tuple(shape)}",
            f"  min  : {stats['min']:.4f}",
            f"  max  : {stats['max']:.4f}",
            f"  mean : {stats['mean']:.4f}",
            f"  std  : {stats['std']:.4f}"]
