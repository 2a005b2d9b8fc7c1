"""The one mask adapter behind the loss operators (opticalflow_amd/_args.py): three rules meet in it, and each input has to reach the
kernels exactly as the operator's own adapter used to hand it over.

  rule        bool          uint8          float32        any other dtype
  threshold   bytes, u8=1   as is, u8=1    as is, u8=0    (mask > 0.5) as bytes, u8=1     proxy loss, epipolar loss
  raw         bytes, u8=1   as is, u8=1    as is, u8=0    .float(), u8=0                  supervised losses
  nonzero     bytes, u8=1   as is, u8=1    as is, u8=0    (mask != 0) as bytes, u8=1      epipolar_pairs

CPU tensors throughout: the adapter compares devices and never asks for a GPU; no library is loaded."""
import pytest
import torch

from opticalflow_amd._args import _mask_arg

B, H, W = 2, 3, 5
CPU = torch.device("cpu")
RULES = ("threshold", "raw", "nonzero")
DTYPES = (torch.bool, torch.uint8, torch.float32, torch.float64, torch.int64)


def _values() -> torch.Tensor:
    """float64 [B,H,W] holding each of 0, 0.4, 0.6, 1, 2 six times, in a fixed shuffled order"""
    v = torch.tensor([0.0, 0.4, 0.6, 1.0, 2.0], dtype=torch.float64).repeat(B * H * W // 5)
    return v[torch.randperm(v.numel(), generator=torch.Generator().manual_seed(3))].reshape(B, H, W)


def _expected(rule: str, mask: torch.Tensor):
    """(tensor, u8) of the table above for a [B,H,W] mask"""
    if mask.dtype == torch.bool:
        return mask.to(torch.uint8), 1
    if mask.dtype == torch.uint8:
        return mask, 1
    if mask.dtype == torch.float32:
        return mask, 0
    if rule == "raw":
        return mask.to(torch.float32), 0
    return ((mask > 0.5) if rule == "threshold" else (mask != 0)).to(torch.uint8), 1


@pytest.mark.parametrize("four_d", (False, True), ids=("BHW", "B1HW"))
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("rule", RULES)
def test_mask_adapter_table(rule, dtype, four_d):
    mask = _values().to(dtype)
    want, want_u8 = _expected(rule, mask)
    m, u8, bs = _mask_arg(mask[:, None] if four_d else mask, B, H, W, CPU, rule)
    assert u8 == want_u8 and bs == H * W
    assert m.dtype == want.dtype and tuple(m.shape) == (B, H, W) and m.is_contiguous()
    assert torch.equal(m, want)
    if dtype in (torch.uint8, torch.float32):
        assert m.data_ptr() == mask.data_ptr()          # "as is": no copy of a contiguous mask


@pytest.mark.parametrize("rule", RULES)
def test_mask_adapter_values_spelled_out(rule):
    """the cells where the rules differ, on the five values themselves (not through _expected)"""
    v = torch.tensor([0.0, 0.4, 0.6, 1.0, 2.0], dtype=torch.float64).repeat(B * H * W // 5).reshape(B, H, W)
    m, u8, _ = _mask_arg(v, B, H, W, CPU, rule)
    got = m.reshape(-1)[:5].tolist()
    if rule == "threshold":
        assert (got, u8, m.dtype) == ([0, 0, 1, 1, 1], 1, torch.uint8)
    elif rule == "nonzero":
        assert (got, u8, m.dtype) == ([0, 1, 1, 1, 1], 1, torch.uint8)
    else:
        assert u8 == 0 and m.dtype == torch.float32 and got == v.float().reshape(-1)[:5].tolist()
    m, u8, _ = _mask_arg(v.to(torch.int64), B, H, W, CPU, rule)      # the cast leaves 0, 0, 0, 1, 2
    got = m.reshape(-1)[:5].tolist()
    assert got == ([0.0, 0.0, 0.0, 1.0, 2.0] if rule == "raw" else [0, 0, 0, 1, 1])
    # float32 and uint8 keep their values under every rule: the kernel applies the rule to them
    m, u8, _ = _mask_arg(v.float(), B, H, W, CPU, rule)
    assert u8 == 0 and torch.equal(m, v.float())
    m, u8, _ = _mask_arg(v.to(torch.uint8), B, H, W, CPU, rule)
    assert u8 == 1 and m.reshape(-1)[:5].tolist() == [0, 0, 0, 1, 2]


@pytest.mark.parametrize("rule", RULES)
def test_mask_adapter_none_noncontiguous_and_errors(rule):
    assert _mask_arg(None, B, H, W, CPU, rule) == (None, 0, 0)
    wide = _values().float().repeat(1, 1, 2)                          # [B,H,2W]: every other column is a strided view
    m, u8, bs = _mask_arg(wide[:, :, ::2], B, H, W, CPU, rule)
    assert m.is_contiguous() and torch.equal(m, wide[:, :, ::2]) and (u8, bs) == (0, H * W)
    for dtype in DTYPES:
        with pytest.raises(ValueError):
            _mask_arg(torch.zeros(B, H, W + 1).to(dtype), B, H, W, CPU, rule)
        with pytest.raises(ValueError):
            _mask_arg(torch.zeros(B, 1, H, W + 1).to(dtype), B, H, W, CPU, rule)
    with pytest.raises(ValueError):
        _mask_arg(torch.zeros(B, H, W), B, H, W, torch.device("meta"), rule)      # another device than the operands'


def test_mask_adapter_unknown_rule():
    with pytest.raises(ValueError):
        _mask_arg(torch.zeros(B, H, W), B, H, W, CPU, "majority")
