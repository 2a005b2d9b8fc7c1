"""GPU checks of the KITTI training augmentation (csrc/pwc_augment.hip, opticalflow_amd/augment.py): every output of every case equals
the NumPy oracle (tests/augment_oracle.py) bit for bit -- the arithmetic is integer, or fp32 / fp64 in a fixed order without fused
multiply-add, so there is no tolerance anywhere -- and the status vector is zero unless a case says otherwise."""
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_oracle as AO  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g14_augment.npz")) as z:
        return {k: z[k] for k in z.files}


def to_params(recs):
    """Oracle record dicts -> the product's PARAMS_DTYPE array."""
    from opticalflow_amd import augment
    p = augment.make_params(len(recs))
    for i, r in enumerate(recs):
        for k in p.dtype.names:
            p[k][i] = r[k]
    return p


def upload(samples, slot, dev, gt_kind=1, with_valid=True):
    """Host samples (im1, im2, png) -> device slot tensors (frames, gt, valid) in the requested ground-truth form."""
    from opticalflow_amd import augment
    if gt_kind == 0:
        samples = [(a, b, np.stack(AO.decode_png(p)[:2], -1), (p[..., 2] != 0) if with_valid else None) for a, b, p in samples]
    frames, gt, valid, _ = augment.pack_slots(samples, slot, gt_kind)
    return (torch.from_numpy(frames).to(dev), torch.from_numpy(gt).to(dev), None if valid is None else torch.from_numpy(valid).to(dev))


def assert_equal(got, want, status=None):
    for name, g, w in zip(("x", "flow", "valid"), got, want):
        g = g.cpu().numpy()
        assert g.dtype == np.float32 and g.shape == w.shape, (name, g.dtype, g.shape, w.shape)
        bad = g != w
        print("%s: %d of %d elements differ" % (name, np.count_nonzero(bad), bad.size))
        assert np.array_equal(g, w), name
    if status is not None:
        assert status.dtype == torch.int32 and not status.cpu().numpy().any()


# ---- (a) - (d) and the tile / line cases: every named case, both ground-truth forms ------------------------------------------------
@pytest.mark.parametrize("gt_kind", [1, 0])
@pytest.mark.parametrize("case", sorted(AO.CASES))
def test_case_equals_the_oracle(dev, case, gt_kind):
    from opticalflow_amd import augment
    samples, recs, crop, slot = AO.case_inputs(case)
    want = AO.case_expected(samples, recs, crop)
    frames, gt, valid = upload(samples, slot, dev, gt_kind)
    *got, status = augment.augment_batch(frames, gt, valid, to_params(recs), crop, return_status=True)
    assert got[0].shape == (len(recs), 6) + crop and got[1].shape == (len(recs), 2) + crop and got[2].shape == (len(recs), 1) + crop
    assert_equal(got, want, status)


# ---- (e) the two ground-truth forms agree, and no valid plane means every pixel valid -------------------------------------------------
def test_gt_forms_agree_and_null_valid_is_all_ones(dev):
    from opticalflow_amd import augment
    samples, recs, crop, slot = AO.case_inputs("mixed")
    p = to_params(recs)
    f1, g1, _ = upload(samples, slot, dev, 1)
    f0, g0, v0 = upload(samples, slot, dev, 0)
    a = augment.augment_batch(f1, g1, None, p, crop)
    b = augment.augment_batch(f0, g0, v0, p, crop)
    for s, t in zip(a, b):
        assert torch.equal(s, t)
    c = augment.augment_batch(f0, g0, None, p, crop)
    assert torch.equal(c[0], a[0]) and torch.equal(c[1], a[1])
    assert (c[2] == 1).all()                                  # the weights add up to exactly 1, warped or not
    assert_equal(c, AO.case_expected(samples, recs, crop, with_valid=False))
    skip = [i for i, r in enumerate(recs) if not r["warp"]]
    assert skip and (c[2][skip] == 1).all()


# ---- (f) the fixture made from the reference's own dataset class -----------------------------------------------------------------------
def test_fixture_through_augment_batch(dev, gold):
    from opticalflow_amd import augment
    samples = [(gold["im1/%d" % i], gold["im2/%d" % i], gold["png/%d" % i]) for i in range(3)]
    sizes = [s[0].shape[:2] for s in samples]
    slot = (max(h for h, _ in sizes), max(w for _, w in sizes))
    crop = tuple(int(v) for v in gold["crop"])
    frames, gt, _ = upload(samples, slot, dev, 1)
    for s in [int(v) for v in gold["seeds"]] + [-1]:          # -1: apply_aug=False under seed 1
        random.seed(abs(s))
        p = augment.sample_params(sizes, crop, apply_aug=s >= 0)
        *got, status = augment.augment_batch(frames, gt, None, p, crop, return_status=True)
        want = [np.stack([gold["%s/%d/%d" % (k, s, i)] for i in range(3)]) for k in ("x", "flow", "valid")]
        assert_equal(got, want, status)


# ---- (g) one train.py-shaped call -------------------------------------------------------------------------------------------------
def test_train_shaped_batch_on_sampled_rows(dev):
    from opticalflow_amd import augment
    sizes = [(375, 1242), (370, 1224), (376, 1241), (375, 1242)]
    crop, slot = (320, 896), (376, 1242)
    samples = [AO.make_sample(s, 1500 + i) for i, s in enumerate(sizes)]
    recs = [AO.record(sizes[0], y0=55, x0=346, warp=(2.0, 1.0815, 0.9215)), AO.record(sizes[1], y0=0, x0=0, flip=True),
            AO.record(sizes[2], y0=56, x0=345, warp=(-1.3, 0.96, 1.05), flip=True), AO.record(sizes[3], y0=17, x0=101)]
    frames, gt, _ = upload(samples, slot, dev, 1)
    *got, status = augment.augment_batch(frames, gt, None, to_params(recs), crop, return_status=True)
    rows = [0] + sorted((1 + np.random.default_rng(5).choice(318, 62, replace=False)).tolist()) + [319]
    assert len(rows) == 64
    want = []
    for (im1, im2, png), rec in zip(samples, recs):
        u, v, m = AO.decode_png(png)
        want.append(AO.augment(im1, im2, u, v, m, rec, crop, rows=rows))
    want = [np.stack([w[i] for w in want]) for i in range(3)]
    assert_equal([g[:, :, rows] for g in got], want, status)


# ---- (h) a record the kernel must refuse: zeros and a flag for that sample only --------------------------------------------------------
def test_out_of_range_records_give_zeros_and_a_flag(dev):
    """The kernel's own bounds CHECK: the host validation is bypassed (ops.kitti_augment takes the raw records) and the refused samples
    are never read."""
    from opticalflow_amd import augment, ops
    samples, recs, crop, slot = AO.case_inputs("mixed")
    want = AO.case_expected(samples, recs, crop)
    p = to_params(recs)
    p["y0"][1] = p["h"][1] - crop[0] + 1                       # origin one row too low
    p["x0"][3] = -1                                            # origin left of the frame
    with pytest.raises(ValueError):
        augment.augment_batch(*upload(samples, slot, dev, 1), p, crop)
    frames, gt, _ = upload(samples, slot, dev, 1)
    pd = torch.from_numpy(p.view(np.uint8).reshape(len(recs), -1)).to(dev)
    out = tuple(torch.full((len(recs), c) + crop, float("nan"), device=dev) for c in (6, 2, 1))
    x, flow, valid, status = ops.kitti_augment(frames, gt, pd, crop, out=out, status=torch.full((5,), 7, dtype=torch.int32, device=dev))
    assert status.cpu().tolist() == [0, 1, 0, 1, 0]
    for b in range(5):
        for g, w in zip((x, flow, valid), want):
            g = g[b].cpu().numpy()
            assert np.array_equal(g, np.zeros_like(g) if b in (1, 3) else w[b]), b
    # the other conditions, one record each: h > Hs, w > Ws, h < crop_h, w < crop_w, origin past the right edge, h = 0
    q = to_params(recs)
    bad = np.repeat(q[:1], 6)
    bad["h"][0], bad["w"][1], bad["h"][2], bad["w"][3], bad["h"][5] = slot[0] + 1, slot[1] + 1, crop[0] - 1, crop[1] - 1, 0
    bad["x0"][4] = bad["w"][4] - crop[1] + 1
    six = [samples[0]] * 6
    frames, gt, _ = upload(six, slot, dev, 1)
    pd = torch.from_numpy(bad.view(np.uint8).reshape(6, -1)).to(dev)
    x, flow, valid, status = ops.kitti_augment(frames, gt, pd, crop)
    assert status.cpu().tolist() == [1] * 6 and not x.any() and not flow.any() and not valid.any()


# ---- (i) the staged path: reproducible, and capturable ----------------------------------------------------------------------------------
def test_device_augmenter_repeats_and_replays_in_a_graph(dev):
    from opticalflow_amd import augment
    samples, recs, crop, slot = AO.case_inputs("mixed")
    want = AO.case_expected(samples, recs, crop)
    p = to_params(recs)
    aug = augment.DeviceAugmenter(dev, 6, slot, crop, gt_kind=1)
    first = [t.clone() for t in aug(samples, p)]
    assert_equal(first, want, aug.status[:5])
    second = aug(samples, p)
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    # records drawn by the augmenter itself, in the reference's order
    random.seed(11)
    drawn = aug.stage(samples)
    random.seed(11)
    assert drawn.tobytes() == augment.sample_params([s[0].shape[:2] for s in samples], crop).tobytes()
    aug.upload()
    got = aug.run()
    assert_equal(got, AO.case_expected(samples, [{k: r[k] for k in r.dtype.names} for r in drawn], crop), aug.status[:5])
    # the kernel inside a captured graph: replayed after each stage + upload
    aug.stage(samples, p)
    aug.upload()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        aug.run()
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = aug.run()
    for t in (aug.x, aug.flow, aug.valid):
        t.fill_(float("nan"))
    graph.replay()
    assert_equal(outs, want, aug.status[:5])
    aug.stage(samples, drawn)
    aug.upload()
    graph.replay()
    assert_equal(outs, AO.case_expected(samples, [{k: r[k] for k in r.dtype.names} for r in drawn], crop), aug.status[:5])
    # float ground truth with a valid plane through the same class
    fl = [(a, b, np.stack(AO.decode_png(g)[:2], -1), g[..., 2] != 0) for a, b, g in samples]
    aug0 = augment.DeviceAugmenter(dev, 5, slot, crop, gt_kind=0)
    assert_equal(aug0(fl, p), want, aug0.status)


# ---- (j) the argument checks with real device pointers: nothing is launched, nothing is written ----------------------------------------
def test_einval_and_ealign_leave_the_outputs_untouched(dev):
    from opticalflow_amd import _lib, augment, ops
    lib = _lib.load()
    samples, recs, crop, slot = AO.case_inputs("skip_flip")
    frames, gt, _ = upload(samples, slot, dev, 1)
    n = len(recs)
    pd = torch.from_numpy(to_params(recs).view(np.uint8).reshape(n, -1)).to(dev)
    pad = torch.zeros(n * 88 + 8, dtype=torch.uint8, device=dev)
    x = torch.full((n, 6) + crop, -1.0, device=dev)
    flow = torch.full((n, 2) + crop, -1.0, device=dev)
    valid = torch.full((n, 1) + crop, -1.0, device=dev)
    status = torch.full((n,), 7, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def call(frames=frames.data_ptr(), gt=gt.data_ptr(), kind=1, valid_in=None, n=n, Hs=slot[0], Ws=slot[1], ch=crop[0], cw=crop[1],
             params=pd.data_ptr(), x=x.data_ptr(), flow=flow.data_ptr(), vout=valid.data_ptr(), status=status.data_ptr()):
        return lib.pwc_kitti_augment(frames, gt, kind, valid_in, n, Hs, Ws, ch, cw, params, x, flow, vout, status, stream)
    for kw in (dict(frames=None), dict(status=None), dict(n=0), dict(n=65536), dict(Hs=32768), dict(ch=slot[0] + 1), dict(cw=slot[1] + 1),
               dict(kind=2), dict(kind=1, valid_in=frames.data_ptr())):
        assert call(**kw) == -1, kw
    for kw in (dict(x=x.data_ptr() + 2), dict(flow=flow.data_ptr() + 1), dict(vout=valid.data_ptr() + 2), dict(status=status.data_ptr() + 2),
               dict(gt=gt.data_ptr() + 1), dict(kind=0, gt=gt.data_ptr() + 2), dict(params=pad.data_ptr() + 4)):
        assert call(**kw) == -3, kw
    torch.cuda.synchronize(dev)
    assert (x == -1).all() and (flow == -1).all() and (valid == -1).all() and (status == 7).all()
    with pytest.raises(ValueError):
        ops.kitti_augment(frames, gt, pd, crop, valid=torch.ones((n,) + slot, dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError):
        ops.kitti_augment(frames, gt, pd, (slot[0] + 1, crop[1]))
    with pytest.raises(ValueError):
        ops.kitti_augment(frames, gt, pd[:, :80].contiguous(), crop)
    with pytest.raises(ValueError):
        ops.kitti_augment(frames, gt.cpu(), pd, crop)
    # 4-byte aligned outputs that are not 16-byte aligned take the 4-byte store path and give the same result
    samples, recs, crop, slot = AO.case_inputs("extremes")
    frames, gt, _ = upload(samples, slot, dev, 1)
    n = len(recs)
    bufs = [torch.zeros(n * c * crop[0] * crop[1] + 1, device=dev) for c in (6, 2, 1)]
    out = tuple(b[1:].view(n, c, *crop) for b, c in zip(bufs, (6, 2, 1)))
    assert all(o.data_ptr() % 16 == 4 for o in out)
    got = augment.augment_batch(frames, gt, None, to_params(recs), crop, out=out)
    assert_equal(got, AO.case_expected(samples, recs, crop))
