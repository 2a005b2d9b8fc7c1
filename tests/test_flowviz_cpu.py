"""Flow pictures without a GPU: the float64 oracle against the reference's own outputs (tests/golden/g13_flowviz.npz, written by
tools/gen_golden_flowviz.py), the C ABI additions, the wrappers' argument checks and the PNG / save_outputs writers.
The knife-edge sets (where a decision may fall either way, see tests/flowviz_oracle.py) are the only places a difference is allowed."""
import ctypes
import os
import re
import struct
import sys
import zlib

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import flowviz_oracle as FO  # noqa: E402

NEW_SYMBOLS = ("pwc_flow_stats_workspace_bytes", "pwc_flow_stats", "pwc_flow_color", "pwc_flow_quiver")


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(HERE, "golden", "g13_flowviz.npz")) as z:
        return {k: z[k] for k in z.files}


def test_fixture_holds_every_case_and_fits(gold):
    assert os.path.getsize(os.path.join(HERE, "golden", "g13_flowviz.npz")) <= 1 << 20
    for name, hw in FO.FIELDS.items():
        assert gold["field/" + name].shape == hw + (2,) and gold["field/" + name].dtype == np.float32
    ax = gold["field/axis"]
    assert (ax[..., 0] > 0).all() and not np.signbit(ax[0, :, 1]).any() and np.signbit(ax[1, :, 1]).all() and (ax[..., 1] == 0).all()


@pytest.mark.parametrize("case", sorted(FO.COLOR_CASES))
def test_oracle_colour_is_the_references(gold, case):
    fname, crop = FO.COLOR_CASES[case]
    flow = FO.cropped(gold["field/" + fname], crop)
    for ci, clip in enumerate(FO.CLIPS):
        rgb, _, knife = FO.color(flow, clip)
        d = gold["color/%s/%d" % (case, ci)].astype(np.int64) - rgb
        assert np.abs(d).max() <= 1 and not (d != 0)[~knife].any()
        assert knife.mean() <= 5e-3


def test_colour_landmarks(gold):
    assert (gold["color/zero/0"] == 255).all() and (gold["color/zero/1"] == 255).all()
    assert (gold["color/axis/0"][0] == (255, 0, 0)).all() and (gold["color/axis/0"][1] == (255, 0, 43)).all()
    w = FO.colorwheel()
    assert w.shape == (55, 3) and tuple(w[0]) == (255, 0, 0) and tuple(w[54]) == (255, 0, 43) and tuple(w[15]) == (255, 255, 0)


@pytest.mark.parametrize("case", sorted(FO.DOMINANT_CASES))
def test_oracle_dominant_direction_is_the_references(gold, case):
    fname, crop, thr = FO.DOMINANT_CASES[case]
    flow = FO.cropped(gold["field/" + fname], crop)
    _, n, mean, knife = FO.stats(flow, thr)
    assert knife == 0 and n == int(gold["domn/" + case])
    sel = flow[np.sqrt((flow.astype(np.float64) ** 2).sum(-1)) > thr]
    bound = 1e-5 * float(np.abs(sel).mean()) if n else 0.0          # pairwise float32 summation, with margin
    assert np.abs(gold["dom/" + case] - mean).max() <= bound


@pytest.mark.parametrize("case", sorted(FO.QUIVER_CASES))
def test_oracle_arrows_are_the_references(gold, case):
    fname, crop, frame, step, style, scale, min_mag, dom, thr, vs = FO.QUIVER_CASES[case]
    flow = FO.cropped(gold["field/" + fname], crop)
    gain, rule = FO.gain_rule(style, scale)
    o = FO.quiver(flow, frame, step, gain, rule, min_mag, vec_scale=vs, dominant=gold["dom/" + dom] if dom else None, angle_threshold=thr)
    keep, tip, aligned = gold["q/%s/keep" % case], gold["q/%s/tip" % case], gold["q/%s/aligned" % case]
    assert keep.shape == (-(-frame[0] // step), -(-frame[1] // step))
    assert not (keep != o["keep"])[~o["knife_keep"]].any()
    both = keep & o["keep"]
    dt = np.abs(tip.astype(np.int64) - o["tip"])
    assert dt[both].max(initial=0) <= 1 and not (dt != 0)[both[..., None] & ~o["knife_tip"]].any()
    assert not (aligned != o["aligned"])[both & ~o["knife_aligned"]].any()
    n = keep.size
    assert o["knife_tip"].sum() <= 1e-2 * 2 * n and o["knife_keep"].sum() <= 1e-2 * n and o["knife_aligned"].sum() <= 1e-2 * n


def test_new_symbols_declared_exported_bound_and_abi_13():
    from opticalflow_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "pwc_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.ABI_VERSION == 13 and _lib.load().pwc_abi_version() == 13
    assert re.search(r"#define PWC_ABI_VERSION 13\b", text)


def test_workspace_query_and_c_argument_checks_launch_nothing():
    from opticalflow_amd import _lib
    lib = _lib.load()
    assert lib.pwc_flow_stats_workspace_bytes(3, 37, 53) == 32 * 3 * 3 * 1
    assert lib.pwc_flow_stats_workspace_bytes(1, 16, 65) == 32 * 2 and lib.pwc_flow_stats_workspace_bytes(0, 4, 4) == -1
    # every call below fails its checks, which come before anything touches a device
    assert lib.pwc_flow_stats(None, 1, 4, 4, 4, 4, 32, 0, 0.0, 1.0, None, 0, None, None) == -1
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    assert lib.pwc_flow_stats(p, 1, 4, 4, 5, 4, 32, 0, 0.0, 1.0, p, 512, p, None) == -1               # crop larger than the map
    assert lib.pwc_flow_stats(p, 1, 4, 4, 4, 4, 32, 0, 0.0, 1.0, p, 8, p, None) == -1                 # workspace too small
    assert lib.pwc_flow_stats(p, 1, 4, 4, 4, 4, 32, 1, 0.0, 1.0, p, 512, p, None) == -1               # clip_flow <= 0
    assert lib.pwc_flow_stats(p, 1, 4, 4, 4, 4, 32, 0, 0.0, 1.0, p + 4, 512, p, None) == -3           # workspace alignment
    assert lib.pwc_flow_color(p, 1, 4, 4, 4, 4, 31, 0, 0.0, p, p, None) == -1                         # batch stride too small
    assert lib.pwc_flow_color(p, 1, 4, 4, 4, 4, 32, 0, 0.0, None, p, None) == -1
    assert lib.pwc_flow_quiver(p, 1, 4, 4, 4, 4, 32, 16, 16, 0, 1.0, 1.0, 1.0, 0, 0.5, None, 0, 30.0, p, p, p, None) == -1   # step < 1
    assert lib.pwc_flow_quiver(p, 1, 4, 4, 4, 4, 32, 16, 16, 4, 1.0, 1.0, 1.0, 2, 0.5, None, 0, 30.0, p, p, p, None) == -1   # tip_rule
    assert lib.pwc_flow_quiver(p, 1, 4, 4, 4, 4, 32, 16, 16, 4, 1.0, 1.0, 1.0, 0, 0.5, None, 0, 30.0, p + 4, p, p, None) == -3
    assert b"pwc_flow_quiver" in lib.pwc_last_error()


def test_wrapper_argument_errors_raise_without_a_device():
    from opticalflow_amd import PwcHipError, flowviz, ops
    host = torch.zeros(1, 2, 8, 12)
    with pytest.raises(PwcHipError):
        ops.flow_stats(host)
    with pytest.raises(PwcHipError):
        flowviz.flow_to_color(host)
    with pytest.raises(PwcHipError):
        flowviz.quiver_arrows(host, (32, 48))
    with pytest.raises(TypeError):
        ops.flow_stats(host.double())
    with pytest.raises(ValueError):
        ops.flow_stats(torch.zeros(1, 3, 8, 12))
    with pytest.raises(ValueError):
        ops.flow_stats(host, crop=(9, 12))
    with pytest.raises(ValueError):
        flowviz.dominant_direction(host, crop=(8, 13))
    with pytest.raises(ValueError):
        flowviz.quiver_arrows(host, (32, 48), step=0)
    with pytest.raises(ValueError):
        flowviz.quiver_arrows(host, (32, 48), style="sideways")
    with pytest.raises(ValueError):
        ops.flow_quiver(host, 32, 48, 16, (1.0, 1.0), 1.0, 2, 0.5)
    with pytest.raises(ValueError):
        flowviz.Renderer(flowviz.RenderSpec(quiver={"step": 16}), (1, 2, 8, 12), torch.device("cpu"))


def _decode_png(path):
    try:
        from PIL import Image
        with Image.open(path) as im:
            assert im.mode == "RGB"
            return np.array(im)
    except ImportError:
        data = open(path, "rb").read()
        assert data[:8] == b"\x89PNG\r\n\x1a\n"
        pos, idat, hdr = 8, b"", None
        while pos < len(data):
            n, kind = struct.unpack(">I4s", data[pos:pos + 8])
            body = data[pos + 8:pos + 8 + n]
            assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(kind + body) & 0xFFFFFFFF
            if kind == b"IHDR":
                hdr = struct.unpack(">IIBBBBB", body)
            elif kind == b"IDAT":
                idat += body
            pos += 12 + n
        w, h, depth, ctype = hdr[:4]
        assert (depth, ctype) == (8, 2)
        rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + 3 * w)
        assert (rows[:, 0] == 0).all()
        return rows[:, 1:].reshape(h, w, 3).copy()


def test_write_png8_rgb_round_trips(tmp_path, gold):
    from opticalflow_amd.flowio import write_png8_rgb
    for img in (gold["color/odd/0"], gold["color/one/1"], np.arange(5 * 7 * 3, dtype=np.uint8).reshape(5, 7, 3)):
        path = str(tmp_path / "c.png")
        write_png8_rgb(path, img)
        assert np.array_equal(_decode_png(path), img)
    write_png8_rgb(str(tmp_path / "t.png"), torch.from_numpy(gold["color/odd/0"]))
    assert np.array_equal(_decode_png(str(tmp_path / "t.png")), gold["color/odd/0"])
    with pytest.raises(ValueError):
        write_png8_rgb(str(tmp_path / "bad.png"), np.zeros((4, 4, 3), np.float32))


def test_save_outputs_writes_the_three_files(tmp_path, gold):
    from opticalflow_amd.flowio import read_flo, save_outputs
    flow, img = gold["field/odd"], gold["color/odd/0"]
    prefix = str(tmp_path / "sub" / "pair0")
    save_outputs(flow, prefix, color=img)
    assert np.array_equal(np.load(prefix + ".npy"), flow)
    assert np.array_equal(read_flo(prefix + ".flo"), flow)
    assert np.array_equal(_decode_png(prefix + ".png"), img)
    with pytest.raises(ValueError):
        save_outputs(flow[..., 0], prefix, color=img)
