"""Middlebury ``.flo`` container, the on-disk format of the reference's single-pair CLI, and the three files
pwc_extract_flow.py's ``save_outputs`` leaves per pair (:182-190): ``.npy``, ``.flo`` and the colour-wheel ``.png``.

Layout (script_pwc.py:12-27 writer; data_processing.py:17-29 and pwc_extract_flow.py:46-56 agree):
    float32  202021.25   (tag; little-endian bytes 'PIEH')
    int32    W
    int32    H
    float32  H*W*2       row-major, (u, v) interleaved per pixel
"""
from __future__ import annotations

import os
import struct
import zlib

import numpy as np

TAG_FLOAT = 202021.25


def write_flo(filename: str, uv) -> None:
    """Write an [H,W,2] flow field (numpy array or CPU tensor)."""
    uv = np.asarray(uv.detach().cpu().numpy() if hasattr(uv, "detach") else uv)
    if uv.ndim != 3 or uv.shape[2] != 2:
        raise ValueError("write_flo: flow must be [H,W,2], got %s" % (uv.shape,))
    h, w = uv.shape[:2]
    with open(filename, "wb") as f:
        np.array(TAG_FLOAT, dtype="<f4").tofile(f)
        np.array([w, h], dtype="<i4").tofile(f)
        np.ascontiguousarray(uv, dtype="<f4").tofile(f)


def read_flo(filename: str) -> np.ndarray:
    """Read a ``.flo`` file into an [H,W,2] float32 array; raises on a bad tag or a short file."""
    with open(filename, "rb") as f:
        tag = np.fromfile(f, dtype="<f4", count=1)
        if tag.size != 1 or float(tag[0]) != TAG_FLOAT:
            raise ValueError("read_flo: %s is not a .flo file (tag %r)" % (filename, tag))
        wh = np.fromfile(f, dtype="<i4", count=2)
        if wh.size != 2 or wh[0] <= 0 or wh[1] <= 0:
            raise ValueError("read_flo: bad header in %s" % filename)
        w, h = int(wh[0]), int(wh[1])
        data = np.fromfile(f, dtype="<f4", count=2 * w * h)
        if data.size != 2 * w * h:
            raise ValueError("read_flo: %s truncated (%d of %d values)" % (filename, data.size, 2 * w * h))
    return data.reshape(h, w, 2)


def write_png8_rgb(path: str, arr) -> None:
    """[H,W,3] uint8 (numpy array or tensor) -> 8-bit RGB PNG (filter 0 on every row, plain zlib: no imaging library needed)."""
    arr = np.asarray(arr.detach().cpu().numpy() if hasattr(arr, "detach") else arr)
    if arr.ndim != 3 or arr.shape[2] != 3 or arr.dtype != np.uint8:
        raise ValueError("write_png8_rgb: expected uint8 [H,W,3], got %s %s" % (arr.dtype, arr.shape))
    arr = np.ascontiguousarray(arr)
    h, w = arr.shape[:2]
    raw = b"".join(b"\x00" + arr[y].tobytes() for y in range(h))

    def chunk(kind, body):
        return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


def save_outputs(flow_uv, out_prefix: str = "flow", color=None) -> None:
    """pwc_extract_flow.py:182-190: out_prefix + ".npy" ([H,W,2] float32), ".flo" and the colour-wheel ".png" of an [H,W,2] flow
    (numpy array or tensor on any device).  color: the uint8 [H,W,3] image when the caller has it already (flowviz.flow_to_color);
    otherwise it is made by the colour kernel, which needs the ROCm device -- there is no host statement of it in the product."""
    is_tensor = hasattr(flow_uv, "detach")
    uv = np.asarray(flow_uv.detach().cpu().numpy() if is_tensor else flow_uv)
    if uv.ndim != 3 or uv.shape[2] != 2:
        raise ValueError("save_outputs: flow must be [H,W,2], got %s" % (uv.shape,))
    if color is None:
        import torch
        from .flowviz import flow_to_color
        t = flow_uv.detach() if is_tensor else torch.from_numpy(np.ascontiguousarray(uv, dtype=np.float32))
        if not t.is_cuda:
            t = t.cuda()
        color = flow_to_color(t.to(torch.float32).permute(2, 0, 1).unsqueeze(0).contiguous())[0]
    os.makedirs(os.path.dirname(out_prefix) or ".", exist_ok=True)
    np.save(out_prefix + ".npy", uv)
    write_flo(out_prefix + ".flo", uv)
    write_png8_rgb(out_prefix + ".png", color)
