"""NumPy statement of csrc/pwc_video.hip (pwc_video_ingest_u8): frame_to_tensor + pad_to_multiple_of_64 of
pwc_extract_flow_video.py:27-42 on a batch of raw frames.  tests/test_video_ingest_cpu.py ties it bit for bit to
opticalflow_amd.video.frame_to_tensor + kitti.pad_to_64, which tests/test_video.py ties to the reference loop; the GPU tests hold the
kernel to it bit for bit."""
import numpy as np

# (n, H, W): no padding | everything is padding | W % 4 == 3, a four-column store group straddles the right edge, Wp = 64 and 128 |
# one row and two columns over a multiple | the size tests/test_video.py uses
CASES = [(1, 64, 64), (1, 1, 1), (2, 5, 7), (3, 61, 67), (1, 66, 130), (2, 100, 150)]


def padded(size: int) -> int:
    return (int(size) + 63) // 64 * 64


def ingest(frames: np.ndarray, bgr: bool = True) -> np.ndarray:
    """uint8 [n,H,W,3] -> float32 [n,3,Hp,Wp]: channel order, astype(float32) / 255.0, transpose, edge padding to multiples of 64."""
    assert frames.dtype == np.uint8 and frames.ndim == 4 and frames.shape[3] == 3
    f = frames[..., ::-1] if bgr else frames
    x = np.transpose(f.astype(np.float32) / 255.0, (0, 3, 1, 2))
    H, W = frames.shape[1:3]
    return np.ascontiguousarray(np.pad(x, ((0, 0), (0, 0), (0, padded(H) - H), (0, padded(W) - W)), mode="edge"))


def case_frames(n: int, H: int, W: int):
    """The frame sets of one case: as many uint8 [n,H,W,3] arrays as it takes for every channel to hold all 256 byte values over the
    case (one set from 256 pixels up; 256 sets for the 1 x 1 frame).  Pixel p of set r holds 97 * (p + r * pixels) + (0, 85, 171) per
    channel, mod 256: multiplication by an odd number permutes the bytes, and the three channels differ everywhere, so a wrong
    channel order, a wrong pixel and a wrong quotient all show."""
    npix = n * H * W
    sets = []
    for r in range(-(-256 // npix)):
        p = np.arange(npix, dtype=np.int64).reshape(n, H, W, 1) + r * npix
        sets.append(((97 * p + np.array([0, 85, 171], dtype=np.int64)) % 256).astype(np.uint8))
    return sets
