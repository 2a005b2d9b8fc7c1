"""opticalflow_amd -- MI355X-native PWC-Net inference path (hand-written gfx950 HIP kernels behind
the reference's Correlation / warp / PWCDCNet interface).  See DESIGN.md."""
from ._lib import LIB_PATH, PwcHipError  # noqa: F401
from .correlation import Correlation, CorrelationFunction  # noqa: F401
from .pwcnet import PWCDCNet, PWCDCNet_old, pwc_dc_net, pwc_dc_net_old  # noqa: F401
from .flowio import read_flo, save_outputs, write_flo, write_png8_rgb  # noqa: F401
from . import validation  # noqa: F401
from . import flowviz  # noqa: F401
from .flowviz import dominant_direction, flow_to_color, quiver_arrows  # noqa: F401
from . import vanishing  # noqa: F401
from .vanishing import vanishing_point  # noqa: F401
from . import augment  # noqa: F401
from .augment import DeviceAugmenter, augment_batch  # noqa: F401
from . import augment_full  # noqa: F401
from .augment_full import DeviceFullAugmenter, augment_full_batch  # noqa: F401
from . import pil_resize  # noqa: F401
from .pil_resize import eval_flow, resize_flow, resize_frames  # noqa: F401
from . import inference_eval  # noqa: F401
from .inference_eval import ResizedEval  # noqa: F401
from . import cv_resize  # noqa: F401
from .cv_resize import CvGraphedInfer  # noqa: F401
from . import cv_warp  # noqa: F401
from .cv_warp import TopviewInfer, TopviewStream  # noqa: F401
from . import optim  # noqa: F401
from .optim import FusedAdam, FusedAdamW  # noqa: F401
from . import compare  # noqa: F401
from .compare import compare_flows  # noqa: F401

__version__ = "0.1.0"
