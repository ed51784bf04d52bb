"""Public names of the package (imported as ``cvsd_amd``)."""
from .graph import build_program, parse_model_name  # noqa: F401
from .results import Boxes, Keypoints, Results  # noqa: F401
from .engine import YOLO  # noqa: F401
from .yuv import YUVFrame  # noqa: F401
from .motion import MotionGate  # noqa: F401
from .render import RenderSpec  # noqa: F401
from .jpeg import JpegSpec  # noqa: F401
from .crops import CropSpec  # noqa: F401
from .jpeg_decode import JPEGFrame  # noqa: F401
from .shopformer import (MultiStreamScorer, Shopformer, StreamScorer, score_poselift, score_poselift_many,  # noqa: F401
                         windows_from_poselift)

__all__ = ["YOLO", "YUVFrame", "MotionGate", "RenderSpec", "JpegSpec", "CropSpec", "JPEGFrame", "Results", "Boxes", "Keypoints", "build_program", "parse_model_name",
           "Shopformer", "StreamScorer", "MultiStreamScorer", "score_poselift", "score_poselift_many", "windows_from_poselift"]
