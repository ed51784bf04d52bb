"""``encode=`` of predict / track / track_cameras: what the JPEG encoder of csrc/jpeg_kernels.hip is asked for.  Pure
Python: nothing here touches a GPU."""
from dataclasses import dataclass
from typing import Optional


@dataclass(frozen=True)
class JpegSpec:
    """``quality``: 1 .. 100, the IJG scaling of the Annex K tables; ``subsampling``: "420" (default) or "444"; ``keep_pixels``: with
    ``render=``, also bring the rendered pixels back as ``Results.rendered`` (without it only the bytes come back)."""
    quality: int = 85
    subsampling: str = "420"
    keep_pixels: bool = False

    def __post_init__(self):
        if isinstance(self.quality, bool) or not isinstance(self.quality, int) or not 1 <= self.quality <= 100:
            raise ValueError(f"quality must be an integer in 1 .. 100, got {self.quality!r}")
        if self.subsampling not in ("420", "444"):
            raise ValueError(f"subsampling must be '420' or '444', got {self.subsampling!r}")


def as_spec(arg) -> Optional[JpegSpec]:
    """``encode=`` of predict / track / track_cameras -> None (off) or a JpegSpec"""
    if arg is None or arg is False:
        return None
    if arg == "jpeg":
        return JpegSpec()
    if isinstance(arg, JpegSpec):
        return arg
    if isinstance(arg, dict):
        return JpegSpec(**arg)
    raise TypeError(f"encode must be None, 'jpeg', a JpegSpec or a dict of its fields, not {arg!r}")
