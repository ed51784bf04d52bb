"""``YOLO`` facade over libmi355yolo.so with the call surface the reference uses.

Drop-in for ``from ultralytics import YOLO`` on the reference's hot path
(``/root/reference/model.py:5,18,38-40``): ``YOLO(path)``, ``model(frame, conf=, iou=, classes=,
max_det=, imgsz=)``, ``model.predict(...)`` and ``model.track(...)`` return ``list[Results]`` whose
``.boxes`` / ``.keypoints`` behave like Ultralytics' (results.py).  All per-frame arithmetic runs in the
HIP engine through the C ABI (include/mi355_yolo.h); nothing here computes on the CPU.
"""
from __future__ import annotations

import ctypes as C
import os
import threading
from contextlib import nullcontext
from typing import Dict, List, Optional, Sequence, Union

import numpy as np
import torch

from . import _lib
from .results import Results
from .sources import (IMGSZ, IOU, MAX_DET, DetArgs, DeviceFrame, DeviceFrames, Ragged, YuvBatch, as_batch, bgr_view, det_args,
                      det_args_from, ready)
from .weights import build_from_state_dict, from_bytes
from .jpeg_decode import decode_sources, has_frames as has_jpeg_frames
from .yuv import YUVFrame, as_frames

COCO_NAMES = ["person", "bicycle", "car", "motorcycle", "airplane", "bus", "train", "truck", "boat", "traffic light",
              "fire hydrant", "stop sign", "parking meter", "bench", "bird", "cat", "dog", "horse", "sheep", "cow",
              "elephant", "bear", "zebra", "giraffe", "backpack", "umbrella", "handbag", "tie", "suitcase", "frisbee",
              "skis", "snowboard", "sports ball", "kite", "baseball bat", "baseball glove", "skateboard", "surfboard",
              "tennis racket", "bottle", "wine glass", "cup", "fork", "knife", "spoon", "bowl", "banana", "apple",
              "sandwich", "orange", "broccoli", "carrot", "hot dog", "pizza", "donut", "cake", "chair", "couch",
              "potted plant", "bed", "dining table", "toilet", "tv", "laptop", "mouse", "remote", "keyboard",
              "cell phone", "microwave", "oven", "toaster", "sink", "refrigerator", "book", "clock", "vase", "scissors",
              "teddy bear", "hair drier", "toothbrush"]


def default_names(nc: int) -> Dict[int, str]:
    if nc == 80:
        return dict(enumerate(COCO_NAMES))
    if nc == 1:
        return {0: "person"}
    return {i: f"class{i}" for i in range(nc)}


class YOLO:
    """MI355X-native stand-in for ``ultralytics.YOLO`` (detect and pose tasks).

    ``model`` may be a ``.mi355w`` path, a ``.pt`` Ultralytics checkpoint (converted on the fly by
    ``cvsd_amd.convert``), or the raw bytes of a ``.mi355w`` image (e.g. received by broadcast).
    """

    def __init__(self, model: Union[str, bytes, os.PathLike], task: Optional[str] = None, device: int = 0,
                 batch_chunk: int = 0, verbose: bool = False, half: bool = False, fast_act: bool = False, autotune: int = 0,
                 streams: int = 0, flags: int = 0, plan_dir: Optional[str] = None, plan_cache_dir: Optional[str] = None,
                 feats: bool = False):
        """Engine options are ``mi355_opts`` (include/mi355_yolo.h): ``fast_act`` = the v_exp / v_rcp SiLU on the fp32 path (tolerance
        mode; the default is the canonical, bit-reproducible arithmetic), ``autotune`` / ``streams`` / ``flags`` (``_lib.OPT_*``) as the
        header documents them, ``plan_dir`` = directory of shipped launch-plan files (default: the package's ``plans/``; "" = none),
        ``plan_cache_dir`` = where freshly timed choices are kept (default ~/.cache/mi355yolo; "" = not persisted).
        ``feats`` = ``mi355_opts.obj_feats``: every predict also returns ``Results.feats``, one appearance embedding per box read from
        the Detect head's own input maps (what Ultralytics' BoT-SORT uses under ``with_reid: True``, ``model: auto``).  Like ``half`` it
        is a property of the engine: ``predict(feats=...)`` with the other value runs on a second engine, created on first use."""
        lib = _lib.lib()
        self._lock = threading.RLock()         # Ultralytics serialises predict() with a per-predictor lock
        self.feats = bool(feats)
        self._h_feats = {}                     # half -> engine with the other value of `feats`, created on first use
        self._h = C.c_void_p()
        self._h_other = C.c_void_p()           # engine of the other precision, created by the first predict(half=...) that needs it
        self.half = bool(half)                 # precision of the primary engine (predict(half=None) uses it)
        self.device = int(device)
        self._batch_chunk = int(batch_chunk)
        self.fast_act = bool(fast_act)
        pd = _lib.PLAN_DIR if plan_dir is None else plan_dir
        self._opt_kw = dict(batch_chunk=int(batch_chunk), fast_act=int(self.fast_act), autotune=int(autotune), streams=int(streams), flags=int(flags),
                            plan_dir=os.fsencode(pd) if pd else None,
                            plan_cache_dir=None if plan_cache_dir is None else os.fsencode(plan_cache_dir))
        opts = _lib.Opts(struct_size=C.sizeof(_lib.Opts), half=int(self.half), obj_feats=int(self.feats), **self._opt_kw)
        if isinstance(model, (bytes, bytearray, memoryview)):
            blob = bytes(model)
            self.ckpt_path = None
        else:
            path = os.fspath(model)
            self.ckpt_path = path
            if not os.path.exists(path):
                raise FileNotFoundError(f"weights file not found: {path!r} (no network: nothing is downloaded)")
            if path.endswith(".pt"):
                from .convert import convert_pt
                blob = convert_pt(path)
            else:
                with open(path, "rb") as f:
                    blob = f.read()
        self._blob_meta = from_bytes(blob)[2] if blob[:8] == b"MI355YW1" else {}
        self._blob = blob
        _lib.check(lib.mi355_yolo_create_from_memory(blob, len(blob), self.device, C.byref(opts), C.byref(self._h)))
        info = _lib.ModelInfo()
        _lib.check(lib.mi355_yolo_info(self._h, C.byref(info)))
        self.info_struct = info
        self.task = "pose" if info.task == 1 else "detect"
        if task is not None and task != self.task:
            raise ValueError(f"checkpoint is a {self.task!r} model, not {task!r}")
        self.nc = info.nc
        self.kpt_shape = (info.nkpt, info.kdim)
        names = self._blob_meta.get("names")
        self.names = {int(k): v for k, v in names.items()} if names else default_names(self.nc)
        self._tracker = None

    # ------------------------------------------------------------------------------------------ construction
    @classmethod
    def from_state_dict(cls, name: str, state_dict: Dict[str, np.ndarray], nc: Optional[int] = None, **kw) -> "YOLO":
        """Build from an unfused Ultralytics-named state dict (what a ``.pt`` holds) for model ``name``."""
        return cls(build_from_state_dict(name, state_dict, nc=nc), **kw)

    def _all_handles(self):
        return [h for h in (getattr(self, "_h", None), getattr(self, "_h_other", None), *getattr(self, "_h_feats", {}).values())
                if h is not None and h.value]

    def __del__(self):
        for h in self._all_handles():
            try:
                _lib.lib().mi355_yolo_destroy(h)
            except Exception:
                pass
        self._h, self._h_other, self._h_feats = C.c_void_p(), C.c_void_p(), {}

    def _handle(self, half: Optional[bool], feats: Optional[bool] = None):
        """Engine handle for the requested precision (``half=True`` = Ultralytics' predictor argument: fp16 storage) and feature
        output (``feats``); None = what the model was constructed with."""
        half = self.half if half is None else bool(half)
        feats = self.feats if feats is None else bool(feats)
        if half == self.half and feats == self.feats:
            return self._h
        if feats == self.feats:
            if not self._h_other.value:
                self._h_other = self._create(half, feats)
            return self._h_other
        if half not in self._h_feats:
            self._h_feats[half] = self._create(half, feats)
        return self._h_feats[half]

    def _create(self, half: bool, feats: bool):
        hnd = C.c_void_p()
        opts = _lib.Opts(struct_size=C.sizeof(_lib.Opts), half=int(half), obj_feats=int(feats), **self._opt_kw)
        _lib.check(_lib.lib().mi355_yolo_create_from_memory(self._blob, len(self._blob), self.device, C.byref(opts), C.byref(hnd)))
        return hnd

    def info(self, detailed: bool = False, verbose: bool = False):
        i = self.info_struct
        return i.n_convs, int(i.n_params), 0, 2.0 * i.macs_640 / 1e9     # (layers, params, gradients, GFLOPs)

    # ------------------------------------------------------------------------------------------ inference
    # the batch kinds and the source normaliser live in sources.py; these names are what tests, tools and bench.py use
    _Ragged, _RaggedDevice, _DeviceFrames, _YuvBatch = Ragged, Ragged.from_pointers, DeviceFrames, YuvBatch
    _as_batch = staticmethod(as_batch)

    def _infer_rows(self, batch, conf, iou, classes, max_det, imgsz, half=None, feats=None, feats_out: Optional[list] = None):
        """-> (rows [n, max_det, 58 words], counts [n], (h, w) or the list of them).  An engine with feature output appends
        float32 [n, max_det, s] to ``feats_out``, parallel to ``rows``.  A dense ``batch`` is used as it is: no check, no copy."""
        a = det_args(conf, iou, classes, max_det, imgsz, half, feats)
        shape = batch.shapes if isinstance(batch, (Ragged, YuvBatch)) else (int(batch.shape[1]), int(batch.shape[2]))
        want = feats_out is not None and (self.feats if feats is None else feats)
        # without features the lock is held around the device wait and the C call alone (inside _run); with them it is held (and
        # re-entered there) until they are fetched, before another thread's call replaces them
        with self._lock if want else nullcontext():
            rows, counts, _ = self._run(batch, a)
            if want:
                dim = C.c_int()
                _lib.check(_lib.lib().mi355_yolo_feat_dim(self._last_handle, C.byref(dim)))
                if dim.value:
                    f = np.empty((len(counts), a.max_det, dim.value), np.float32)      # only f[i, :counts[i]] are written / meaningful
                    _lib.check(_lib.lib().mi355_yolo_last_feats(self._last_handle, f.ctypes.data, a.max_det, len(counts)))
                    feats_out.append(f)
        return rows, counts, shape

    def _run(self, batch, a: DetArgs, tile_opts=None):
        """THE blocking detector call: allocates the outputs, takes the lock, waits for the batch (``sources.ready``), notes the engine
        that runs (``_last_handle``) and dispatches on the batch kind -- the only place that does.  -> (rows [n, max_det, 58 words],
        counts [n], tile_idx [n, max_det] of a tiled call or None).  ``tile_opts``: the ``mi355_tile_opts`` of a tiled call, whose batch
        is by pointer (Ragged or YuvBatch)."""
        lib = _lib.lib()
        hnd = self._handle(a.half, a.feats)
        n = int(batch.shape[0])
        rows = np.empty((n, a.max_det, _lib.DET_WORDS), dtype=np.float32)    # only rows[i, :counts[i]] are written / meaningful
        counts = np.zeros(n, dtype=np.int32)
        det = (a.conf, a.iou, *a.classes, a.max_det, a.imgsz, rows.ctypes.data, a.max_det, counts.ctypes.data_as(C.POINTER(C.c_int)))
        tile_idx = None if tile_opts is None else np.full((n, a.max_det), -1, np.int32)
        with self._lock:
            self._last_handle = hnd           # inside the lock: what _build_results, _render_into, plan_info and last_timing read is this call's
            ready(batch, self.device)
            if tile_opts is not None:
                if isinstance(batch, YuvBatch):
                    rc = lib.mi355_yolo_infer_tiled_yuv(hnd, batch.structs, int(batch.on_device), n, C.byref(tile_opts), *det, tile_idx.ctypes.data)
                else:
                    rc = lib.mi355_yolo_infer_tiled(hnd, *batch.args(), C.byref(tile_opts), *det, tile_idx.ctypes.data)
            elif isinstance(batch, YuvBatch):
                rc = lib.mi355_yolo_infer_yuv(hnd, batch.structs, int(batch.on_device), n, *det)
            elif isinstance(batch, Ragged):
                rc = lib.mi355_yolo_infer_multi(hnd, *batch.args(), *det)
            elif isinstance(batch, DeviceFrames) or (isinstance(batch, torch.Tensor) and batch.is_cuda):
                rc = lib.mi355_yolo_infer_device(hnd, batch.data_ptr(), *batch.shape[:3], *det)
            else:
                if isinstance(batch, torch.Tensor):
                    batch = batch.numpy()     # a CPU tensor goes in as the array it is
                rc = lib.mi355_yolo_infer(hnd, batch.ctypes.data, *batch.shape[:3], 0, *det)
            _lib.check(rc)
        return rows, counts, tile_idx

    # ---- device-resident results (multi-GPU pipelines): nothing crosses PCIe, nothing blocks --------------------------
    def new_device_rows(self, n: int, max_det: int = 300):
        """Output buffers for :meth:`infer_async`: (rows [n*max_det, 58] f32, counts [n] i32, total [1] i32) on the engine's GPU."""
        dev = torch.device("cuda", self.device)
        return (torch.empty((n * max_det, _lib.DET_WORDS), dtype=torch.float32, device=dev),
                torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev))

    def infer_async(self, frames: torch.Tensor, out, conf: float = 0.25, iou: float = IOU, classes=None, max_det: int = MAX_DET,
                    imgsz: int = IMGSZ, half=None) -> None:
        """Enqueue one batch of CUDA-resident uint8 frames [n,H,W,3]; the packed post-NMS rows (frame order), the per-frame
        counts and their sum land in ``out`` (from :meth:`new_device_rows`) -- all in HBM.  Returns at once; order other
        streams behind :attr:`stream` (or call :meth:`sync`) before reading ``out``.  ``frames`` may also be a list of CUDA
        :class:`YUVFrame`s of one size (NV12 / I420, formats may differ): their planes are converted on the GPU from where they lie."""
        rows, counts, total = out
        yuv = as_frames(frames)
        if yuv is not None:
            frames = YuvBatch(yuv)
            if not frames.on_device or len(set(frames.shapes)) != 1:
                raise ValueError("infer_async needs YUVFrames of one size with planes on the engine's GPU")
        elif not frames.is_cuda or frames.dtype != torch.uint8 or frames.device.index != self.device:
            raise ValueError("infer_async needs uint8 frames on the engine's GPU")
        n = int(frames.shape[0])
        if rows.shape[0] < n * max_det or counts.numel() < n:
            raise ValueError("output buffers are too small for n * max_det rows")
        a = det_args(conf, iou, classes, max_det, imgsz, half)
        det = (a.conf, a.iou, *a.classes, a.max_det, a.imgsz, rows.data_ptr(), counts.data_ptr(), total.data_ptr())
        hnd = self._handle(half)
        self._async_handle = hnd              # `stream` / `sync()` refer to the engine that received the last asynchronous call
        with self._lock:
            ready(frames, self.device)        # the frames must be complete; the engine has its own stream
            if yuv is not None:
                _lib.check(_lib.lib().mi355_yolo_infer_yuv_device_async(hnd, frames.structs, n, *det))
            else:
                _lib.check(_lib.lib().mi355_yolo_infer_device_async(hnd, frames.data_ptr(), *frames.shape[:3], *det))

    @property
    def stream(self) -> "torch.cuda.ExternalStream":
        """The HIP stream of the engine that received the last :meth:`infer_async` call (the primary engine before any), as
        a torch stream: ``torch.cuda.current_stream().wait_stream(model.stream)``.  A ``half=`` override runs on the second
        engine, which has a stream of its own -- this property follows it."""
        hnd = getattr(self, "_async_handle", None) or self._h
        cache = self.__dict__.setdefault("_ext_streams", {})
        if hnd.value not in cache:
            cache[hnd.value] = torch.cuda.ExternalStream(int(_lib.lib().mi355_yolo_stream(hnd)), device=torch.device("cuda", self.device))
        return cache[hnd.value]

    def sync(self) -> None:
        """Wait for every asynchronous call enqueued so far (both engines, when a ``half=`` override created the second)."""
        for hnd in self._all_handles():
            _lib.check(_lib.lib().mi355_yolo_sync(hnd))

    def predict(self, source=None, conf: Optional[float] = None, iou: float = IOU, classes=None, max_det: int = MAX_DET,
                imgsz: int = IMGSZ, half: Optional[bool] = None, verbose: bool = False, stream: bool = False,
                feats: Optional[bool] = None, tile=None, overlap: float = 0.2, full_frame: bool = True, tile_iou: float = 0.5,
                tile_metric: str = "ios", render=None, encode=None, crops=None, save_crop: bool = False, **kwargs) -> List[Results]:
        """``model.predict`` / ``model(...)``: ultralytics/engine/model.py:Model.predict.
        ``half=True`` runs the fp16-storage engine (fp32 accumulate; results differ from fp32 by fp16 rounding);
        ``None`` = the precision the model was constructed with (fp32 unless ``YOLO(..., half=True)``).
        ``feats=True`` also fills ``Results.feats`` (float32 [M, s]: the detector's own appearance embedding of every box);
        ``None`` = as constructed.  Boxes and keypoints are bit for bit the same either way.
        ``tile`` (int or (tile_h, tile_w)): tiled inference for high-resolution frames -- every frame is cut into tiles overlapping by
        ``overlap`` (a fraction of the tile), the tiles (and with ``full_frame`` the frame itself) run through ONE detector pass at
        ``imgsz`` each, and their rows are merged per frame on the GPU: a row dies when an earlier row of its class overlaps it by more
        than ``tile_iou`` under ``tile_metric`` ("ios": intersection over the smaller box, "iou").  ``Results.tile_idx`` / ``.tiles``
        say which entry every row came from.  ``None`` (default): the call as it always was.
        ``render``: True or a :class:`cvsd_amd.render.RenderSpec` (or a dict of its fields) -- every ``Results`` also
        carries ``rendered``, uint8 [H, W, 3]: a COPY of its frame with its boxes, labels and skeletons drawn in (and people pixelated,
        ``anonymize=``), rendered on the GPU from the copy of the frame this call already put there.  The source frames, the rows and
        the keypoints are what they are without it.  ``None`` (default): the call as it always was.
        ``source`` may hold :class:`cvsd_amd.JPEGFrame`s: baseline JPEG streams, all decoded to BGR on the GPU in one call
        in front of everything else; the call then is what it is for CUDA BGR tensors of the same pixels.
        ``encode``: "jpeg" or a :class:`cvsd_amd.jpeg.JpegSpec` (or a dict of its fields) -- every ``Results`` carries
        ``jpeg``, the bytes of a baseline JFIF stream encoded on the GPU: of the rendered picture with ``render=`` (the picture stays
        on the GPU and ``Results.rendered`` stays None unless ``keep_pixels``), of the source frame itself without.  Only the bytes
        come back.  ``None`` (default): the call as it always was.
        ``crops``: True or a :class:`cvsd_amd.crops.CropSpec` (or a dict of its fields) -- every ``Results`` carries
        ``crops``, crop i the picture of box i (``save_one_box``'s rectangle; native size, or all resampled to ``size``), cut on the
        GPU in ONE launch from the copy of the frames this call already put there (``source="rendered"``: from the drawn picture of
        ``render=``); ``out="cuda"`` with a size leaves one uint8 tensor [M, h, w, 3] per frame on the GPU for a downstream torch
        model.  With ``encode=`` the crops are encoded as well (``Results.crop_jpegs``; their pixels then come back only with
        ``keep_pixels`` or stay on the GPU with ``out="cuda"``).  ``save_crop=True`` is ``crops=True, encode="jpeg"`` when neither is
        given; ``Results.save_crop(dir)`` writes the files.  ``None`` (default): the call as it always was."""
        from .crops import crop_call_args
        from .jpeg import as_spec as as_jpeg_spec
        from .render import as_spec
        a = det_args(0.25 if conf is None else conf, iou, classes, max_det, imgsz, half, feats)
        if has_jpeg_frames(source):
            # JPEG ingest: every JPEGFrame of the call is decoded in ONE call on the engine's stream into CUDA tensors;
            # from here on the call is the one it is for CUDA BGR tensors
            with self._lock:                   # the handle's stream and decode scratch: no other call of this model in between
                source = decode_sources(source, self.device, self._handle(half, feats))
        cspec, encode = crop_call_args(crops, encode, save_crop, render)
        spec, jspec = as_spec(render), as_jpeg_spec(encode)
        tiling = None if tile is None else dict(tile=tile, overlap=overlap, full_frame=full_frame, tile_iou=tile_iou, tile_metric=tile_metric)
        plain = spec is None and jspec is None and cspec is None
        # render= / encode=: the picture is drawn from the frames this call leaves on the GPU, so no other call may come in between
        # (the lock is re-entrant); a plain call holds the lock around its C call only
        with nullcontext() if plain else self._lock:
            batch, originals = as_batch(source, by_pointer=tiling is not None)
            res = self._detect(batch, originals, a, tiling)
            return res if plain else self._render_into(res, spec, None, lambda: self._batch_frames(batch), jspec, cspec)

    def _detect(self, batch, originals, a: DetArgs, tiling: Optional[dict] = None) -> List[Results]:
        """one detector call on a batch: tiled (``tiling``: the tile arguments of :meth:`predict`) or not"""
        if tiling is not None:
            return self._predict_tiled(batch, originals, *a, **tiling)
        return self._predict_batch(batch, originals, *a)

    @staticmethod
    def _batch_frames(batch) -> list:
        """the frames of a call as ``ops.render`` takes them (the fallback of ``_render_into``: a copy that has left the GPU)"""
        return batch.render_frames() if isinstance(batch, (Ragged, YuvBatch)) else list(batch)

    def _render_into(self, results, spec, sources, fallback=None, jspec=None, cspec=None):
        """Fills ``Results.rendered`` of every non-None result with ONE render call on the engine that ran the detector.  ``sources``
        None: the frames of that engine's last call, from where the call left them on the GPU (``fallback()`` -> the frames to pass again
        when a copy has been overwritten: host calls of more than two chunks); else one frame per result as ``ops.render`` takes them.
        ``jspec`` (``encode=``): the pictures stay on the GPU and ONE encode call on the same stream fills ``Results.jpeg`` (the pixels
        come back only with ``keep_pixels``); with ``spec`` None the source frames themselves are encoded.
        ``cspec`` (``crops=``): ONE crop call on the same stream, after the render call and before the encode calls, fills
        ``Results.crops`` from the boxes the results carry (the tracker's, after a tracker step); with ``jspec`` ONE more encode call
        fills ``Results.crop_jpegs``."""
        from . import ops
        from .crops import crop_rects
        from .render import primitives
        idx = [i for i, r in enumerate(results) if r is not None]
        if not idx:
            return results
        hnd = getattr(self, "_last_handle", None) or self._h
        from_pics = cspec is not None and cspec.source == "rendered"
        where = "numpy" if jspec is None and not from_pics else "cuda"

        def on_frames(call):
            if sources is not None:
                return call([sources[i] for i in idx])
            try:
                return call(None)
            except LookupError:
                return call(fallback())

        with self._lock:
            pics = None
            if spec is not None:
                prims = [primitives(results[i], spec) for i in idx]
                pics = on_frames(lambda fr: ops.render(fr, prims, device=self.device, handle=hnd, out=where))
            if cspec is not None:
                rects = [crop_rects(results[i].boxes.xyxy.numpy(), results[i].orig_shape, cspec.gain, cspec.pad, cspec.square) for i in idx]
                cwhere = "cuda" if jspec is not None else cspec.out
                cut = lambda fr: ops.crop_resize(fr, rects, cspec.size, cspec.fit, cspec.fill, device=self.device, out=cwhere, handle=hnd)   # noqa: E731
                cuts = cut(pics) if from_pics else on_frames(cut)
                if jspec is not None:
                    # the crops of non-empty rectangles, all results' in one encode call; an empty rectangle has no stream
                    live = [[bool(r[2] > r[0] and r[3] > r[1]) for r in rr.tolist()] for rr in rects]
                    flat = [c for cc, ll in zip(cuts, live) for c, ok in zip(cc, ll) if ok]
                    enc = iter(ops.jpeg_encode(flat, jspec.quality, jspec.subsampling, device=self.device, handle=hnd) if flat else [])
                    for i, ll in zip(idx, live):
                        results[i].crop_jpegs = [next(enc) if ok else None for ok in ll]
                    if cspec.out != "cuda":
                        cuts = [[c.cpu().numpy() for c in cc] for cc in cuts] if jspec.keep_pixels else None
                if cuts is not None:
                    for i, cc in zip(idx, cuts):
                        results[i].crops = cc
            if jspec is not None:
                enc = lambda fr: ops.jpeg_encode(fr, jspec.quality, jspec.subsampling, device=self.device, handle=hnd)   # noqa: E731
                streams = enc(pics) if pics is not None else on_frames(enc)
                for i, b in zip(idx, streams):
                    results[i].jpeg = b
                if pics is not None:
                    pics = [p.cpu().numpy() for p in pics] if jspec.keep_pixels else None
            elif from_pics:
                pics = [p.cpu().numpy() for p in pics]
        if pics is not None:
            for i, pic in zip(idx, pics):
                results[i].rendered = pic
        return results

    def detect_rows(self, batch, conf: float = 0.25, iou: float = IOU, classes=None, max_det: int = MAX_DET, imgsz: int = IMGSZ, half=None):
        """``Results.boxes.data`` of every frame of ``batch`` -- float32 [M, 6] rows x1, y1, x2, y2, conf, cls -- and the frames' (h, w),
        without building the Results objects (a sweep reads nothing else: cvsd_amd/sweep.py).  ``batch``: what :meth:`predict` takes
        after stacking, or frames already on the engine's GPU (:class:`_DeviceFrames`).  For frames of different shapes
        (:class:`_Ragged`) the second value is the list of every frame's (h, w)."""
        rows, counts, shape = self._infer_rows(batch, conf, iou, classes, max_det, imgsz, half)
        out = []
        for i in range(len(counts)):
            r = rows[i, :counts[i]]
            d = np.empty((len(r), 6), np.float32)
            d[:, :5] = r[:, :5]
            d[:, 5] = r[:, 5:6].view(np.int32)[:, 0]
            out.append(d)
        return out, shape

    def _predict_batch(self, batch, originals, conf, iou, classes, max_det, imgsz, half, feats=None) -> List[Results]:
        fout = []
        rows, counts, shape = self._infer_rows(batch, conf, iou, classes, max_det, imgsz, half, feats, fout)
        return self._build_results(rows, counts, shape, originals, fout)

    def _build_results(self, rows, counts, shape, originals, fout, tile_idx=None, tiles=None) -> List[Results]:
        """rows [n, max_det, 58 words] and counts [n] of a call -> its ``Results``; a tiled call adds every frame's entry indices
        ``tile_idx`` [n, max_det] and entry list ``tiles`` (one int32 [E, 4] array per frame)"""
        t = _lib.Timing()
        _lib.lib().mi355_yolo_last_timing(self._last_handle, C.byref(t))
        per_img_ms = t.total_ms / max(1, len(counts))
        out = []
        for i in range(len(counts)):
            r = rows[i, :counts[i]]
            ints = r[:, 5:7].view(np.int32)
            data = np.concatenate([r[:, :5], ints[:, :1].astype(np.float32)], axis=1)       # x1,y1,x2,y2,conf,cls
            kp = None
            if self.task == "pose":
                nk = self.kpt_shape[0] * self.kpt_shape[1]
                kp = torch.from_numpy(r[:, 7:7 + nk].reshape(len(r), *self.kpt_shape).copy())
            res = Results(originals[i] if originals is not None else None, f"image{i}.jpg", self.names,
                          boxes=torch.from_numpy(data), keypoints=kp.clone() if kp is not None else None,
                          orig_shape=shape[i] if isinstance(shape, list) else shape,
                          speed={"preprocess": 0.0, "inference": per_img_ms, "postprocess": 0.0},
                          anchor_idx=ints[:, 1].copy(), feats=fout[0][i, :counts[i]].copy() if fout else None,
                          tile_idx=tile_idx[i, :counts[i]].copy() if tile_idx is not None else None,
                          tiles=tiles[i] if tiles is not None else None)
            if kp is not None:
                res.keypoints_raw = kp.numpy()          # before Keypoints() zeroes x,y of joints with conf < 0.5
            res._render_device = self.device            # Results.plot() renders where the engine lives
            out.append(res)
        return out

    __call__ = predict

    # ---- tiled predict -----------------------------------------------------------------------------------------
    def _predict_tiled(self, batch, originals, conf, iou, classes, max_det, imgsz, half, feats, tile, overlap=0.2, full_frame=True,
                       tile_iou=0.5, tile_metric="ios") -> List[Results]:
        """One tiled call (``mi355_yolo_infer_tiled`` / ``_tiled_yuv``): every argument is checked here, before any launch."""
        from . import ops
        if self.feats if feats is None else feats:
            raise ValueError("feats=True cannot be combined with tile: a merged row's anchor index no longer identifies its map position")
        th, tw, oy, ox = ops.tile_overlap_px(tile, overlap)
        if tile_metric not in ops.TILE_METRICS:
            raise ValueError(f"tile_metric must be 'ios' or 'iou', got {tile_metric!r}")
        if isinstance(tile_iou, bool) or not isinstance(tile_iou, (int, float, np.integer, np.floating)):
            raise TypeError(f"tile_iou must be a number in [0, 1], got {tile_iou!r}")
        if not 0 <= float(tile_iou) <= 1:
            raise ValueError(f"tile_iou must be in [0, 1], got {tile_iou!r}")
        max_det = int(max_det)
        tiles = []
        for h, w in batch.shapes:
            g = self._grid_px(h, w, th, tw, oy, ox)
            if full_frame:
                g = np.concatenate([g, np.array([[0, 0, w, h]], np.int32)])
            if len(g) > _lib.TILE_MAX_ENTRIES or len(g) * max(1, max_det) > _lib.TILE_MAX_CANDIDATES:
                raise ValueError(f"tile={tile!r} cuts a {h}x{w} frame into {len(g)} entries: at most {_lib.TILE_MAX_ENTRIES} entries and "
                                 f"{_lib.TILE_MAX_CANDIDATES} entries x max_det candidates per frame are merged")
            tiles.append(g)
        opts = _lib.TileOpts(struct_size=C.sizeof(_lib.TileOpts), tile_h=th, tile_w=tw, overlap_y_px=oy, overlap_x_px=ox,
                             full_frame=int(bool(full_frame)), metric=ops.TILE_METRICS[tile_metric], thr=float(tile_iou))
        with self._lock:                       # re-entered by the call: the Results read the timing of the engine that ran it
            rows, counts, tile_idx = self._run(batch, det_args(conf, iou, classes, max_det, imgsz, half, False), opts)
            return self._build_results(rows, counts, list(batch.shapes), originals, [], tile_idx, tiles)

    @staticmethod
    def _grid_px(h, w, th, tw, oy, ox) -> np.ndarray:
        """``mi355_tile_grid`` with the overlaps already in pixels"""
        cnt = C.c_int()
        _lib.check(_lib.lib().mi355_tile_grid(int(h), int(w), th, tw, oy, ox, None, 0, C.byref(cnt)))
        g = np.zeros((cnt.value, 4), np.int32)
        _lib.check(_lib.lib().mi355_tile_grid(int(h), int(w), th, tw, oy, ox, g.ctypes.data, cnt.value, C.byref(cnt)))
        return g

    def track(self, source=None, persist: bool = False, show: bool = False, conf: Optional[float] = None, tracker=None, **kwargs
              ) -> List[Results]:
        """``model.track`` (``/root/reference/model.py:38``): predict at conf 0.1, then the tracker callback adds
        ids.  ultralytics/engine/model.py:Model.track forces batch 1; frames are handled one at a time, in order.
        ``tracker``: a ``botsort.yaml``-style file path or dict (``tracker.tracker_config`` says which keys are honoured and refuses the
        rest); it configures the tracker this call creates.  A ``persist=True`` call that continues a tracker may repeat the argument
        (it is not parsed again) or omit it; settings that differ from the continued tracker's are a ``ValueError``, not ignored.
        With ``with_reid: True`` the detector pass also produces its per-box embeddings and the tracker matches on them.
        ``tile=...`` (with ``overlap``, ``full_frame``, ``tile_iou``, ``tile_metric``) is passed on to :meth:`predict`: the tracker consumes
        the merged rows of the tiled call (not together with ``with_reid``: a tiled call has no features).
        ``render=`` as in :meth:`predict`: drawn after the tracker step, so ``Results.rendered`` shows the tracker's boxes and ids; the
        picture is rendered from the copy of the frame the motion compensation uploaded.  ``encode=`` as in :meth:`predict`.
        ``crops=`` / ``save_crop=`` as in :meth:`predict`: cut after the tracker step, of the tracker's boxes -- the rows the ``Results``
        carry, the ones ``render=`` draws."""
        from .crops import crop_call_args
        from .jpeg import as_spec as as_jpeg_spec
        from .render import as_spec
        from .tracker import BYTETracker
        kwargs.pop("batch", None)
        cspec, encode = crop_call_args(kwargs.pop("crops", None), kwargs.pop("encode", None), kwargs.pop("save_crop", False), kwargs.get("render"))
        spec = as_spec(kwargs.pop("render", None))
        jspec = as_jpeg_spec(encode)
        conf = 0.1 if conf is None else conf
        cfg = self._tracker_settings("track", tracker, continuing=self._tracker is not None and persist)
        if cfg is not None:
            # the frame preparation and the optical flow of its motion compensation run on the engine's GPU (csrc/gmc_kernels.hip)
            self._tracker = BYTETracker(gmc_device=getattr(self, "device", None), **cfg)
        reid = self._tracker.with_reid
        if reid:
            kwargs["feats"] = True
        if has_jpeg_frames(source):
            # JPEG frames are decoded on the GPU in one call and, as YUV frames below, brought to the host for the motion compensation
            with self._lock:
                source = decode_sources(source, self.device, self._h, to_host=True)
        yuv = as_frames(source)
        if yuv is not None:
            # the convenience form: the motion compensation takes a host BGR frame, so a YUV frame is converted on the GPU and its BGR
            # bytes come back to the host (one device-to-host copy per frame); the call then proceeds as on BGR frames
            source = [f.to_bgr(self.device) for f in yuv]
        batch, originals = as_batch(source)
        if isinstance(batch, Ragged):
            raise ValueError("frames of different shapes in one call are not supported; call once per shape")
        a = det_args_from(conf, kwargs)
        tiling = None if kwargs.get("tile") is None else {k: kwargs[k] for k in ("tile", "overlap", "full_frame", "tile_iou", "tile_metric") if k in kwargs}
        results = []
        for i in range(int(batch.shape[0])):
            frame = originals[i] if originals is not None else batch[i].cpu().numpy()
            # the tracker's motion compensation for this frame (frame preparation + optical flow, a stream of its own on the GPU) is
            # enqueued before the detector pass and collected inside tracker.update: the two share the GPU instead of queueing
            self._tracker.gmc.begin(frame)
            # ... and the detector pass reads the copy of the frame that step has just put on the GPU: one upload, and no second host -> device
            # copy queueing behind the step's device -> host copies (which wait for its Lucas-Kanade launch -- the two used to run one after
            # the other, tools/track_timeline.py)
            share = os.environ.get("MI355_TRACK_SHARED_FRAME", "1") != "0"            # A/B and tests only
            dev = self._tracker.gmc.pending_device_frame() if share and isinstance(frame, np.ndarray) and frame.ndim == 3 else None
            if dev is not None and (dev[1:] != tuple(frame.shape[:2]) or kwargs.get("stream")):
                dev = None
            if dev is None:
                res = self.predict(batch[i:i + 1], conf=conf, **kwargs)[0]
            else:
                # tiled: the tiles are cut from the same uploaded copy (by pointer), and the tracker consumes the merged rows
                shared = DeviceFrames(dev[0], 1, dev[1], dev[2]) if tiling is None else Ragged.from_pointers([dev[0]], [dev[1:]])
                res = self._detect(shared, None, a, tiling)[0]
            if originals is not None:
                res.orig_img = originals[i]
            # trackers/track.py:on_predict_postprocess_end: the tracker steps on EVERY frame (an empty frame still advances
            # frame_id, ages lost tracks against track_buffer and runs the Kalman predict); only the rewrite of the
            # result is skipped when no track comes back
            tracks = self._tracker.update(res.boxes.data.numpy(), frame, feats=res.feats if reid else None)   # trackers/track.py: tracker.update(det, im0, feats)
            res = self._with_tracks(res, tracks)
            if spec is not None or jspec is not None or cspec is not None:
                # the motion compensation's copy stays where it is until its next step; without one, the detector call's own copy
                self._render_into([res], spec, None if dev is None else [DeviceFrame(dev[0], dev[1], dev[2])], lambda: [frame], jspec, cspec)
            results.append(res)
        return results

    def _tracker_settings(self, which: str, tracker, continuing: bool) -> Optional[dict]:
        """``tracker=`` of :meth:`track` / :meth:`track_cameras` -> the ``BYTETracker`` keywords of the tracker(s) to create, or None when
        the call continues existing ones.  The argument is parsed where a tracker is created; a continuing call that brings the argument
        it was created with (or none) parses nothing, and one that brings other settings is refused."""
        from .tracker import tracker_config
        made = self.__dict__.setdefault("_tracker_made", {})
        if not continuing:
            cfg = tracker_config(tracker)
            made[which] = (dict(tracker) if isinstance(tracker, dict) else tracker, cfg)
            return cfg
        arg0, cfg0 = made.get(which, (None, {}))
        if tracker is not None and not (type(tracker) is type(arg0) and tracker == arg0):
            full = lambda c: {"with_reid": False, "proximity_thresh": 0.5, "appearance_thresh": 0.8, **c}
            if full(tracker_config(tracker)) != full(cfg0):
                raise ValueError("tracker: these settings differ from those of the tracker this call continues (persist=True); "
                                 "start a new tracker with persist=False")
            made[which] = (dict(tracker) if isinstance(tracker, dict) else tracker, cfg0)
        return None

    @staticmethod
    def _with_tracks(res: Results, tracks: np.ndarray) -> Results:
        """trackers/track.py:on_predict_postprocess_end: the result re-indexed to the detections that carry a track, its boxes rewritten
        with the ids; untouched when no track came back"""
        if len(tracks):
            idx = tracks[:, -1].astype(int)
            res = res[idx]
            res.update(boxes=torch.as_tensor(tracks[:, :-1], dtype=torch.float32))
        return res

    def track_cameras(self, frames: Sequence[Optional[np.ndarray]], persist: bool = False, conf: Optional[float] = None, **kwargs
                      ) -> List[Optional[Results]]:
        """One tick of several cameras: ``frames[i]`` is camera i's BGR frame (any size, each camera its own) or None when it delivered
        none; -> per camera the tracked ``Results`` of :meth:`track`, None for an absent camera (whose tracker does not step).  Ultralytics
        tracks several streams with one tracker per stream; so does this call -- ids are per camera, each starting at 1 -- but the tick costs
        ONE detector pass over all present frames (the mixed-shape path of :meth:`predict`) and ONE motion-compensation step
        (``gmc.MultiGMC``), whose uploaded frames the detector reads in place.  ``persist=True`` continues the cameras' tracks (the list
        length is the number of cameras and must not change); otherwise every camera starts afresh.  Keyword arguments: ``iou``,
        ``classes``, ``max_det``, ``imgsz``, ``half``, ``feats`` as in :meth:`predict`, ``tracker`` as in :meth:`track` (every camera's
        tracker gets the same settings); ``show`` / ``verbose`` are accepted and ignored; anything else is a ``TypeError``.

        ``motion_gate``: None (default) -- the call as it always was; True, a dict of ``MotionGate`` options (``block``,
        ``level``, ``min_blocks``, ``max_skip``) or a :class:`MotionGate` for exactly this many cameras -- the detector runs only on the
        present cameras the gate calls moving (not at all when there are none), and a static camera's tracker steps, with this tick's warp,
        on the rows the detector last produced for that camera: it ages, predicts and keeps its ids as if the detector had returned the
        same rows again.  The gate reads the frames the motion compensation uploaded.  Every returned ``Results`` then carries
        ``motion = {"moving", "changed", "skipped"}`` and, for a static camera, this tick's frame as ``orig_img``.  The letterbox geometry
        follows the list handed to the detector, as with absent cameras: moving frames of one shape take the rect path, of mixed shapes
        the square canvas.  ``persist=False`` resets the gate along with the trackers.

        ``render``: as in :meth:`predict` -- every present camera's ``Results.rendered`` is its frame with the tracker's
        boxes and ids drawn in, all cameras in ONE render call reading the frames the motion compensation uploaded; an absent camera has
        no picture, and a camera the motion gate skipped is drawn with the rows its tracker stepped on.
        ``encode``: as in :meth:`predict` -- ``Results.jpeg`` of every present camera, all cameras in ONE encode call;
        an absent camera has no bytes.
        ``crops`` / ``save_crop``: as in :meth:`predict` -- ``Results.crops`` of every present camera, the tracker's
        boxes, all cameras in ONE crop launch; an absent camera stays None, and a camera the motion gate skipped has its carried rows
        cut out of this tick's frame."""
        from .crops import crop_call_args
        from .gmc import MultiGMC
        from .jpeg import as_spec as as_jpeg_spec
        from .render import as_spec
        from .tracker import BYTETracker
        tracker = kwargs.pop("tracker", None)
        motion_gate = kwargs.pop("motion_gate", None)
        cspec, encode = crop_call_args(kwargs.pop("crops", None), kwargs.pop("encode", None), kwargs.pop("save_crop", False), kwargs.get("render"))
        rspec = as_spec(kwargs.pop("render", None))
        jspec = as_jpeg_spec(encode)
        unknown = set(kwargs) - {"iou", "classes", "max_det", "imgsz", "half", "feats", "show", "verbose"}
        if unknown:                                              # show / verbose are accepted and ignored, as in track()
            raise TypeError(f"track_cameras: unsupported argument(s) {sorted(unknown)} (iou, classes, max_det, imgsz, half pass through)")
        a = det_args_from(0.1 if conf is None else conf, kwargs)
        # a camera that delivers a YUVFrame: converted on the GPU, its BGR bytes brought to the host for the motion compensation (as track())
        if has_jpeg_frames(frames):                              # ... and the cameras that deliver JPEGFrames: one decode call for all of them
            with self._lock:
                frames = decode_sources(list(frames), self.device, self._h, to_host=True)
        frames = [f.to_bgr(self.device) if isinstance(f, YUVFrame) else f for f in frames]
        n = len(frames)
        if n == 0:
            raise ValueError("empty list of cameras")
        for i, f in enumerate(frames):
            if f is None:
                continue
            if not isinstance(f, np.ndarray):
                raise ValueError("frames must be uint8 arrays of shape [H,W,3] (BGR, as cv2 delivers them), or None for an absent camera")
            frames[i] = bgr_view(f, dense=True).keep             # dense: the motion compensation takes C-contiguous frames
        spec = self._motion_gate_spec(motion_gate, n)
        cams = getattr(self, "_cameras", None)
        if persist and cams is not None and len(cams[0]) != n:
            raise ValueError(f"{n} frames for {len(cams[0])} tracked cameras: the list length is the number of cameras (None = absent)")
        cfg = self._tracker_settings("cameras", tracker, continuing=cams is not None and persist)
        if cfg is not None:
            # one BoT-SORT core per camera, stepped with the warp of the shared motion-compensation object (on the engine's GPU)
            cams = self._cameras = ([BYTETracker(gmc_method=None, **cfg) for _ in range(n)], MultiGMC(n, device=self.device))
        trackers, gmc = cams
        reid = trackers[0].with_reid
        gate = self._camera_gate_for(spec, n, restart=cfg is not None)
        present = [i for i, f in enumerate(frames) if f is not None]
        out: List[Optional[Results]] = [None] * n
        if not present:
            return out
        # the tick's motion compensation (all cameras: frame preparation + optical flow, one launch per stage on a stream of its own) is
        # enqueued before the detector pass, which reads the frames that step has just uploaded; RANSAC runs on host threads meanwhile
        gmc.begin(frames)
        share = os.environ.get("MI355_TRACK_SHARED_FRAME", "1") != "0"                # A/B and tests only
        run = present                                            # the cameras the detector sees
        try:
            dev = gmc.pending_device_frames() if share else None
            if dev is not None and any(dev[i] is None for i in present):
                raise RuntimeError("track_cameras: the motion compensation's pending tick is not this call's")
            if gate is not None:
                # the gate's launch reads the frames that step uploaded: their pointers came back behind the event wait for that upload
                # (mi355_gmc_multi_frames), which is what orders the detector pass behind it as well
                g, cache = gate
                if dev is not None and g.device == self.device:
                    moving, changed = g._update_device_bgr(dev, [None if f is None else f.shape[:2] for f in frames])
                else:
                    moving, changed = g.update(frames)
                run = [i for i in present if moving[i] or cache[i] is None]
        except BaseException:
            gmc.reset()
            raise
        originals = [frames[i] for i in run]
        res = []
        if run:
            if dev is not None:
                batch = Ragged.from_pointers([dev[i] for i in run], [f.shape[:2] for f in originals])
            else:
                batch = Ragged(originals, False)
            try:
                res = self._predict_batch(batch, originals, *a._replace(feats=True if reid else a.feats))
            except BaseException:
                gmc.reset()                                      # the enqueued tick must not be taken for the next call's frames
                if gate is not None:
                    gate[0].reset()                              # its references are this tick's grids, for which no rows exist
                raise
        warps = gmc.apply(frames)
        if gate is None:
            for r, i in zip(res, present):
                out[i] = self._with_tracks(r, trackers[i].update(r.boxes.data.numpy(), warp=warps[i], feats=r.feats if reid else None))    # an empty frame still steps
            return out if rspec is None and jspec is None and cspec is None else self._render_cameras(out, rspec, frames, dev, jspec, cspec)
        fresh = dict(zip(run, res))
        for i in present:
            r = fresh.get(i)
            if r is not None:
                cache[i] = self._result_snapshot(r)
            else:
                r = self._result_from_snapshot(cache[i], frames[i])    # the rows the detector last produced for this camera, on this tick's frame
                r._render_device = self.device
            r = self._with_tracks(r, trackers[i].update(r.boxes.data.numpy(), warp=warps[i], feats=r.feats if reid else None))
            r.motion = {"moving": bool(moving[i]), "changed": int(changed[i]), "skipped": i not in fresh}
            out[i] = r
        return out if rspec is None and jspec is None and cspec is None else self._render_cameras(out, rspec, frames, dev, jspec, cspec)

    def _render_cameras(self, out, spec, frames, dev, jspec=None, cspec=None):
        """``track_cameras(render=..., encode=...)``: the present cameras' pictures from the tick's uploaded frames (valid until the next tick's
        motion-compensation step), or from the host frames when that step shared none"""
        src = [None if f is None else (f if dev is None else DeviceFrame(dev[i], f.shape[0], f.shape[1])) for i, f in enumerate(frames)]
        return self._render_into(out, spec, src, None, jspec, cspec)

    # ---- motion gate of track_cameras --------------------------------------------------------------------------
    @staticmethod
    def _motion_gate_spec(arg, n: int):
        """``motion_gate=`` of :meth:`track_cameras` -> None, the validated options of the gate to create, or the caller's MotionGate"""
        if arg is None or arg is False:
            return None
        from .motion import OPTIONS, MotionGate, check_options
        if arg is True:
            return check_options()
        if isinstance(arg, MotionGate):
            if arg.n != n:
                raise ValueError(f"motion_gate: a MotionGate for {arg.n} cameras given to a call with {n} cameras")
            return arg
        if isinstance(arg, dict):
            unknown = sorted(set(arg) - set(OPTIONS))
            if unknown:
                raise ValueError(f"motion_gate: unknown option(s) {unknown} (the options are {list(OPTIONS)})")
            return check_options(**arg)
        raise TypeError(f"motion_gate must be None, True, a dict of MotionGate options or a MotionGate, not {type(arg).__name__}")

    def _camera_gate_for(self, spec, n: int, restart: bool):
        """-> (gate, per-camera cache of the last detector result) of a gated call, None for an ungated one.  The gate is kept between
        ``persist=True`` calls that bring the same argument; new trackers, another argument or an ungated call in between start it afresh."""
        from .motion import MotionGate
        held = self.__dict__.get("_camera_gate")
        if spec is None:
            if held is not None:
                self._camera_gate = None                         # a later gated call must not step trackers on rows older than this call's
            return None
        if held is not None and not restart and (held[0] is spec if isinstance(spec, MotionGate) else (held[1] == spec and held[0].n == n)):
            return held[0], held[2]
        g = spec if isinstance(spec, MotionGate) else MotionGate(n, device=self.device, **spec)
        g.reset()
        self._camera_gate = (g, None if isinstance(spec, MotionGate) else spec, [None] * n)
        return g, self._camera_gate[2]

    @staticmethod
    def _result_snapshot(r: Results) -> dict:
        """private copies of a pre-tracker result: what a static camera's tracker steps on until the detector sees that camera again"""
        return {"boxes": r.boxes.data.clone(), "keypoints": None if r.keypoints is None else r.keypoints.data.clone(),
                "keypoints_raw": None if getattr(r, "keypoints_raw", None) is None else r.keypoints_raw.copy(),
                "anchor_idx": None if r.anchor_idx is None else r.anchor_idx.copy(), "feats": None if r.feats is None else r.feats.copy(),
                "orig_shape": r.orig_shape, "path": r.path, "names": r.names}

    @staticmethod
    def _result_from_snapshot(c: dict, frame) -> Results:
        kp = c["keypoints"]
        r = Results(frame, c["path"], c["names"], boxes=c["boxes"].clone(), keypoints=kp.clone() if kp is not None else None,
                    orig_shape=c["orig_shape"], speed={"preprocess": 0.0, "inference": 0.0, "postprocess": 0.0},
                    anchor_idx=None if c["anchor_idx"] is None else c["anchor_idx"].copy(), feats=None if c["feats"] is None else c["feats"].copy())
        if c["keypoints_raw"] is not None:
            r.keypoints_raw = c["keypoints_raw"].copy()
        return r

    # ------------------------------------------------------------------------------------------ test hooks
    def raw_head(self, source, imgsz: int = 640, half: Optional[bool] = None) -> np.ndarray:
        """Pre-NMS head tensor ``[N, 4+nc+nk, A]`` exactly as ``Detect/Pose.forward`` returns it (a list of frames of different
        shapes: the square ``imgsz x imgsz`` canvas, A = its anchors)."""
        lib = _lib.lib()
        hnd = self._handle(half)
        if as_frames(source) is not None:
            raise TypeError("raw_head takes BGR frames: convert a YUVFrame with .to_bgr() first")
        batch, _ = as_batch(source)
        if isinstance(batch, Ragged):
            call = lambda data: lib.mi355_yolo_raw_head_multi(hnd, *batch.args(), imgsz, data, C.byref(ch), C.byref(an))     # noqa: E731
        else:
            if isinstance(batch, torch.Tensor):
                batch = batch.cpu().numpy()   # a dense tensor is brought to the host: the hook takes host memory
            call = lambda data: lib.mi355_yolo_raw_head(hnd, batch.ctypes.data if data else None, *batch.shape[:3], 0, imgsz, data,     # noqa: E731
                                                        C.byref(ch), C.byref(an))
        ch, an = C.c_int(), C.c_int()
        _lib.check(call(None))                # the sizing call: null output, nothing is launched
        out = np.empty((batch.shape[0], ch.value, an.value), dtype=np.float32)
        with self._lock:
            ready(batch, self.device)
            _lib.check(call(out.ctypes.data))
        return out

    def plan_info(self) -> dict:
        """Launch plans of the shape last run: hash (candidates + choices), where the choices came from, launches per pass and
        the activation footprint in bytes."""
        hsh, src, nl, ab, au = C.c_ulonglong(), C.c_int(), C.c_int(), C.c_longlong(), C.c_longlong()
        _lib.check(_lib.lib().mi355_yolo_plan_info(getattr(self, "_last_handle", self._h), C.byref(hsh), C.byref(src), C.byref(nl), C.byref(ab),
                                                   C.byref(au)))
        return {"plan_hash": f"{hsh.value:016x}", "plan_source": ("static", "memory", "cache", "tuned", "file")[src.value] if 0 <= src.value <= 4 else str(src.value),
                "launches_per_pass": nl.value, "activation_bytes": ab.value, "activation_bytes_unshared": au.value}

    def sparse_stats(self) -> dict:
        """The sparse box branch of the shape last run: whether it is on, passes that enqueued it, passes in which a position list
        overflowed (the dense box branch did the work), and the last pass's dilated / candidate positions per head level."""
        v = (C.c_longlong * 10)()
        _lib.check(_lib.lib().mi355_yolo_sparse_stats(getattr(self, "_last_handle", self._h), v))
        why = ("", "no such head, half or switched off", "below the frames-per-pass threshold", "plan of cv2.i.1 is not the fused 3x3 + 1x1 launch",
               "plan of cv2.i.0 is not a gated 3x3 kernel")
        return {"enabled": v[0] == 1, "dense_because": "" if v[0] == 1 else why[min(4, max(1, -int(v[0])))], "passes": int(v[1]), "dense_fallbacks": int(v[2]), "dilated": [int(v[3]), int(v[4]), int(v[5])],
                "candidates": [int(v[6]), int(v[7]), int(v[8])], "last_overflow": bool(v[9])}

    def set_profiling(self, on: bool = True) -> None:
        for hnd in self._all_handles():
            _lib.check(_lib.lib().mi355_yolo_set_profiling(hnd, int(on)))

    def last_timing(self) -> dict:
        t = _lib.Timing()
        _lib.check(_lib.lib().mi355_yolo_last_timing(getattr(self, "_last_handle", self._h), C.byref(t)))
        return {k: getattr(t, k) for k, _ in _lib.Timing._fields_}
