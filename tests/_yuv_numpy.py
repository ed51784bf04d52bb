"""numpy restatement of the 4:2:0 YUV -> BGR conversion, written from the formula with int64 intermediates, independently
of csrc/yuv_kernels.hip; the test inputs of tests/test_yuv_convert.py and tests/test_gpu_yuv.py (planes, layout cases, guarded outputs)."""
import numpy as np

CY, CUB, CUG, CVG, CVR, SHIFT = 1220542, 2116026, -409993, -852492, 1673527, 20

# (Y, U, V) -> (B, G, R)
KNOWN = [((16, 128, 128), (0, 0, 0)), ((235, 128, 128), (255, 255, 255)), ((0, 128, 128), (0, 0, 0)), ((255, 128, 128), (255, 255, 255)),
         ((81, 90, 240), (0, 0, 254)), ((145, 54, 34), (1, 255, 0)), ((41, 240, 110), (255, 0, 0)), ((128, 0, 0), (0, 255, 0)),
         ((128, 255, 255), (255, 0, 255))]


def yuv_to_bgr(y, u, v):
    """y [H, W], u and v [H/2, W/2] uint8 -> BGR [H, W, 3] uint8: one (U, V) sample per 2x2 block, floor shift, saturation"""
    yy = np.maximum(0, y.astype(np.int64) - 16) * CY
    uu = np.repeat(np.repeat(u.astype(np.int64) - 128, 2, axis=0), 2, axis=1)
    vv = np.repeat(np.repeat(v.astype(np.int64) - 128, 2, axis=0), 2, axis=1)
    half = 1 << (SHIFT - 1)
    r = (yy + half + CVR * vv) >> SHIFT                    # numpy's >> on signed integers is arithmetic: floor
    g = (yy + half + CVG * vv + CUG * uu) >> SHIFT
    b = (yy + half + CUB * uu) >> SHIFT
    return np.clip(np.stack([b, g, r], axis=-1), 0, 255).astype(np.uint8)


def bgr_to_yuv420(bgr):
    """float BT.601 limited range with 2x2 chroma averaging: makes test inputs out of BGR frames (need not be exact)"""
    f = bgr.astype(np.float64)
    b, g, r = f[..., 0], f[..., 1], f[..., 2]
    y = 16 + 0.257 * r + 0.504 * g + 0.098 * b
    u = 128 - 0.148 * r - 0.291 * g + 0.439 * b
    v = 128 + 0.439 * r - 0.368 * g - 0.071 * b
    h, w = y.shape
    pool = lambda a: a.reshape(h // 2, 2, w // 2, 2).mean(axis=(1, 3))
    q = lambda a: np.clip(np.rint(a), 0, 255).astype(np.uint8)
    return q(y), q(pool(u)), q(pool(v))


def _pitched(plane, stride, offset=0):
    """a copy of `plane` whose rows are `stride` bytes apart, starting `offset` bytes into a 64-byte aligned block; the padding is 0xEE"""
    h, w = plane.shape
    stride = w if stride is None else stride
    raw = np.full(h * stride + offset + 64, 0xEE, np.uint8)
    start = (-raw.ctypes.data) % 64 + offset
    view = np.lib.stride_tricks.as_strided(raw[start:], shape=(h, w), strides=(stride, 1))
    view[...] = plane
    return view


def make_frame(y, u, v, fmt, y_stride=None, uv_stride=None, y_offset=0):
    """a cvsd_amd.YUVFrame of the samples in layout `fmt`, with the given pitches (None = dense) and Y base offset"""
    from cvsd_amd import YUVFrame
    yp = _pitched(y, y_stride, y_offset)
    if fmt == "nv12":
        uv = np.stack([u, v], axis=-1).reshape(u.shape[0], u.shape[1] * 2)
        return YUVFrame(yp, uv=_pitched(uv, uv_stride), fmt="nv12")
    return YUVFrame(yp, u=_pitched(u, uv_stride), v=_pitched(v, uv_stride), fmt="i420")


def ramp_samples(h, w, y_value=120):
    """constant Y and a per-block chroma ramp: every 2x2 block gets its own (U, V), so a sample that coloured a neighbouring block shows"""
    k = np.arange((h // 2) * (w // 2)).reshape(h // 2, w // 2)
    return np.full((h, w), y_value, np.uint8), ((k * 37 + 11) % 256).astype(np.uint8), ((k * 101 + 7) % 256).astype(np.uint8)


# name -> (h, w, NV12 (y_stride, uv_stride), I420 (y_stride, uv_stride), y base offset); None = dense
LAYOUT_CASES = {
    "2x2 minimum": (2, 2, (None, None), (None, None), 0),
    "4x6 generic": (4, 6, (None, None), (None, None), 0),
    "2x16 one vector lane": (2, 16, (None, None), (None, None), 0),
    "6x48 pitched vector": (6, 48, (64, 64), (64, 32), 0),
    "4x18 width not a multiple of 16": (4, 18, (None, None), (None, None), 0),
    "4x16 Y base offset by 1": (4, 16, (32, None), (32, None), 1),
}


def layout_frame(name, fmt):
    """-> (YUVFrame, expected BGR) of a layout case"""
    h, w, nv12, i420, off = LAYOUT_CASES[name]
    y, u, v = ramp_samples(h, w)
    ys, uvs = nv12 if fmt == "nv12" else i420
    return make_frame(y, u, v, fmt, ys, uvs, off), yuv_to_bgr(y, u, v)


def all_triples():
    """every (Y, U, V) triple once, as a 4096 x 4096 image: each of the 256 x 256 (U, V) pairs owns a 16 x 16 pixel square = 8 patches of
    2 x 16 pixels stacked vertically; a patch holds 32 Y samples, the 8 patches of a pair the 256 Y values"""
    bi, bj = np.meshgrid(np.arange(2048), np.arange(2048), indexing="ij")        # chroma sample (bi, bj) belongs to pair (bi // 8, bj // 8)
    u = (bi // 8).astype(np.uint8)
    v = (bj // 8).astype(np.uint8)
    py, px = np.meshgrid(np.arange(4096), np.arange(4096), indexing="ij")
    y = (((py // 2) % 8) * 32 + (py % 2) * 16 + (px % 16)).astype(np.uint8)       # patch, row of the patch, column of the patch
    return y, u, v


def guarded(shape, guard=64, sentinel=0x5C):
    """-> (array view of `shape`, whole buffer, guard slice): the array is followed by `guard` sentinel bytes"""
    n = int(np.prod(shape))
    buf = np.full(n + guard, sentinel, np.uint8)
    return buf[:n].reshape(shape), buf, buf[n:]


def convert_guarded(frames, device=-1):
    """ops.yuv_to_bgr into buffers with 64 guard bytes behind them -> the BGR arrays; asserts the guards kept their sentinel"""
    from cvsd_amd import ops
    outs = [guarded((f.shape[0], f.shape[1], 3)) for f in frames]
    got = ops.yuv_to_bgr(frames, device=device, out=[o[0] for o in outs])
    for (_, _, guard), f in zip(outs, frames):
        assert (guard == 0x5C).all(), f"guard bytes behind a {f.shape} frame changed"
    return got
