"""The opt-in JPEG frame sources of preprocess_driver: ``MjpegCapture`` over a raw concatenated MJPEG file and
``ImageDirCapture(decode=False)`` hand on ``JPEGFrame``s without decoding; the defaults are what they were."""
import io

import numpy as np
from PIL import Image

import _jpeg_decode_cases as K
from cvsd_amd import JPEGFrame
from cvsd_amd import preprocess_driver as D
from cvsd_amd.jpeg_decode import split_mjpeg


def _streams():
    picks = [("33x70", "420", 85, "rr1"), ("17x17", "444", 100, "opt"), ("35x18", "gray", 50, "std"), ("rows72x8", "444", 50, "own")]
    return [K.stream(*p) for p in picks]


def test_mjpeg_capture_splits_outside_entropy_data(tmp_path):
    streams = _streams()
    thumb = io.BytesIO()
    Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(thumb, "JPEG")
    # a stream with a whole JPEG (SOI .. EOI) inside an APP1 segment: stepped over by its length, it cuts nothing
    t = thumb.getvalue()
    nested = streams[0][:2] + b"\xff\xe1" + (len(t) + 2).to_bytes(2, "big") + t + streams[0][2:]
    path = tmp_path / "cam.mjpeg"
    path.write_bytes(b"junk" + streams[0] + streams[1] + b"\r\n--frame\r\n" + nested + streams[2] + streams[3] + streams[1][:-5])
    assert split_mjpeg(path.read_bytes()) == [streams[0], streams[1], nested, streams[2], streams[3]]
    cap = D.MjpegCapture(str(path))
    assert cap.isOpened() and cap.get(D.CAP_PROP_FRAME_COUNT) == 5.0
    want = [streams[0], streams[1], nested, streams[2], streams[3]]
    for i, w in enumerate(want):
        ok, f = cap.read()
        assert ok and isinstance(f, JPEGFrame) and f.data == w and cap.get(D.CAP_PROP_POS_FRAMES) == i + 1
        assert np.array_equal(f.to_bgr(device=-1), K.pillow_decode(w))
    assert cap.read() == (False, None)
    cap.release()
    assert not cap.isOpened()
    assert not D.MjpegCapture(str(tmp_path / "none.mjpeg")).isOpened() and not D.MjpegCapture(str(tmp_path)).isOpened()
    (tmp_path / "empty.mjpg").write_bytes(b"no frames here")
    assert not D.MjpegCapture(str(tmp_path / "empty.mjpg")).isOpened()


def test_image_dir_capture_without_decoding(tmp_path):
    streams = _streams()
    clip = tmp_path / "clip"
    clip.mkdir()
    for i, s in enumerate(streams[:3]):
        (clip / f"{i + 1}.jpg").write_bytes(s)
    Image.fromarray(np.full((4, 6, 3), 7, np.uint8)).save(clip / "10.png")
    cap = D.ImageDirCapture(str(clip), decode=False)
    for s in streams[:3]:
        ok, f = cap.read()
        assert ok and isinstance(f, JPEGFrame) and f.data == s
    ok, f = cap.read()
    assert ok and isinstance(f, np.ndarray) and f.shape == (4, 6, 3) and (f == 7).all()      # a PNG is decoded as always
    assert cap.read() == (False, None)
    cap = D.ImageDirCapture(str(clip))                                                           # the default: unchanged
    for s in streams[:3]:
        ok, f = cap.read()
        assert ok and isinstance(f, np.ndarray) and np.array_equal(f, K.pillow_decode(s))
