"""YUYV422 / UYVY422, GRAY8 and BGR24 frames, and the BT.709 / full-range colour flags on the four YUV formats, through the HIP path
(the decoder side).  The colour conversion is integer arithmetic and only decides which bytes a tap is made of: the
resize kernels must see exactly the RGB bytes tests/pixfmt_oracle.py works out, so everything downstream -- network input, rows --
is bit-identical to the RGB24 path on those bytes.  Both kernels: the per-pixel form and the row-staged form (WZ_PRE_ROWS=1, and
frames read in place from page-locked host memory)."""
import functools
import os

import numpy as np
import pytest

import conftest
import pixfmt_oracle as px
from watsor_amd.runtime import (CSP_BT709, FMT_BGR24, FMT_GRAY8, FMT_I420, FMT_NV12, FMT_RGB24, FMT_UYVY422, FMT_YUYV422, RANGE_FULL,
                                ROW_DTYPE)
from watsor_amd.synth import synthetic_frame

pytestmark = pytest.mark.gpu

FMT = {"nv12": FMT_NV12, "i420": FMT_I420, "yuyv422": FMT_YUYV422, "uyvy422": FMT_UYVY422, "gray": FMT_GRAY8, "bgr24": FMT_BGR24}
YUV = ["nv12", "i420", "yuyv422", "uyvy422"]
COLOURS = {"601-limited": 0, "601-full": RANGE_FULL, "709-limited": CSP_BT709, "709-full": CSP_BT709 | RANGE_FULL}


def engine_with(model_dir, env, **kw):
    saved = {k: os.environ.get(k) for k in ("WZ_PRE_ROWS", "WZ_HOST_READ")}
    for k in saved:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        return conftest.make_engine(model_dir, dev=True, **kw)         # (the knobs are read when the engine is created)
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@pytest.fixture(scope="module")
def engines(model_dir):
    """The per-pixel kernel and the row-staged kernel, one engine each."""
    e = {"pixel": engine_with(model_dir, {"WZ_PRE_ROWS": "0"}), "rows": engine_with(model_dir, {"WZ_PRE_ROWS": "1"})}
    yield e
    for x in e.values():
        x.close()


@functools.lru_cache(maxsize=None)
def _case(w, h, word):
    """(frame, the RGB24 frame the restatement converts it to), built once and shared (read-only).  A picture with real chroma
    detail: the synthetic RGB frame converted, then every byte perturbed (so that out-of-range levels, clipping and odd chroma
    values occur), as `_yuv_frame` of tests/test_gpu_yuv.py does."""
    seed = 31 * w + h + word
    rng = np.random.default_rng(seed)
    rgb = synthetic_frame(w, h, seed) if w > 8 else rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    f = px.frame_from_rgb(rgb, word).astype(np.int16)
    f += rng.integers(-24, 25, f.shape, dtype=np.int16)
    f[::37, ::11] = rng.integers(0, 256, f[::37, ::11].shape)
    f = np.clip(f, 0, 255).astype(np.uint8)
    want = px.rgb_from_frame(f, w, h, word)
    f.setflags(write=False)
    want.setflags(write=False)
    return f, want


def _same_network_input(eng, w, h, word):
    frame, rgb = _case(w, h, word)
    got = eng.stage_preprocess(frame, word)
    want = eng.stage_preprocess(rgb)
    assert got.shape == want.shape
    np.testing.assert_array_equal(got.view(np.uint16), want.view(np.uint16))


# the smallest sizes at which each kernel can go wrong: one / two macropixels; identity; a scale just above 1 (several output rows
# per workgroup of the row-staged kernel); odd height (4:2:2) / odd width and height (gray, BGR24); 1080p (the resize skips rows)
SIZES = [(fmt, size) for fmt in FMT for size in [(2, 2), (4, 2), (300, 300), (322, 242), (1920, 1080)]] + \
        [(fmt, (646, 481)) for fmt in ("yuyv422", "uyvy422")] + [(fmt, (643, 481)) for fmt in ("gray", "bgr24")]


@pytest.mark.parametrize("kernel", ["pixel", "rows"])
@pytest.mark.parametrize("fmt,size", SIZES, ids=["%s-%dx%d" % (f, s[0], s[1]) for f, s in SIZES])
def test_resize_kernels_see_the_restated_rgb(engines, kernel, fmt, size):
    _same_network_input(engines[kernel], size[0], size[1], FMT[fmt])


@pytest.mark.parametrize("kernel", ["pixel", "rows"])
@pytest.mark.parametrize("colour", list(COLOURS))
@pytest.mark.parametrize("fmt", YUV)
@pytest.mark.parametrize("size", [(4, 2), (322, 242)], ids=["4x2", "322x242"])
def test_every_matrix_and_range_on_every_yuv_format(engines, kernel, colour, fmt, size):
    _same_network_input(engines[kernel], size[0], size[1], FMT[fmt] | COLOURS[colour])


def test_the_flags_change_the_network_input(engines):
    """... so the cases above are not four spellings of one conversion."""
    frame, _ = _case(322, 242, FMT_YUYV422)
    outs = [engines["pixel"].stage_preprocess(frame, FMT_YUYV422 | c).view(np.uint16) for c in COLOURS.values()]
    for i in range(4):
        for j in range(i):
            assert (outs[i] != outs[j]).any()


MIXED = [(FMT_RGB24, 640, 480), (FMT_NV12 | CSP_BT709, 1280, 720), (FMT_YUYV422 | RANGE_FULL, 640, 480), (FMT_UYVY422, 646, 481),
         (FMT_GRAY8, 643, 481), (FMT_BGR24, 1920, 1080)]


def test_rows_of_a_mixed_batch(engines):
    """RGB24, NV12 | 709, YUYV | full, UYVY, gray and BGR24 frames of different sizes in ONE batch == each of them as the RGB24 frame
    the restatement converts it to; synchronously and through the asynchronous host path."""
    eng = engines["pixel"]
    frames, as_rgb = zip(*[_case(w, h, word) for word, w, h in MIXED])
    formats = [word for word, _, _ in MIXED]
    ref = [np.zeros(100, ROW_DTYPE) for _ in frames]
    eng.detect_batch(list(as_rgb), ref)
    got = [np.zeros(100, ROW_DTYPE) for _ in frames]
    eng.detect_batch(list(frames), got, formats=formats)
    for a, b in zip(got, ref):
        assert a.tobytes() == b.tobytes()
    assert any((r["confidence"] > 0.3).any() for r in got)
    eng.submit_host(0, list(frames), formats=formats)
    again = [np.zeros(100, ROW_DTYPE) for _ in frames]
    eng.collect(0, again)
    for a, b in zip(again, ref):
        assert a.tobytes() == b.tobytes()


def test_frames_at_odd_device_addresses(engines):
    """The per-pixel kernel's wide loads need a frame address that is a multiple of 4; one byte off it reads byte-wise, same rows."""
    eng = engines["pixel"]
    specs = [(FMT_YUYV422, 322, 242), (FMT_UYVY422 | CSP_BT709, 646, 481), (FMT_BGR24, 643, 481), (FMT_GRAY8, 643, 481)]
    frames, as_rgb = zip(*[_case(w, h, word) for word, w, h in specs])
    ref = [np.zeros(100, ROW_DTYPE) for _ in frames]
    eng.detect_batch(list(as_rgb), ref)
    ptrs = [eng.upload(np.concatenate([np.zeros(1 + 2 * i, np.uint8), f.reshape(-1)])) for i, f in enumerate(frames)]
    try:
        eng.submit_device(0, [p + 1 + 2 * i for i, p in enumerate(ptrs)], [s[1] for s in specs], [s[2] for s in specs],
                          formats=[s[0] for s in specs])
        got = [np.zeros(100, ROW_DTYPE) for _ in frames]
        eng.collect(0, got)
    finally:
        eng.sync()
        for p in ptrs:
            eng.free(p)
    for a, b in zip(got, ref):
        assert a.tobytes() == b.tobytes()
    assert any((r["confidence"] > 0).any() for r in got)


def test_frames_read_in_place_give_the_same_rows_as_staged_frames(model_dir):
    """1920x1080 YUYV, gray and BGR24 frames at odd offsets of one page-locked arena, read in place over PCIe by the row-staged
    kernel (WZ_HOST_READ=1): rows == a staged engine's rows for the converted RGB24 frames, bit for bit."""
    specs = [(FMT_YUYV422, 1920, 1080), (FMT_GRAY8, 1920, 1080), (FMT_BGR24, 1920, 1080)]
    cases = [_case(w, h, word) for word, w, h in specs]
    fmts = [s[0] for s in specs]
    staged = engine_with(model_dir, {"WZ_PRE_ROWS": "0", "WZ_HOST_READ": "0"}, max_batch=4)
    try:
        want = [np.zeros(100, ROW_DTYPE) for _ in cases]
        staged.detect_batch([rgb for _, rgb in cases], want)
    finally:
        staged.close()
    arena = np.zeros(sum(f.size for f, _ in cases) + 64 * len(cases) + 7, np.uint8)
    frames, off = [], 5
    for i, (f, _) in enumerate(cases):
        view = arena[off:off + f.size].reshape(f.shape)
        view[...] = f
        frames.append(view)
        off += f.size + 13 + 2 * i
    direct = engine_with(model_dir, {"WZ_HOST_READ": "1"}, max_batch=4)
    try:
        direct.host_register(arena)
        try:
            direct.submit_host(1, frames, formats=fmts)
            direct.wait(1)
            got = direct.slot_rows(1, len(frames)).copy()
        finally:
            direct.sync()
            direct.host_unregister(arena)
    finally:
        direct.close()
    for i in range(len(frames)):
        assert got[i].tobytes() == want[i].tobytes(), i
        assert got[i]["confidence"][0] > 0


def test_refusals(engines):
    """Odd width for 4:2:2, a colour flag on RGB24 / gray / BGR24, an unknown flag bit, base format 9: ValueError from Python's
    geometry check, and again from the C ABI (submit_device hands the word over unchecked)."""
    eng = engines["pixel"]
    rows = [np.zeros(100, ROW_DTYPE)]
    z = lambda *s: np.zeros(s, np.uint8)
    py = [(z(480, 641, 2), FMT_YUYV422), (z(480, 1282), FMT_UYVY422), (z(480, 640, 3), FMT_RGB24 | CSP_BT709),
          (z(480, 640), FMT_GRAY8 | RANGE_FULL), (z(480, 640, 3), FMT_BGR24 | CSP_BT709 | RANGE_FULL), (z(720, 640), FMT_NV12 | 0x400),
          (z(480, 640, 2), FMT_YUYV422 | 0x1000), (z(480, 640, 3), 9)]
    for frame, word in py:
        with pytest.raises(ValueError):
            eng.detect_batch([frame], rows, formats=[word])
        with pytest.raises(ValueError):
            eng.submit_host(0, [frame], formats=[word])
    d = eng.upload(z(480, 641, 3))
    try:
        abi = [(641, 480, FMT_YUYV422), (641, 480, FMT_UYVY422 | CSP_BT709), (640, 480, FMT_RGB24 | CSP_BT709), (640, 480, FMT_RGB24 | RANGE_FULL),
               (640, 480, FMT_GRAY8 | RANGE_FULL), (640, 480, FMT_BGR24 | CSP_BT709), (640, 480, FMT_NV12 | 0x400), (640, 480, FMT_YUYV422 | 0x1000),
               (640, 480, 9), (640, 480, 7)]
        for w, h, word in abi:
            with pytest.raises(ValueError):
                eng.submit_device(0, [d], [w], [h], formats=[word])
        eng.submit_device(0, [d], [640], [480], formats=[FMT_YUYV422 | CSP_BT709 | RANGE_FULL])      # (and a good word is taken)
        eng.wait(0)
    finally:
        eng.sync()
        eng.free(d)
