"""Device-side Resize / CenterCrop, the parts that need no GPU: the library's host plan (mirx_resample_plan) applied with a numpy
integer multiply-accumulate must equal default_transform's Pillow path byte for byte; mirx_resample_batch must refuse a bad
descriptor or table before any HIP call; on a CPU device the batch attributes are the host path."""
import ctypes

import numpy as np
import pytest
import torch
from PIL import Image

from mirx import _lib as L
from mirx import preprocess as P
from mirx.retriever import IMAGENET_MEAN, IMAGENET_STD, SIGLIP_MEAN, SIGLIP_STD, default_transform

_SIZES = [(1, 1), (3, 2), (100, 80), (255, 256), (257, 256), (341, 256), (343, 256), (300, 280), (257, 511), (7, 300), (640, 480),
          (1024, 1024), (2048, 1500)]
_SHAPES = [(256, 224), (432, 384), (512, 448), (518, 518)]


def _sources(resize):
    sizes = []
    for w, h in _SIZES + ([(4000, 3000)] if resize == 256 else []):
        sizes.append((w, h))
        if w != h:
            sizes.append((h, w))
    return sizes


def _image(w, h, mode, seed, fill=None):
    shape = (h, w, 3) if mode == "RGB" else (h, w)
    if fill is not None:
        return Image.fromarray(np.full(shape, fill, dtype=np.uint8))
    return Image.fromarray(np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8))


def _apply_plan(src, xt, yt):
    """The two integer passes of the kernel in numpy, on a [h, w] or [h, w, c] uint8 array -> [S, S(, c)] uint8: horizontal into
    8 bits, then vertical, out = clip((2^21 + sum pixel * coeff) >> 22, 0, 255) in 32-bit integers."""
    a = np.asarray(src, dtype=np.uint8)
    a = a[:, :, None] if a.ndim == 2 else a

    def one_pass(img, table):                                # resamples axis 1
        taps, bounds, coef = P.table_parts(table)
        out = np.empty((img.shape[0], bounds.shape[0], img.shape[2]), dtype=np.uint8)
        for i, (first, count) in enumerate(bounds):
            acc = np.full((img.shape[0], img.shape[2]), 1 << 21, dtype=np.int32)
            for t in range(count):
                acc += img[:, first + t, :].astype(np.int32) * coef[i, t]
            out[:, i, :] = np.clip(acc >> 22, 0, 255)
        return out

    mid = one_pass(a, xt)
    out = one_pass(mid.transpose(1, 0, 2), yt).transpose(1, 0, 2)
    return out[:, :, 0] if np.asarray(src).ndim == 2 else out


def _planned_pixels(img, resize, size):
    """[3, S, S] uint8 from the library's plan and integer arithmetic alone (no Pillow resize)."""
    w, h = img.size
    tables = P.plan(w, h, resize, size)
    assert tables is not None, (w, h, resize, size)
    got = _apply_plan(np.asarray(img), *tables)
    if img.mode == "L":
        return np.ascontiguousarray(np.broadcast_to(got, (3, size, size)))
    return np.ascontiguousarray(got.transpose(2, 0, 1))


@pytest.mark.parametrize("mode", ["RGB", "L"])
@pytest.mark.parametrize("resize,size", _SHAPES)
def test_plan_equals_pillow_byte_for_byte(resize, size, mode):
    tf = default_transform(size, resize=resize)
    for n, (w, h) in enumerate(_sources(resize)):
        img = _image(w, h, mode, 1000 * resize + n)
        want = tf.pixels(img)
        got = _planned_pixels(img, resize, size)
        assert got.shape == want.shape == (3, size, size)
        assert np.array_equal(got, want), (w, h, resize, size, mode, int((got != want).sum()))


@pytest.mark.parametrize("resize,size", _SHAPES)
def test_plan_on_constant_images(resize, size):
    tf = default_transform(size, resize=resize)
    for w, h in [(3, 2), (343, 256), (300, 280), (1024, 1024), (257, 511)]:
        for fill in (0, 255):
            for mode in ("RGB", "L"):
                img = _image(w, h, mode, 0, fill)
                got = _planned_pixels(img, resize, size)
                assert np.array_equal(got, tf.pixels(img)) and (got == fill).all(), (w, h, fill, mode)


def test_coefficient_runs_stay_inside_the_image_and_sum_to_one():
    for w, h, resize, size in [(1, 1, 256, 224), (2048, 1500, 256, 224), (7, 300, 518, 518), (4000, 3000, 256, 224)]:
        for table, side in zip(P.plan(w, h, resize, size), (w, h)):
            taps, bounds, coef = P.table_parts(table)
            assert taps <= L.RESAMPLE_MAX_TAPS and table[2] == side and len(table) % 4 == 0
            assert (bounds[:, 0] >= 0).all() and (bounds[:, 1] >= 1).all() and (bounds.sum(axis=1) <= side).all()
            assert (coef >= 0).all() and (np.abs(coef.sum(axis=1) - (1 << 22)) <= taps).all()
            assert all((coef[i, c:] == 0).all() for i, (_, c) in enumerate(bounds))


@pytest.mark.parametrize("mean,std", [(IMAGENET_MEAN, IMAGENET_STD), (SIGLIP_MEAN, SIGLIP_STD)])
def test_normalised_form_equals_the_transform_bitwise(mean, std):
    tf = default_transform(224, mean, std)
    m = np.asarray(mean, dtype=np.float32).reshape(3, 1, 1)
    s = np.asarray(std, dtype=np.float32).reshape(3, 1, 1)
    for n, (w, h, mode) in enumerate([(300, 280, "RGB"), (343, 256, "L"), (3, 2, "RGB"), (1024, 1024, "L")]):
        img = _image(w, h, mode, 77 + n)
        x = _planned_pixels(img, 256, 224).astype(np.float32) / np.float32(255.0)
        got = (x - m) / s
        want = tf(img).numpy()
        assert got.dtype == want.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def _blob(images, resize=256, size=224):
    items = [(im, P.plan(im.size[0], im.size[1], resize, size)) for im in images]
    tables, layout, nbytes = P.blob_layout(items)
    blob = np.zeros(nbytes, dtype=np.uint8)
    P.blob_fill(blob, items, tables, layout)
    return blob, layout


def _call(lib, blob, nbytes, b, size=224, kind=L.RESAMPLE_OUT_U8):
    # blob_dev and out are never dereferenced: every check below fails before the first HIP call
    fake = ctypes.c_void_p(1 << 20)
    return lib.mirx_resample_batch(blob.ctypes.data, fake, nbytes, b, size, kind, None, None, fake, None)


def test_bad_descriptors_and_tables_report_errors_without_gpu():
    lib = L.load()
    images = [_image(300, 280, "RGB", 1), _image(64, 100, "L", 2)]
    blob, layout = _blob(images)
    n = len(blob)

    # a descriptor that runs past the buffer: the buffer ends inside the last image; a height the buffer does not hold
    assert _call(lib, blob, n - 64, 2) == -1 and b"runs past the buffer" in lib.mirx_last_error()
    bad = blob.copy()
    bad[:128].view(np.int64)[8 + 3] = 64 * 200                                      # the second image's pitch
    assert _call(lib, bad, n, 2) == -1 and b"runs past the buffer" in lib.mirx_last_error()
    bad = blob.copy()
    bad[:128].view(np.int64)[0] = n + 16                                            # offset behind the end
    assert _call(lib, bad, n, 2) == -1 and b"runs past the buffer" in lib.mirx_last_error()
    assert _call(lib, blob, 100, 2) == -1 and b"smaller than its descriptors" in lib.mirx_last_error()

    # a tap range outside the image: the last x run of the first image moved one pixel right; a negative first tap
    xoff = layout[0][5]
    for row, first in ((223, None), (0, -1)):
        bad = blob.copy()
        bounds = bad[xoff + 16:xoff + 16 + 224 * 8].view(np.int32).reshape(224, 2)
        bounds[row, 0] = 300 - bounds[row, 1] + 1 if first is None else first
        assert _call(lib, bad, n, 2) == -1 and b"tap range lies outside the image" in lib.mirx_last_error()
    yoff = layout[1][6]
    bad = blob.copy()
    bad[yoff + 16:yoff + 16 + 224 * 8].view(np.int32).reshape(224, 2)[5, 1] = 0     # an empty run
    assert _call(lib, bad, n, 2) == -1 and b"tap range lies outside the image" in lib.mirx_last_error()
    bad = blob.copy()
    bad[yoff:yoff + 16].view(np.int32)[2] = 101                                     # planned for another height
    assert _call(lib, bad, n, 2) == -1 and b"another output or source size" in lib.mirx_last_error()
    bad = blob.copy()
    taps = int(bad[xoff:xoff + 4].view(np.int32)[0])
    bad[xoff + 16 + 224 * 8:xoff + 16 + 224 * 8 + 4 * taps].view(np.int32)[0] = -5
    assert _call(lib, bad, n, 2) == -1 and b"negative coefficient" in lib.mirx_last_error()
    bad = blob.copy()
    bad[xoff + 16 + 224 * 8:xoff + 16 + 224 * 8 + 4 * taps].view(np.int32)[0] = 1 << 24
    assert _call(lib, bad, n, 2) == -1 and b"more than 2^23" in lib.mirx_last_error()

    # a scale over the cap: in the plan, in a table's header, and in what the selection rule makes of such a source
    assert lib.mirx_resample_taps(4096, 64) == -1 and b"over the cap" in lib.mirx_last_error()
    assert lib.mirx_resample_taps(4096, 128) == L.RESAMPLE_MAX_TAPS
    table = np.zeros(4 + 2 * 8 + 8 * 200, dtype=np.int32)
    assert lib.mirx_resample_plan(4096, 64, 0, 8, table.ctypes.data, len(table)) == -1 and b"over the cap" in lib.mirx_last_error()
    assert lib.mirx_resample_plan(8193, 8193, 0, 8, table.ctypes.data, len(table)) == -1 and b"source side" in lib.mirx_last_error()
    assert lib.mirx_resample_plan(300, 256, 250, 8, table.ctypes.data, len(table)) == -1 and b"window" in lib.mirx_last_error()
    assert lib.mirx_resample_plan(300, 256, 0, 8, table.ctypes.data, 10) == -1 and b"table smaller" in lib.mirx_last_error()
    bad = blob.copy()
    bad[xoff:xoff + 4].view(np.int32)[0] = L.RESAMPLE_MAX_TAPS + 1
    assert _call(lib, bad, n, 2) == -1 and b"over the cap" in lib.mirx_last_error()
    assert P.plan(4096, 4096, 64, 64) is None and P.plan(8193, 300, 256, 224) is None and P.plan(300, 280, 200, 224) is None
    assert P.plan(4096, 4096, 256, 224) is not None and P.plan(8192, 8192, 256, 224) is not None

    # the plain argument checks
    assert _call(lib, blob, n, 0) == -1 and b"b must be" in lib.mirx_last_error()
    assert _call(lib, blob, n, 2, size=2000) == -1 and b"s must be" in lib.mirx_last_error()
    assert _call(lib, blob, n, 2, kind=7) == -1 and b"output kind" in lib.mirx_last_error()
    assert _call(lib, blob, n, 2, kind=L.RESAMPLE_OUT_F32) == -1 and b"mean and std" in lib.mirx_last_error()
    assert _call(lib, blob, n, 2, size=225) == -1 and b"another output or source size" in lib.mirx_last_error()
    bad = blob.copy()
    bad[:128].view(np.int64)[4] = 2
    assert _call(lib, bad, n, 2) == -1 and b"channels must be 1 or 3" in lib.mirx_last_error()


def test_cpu_device_takes_the_host_path():
    tf = default_transform(224)
    images = [_image(300, 280, "RGB", 5), _image(128, 200, "L", 6), _image(90, 70, "RGB", 7).convert("RGBA")]
    got = tf.batch(images, torch.device("cpu"))
    assert got.device.type == "cpu" and got.dtype == torch.float32
    assert torch.equal(got.view(torch.int32), torch.stack([tf(i) for i in images]).view(torch.int32))
    assert tf.last_preprocess == {"device": 0, "host": 3}
    px = tf.batch_pixels(images[:2], "cpu")
    assert px.dtype == torch.uint8 and np.array_equal(px.numpy(), np.stack([tf.pixels(i) for i in images[:2]]))
    assert tf.last_preprocess == {"device": 0, "host": 2}
    assert tf.batch_pixels([], "cpu").shape == (0, 3, 224, 224)
