"""The square stretch Resize((S, S)) and BICUBIC on the device path, the parts that need no GPU: the library's plan
(mirx_resample_plan_filter) applied with a numpy integer multiply-accumulate must equal Pillow byte for byte in every shape
default_transform builds; the bilinear tables must not have moved; mirx_resample_batch must refuse what the kernel's 32-bit
sums could not take, by the filter a table names, before any HIP call."""
import ctypes

import numpy as np
import pytest
import torch
from PIL import Image

from mirx import _lib as L
from mirx import preprocess as P
from mirx.retriever import IMAGENET_MEAN, IMAGENET_STD, SIGLIP_MEAN, SIGLIP_STD, default_transform

_SIZES = [(1, 1), (3, 2), (100, 80), (255, 256), (257, 256), (300, 280), (280, 300), (257, 511), (7, 300), (100, 400), (640, 480),
          (1024, 1024), (2048, 1500)]
_CROPS = [(256, 224), (432, 384), (480, 448), (518, 518)]                  # bicubic, shorter side + crop
_STRETCH = [224, 384, 448, 518]                                            # both filters
# (resize, S, interpolation) of every new shape
_FORMS = [(r, s, "bicubic") for r, s in _CROPS] + [((s, s), s, f) for s in _STRETCH for f in ("bilinear", "bicubic")]


def _image(w, h, mode, content):
    """content = a seed (noise) or "checker": the 3-pixel 0 / 255 checkerboard, which drives the cubic's sums past both ends."""
    if content == "checker":
        y, x = np.mgrid[0:h, 0:w]
        a = (((x // 3 + y // 3) % 2) * 255).astype(np.uint8)
        a = np.repeat(a[:, :, None], 3, axis=2) if mode == "RGB" else a
    else:
        a = np.random.default_rng([w, h, len(mode), content]).integers(0, 256, (h, w, 3) if mode == "RGB" else (h, w), dtype=np.uint8)
    return Image.fromarray(np.ascontiguousarray(a))


def _one_pass(img, table):
    """Resamples axis 1 of a [rows, in, c] uint8 array by an axis table: clip((2^21 + sum pixel * coeff) >> 22, 0, 255) in 32-bit
    integers, all outputs of a tap at once (coefficients are zero past a run's count, so a clamped index adds nothing)."""
    taps, bounds, coef = P.table_parts(table)
    acc = np.full((img.shape[0], bounds.shape[0], img.shape[2]), 1 << 21, dtype=np.int32)
    for t in range(int(bounds[:, 1].max())):
        idx = np.minimum(bounds[:, 0] + t, img.shape[1] - 1)
        acc += img[:, idx, :].astype(np.int32) * coef[None, :, t, None]
    return np.clip(acc >> 22, 0, 255).astype(np.uint8), acc


def _planned_pixels(img, resize, size, interpolation):
    """[3, S, S] uint8 from the library's plan and integer arithmetic alone (no Pillow resize): horizontal into 8 bits, then
    vertical."""
    tables = P.plan(img.size[0], img.size[1], resize, size, interpolation)
    assert tables is not None, (img.size, resize, size, interpolation)
    a = np.asarray(img, dtype=np.uint8)
    a = a[:, :, None] if a.ndim == 2 else a
    mid, _ = _one_pass(a, tables[0])
    out, _ = _one_pass(mid.transpose(1, 0, 2), tables[1])
    out = out.transpose(2, 1, 0)                                            # [c, S, S]
    return np.ascontiguousarray(np.broadcast_to(out, (3, size, size)))


def _pillow_pixels(img, resize, size, interpolation):
    """The reference composition written out with Pillow alone: convert, Resize(int) + CenterCrop or Resize((S, S))."""
    flt = {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC}[interpolation]
    img = img.convert("RGB")
    if isinstance(resize, tuple):
        img = img.resize(resize, flt)
    else:
        w, h = img.size
        nw, nh = (resize, int(resize * h / w)) if w <= h else (int(resize * w / h), resize)
        img = img.resize((nw, nh), flt)
        left, top = int(round((nw - size) / 2.0)), int(round((nh - size) / 2.0))
        img = img.crop((left, top, left + size, top + size))
    return np.ascontiguousarray(np.asarray(img).transpose(2, 0, 1))


@pytest.mark.parametrize("mode", ["RGB", "L"])
@pytest.mark.parametrize("resize,size,interpolation", _FORMS)
def test_plan_equals_pillow_byte_for_byte(resize, size, interpolation, mode):
    tf = default_transform(size, resize=resize, interpolation=interpolation)
    for w, h in _SIZES:
        for content in (7, "checker"):
            img = _image(w, h, mode, content)
            want = tf.pixels(img)
            assert np.array_equal(want, _pillow_pixels(img, resize, size, interpolation))
            got = _planned_pixels(img, resize, size, interpolation)
            assert got.shape == want.shape == (3, size, size)
            assert np.array_equal(got, want), (w, h, resize, size, interpolation, mode, content, int((got != want).sum()))


@pytest.mark.parametrize("mean,std", [(IMAGENET_MEAN, IMAGENET_STD), (SIGLIP_MEAN, SIGLIP_STD), ((0, 0, 0), (1, 1, 1))])
def test_normalised_form_equals_the_transform_bitwise(mean, std):
    m = np.asarray(mean, dtype=np.float32).reshape(3, 1, 1)
    s = np.asarray(std, dtype=np.float32).reshape(3, 1, 1)
    for (resize, size, interpolation), (w, h, mode) in zip([_FORMS[0], _FORMS[4], _FORMS[7]],
                                                           [(300, 280, "RGB"), (257, 511, "L"), (100, 400, "RGB")]):
        tf = default_transform(size, mean, std, resize=resize, interpolation=interpolation)
        img = _image(w, h, mode, "checker" if mode == "L" else 3)
        x = _planned_pixels(img, resize, size, interpolation).astype(np.float32) / np.float32(255.0)
        got = (x - m) / s
        want = tf(img).numpy()
        assert got.dtype == want.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
        if tuple(mean) == (0, 0, 0):                                        # ToTensor alone
            assert np.array_equal(want.view(np.uint32), x.view(np.uint32))


def test_bilinear_tables_did_not_move():
    """mirx_resample_plan_filter(BILINEAR) and the earlier entry point fill identical tables, header word 3 = 0."""
    lib = L.load()
    for in_size, out_size, first, n in [(300, 256, 16, 224), (1, 256, 16, 224), (2048, 349, 62, 224), (7, 518, 0, 518),
                                        (4096, 128, 0, 128), (100, 224, 0, 224), (400, 224, 0, 224), (224, 224, 0, 224)]:
        taps = lib.mirx_resample_taps(in_size, out_size)
        assert taps == lib.mirx_resample_taps_filter(in_size, out_size, L.RESAMPLE_BILINEAR) > 0
        words = 4 + 2 * n + n * taps
        a, b = np.full(words, -7, dtype=np.int32), np.full(words, -9, dtype=np.int32)
        assert lib.mirx_resample_plan(in_size, out_size, first, n, a.ctypes.data, words) == 0
        assert lib.mirx_resample_plan_filter(in_size, out_size, first, n, L.RESAMPLE_BILINEAR, b.ctypes.data, words) == 0
        assert a.tobytes() == b.tobytes() and a[3] == 0 and (a[4 + 2 * n:] >= 0).all()
    assert P.plan(300, 280, 256, 224) is P.plan(300, 280, 256, 224, "bilinear") is P.plan(300, 280, 256, 224, Image.BILINEAR)
    assert P.plan(300, 280, 256, 224, "bicubic") is not P.plan(300, 280, 256, 224)
    assert P.plan(300, 280, (224, 224), 224) is not P.plan(300, 280, 256, 224)


def test_bicubic_runs_stay_inside_the_32_bit_sums():
    """sum |coeff| <= 2^23 for every run of every planned bicubic table, so 255 * 2^23 + 2^21 < 2^31 bounds every partial sum;
    the tables carry the filter in header word 3, have negative coefficients and sum to one."""
    worst = 0
    for resize, size, interpolation in _FORMS:
        if interpolation != "bicubic":
            continue
        for w, h in _SIZES + ([(3584, 3600), (4096, 4096)] if resize == 256 else []):    # scales 14 and 16, the cap
            for table, side in zip(P.plan(w, h, resize, size, "bicubic"), (w, h)):
                taps, bounds, coef = P.table_parts(table)
                assert table[3] == L.RESAMPLE_BICUBIC and table[2] == side and taps <= L.RESAMPLE_MAX_TAPS and len(table) % 4 == 0
                assert (bounds[:, 0] >= 0).all() and (bounds[:, 1] >= 1).all() and (bounds.sum(axis=1) <= side).all()
                assert (np.abs(coef.sum(axis=1) - (1 << 22)) <= taps).all()
                assert all((coef[i, c:] == 0).all() for i, (_, c) in enumerate(bounds))
                worst = max(worst, int(np.abs(coef.astype(np.int64)).sum(axis=1).max()))
    print(f"largest sum |coeff| of a planned bicubic run: {worst} = {worst / (1 << 22):.4f} x 2^22")
    assert (1 << 22) < worst <= (1 << 23)
    assert (P.table_parts(P.plan(300, 280, 256, 224, "bicubic")[0])[2] < 0).any()


def _blob(images, resize, size, interpolation):
    items = [(im, P.plan(im.size[0], im.size[1], resize, size, interpolation)) for im in images]
    tables, layout, nbytes = P.blob_layout(items)
    blob = np.zeros(nbytes, dtype=np.uint8)
    P.blob_fill(blob, items, tables, layout)
    return blob, layout


def _call(lib, blob, b, size=224):
    # blob_dev and out are never dereferenced: every check below fails before the first HIP call
    fake = ctypes.c_void_p(1 << 20)
    return lib.mirx_resample_batch(blob.ctypes.data, fake, len(blob), b, size, L.RESAMPLE_OUT_U8, None, None, fake, None)


def _coef(blob, off, size=224):
    taps = int(blob[off:off + 4].view(np.int32)[0])
    return blob[off + 16 + size * 8:off + 16 + size * 8 + 4 * taps * size].view(np.int32).reshape(size, taps)


def test_refusals_by_filter_without_gpu():
    lib = L.load()
    images = [_image(300, 280, "RGB", 1), _image(64, 100, "L", 2)]
    cubic, layout = _blob(images, 256, 224, "bicubic")
    xoff, yoff = layout[0][5], layout[0][6]
    assert xoff != yoff and cubic[xoff + 12:xoff + 16].view(np.int32)[0] == cubic[yoff + 12:yoff + 16].view(np.int32)[0] == 1

    # a bicubic run whose magnitudes sum to more than 2^23: a pair of large coefficients that cancel, so the plain sum is small
    bad = cubic.copy()
    k = _coef(bad, xoff)
    k[5, 0] += 1 << 22
    k[5, 1] -= 1 << 22
    assert abs(int(k[5].sum()) - (1 << 22)) <= 8 and int(np.abs(k[5].astype(np.int64)).sum()) > (1 << 23)
    assert _call(lib, bad, 2) == -1 and b"bicubic coefficient run's magnitudes sum to more than 2^23" in lib.mirx_last_error()

    # the same (genuine, signed) tables under header word 3 = 0: the bilinear rule, today's message
    assert (_coef(cubic, xoff) < 0).any()
    bad = cubic.copy()
    for img_layout in layout:
        for off in img_layout[5:7]:
            bad[off + 12:off + 16].view(np.int32)[0] = 0
    assert _call(lib, bad, 2) == -1 and lib.mirx_last_error().endswith(b"resample: negative coefficient")

    # header word 3 = 2
    bad = cubic.copy()
    bad[xoff + 12:xoff + 16].view(np.int32)[0] = 2
    assert _call(lib, bad, 2) == -1 and b"unknown filter in a table's header" in lib.mirx_last_error()

    # x and y tables of one image with different filters (bilinear tables, x relabelled: its coefficients pass either rule)
    linear, layout = _blob(images, 256, 224, "bilinear")
    bad = linear.copy()
    bad[layout[0][5] + 12:layout[0][5] + 16].view(np.int32)[0] = 1
    assert _call(lib, bad, 2) == -1 and b"x and y tables of an image name different filters" in lib.mirx_last_error()

    # a negative coefficient in a bilinear table is still refused, an oversized one by the unchanged message
    bad = linear.copy()
    _coef(bad, layout[0][5])[0, 0] = -5
    assert _call(lib, bad, 2) == -1 and b"negative coefficient" in lib.mirx_last_error()
    bad = linear.copy()
    _coef(bad, layout[0][5])[0, 0] = 1 << 24
    assert _call(lib, bad, 2) == -1 and b"a coefficient run sums to more than 2^23" in lib.mirx_last_error()

    # an unknown filter in the plan
    table = np.zeros(4 + 2 * 8 + 8 * 70, dtype=np.int32)
    assert lib.mirx_resample_taps_filter(300, 256, 2) == -1 and b"unknown filter" in lib.mirx_last_error()
    assert lib.mirx_resample_plan_filter(300, 256, 0, 8, -1, table.ctypes.data, len(table)) == -1 and b"unknown filter" in lib.mirx_last_error()


def test_bicubic_stops_at_a_scale_of_16():
    lib = L.load()
    assert lib.mirx_resample_taps_filter(4096, 256, L.RESAMPLE_BICUBIC) == L.RESAMPLE_MAX_TAPS == 65
    assert lib.mirx_resample_taps_filter(3584, 256, L.RESAMPLE_BICUBIC) == 57
    assert lib.mirx_resample_taps_filter(4224, 256, L.RESAMPLE_BICUBIC) == -1             # scale 16.5: 67 taps
    assert b"over the cap" in lib.mirx_last_error() and b"bicubic scale > 16" in lib.mirx_last_error()
    assert lib.mirx_resample_taps_filter(4224, 256, L.RESAMPLE_BILINEAR) == 35
    table = np.zeros(4 + 2 * 8 + 8 * 70, dtype=np.int32)
    assert lib.mirx_resample_plan_filter(4224, 256, 0, 8, L.RESAMPLE_BICUBIC, table.ctypes.data, len(table)) == -1
    assert b"over the cap" in lib.mirx_last_error()
    assert P.axis_table(4224, 256, 16, 224, "bicubic") is None
    assert P.plan(4224, 4300, 256, 224, "bicubic") is None and P.plan(4224, 4300, 256, 224) is not None
    assert P.plan(4096, 4096, 256, 224, "bicubic") is not None                              # scale 16 exactly: 65 taps
    assert P.plan(4224, 300, (224, 224), 224, "bicubic") is None                            # the stretch: one axis over the cap
    assert P.plan(3500, 300, (224, 224), 224, "bicubic") is not None
    tf = default_transform(224, resize=256, interpolation="bicubic")
    img = Image.fromarray(np.random.default_rng(4).integers(0, 256, (4300, 4224), dtype=np.uint8))
    px = tf.batch_pixels([img], "cpu")
    assert tf.last_preprocess == {"device": 0, "host": 1} and np.array_equal(px[0].numpy(), tf.pixels(img))


def test_get_transforms_medsiglip_is_the_pillow_composition():
    from mirx.xai import get_transforms_medsiglip
    for size in (224, 448):
        train, tf = get_transforms_medsiglip(size)
        assert train is None and tf.mean == (0.0, 0.0, 0.0) and tf.std == (1.0, 1.0, 1.0)
        for w, h, mode in [(300, 280, "RGB"), (257, 511, "L"), (1024, 1024, "L")]:
            img = _image(w, h, mode, 11)
            px = _pillow_pixels(img, size + 32, size, "bicubic")
            want = torch.from_numpy(px.astype(np.float32) / np.float32(255.0))              # ToTensor
            got = tf(img)
            assert got.dtype == torch.float32 and torch.equal(got.view(torch.int32), want.view(torch.int32))
            assert np.array_equal(tf.pixels(img), px)
    _, tf = get_transforms_medsiglip()
    assert tf(_image(300, 280, "RGB", 1)).shape == (3, 224, 224) and hasattr(tf, "batch")


def test_the_arguments_of_default_transform():
    img = _image(300, 280, "RGB", 2)
    with pytest.raises(ValueError):
        default_transform(224, resize=(224, 256))
    with pytest.raises(ValueError):
        default_transform(224, resize=(256, 256))
    with pytest.raises(ValueError):
        default_transform(224, interpolation="lanczos")
    with pytest.raises(ValueError):
        default_transform(224, interpolation=Image.NEAREST)
    with pytest.raises(ValueError):
        P.plan(300, 280, (224, 256), 224)
    # the defaults are today's transform; PIL's constants name the same filters
    for a, b in [(default_transform(224), default_transform(224, resize=256, interpolation=Image.BILINEAR)),
                 (default_transform(384, resize=(384, 384), interpolation="bicubic"),
                  default_transform(384, resize=[384, 384], interpolation=Image.BICUBIC))]:
        assert torch.equal(a(img).view(torch.int32), b(img).view(torch.int32))
    assert np.array_equal(default_transform(224).pixels(img), _pillow_pixels(img, 256, 224, "bilinear"))
    # a CPU device takes the host path in the new shapes as well
    tf = default_transform(224, resize=(224, 224), interpolation="bicubic")
    images = [img, _image(128, 200, "L", 6)]
    got = tf.batch(images, torch.device("cpu"))
    assert torch.equal(got.view(torch.int32), torch.stack([tf(i) for i in images]).view(torch.int32))
    assert tf.last_preprocess == {"device": 0, "host": 2}
