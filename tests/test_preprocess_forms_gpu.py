"""The square stretch Resize((S, S)) and BICUBIC on the device: mirx_resample_batch against default_transform's Pillow
path, bit for bit, in both output forms with guard slots around the output; the cubic's negative coefficients and clipped sums;
unequal x / y scales; the tap cap; MilvusRetriever and nih.encode_npy_paths end to end."""
import numpy as np
import pytest
import torch
from PIL import Image

from mirx import _lib as L
from mirx import preprocess as P
from mirx.retriever import IMAGENET_MEAN, IMAGENET_STD, default_transform

pytestmark = pytest.mark.gpu

# (w, h, mode): the bicubic batch
_SOURCES = [(3, 2, "RGB"), (300, 280, "RGB"), (280, 300, "RGB"), (257, 511, "RGB"), (1024, 1024, "L"), (2048, 1500, "RGB")]
_images = {}


def _image(w, h, mode, content=0):
    """A source per (size, mode, content), made once: content is a seed (noise) or "checker", the 3-pixel 0 / 255
    checkerboard."""
    key = (w, h, mode, content)
    if key not in _images:
        if content == "checker":
            y, x = np.mgrid[0:h, 0:w]
            a = (((x // 3 + y // 3) % 2) * 255).astype(np.uint8)
            a = np.repeat(a[:, :, None], 3, axis=2) if mode == "RGB" else a
        else:
            a = np.random.default_rng([w, h, len(mode), content]).integers(0, 256, (h, w, 3) if mode == "RGB" else (h, w),
                                                                         dtype=np.uint8)
        _images[key] = Image.fromarray(np.ascontiguousarray(a))
    return _images[key]


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _check_launch(images, resize, size, interpolation, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """The harness of tests/test_preprocess_gpu.py: one launch per output form into a buffer with an image-sized guard slot on
    either side, all 0xA5 bytes beforehand; the slots must come back untouched and EVERY image must equal the host path
    bitwise.  Returns the host path's pixels."""
    tf = default_transform(size, mean, std, resize=resize, interpolation=interpolation)
    items = [(im, P.plan(im.size[0], im.size[1], resize, size, interpolation)) for im in images]
    assert all(p is not None for _, p in items)
    b = len(images)
    want_px = torch.from_numpy(np.stack([tf.pixels(im) for im in images]))
    want_f = torch.stack([tf(im) for im in images])
    for dtype, want in ((torch.uint8, want_px), (torch.float32, want_f)):
        slot = 3 * size * size * want.element_size()
        raw = torch.full(((b + 2) * slot,), 0xA5, dtype=torch.uint8, device="cuda")
        out = raw[slot:(b + 1) * slot].view(dtype).view(b, 3, size, size)
        P.resample_into(items, size, out, tf.mean, tf.std)
        torch.cuda.synchronize()
        got = out.cpu()
        bad = [i for i in range(b) if not torch.equal(_bits(got[i]), _bits(want[i]))]
        assert not bad, (dtype, [(images[i].size, images[i].mode, int((_bits(got[i]) != _bits(want[i])).sum())) for i in bad])
        assert bool((raw[:slot] == 0xA5).all()) and bool((raw[(b + 1) * slot:] == 0xA5).all()), dtype
    return want_px


def _lds_request(img, tables):
    """The dynamic LDS a launch of this image asks for (the library's rule: x coefficients + the source rows the tallest tile
    row taps, 32 columns of 8 bits per channel)."""
    _, yb, _ = P.table_parts(tables[1])
    span = max(int(yb[y0:y0 + L.RESAMPLE_TILE_H].sum(axis=1).max() - yb[y0:y0 + L.RESAMPLE_TILE_H, 0].min())
               for y0 in range(0, len(yb), L.RESAMPLE_TILE_H))
    return int(tables[0][0]) * L.RESAMPLE_TILE_W * 4 + span * (3 if img.mode == "RGB" else 1) * L.RESAMPLE_TILE_W


def test_bicubic_mixed_batch_in_one_launch():
    _check_launch([_image(*s) for s in _SOURCES], 256, 224, "bicubic")


def test_bicubic_partial_tiles_and_single_stores():
    # 518 = 16 x 32 + 6 columns and 32 x 16 + 6 rows, and 518 % 4 != 0
    _check_launch([_image(300, 280, "RGB"), _image(1024, 1024, "L"), _image(257, 511, "RGB")], 518, 518, "bicubic")


def _unclipped_range(img, tables):
    """(min, max) of the unclipped values (2^21 + sum) >> 22 of the horizontal pass over the whole source and of the vertical
    pass over its 8-bit result, from the plan alone."""
    a = np.asarray(img, dtype=np.uint8)
    a = a[:, :, :1] if a.ndim == 3 else a[:, :, None]                      # the checkerboard's channels are equal
    rng = []
    for table in tables:
        _, bounds, coef = P.table_parts(table)
        acc = np.full((a.shape[0], bounds.shape[0], 1), 1 << 21, dtype=np.int64)
        for t in range(int(bounds[:, 1].max())):
            acc += a[:, np.minimum(bounds[:, 0] + t, a.shape[1] - 1), :].astype(np.int64) * coef[None, :, t, None]
        assert np.abs(acc).max() < 2 ** 31
        v = acc >> 22
        rng.append((int(v.min()), int(v.max())))
        a = np.clip(v, 0, 255).astype(np.uint8).transpose(1, 0, 2)
    return rng


@pytest.mark.parametrize("resize,size,sources", [(256, 224, _SOURCES), (518, 518, [_SOURCES[1], _SOURCES[4], _SOURCES[3]])])
def test_bicubic_checkerboard_clips_at_both_ends(resize, size, sources):
    """The path this test names: negative partial sums, sums past 255, the arithmetic shift in front of the clip.  Its
    precondition is asserted from the plan before the comparison."""
    images = [_image(w, h, mode, "checker") for w, h, mode in sources]
    ranges = [_unclipped_range(im, P.plan(im.size[0], im.size[1], resize, size, "bicubic")) for im in images]
    print("unclipped (min, max) per image, horizontal then vertical:", ranges)
    for axis in (0, 1):
        assert min(r[axis][0] for r in ranges) < 0 and max(r[axis][1] for r in ranges) > 255, (axis, ranges)
    want = _check_launch(images, resize, size, "bicubic")
    assert bool((want == 0).any()) and bool((want == 255).any())


@pytest.mark.parametrize("interpolation", ["bilinear", "bicubic"])
def test_stretch_with_unequal_scales(interpolation):
    # x upscaled and y downscaled in one image, and the other way round
    _check_launch([_image(100, 400, "RGB"), _image(400, 100, "RGB"), _image(100, 400, "L", "checker")], (224, 224), 224, interpolation)
    _check_launch([_image(300, 280, "RGB")], (384, 384), 384, interpolation)
    _check_launch([_image(2048, 1500, "L")], (448, 448), 448, interpolation)


@pytest.mark.parametrize("interpolation", ["bilinear", "bicubic"])
def test_stretch_batch_of_65_from_two_sizes_and_modes(interpolation):
    images = [_image(300, 280, "RGB", i) if i % 2 else _image(100, 400, "L", i) for i in range(65)]
    _check_launch(images, (224, 224), 224, interpolation)


def test_bicubic_near_the_tap_cap_and_over_it():
    """3584 x 3600 at resize 256: a scale of 14, 57 taps.  The selection rule sizes a source for three channels (one answer per
    size, whatever the mode): that figure is the one asserted under the cap and above 32 KB, and the RGB source of that size
    makes the launch request it; the L source the issue names asks for a third of the rows."""
    grey, rgb = _image(3584, 3600, "L"), _image(3584, 3600, "RGB")
    tables = P.plan(3584, 3600, 256, 224, "bicubic")
    assert int(tables[0][0]) == 57
    need_l, need_rgb = _lds_request(grey, tables), _lds_request(rgb, tables)
    print("LDS bytes requested: L", need_l, "RGB", need_rgb)
    assert 32 * 1024 < need_rgb <= L.RESAMPLE_MAX_LDS and need_l < need_rgb
    _check_launch([grey, rgb], 256, 224, "bicubic")
    # 4300 x 4200: the shorter side at a scale of 16.4 has 67 taps, over the cap, and goes to the host
    tf = default_transform(224, resize=256, interpolation="bicubic")
    wide = _image(4300, 4200, "L")
    assert P.plan(4300, 4200, 256, 224, "bicubic") is None
    px = tf.batch_pixels([grey, wide], "cuda")
    assert tf.last_preprocess == {"device": 1, "host": 1}
    assert np.array_equal(px.cpu().numpy(), np.stack([tf.pixels(grey), tf.pixels(wide)]))


_retriever = {}


def _densenet():
    """A seeded DenseNet121 over a 64-row collection, made once."""
    if not _retriever:
        from mirx.model import DenseNet121
        from mirx.retriever import MilvusManager
        torch.manual_seed(0)
        m = DenseNet121().eval().cuda()
        mgr = MilvusManager(dataset="covid")
        mgr.connect()
        mgr.create_collection("densenet121", drop_old=True)
        g = torch.nn.functional.normalize(torch.randn(64, 1024, generator=torch.Generator().manual_seed(5)), dim=1)
        mgr.collections["densenet121"].insert([[f"/d/{i}.png" for i in range(64)], ["normal"] * 64, g])
        _retriever.update(m=m, mgr=mgr)
    return _retriever["m"], _retriever["mgr"]


@pytest.mark.parametrize("form", ["stretch", "medsiglip_val"])
def test_retriever_end_to_end_on_densenet121(form):
    from mirx.retriever import MilvusRetriever
    from mirx.xai import get_transforms_medsiglip
    m, mgr = _densenet()
    # stretch: ImageNet constants, which the model applies itself to 8-bit input (tf.batch_pixels); the bicubic val transform
    # is ToTensor alone, so the floats are made by the kernel (tf.batch)
    tf = default_transform(224, resize=(224, 224)) if form == "stretch" else get_transforms_medsiglip(224)[1]
    r = MilvusRetriever(mgr, "densenet121", m, tf)
    plain = MilvusRetriever(mgr, "densenet121", m, lambda im: tf(im))
    sources = [_image(300, 280, "RGB"), _image(1024, 1024, "L"), _image(100, 400, "RGB"), _image(257, 511, "RGB", "checker")]
    for img in sources[:2]:
        res, qemb = r.search(img, top_k=5)
        assert r.last_preprocess == {"device": 1, "host": 0}
        q = r._query_tensor(img)
        assert q.is_cuda and q.dtype == (torch.uint8 if form == "stretch" else torch.float32)
        assert torch.equal(qemb, r.embed(tf(img)[None])), (img.size, img.mode)
        assert res == plain.search(img, top_k=5)[0]
    batch = r.batch_search(sources, top_k=5)
    assert r.last_preprocess == {"device": 4, "host": 0}
    assert plain.last_preprocess is None
    assert batch == plain.batch_search(sources, top_k=5)


def test_encode_npy_paths_hands_the_model_the_stretched_host_transform(tmp_path):
    from mirx import nih
    rng = np.random.default_rng(11)
    paths = []
    for i, label in enumerate(("Mass", "Nodule")):
        p = tmp_path / f"0000{i}_Chest_X-ray_{label}_{i}.npy"
        np.save(p, rng.integers(0, 256, (64, 80), dtype=np.uint8))
        paths.append(str(p))
    tf = default_transform(384, resize=(384, 384))
    seen = []

    class _Stub(torch.nn.Module):
        def forward(self, x):
            seen.append(x)
            return {"embedding": x.flatten(1)[:, :nih.EMBEDDING_DIM].contiguous()}

    nih.encode_npy_paths(_Stub(), tf, paths, torch.device("cuda"), batch_size=2)
    assert tf.last_preprocess == {"device": 2, "host": 0}
    want = torch.stack([tf(nih.load_npy_as_pil(p)) for p in paths])
    assert len(seen) == 1 and seen[0].is_cuda and seen[0].dtype == torch.float32
    assert torch.equal(seen[0].cpu().view(torch.int32), want.view(torch.int32))
