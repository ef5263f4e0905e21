"""Device-side Resize / CenterCrop on the GPU: mirx_resample_batch against default_transform's Pillow path, bit for bit, in both
output forms; guard slots around the output; the selection rule on mixed modes; MilvusRetriever and nih.encode_npy_paths end to
end."""
import numpy as np
import pytest
import torch
from PIL import Image

from mirx import preprocess as P
from mirx.retriever import IMAGENET_MEAN, IMAGENET_STD, SIGLIP_MEAN, SIGLIP_STD, default_transform

pytestmark = pytest.mark.gpu

# (w, h, mode): the mixed batch of the issue
_MIXED = [(3, 2, "RGB"), (300, 280, "RGB"), (280, 300, "RGB"), (343, 256, "RGB"), (256, 341, "RGB"), (257, 511, "RGB"),
          (1024, 1024, "L"), (2048, 1500, "RGB")]
_images = {}


def _image(w, h, mode, seed=0):
    """A source with its own content per (size, mode, seed), made once."""
    key = (w, h, mode, seed)
    if key not in _images:
        shape = (h, w, 3) if mode == "RGB" else (h, w)
        rng = np.random.default_rng([w, h, len(mode), seed])
        _images[key] = Image.fromarray(rng.integers(0, 256, shape, dtype=np.uint8))
    return _images[key]


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _check_launch(images, resize, size, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """One launch per output form into a buffer with an image-sized guard slot on either side, all 0xA5 bytes beforehand: the
    slots must come back untouched and EVERY image must equal the host path bitwise.  The sources lie back to back in the
    launch's buffer, each with its own content, so a read past an image's edge gives a wrong pixel rather than a fault."""
    tf = default_transform(size, mean, std, resize=resize)
    items = [(im, P.plan(im.size[0], im.size[1], resize, size)) for im in images]
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


def test_mixed_batch_of_sizes_in_one_launch():
    _check_launch([_image(*s) for s in _MIXED], 256, 224)


@pytest.mark.parametrize("resize,size", [(432, 384), (518, 518)])
def test_tile_edges_that_do_not_divide_the_crop(resize, size):
    # 384 = 12 x 32 columns but 24 x 16 rows exactly; 518 = 16 x 32 + 6 columns and 32 x 16 + 6 rows, and 518 % 4 != 0
    _check_launch([_image(343, 256, "RGB"), _image(1024, 1024, "L"), _image(257, 511, "RGB")], resize, size)


def test_siglip_constants():
    _check_launch([_image(300, 280, "RGB"), _image(256, 341, "RGB"), _image(1024, 1024, "L")], 256, 224, SIGLIP_MEAN, SIGLIP_STD)


def test_batch_of_one():
    _check_launch([_image(300, 280, "RGB")], 256, 224)


def test_batch_of_65_from_two_source_sizes():
    images = [_image(300, 280, "RGB", seed=i) if i % 2 else _image(280, 300, "L", seed=i) for i in range(65)]
    _check_launch(images, 256, 224)


def test_mixed_modes_go_to_the_host_and_are_counted():
    tf = default_transform(224)
    rgb, grey = _image(300, 280, "RGB"), _image(1024, 1024, "L")
    rgba = _image(343, 256, "RGB", seed=9).convert("RGBA")
    pal = _image(256, 341, "RGB", seed=9).convert("P")
    images = [rgb, rgba, grey, pal, _image(280, 300, "RGB")]
    px = tf.batch_pixels(images, "cuda")
    assert tf.last_preprocess == {"device": 3, "host": 2}
    assert px.is_cuda and px.dtype == torch.uint8
    assert np.array_equal(px.cpu().numpy(), np.stack([tf.pixels(i) for i in images]))
    fl = tf.batch(images, torch.device("cuda", 0))
    assert tf.last_preprocess == {"device": 3, "host": 2}
    assert torch.equal(fl.cpu().view(torch.int32), torch.stack([tf(i) for i in images]).view(torch.int32))
    assert torch.equal(tf.batch([rgba, pal], "cuda").cpu().view(torch.int32), torch.stack([tf(rgba), tf(pal)]).view(torch.int32))
    assert tf.last_preprocess == {"device": 0, "host": 2}
    # a source over the caps (a side above 8192) takes the host path as well
    wide = Image.fromarray(np.random.default_rng(3).integers(0, 256, (40, 8200), dtype=np.uint8))
    assert np.array_equal(tf.batch_pixels([wide, rgb], "cuda").cpu().numpy(), np.stack([tf.pixels(wide), tf.pixels(rgb)]))
    assert tf.last_preprocess == {"device": 1, "host": 1}


_retriever = {}


def _densenet_retriever():
    """A seeded DenseNet121 over a 64-row collection, five sources and their five single searches, made once."""
    if not _retriever:
        from mirx.model import DenseNet121
        from mirx.retriever import MilvusManager, MilvusRetriever
        torch.manual_seed(0)
        m = DenseNet121().eval().cuda()
        mgr = MilvusManager(dataset="covid")
        mgr.connect()
        mgr.create_collection("densenet121", drop_old=True)
        g = torch.nn.functional.normalize(torch.randn(64, 1024, generator=torch.Generator().manual_seed(5)), dim=1)
        mgr.collections["densenet121"].insert([[f"/d/{i}.png" for i in range(64)], ["normal"] * 64, g])
        tf = default_transform(224)
        r = MilvusRetriever(mgr, "densenet121", m, tf)
        sources = [_image(300, 280, "RGB"), _image(1024, 1024, "L"), _image(280, 300, "RGB"), _image(343, 256, "RGB"),
                   _image(257, 511, "RGB")]
        _retriever.update(r=r, tf=tf, sources=sources, singles=[r.search(img, top_k=5) for img in sources],
                          plain=MilvusRetriever(mgr, "densenet121", m, lambda im: tf(im)))
    return _retriever


def test_retriever_end_to_end_on_densenet121():
    s = _densenet_retriever()
    r, tf = s["r"], s["tf"]
    for img, (res, qemb) in zip(s["sources"][:2], s["singles"]):             # RGB 300 x 280 and L 1024 x 1024
        r.search(img, top_k=5)
        assert r.last_preprocess == {"device": 1, "host": 0}
        assert r._query_tensor(img).is_cuda and r._query_tensor(img).dtype == torch.uint8
        assert torch.equal(qemb, r.embed(r.transform(img)[None])), (img.size, img.mode)
    # batch_search makes one device-side tf.batch call and returns what the stacked host transform gave, to the bit: a plain
    # callable has no batch attributes and takes the earlier code (torch.stack of transform(i))
    batch = r.batch_search(s["sources"], top_k=5)
    assert r.last_preprocess == {"device": 5, "host": 0}
    assert s["plain"].last_preprocess is None
    assert batch == s["plain"].batch_search(s["sources"], top_k=5)
    singles = [res for res, _ in s["singles"]]
    assert [[d["id"] for d in hits] for hits in batch] == [[d["id"] for d in hits] for hits in singles]


def test_batch_search_equals_five_search_calls():
    """The row dicts of one batch_search of the five sources equal those of five search calls, distances included.  The model's
    rows and the search do not depend on the batch; F.normalize of a [5, 1024] tensor does (two of these five rows came out
    one ulp from their [1, 1024] normalisation, 7.45e-9 / 3.73e-9 on the distances), so batch_search normalises row by row
    (MilvusRetriever._embed_rows)."""
    s = _densenet_retriever()
    batch = s["r"].batch_search(s["sources"], top_k=5)
    singles = [res for res, _ in s["singles"]]
    print("batch - single distances:", [[a["distance"] - b["distance"] for a, b in zip(x, y)] for x, y in zip(batch, singles)])
    assert batch == singles
    assert s["plain"].batch_search(s["sources"], top_k=5) == singles        # the stacked host transform: the same rule
    emb = s["r"]._embed_rows(s["tf"].batch(s["sources"], "cuda"))
    assert all(torch.equal(emb[i:i + 1], q) for i, (_, q) in enumerate(s["singles"]))


def test_encode_npy_paths_hands_the_model_the_host_transform(tmp_path):
    from mirx import nih
    rng = np.random.default_rng(11)
    paths = []
    for i, label in enumerate(("Mass", "Nodule")):
        p = tmp_path / f"0000{i}_Chest_X-ray_{label}_{i}.npy"
        np.save(p, rng.integers(0, 256, (64, 64), dtype=np.uint8))
        paths.append(str(p))
    tf = nih.build_nih_val_transform(384, 432)
    seen = []

    class _Stub(torch.nn.Module):
        def forward(self, x):
            seen.append(x)
            return {"embedding": x.flatten(1)[:, :nih.EMBEDDING_DIM].contiguous()}

    rows = nih.encode_npy_paths(_Stub(), tf, paths, torch.device("cuda"), batch_size=2)
    assert tf.last_preprocess == {"device": 2, "host": 0}
    want = torch.stack([tf(nih.load_npy_as_pil(p)) for p in paths])
    assert len(seen) == 1 and seen[0].is_cuda and seen[0].dtype == torch.float32
    assert torch.equal(seen[0].cpu().view(torch.int32), want.view(torch.int32))
    assert [r["label_names"] for r in rows] == [["Mass"], ["Nodule"]]
    assert np.array_equal(rows[1]["embedding"], want[1].flatten()[:nih.EMBEDDING_DIM].numpy())
