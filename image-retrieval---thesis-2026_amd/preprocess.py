"""Batched convert('RGB') -> Resize -> CenterCrop (-> ToTensor -> Normalize) on the device, bit-equal to the host path.

`default_transform` (mirx.retriever) resizes one image at a time in Pillow.  `attach` gives the function it returns two more
attributes that take a LIST of PIL images of any mix of sizes and return the whole batch on the device:

    tf.batch_pixels(images, device) -> uint8   [B, 3, S, S]      what tf.pixels(img) returns, stacked
    tf.batch(images, device)        -> float32 [B, 3, S, S]      what tf(img) returns, stacked

Both equal the host path byte for byte (mirx_resample_batch, DESIGN 28 and 30: Pillow's BILINEAR and BICUBIC for 8-bit images
restated as a host plan of integer coefficients plus one integer kernel), for the three shapes default_transform builds:
Resize(int) + CenterCrop and the stretch Resize((S, S)) without a crop, each in either filter.  Which path an image takes is
decided from what can be observed, with no option and no environment variable:

    device path   the target device is CUDA, the image's mode is "RGB" or "L", its sides are within the kernel's caps (8192
                  pixels, a scale of at most 32 per axis, 16 for bicubic) and, for Resize(int), the resized image covers the
                  crop (resize >= img_size)
    host path     everything else -- other modes ("P", "RGBA", "I;16", "F", ...), CPU devices, oversize sources: tf.pixels / tf
                  on the host, copied into the image's slot.  It is the only path without a GPU and the tests' reference.

`tf.last_preprocess` = {"device": n, "host": m} says how many images of the last batch took each path.

The sources of a batch are packed with np.asarray into one reused pinned staging buffer together with their descriptors and
coefficient tables (plans are cached by (w, h, resize, S, filter); images of one size share their tables) and reach the device
in ONE copy; an event recorded behind the kernel guards the staging buffer and its device twin until the next batch reuses
them.  A lock serialises the launches of concurrent callers.
"""
import ctypes
import threading

import numpy as np
import torch

from . import _lib as L

_DEVICE_MODES = ("RGB", "L")
_CHUNK_BYTES = 256 << 20           # sources per launch: bounds the pinned buffer (64 RGB images of 1024 x 1024 are 192 MiB)
_PLAN_CACHE_MAX = 512
_FILTERS = {"bilinear": L.RESAMPLE_BILINEAR, "bicubic": L.RESAMPLE_BICUBIC}
_plans = {}
_stages = {}
_lock = threading.Lock()


def _round16(n):
    return (n + 15) & ~15


def filter_name(interpolation):
    """"bilinear" or "bicubic" from either name or from PIL's Image.BILINEAR / Image.BICUBIC; anything else raises ValueError."""
    from PIL import Image
    if isinstance(interpolation, str):
        if interpolation.lower() in _FILTERS:
            return interpolation.lower()
    elif interpolation == Image.BILINEAR:
        return "bilinear"
    elif interpolation == Image.BICUBIC:
        return "bicubic"
    raise ValueError(f"interpolation must be 'bilinear' or 'bicubic' (or PIL's Image.BILINEAR / Image.BICUBIC), got {interpolation!r}")


def resized_geometry(w, h, resize, size):
    """(nw, nh, left, top): torchvision's Resize(int) output size and CenterCrop offsets, the expressions of
    retriever.default_transform (Python's round: half to even).  resize = (size, size) is the stretch Resize((S, S)): the
    whole resized image, no crop."""
    if isinstance(resize, tuple):
        return size, size, 0, 0
    if w <= h:
        nw, nh = resize, int(resize * h / w)
    else:
        nw, nh = int(resize * w / h), resize
    return nw, nh, int(round((nw - size) / 2.0)), int(round((nh - size) / 2.0))


def axis_table(in_size, out_size, first, n, interpolation="bilinear"):
    """The library's plan of one axis and crop window (mirx_resample_plan_filter): int32 [4 + 2 n + n taps] padded to 16 bytes,
    or None when the axis is over a cap."""
    lib = L.load()
    filt = _FILTERS[filter_name(interpolation)]
    taps = lib.mirx_resample_taps_filter(int(in_size), int(out_size), filt)
    if taps < 0:
        return None
    words = 4 + 2 * n + n * taps
    table = np.zeros((words + 3) & ~3, dtype=np.int32)
    L.check(lib.mirx_resample_plan_filter(int(in_size), int(out_size), int(first), int(n), filt, table.ctypes.data, words),
            "mirx_resample_plan_filter")
    return table


def table_parts(table):
    """(taps, bounds [n, 2], coefficients [n, taps]) views of an axis table."""
    taps, n = int(table[0]), int(table[1])
    return taps, table[4:4 + 2 * n].reshape(n, 2), table[4 + 2 * n:4 + 2 * n + n * taps].reshape(n, taps)


def plan(w, h, resize, size, interpolation="bilinear"):
    """(x table, y table) for a w x h source, or None when the device path does not take it (a cap, or a crop window that
    reaches outside the resized image).  resize is the int of Resize(int) + CenterCrop(size), or (size, size) for the stretch
    (each axis planned over the whole output with its own scale).  Cached."""
    interpolation = filter_name(interpolation)
    if isinstance(resize, (tuple, list)):
        if tuple(resize) != (size, size):
            raise ValueError(f"a resize pair must be (size, size) = ({size}, {size}), got {resize!r}")
        resize = (size, size)
    key = (w, h, resize, size, interpolation)
    if key in _plans:
        return _plans[key]
    got = None
    nw, nh, left, top = resized_geometry(w, h, resize, size)
    if (1 <= w <= L.RESAMPLE_MAX_SIDE and 1 <= h <= L.RESAMPLE_MAX_SIDE and 1 <= size <= L.RESAMPLE_MAX_OUT
            and left >= 0 and top >= 0 and left + size <= nw and top + size <= nh):
        xt = axis_table(w, nw, left, size, interpolation)
        yt = axis_table(h, nh, top, size, interpolation) if xt is not None else None
        if yt is not None:
            _, yb, _ = table_parts(yt)
            span = max(int((yb[y0:y0 + L.RESAMPLE_TILE_H].sum(axis=1)).max() - yb[y0:y0 + L.RESAMPLE_TILE_H, 0].min())
                       for y0 in range(0, size, L.RESAMPLE_TILE_H))
            # three channels: one answer per size, whatever the mode
            if int(xt[0]) * L.RESAMPLE_TILE_W * 4 + span * 3 * L.RESAMPLE_TILE_W <= L.RESAMPLE_MAX_LDS:
                got = (xt, yt)
    if len(_plans) >= _PLAN_CACHE_MAX:
        _plans.clear()
    _plans[key] = got
    return got


class _Stage:
    """The pinned staging buffer of one device, its device twin and the event that guards both."""

    def __init__(self, dev):
        self.dev, self.cap, self.pinned, self.host, self.gpu, self.event = dev, 0, None, None, None, None

    def reserve(self, n):
        if self.event is not None:
            self.event.synchronize()                         # the last batch's copy and kernel are done with both buffers
        if n > self.cap:
            cap = max(_round16(n + n // 4), 1 << 20)
            self.pinned = torch.empty(cap, dtype=torch.uint8, pin_memory=True)
            self.host = self.pinned.numpy()
            self.gpu = torch.empty(cap, dtype=torch.uint8, device=self.dev)
            self.cap = cap


def blob_layout(items):
    """items = [(PIL image, (x table, y table))] -> (tables {id: (offset, table)}, descriptors, bytes): where everything of a
    launch lies in its byte buffer (include/mirx.h, mirx_resample_batch).  Tables shared by several images are laid out once."""
    at = len(items) * L.RESAMPLE_DESC_WORDS * 8
    tables, layout = {}, []
    for img, (xt, yt) in items:
        for t in (xt, yt):
            if id(t) not in tables:
                tables[id(t)] = (at, t)
                at += t.nbytes
    for img, (xt, yt) in items:
        w, h = img.size
        ch = 3 if img.mode == "RGB" else 1
        layout.append((at, w, h, w * ch, ch, tables[id(xt)][0], tables[id(yt)][0], 0))
        at = _round16(at + w * h * ch)
    return tables, layout, at


def blob_fill(host, items, tables, layout):
    """Write descriptors, tables and the images' bytes (np.asarray) into the uint8 array `host`."""
    host[:len(items) * 64].view(np.int64)[:] = np.asarray(layout, dtype=np.int64).reshape(-1)
    for off, t in tables.values():
        host[off:off + t.nbytes].view(np.int32)[:] = t
    for (off, w, h, pitch, ch, _, _, _), (img, _) in zip(layout, items):
        host[off:off + h * pitch] = np.asarray(img).reshape(-1)


def _launch(stage, items, size, f32, norm, out):
    """Pack, copy, launch into out [len(items), 3, size, size]."""
    n = len(items)
    tables, layout, at = blob_layout(items)
    stage.reserve(at)
    blob_fill(stage.host, items, tables, layout)
    stage.gpu[:at].copy_(stage.pinned[:at], non_blocking=True)
    stream = torch.cuda.current_stream(stage.dev)
    L.check(L.load().mirx_resample_batch(stage.pinned.data_ptr(), stage.gpu.data_ptr(), at, n, size,
                                         L.RESAMPLE_OUT_F32 if f32 else L.RESAMPLE_OUT_U8, norm[0], norm[1], out.data_ptr(),
                                         stream.cuda_stream), "mirx_resample_batch")
    if stage.event is None:
        stage.event = torch.cuda.Event()
    stage.event.record(stream)


def resample_into(items, size, out, mean=None, std=None):
    """One launch: items = [(PIL image in mode "RGB" or "L", plan(...) of its size)] -> out, a contiguous CUDA tensor
    [len(items), 3, size, size] that is uint8 (the pixels) or float32 (normalised with mean / std, three floats each)."""
    assert out.is_cuda and out.is_contiguous() and tuple(out.shape) == (len(items), 3, size, size)
    f32 = out.dtype == torch.float32
    assert f32 or out.dtype == torch.uint8
    norm = ((ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)) if f32 else (None, None)
    with _lock, torch.cuda.device(out.device):
        stage = _stages.get(out.device.index)
        if stage is None:
            stage = _stages[out.device.index] = _Stage(out.device)
        _launch(stage, items, size, f32, norm, out)


def _run(tf, images, device, size, resize, interpolation, f32, norm):
    dev = torch.device(device)
    images = list(images)
    dtype = torch.float32 if f32 else torch.uint8
    host_fn = (lambda im: tf(im)) if f32 else (lambda im: torch.from_numpy(tf.pixels(im)))
    on_dev = []
    if dev.type == "cuda":
        for i, im in enumerate(images):
            if getattr(im, "mode", None) in _DEVICE_MODES:
                p = plan(im.size[0], im.size[1], resize, size, interpolation)
                if p is not None:
                    on_dev.append((i, im, p))
    tf.last_preprocess = {"device": len(on_dev), "host": len(images) - len(on_dev)}
    if not on_dev:
        if not images:
            return torch.empty((0, 3, size, size), dtype=dtype, device=dev)
        return torch.stack([host_fn(im) for im in images]).to(dev)
    with torch.cuda.device(dev):
        dev = torch.device("cuda", torch.cuda.current_device())
        dense = torch.empty((len(on_dev), 3, size, size), dtype=dtype, device=dev)
        k0 = 0
        while k0 < len(on_dev):                              # one launch unless the sources outgrow the staging bound
            k1, nbytes = k0, 0
            while k1 < len(on_dev) and k1 - k0 < L.RESAMPLE_MAX_BATCH and (k1 == k0 or nbytes < _CHUNK_BYTES):
                w, h = on_dev[k1][1].size
                nbytes += w * h * 3
                k1 += 1
            resample_into([(im, p) for _, im, p in on_dev[k0:k1]], size, dense[k0:k1], *norm)
            k0 = k1
        if len(on_dev) == len(images):
            return dense
        out = torch.empty((len(images), 3, size, size), dtype=dtype, device=dev)
        out[torch.tensor([i for i, _, _ in on_dev], device=dev)] = dense
        taken = {i for i, _, _ in on_dev}
        for i, im in enumerate(images):
            if i not in taken:
                out[i].copy_(host_fn(im))
        return out


def attach(tf, img_size, resize, interpolation="bilinear"):
    """Give a default_transform function its batch attributes (see the module docstring)."""
    def batch_pixels(images, device):
        return _run(tf, images, device, img_size, resize, interpolation, False, (None, None))

    def batch(images, device):
        return _run(tf, images, device, img_size, resize, interpolation, True, (tf.mean, tf.std))

    tf.batch_pixels, tf.batch = batch_pixels, batch
    tf.last_preprocess = {"device": 0, "host": 0}
    return tf
