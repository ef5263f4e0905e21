"""ATH: the reference's attention-based triplet hashing network (ath_model.py:ATHNet there) and its retrieval evaluation
(test_ath.py:extract_codes_logits_labels / compute_metrics, train_ath.py:compute_retrieval_metrics), MI355X-native.

  ATHNet            same module tree, state-dict keys and init as the reference; in eval mode, without grad, in fp32 on CUDA and at
                    H = W = input_size the forward is one fp32 VALU pipeline (k_ath.hip) on BatchNorm-folded weights.  Anything else
                    runs the torch graph.
  hamming_topk      exact top-k by Hamming distance on the GPU (k_hamming.hip): (distance ascending, id ascending).
  compute_metrics / compute_retrieval_metrics
                    the reference's metrics on one [Q, max(topk)] ranking from the device: hamming_topk for binary codes,
                    FlatIndex(dim, "L2") for real-valued ones.  No Q x N matrix is built and there is no Python loop per query.
"""
import ctypes

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from ._lib import MirxError
from .model import _InferenceCache

HAMMING_MAX_BITS = 1024
HAMMING_MAX_K = 1024
_ATH_CHUNK = 1024          # images per native launch sequence (bounds the workspace at ~4.3 MB per image at S = 256)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


# ---- model --------------------------------------------------------------------------------------------------------------------
def _xavier(module):
    if isinstance(module, (nn.Conv2d, nn.Linear)):
        nn.init.xavier_normal_(module.weight)


class SpatialAttention(nn.Module):
    """sigmoid(conv3x3([mean_c x, max_c x])), no bias (ath_model.py SpatialAttention)."""

    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(2, 1, kernel_size=3, padding=1, bias=False)
        self.sigmoid = nn.Sigmoid()

    def forward(self, x):
        pooled = torch.cat([torch.mean(x, dim=1, keepdim=True), torch.max(x, dim=1, keepdim=True)[0]], dim=1)
        return self.sigmoid(self.conv(pooled))


class ResBlock(nn.Module):
    """relu(BN(conv3x3(relu(BN(conv3x3/s(x))))) + identity), identity = BN(conv3x3/s(x)) when the shape changes."""

    def __init__(self, in_channels, out_channels, stride=1):
        super().__init__()

        def conv(cin, s):
            return nn.Conv2d(cin, out_channels, kernel_size=3, stride=s, padding=1, bias=False)

        self.net = nn.Sequential(conv(in_channels, stride), nn.BatchNorm2d(out_channels), nn.ReLU(inplace=True),
                                 conv(out_channels, 1), nn.BatchNorm2d(out_channels))
        self.downsample = None
        if in_channels != out_channels or stride != 1:
            self.downsample = nn.Sequential(conv(in_channels, stride), nn.BatchNorm2d(out_channels))
        self.apply(_xavier)

    def forward(self, x):
        identity = x if self.downsample is None else self.downsample(x)
        return F.relu(self.net(x) + identity, inplace=True)


def _fold(conv, bn):
    """Eval-mode BatchNorm folded into the bias-free conv before it, in fp64 -> (w' [out, in, 3, 3], b' [out])."""
    s = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    w = conv.weight.detach().double() * s.view(-1, 1, 1, 1)
    b = bn.bias.detach().double() - bn.running_mean.detach().double() * s
    return w, b


class ATHNet(_InferenceCache, nn.Module):
    """Reference ath_model.py:ATHNet: forward(x) -> (hash_codes [B, hash_size], logits [B, num_classes])."""

    def __init__(self, hash_size, num_classes, input_size=256):
        super().__init__()
        if input_size % 8 != 0:
            raise ValueError("input_size must be divisible by 8 for ATHNet.")
        flat = (input_size // 8) ** 2
        self.input_size = input_size
        self.hash_size = hash_size
        self.num_classes = num_classes
        self.net1 = nn.Sequential(ResBlock(3, 16, stride=2), nn.MaxPool2d(kernel_size=3, stride=1, padding=1))
        self.sa = SpatialAttention()
        self.net2 = nn.Sequential(ResBlock(16, 8, stride=2), nn.AvgPool2d(kernel_size=3, stride=1, padding=1))
        self.dense = ResBlock(8, 1, stride=2)
        self.hashlayer = nn.Linear(flat, hash_size)
        self.typelayer = nn.Linear(flat, num_classes)
        self.apply(_xavier)
        self._infer_cache = None

    def forward_eager(self, x):
        x = self.net1(x)
        x = self.sa(x) * x
        x = self.net2(x)
        x = torch.flatten(self.dense(x), 1)
        return self.hashlayer(x), self.typelayer(x)

    # -- MI355X inference path -------------------------------------------------------------------
    def _watch_root(self):
        return self

    def _prepare_inference(self):
        """The flat fp32 parameter block of include/mirx.h (mirx_ath_forward), BatchNorm folded, once per weight version."""
        parts = []
        for blk in (self.net1[0], self.net2[0], self.dense):
            w1, b1 = _fold(blk.net[0], blk.net[1])
            w2, b2 = _fold(blk.net[3], blk.net[4])
            wd, bd = _fold(blk.downsample[0], blk.downsample[1])
            parts += [w1, b1, w2, b2, wd, bd]
            if blk is self.net1[0]:
                parts.append(self.sa.conv.weight.detach().double())
        flat = torch.cat([p.reshape(-1) for p in parts])
        assert flat.numel() == 6294
        heads = [self.hashlayer.weight, self.hashlayer.bias, self.typelayer.weight, self.typelayer.bias]
        dev = self.hashlayer.weight.device
        params = torch.cat([flat.to(dev), torch.zeros(2, dtype=torch.float64, device=dev)]
                           + [h.detach().double().reshape(-1) for h in heads]).float().contiguous()
        cache = {"params": params, "_cuda": params.is_cuda}
        self._infer_cache = cache
        self._mark_built(cache)
        return cache

    def _native_ok(self, x):
        w = self.hashlayer.weight
        return (x.is_cuda and not self.training and not torch.is_grad_enabled() and x.dtype == torch.float32 and x.dim() == 4
                and x.shape[1] == 3 and x.shape[2] == self.input_size and x.shape[3] == self.input_size
                and w.is_cuda and w.device == x.device and w.dtype == torch.float32)

    def _forward_native(self, x, cache):
        lib = _lib.load()
        b, s = x.shape[0], self.input_size
        dev = x.device
        hash_out = torch.empty((b, self.hash_size), dtype=torch.float32, device=dev)
        logits = torch.empty((b, self.num_classes), dtype=torch.float32, device=dev)
        if b == 0:
            return hash_out, logits
        x = x.contiguous()
        for i in range(0, b, _ATH_CHUNK):
            n = min(_ATH_CHUNK, b - i)
            wsz = int(lib.mirx_ath_workspace_floats(n, s))
            ws = torch.empty((wsz,), dtype=torch.float32, device=dev)
            _lib.check(lib.mirx_ath_forward(_ptr(x[i:i + n]), n, s, _ptr(cache["params"]), self.hash_size, self.num_classes,
                                            _ptr(ws), wsz, _ptr(hash_out[i:i + n]), _ptr(logits[i:i + n]), _stream(dev)),
                       "mirx_ath_forward")
        return hash_out, logits

    def forward(self, x):
        if self._native_ok(x):
            with torch.cuda.device(x.device):
                return self._forward_native(x, self._cache())
        return self.forward_eager(x)


# ---- evaluation -----------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def extract_codes_logits_labels(model, data_loader, device, binary_codes):
    """test_ath.py:57-77: (codes, logits, labels) over the loader as CPU tensors; binary_codes -> (codes >= 0) as float."""
    model.eval()
    codes_l, logits_l, labels_l = [], [], []
    for images, labels in data_loader:
        codes, logits = model(images.to(device))
        if binary_codes:
            codes = (codes >= 0).float()
        codes_l.append(codes.cpu())
        logits_l.append(logits.cpu())
        labels_l.append(labels.cpu())
    return torch.cat(codes_l, dim=0), torch.cat(logits_l, dim=0), torch.cat(labels_l, dim=0)


def _bits_operand(t, name):
    t = torch.as_tensor(t)
    if t.dim() != 2:
        raise ValueError(f"{name}: expected [rows, bits], got {tuple(t.shape)}")
    if t.dtype == torch.bool:
        t = t.view(torch.uint8)
    elif t.dtype not in (torch.float32, torch.uint8):
        t = t.to(torch.float32)          # 0 / 1 stay exact; anything else is refused by the pack kernel
    return t


def hamming_topk(query_bits, gallery_bits, k, exclude_ids=None):
    """Exact top-k by Hamming distance: -> (dist int32 [Q, k], ids int64 [Q, k]) on the GPU.

    query_bits [Q, bits], gallery_bits [N, bits]: 0 / 1 tensors (float, uint8 or bool).  Ranking = (distance ascending, id
    ascending); exclude_ids [Q] (int64) removes that row from its query's ranking.  ValueError: bits outside [1, 1024], k outside
    [1, 1024] or above the rows that can be returned, or a value other than 0 / 1.  MirxError without a GPU."""
    q = _bits_operand(query_bits, "query_bits")
    g = _bits_operand(gallery_bits, "gallery_bits")
    bits, n, nq, k = q.shape[1], g.shape[0], q.shape[0], int(k)
    if g.shape[1] != bits:
        raise ValueError(f"query and gallery bits disagree: {bits} vs {g.shape[1]}")
    if not 1 <= bits <= HAMMING_MAX_BITS:
        raise ValueError(f"bits must be in [1, {HAMMING_MAX_BITS}], got {bits}")
    if not 1 <= k <= HAMMING_MAX_K:
        raise ValueError(f"k must be in [1, {HAMMING_MAX_K}], got {k}")
    if k > n:
        raise ValueError(f"k = {k} exceeds the {n} gallery rows")
    if exclude_ids is not None:
        exclude_ids = torch.as_tensor(exclude_ids)
        if exclude_ids.numel() != nq:
            raise ValueError("exclude_ids needs one id per query")
    if not torch.cuda.is_available():
        raise MirxError("hamming_topk needs a GPU: libmirx has no CPU path")
    lib = _lib.load()
    dev = q.device if q.is_cuda else (g.device if g.is_cuda else torch.device("cuda", torch.cuda.current_device()))
    with torch.cuda.device(dev):
        st = _stream(dev)
        q = q.to(dev).contiguous()
        g = g.to(dev).contiguous()
        ex = None
        if exclude_ids is not None:
            ex = exclude_ids.to(device=dev, dtype=torch.int64).contiguous().view(-1)
            if k > n - 1 and bool(((ex >= 0) & (ex < n)).any()):
                raise ValueError(f"k = {k} exceeds the {n - 1} rows left after an exclusion")
        words = int(lib.mirx_hamming_words(bits))
        qp = torch.empty((nq, words), dtype=torch.int32, device=dev)
        gp = torch.empty((n, words), dtype=torch.int32, device=dev)
        bad = torch.zeros((1,), dtype=torch.int32, device=dev)
        code = {torch.float32: 0, torch.uint8: 1}
        _lib.check(lib.mirx_hamming_pack(_ptr(q), code[q.dtype], nq, bits, _ptr(qp), _ptr(bad), st), "mirx_hamming_pack")
        _lib.check(lib.mirx_hamming_pack(_ptr(g), code[g.dtype], n, bits, _ptr(gp), _ptr(bad), st), "mirx_hamming_pack")
        if int(bad.item()):
            raise ValueError("binary codes must contain only 0 and 1")
        dist = torch.empty((nq, k), dtype=torch.int32, device=dev)
        ids = torch.empty((nq, k), dtype=torch.int64, device=dev)
        if nq == 0:
            return dist, ids
        wsb = int(lib.mirx_hamming_workspace_bytes(nq, n, bits, k))
        _lib.check(wsb if wsb < 0 else 0, "mirx_hamming_workspace_bytes")
        ws = torch.empty((wsb,), dtype=torch.uint8, device=dev)
        _lib.check(lib.mirx_hamming_topk(_ptr(qp), nq, _ptr(gp), n, bits, k, _ptr(ex), _ptr(ws), wsb, _ptr(dist), _ptr(ids), st),
                   "mirx_hamming_topk")
    return dist, ids


def _ranking(query_codes, gallery_codes, kmax, binary_codes):
    """One [Q, kmax] ranking (CPU int64) from the device."""
    if not torch.cuda.is_available():
        raise MirxError("ranking ATH codes needs a GPU: libmirx has no CPU path")
    if binary_codes:
        return hamming_topk(query_codes, gallery_codes, kmax)[1].cpu()
    from .index import FlatIndex
    g = torch.as_tensor(gallery_codes).float()
    ix = FlatIndex(g.shape[1], "L2")
    ix.add(g)
    return ix.search(torch.as_tensor(query_codes).float(), kmax)[1].cpu()


def _check_binary(*codes):
    for c in codes:
        c = torch.as_tensor(c)
        if c.numel() and not bool(((c == 0) | (c == 1)).all()):
            raise ValueError("binary codes must contain only 0 and 1")


def _ap_rr(matches):
    """matches [Q, k] 0/1 -> (AP, RR) per query, as the reference's loop: sum_{hits} (hits so far / rank) / hits, 1 / first rank."""
    m = matches.astype(np.int64)
    ranks = np.arange(1, m.shape[1] + 1, dtype=np.int64)
    pos = np.cumsum(m, axis=1)
    terms = np.where(m > 0, pos / ranks, 0.0)
    psum = np.cumsum(terms, axis=1)[:, -1] if m.shape[1] else np.zeros(m.shape[0])
    npos = pos[:, -1] if m.shape[1] else np.zeros(m.shape[0], dtype=np.int64)
    first = np.argmax(m > 0, axis=1) + 1
    hit = npos > 0
    ap = np.where(hit, psum / np.maximum(npos, 1), 0.0)
    rr = np.where(hit, 1.0 / first, 0.0)
    return ap, rr


def _first_most_common(lab):
    """Per row of lab [Q, k]: the most frequent label, count ties to the one seen first (Counter.most_common)."""
    _, inv = np.unique(lab, return_inverse=True)
    inv = inv.reshape(lab.shape)
    nl = int(inv.max()) + 1 if inv.size else 1
    out = np.empty(lab.shape[0], dtype=lab.dtype)
    step = max(1, (1 << 24) // max(nl, 1))
    for r0 in range(0, lab.shape[0], step):              # chunks of rows, not queries one by one
        iv = inv[r0:r0 + step]
        cnt = np.zeros((iv.shape[0], nl), dtype=np.int64)
        np.add.at(cnt, (np.arange(iv.shape[0])[:, None], iv), 1)
        c = np.take_along_axis(cnt, iv, axis=1)
        first = np.argmax(c == c.max(axis=1, keepdims=True), axis=1)
        out[r0:r0 + step] = lab[r0:r0 + step][np.arange(iv.shape[0]), first]
    return out


def _prepare(query_codes, query_labels, gallery_codes, gallery_labels, topk_values, binary_codes):
    topk_values = list(topk_values)
    if binary_codes:
        _check_binary(query_codes, gallery_codes)
    n = torch.as_tensor(gallery_codes).shape[0]
    kmax = min(max(topk_values), n)
    ranked = _ranking(query_codes, gallery_codes, kmax, binary_codes).numpy()
    ql = torch.as_tensor(query_labels).cpu().numpy().astype(np.int64)
    gl = torch.as_tensor(gallery_labels).cpu().numpy().astype(np.int64)
    return topk_values, ranked, ql, gl


def compute_metrics(query_codes, query_labels, gallery_codes, gallery_labels, query_logits, topk_values, binary_codes):
    """test_ath.py:90-172: {"classification_acc", "retrieval": {topk: {mhr, map, mrr, mp@k, r@k, majority_acc}}}."""
    topk_values, ranked, ql, gl = _prepare(query_codes, query_labels, gallery_codes, gallery_labels, topk_values, binary_codes)
    labs, cnts = np.unique(gl, return_counts=True)
    pos = np.searchsorted(labs, ql)
    total_rel = np.where((pos < labs.size) & (labs[np.minimum(pos, labs.size - 1)] == ql), cnts[np.minimum(pos, labs.size - 1)], 0)
    retrieval = {}
    for topk in topk_values:
        rl = gl[ranked[:, :topk]]
        matches = (rl == ql[:, None]).astype(np.int32)
        nrel = matches.sum(axis=1)
        ap, rr = _ap_rr(matches)
        recall = np.where(total_rel > 0, nrel / np.maximum(total_rel, 1), 0.0)
        vote = _first_most_common(rl)
        retrieval[topk] = {
            "mhr": float(np.mean((nrel > 0).astype(np.float64))),
            "map": float(np.mean(ap)),
            "mrr": float(np.mean(rr)),
            "mp@k": float(np.mean(nrel / topk)),
            "r@k": float(np.mean(recall)),
            "majority_acc": float(np.mean((vote == ql).astype(np.float64))),
        }
    logits = torch.as_tensor(query_logits).cpu()
    acc = logits.argmax(dim=1).eq(torch.as_tensor(query_labels).cpu()).float().mean().item()
    return {"classification_acc": acc, "retrieval": retrieval}


def compute_retrieval_metrics(query_codes, query_labels, gallery_codes, gallery_labels, topk_values, binary_codes):
    """train_ath.py:171-218: {topk: {mhr, map, mrr, majority_acc}}; the majority label is torch.mode's over the top-k labels."""
    topk_values, ranked, ql, gl = _prepare(query_codes, query_labels, gallery_codes, gallery_labels, topk_values, binary_codes)
    gl_t = torch.as_tensor(gallery_labels).cpu()
    results = {}
    for topk in topk_values:
        rl = gl[ranked[:, :topk]]
        matches = (rl == ql[:, None]).astype(np.int32)
        ap, rr = _ap_rr(matches)
        mode = torch.mode(gl_t[torch.from_numpy(ranked[:, :topk])], dim=1).values.numpy().astype(np.int64)
        results[topk] = {
            "mhr": float(np.mean((matches.sum(axis=1) > 0).astype(np.float64))),
            "map": float(np.mean(ap)),
            "mrr": float(np.mean(rr)),
            "majority_acc": float(np.mean((mode == ql).astype(np.float64))),
        }
    return results
