"""Insertion / deletion curves of one query as one device job.

Mirrors (paths into the reference):
  InsDel                          evaluate_saliency.py:33-91 (load_query / evaluate / forward, counters swapped as there)
  the per-hit driver loop         evaluate_test_dataset_milvus.py:446-590 (one deletion and one insertion curve per hit)
  CausalMetric.single_run         evaluation.py:65-138 (scores, the negative-value rule, auc)

`mirx.xai.CausalMetric.evaluate` handles one (pair, mode) per call: a host argsort, a copy, torch.where, a dense
[3, 3, 51, 51] conv2d for the blur and one small embed.  Here all curves of a query -- M modes x K hits x (n_steps + 1) images
-- are ranked (mirx_insdel_steps), blurred (mirx_blur2d_same) and composed (mirx_insdel_compose) on the device, go to the
embedder in full `max_batch` chunks that cross curve boundaries, and one call scores them (mirx_insdel_curves).

The tie rule is DEFINED: pixels go in the order np.flip(np.argsort(saliency, kind="stable")) of the float32 map -- saliency
descending, equal values by descending flat index, -0.0 equal to +0.0, NaN first.  (The reference's default argsort is not
stable: its order on ties depends on the numpy build, and ReLU'd maps are full of ties.)  The native path and the torch
restatement that serves every other input follow the same rule and the same float64 scoring.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib

INSDEL_MAX_HW = 1 << 20        # include/mirx.h MIRX_INSDEL_MAX_HW
INSDEL_MAX_K = 65535
BLUR_MAX_KLEN = 63
_MODES = ("del", "ins")


def _xai():
    from . import xai          # xai re-exports this module: resolved at call time, whichever is imported first
    return xai


def _ptr(t):
    import ctypes
    return ctypes.c_void_p(t.data_ptr())


def _stream(dev):
    import ctypes
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


# ---- kernel wrappers ----------------------------------------------------------------------------------------------------
def insdel_steps(sal, step):
    """[HIP] mirx_insdel_steps: sal [K, hw] CUDA fp32 -> int32 [K, hw], t[p] = rank(p) // step under the stable tie rule."""
    if not (torch.is_tensor(sal) and sal.is_cuda and sal.dtype == torch.float32 and sal.dim() == 2):
        raise ValueError("insdel_steps: sal must be a [K, hw] float32 CUDA tensor")
    k, hw = sal.shape
    step = int(step)
    if not (1 <= hw <= INSDEL_MAX_HW and 1 <= k <= INSDEL_MAX_K and step >= 1):
        raise ValueError(f"insdel_steps: needs 1 <= hw <= 2^20, 1 <= K <= {INSDEL_MAX_K}, step >= 1 (got hw = {hw}, K = {k}, "
                         f"step = {step})")
    lib = _lib.load()
    sal = sal.contiguous()
    n_ws = lib.mirx_insdel_steps_workspace_bytes(k, hw)
    if n_ws < 0:
        _lib.check(int(n_ws), "mirx_insdel_steps_workspace_bytes")
    with torch.cuda.device(sal.device):
        ws = torch.empty((n_ws,), dtype=torch.uint8, device=sal.device)
        t = torch.empty((k, hw), dtype=torch.int32, device=sal.device)
        _lib.check(lib.mirx_insdel_steps(_ptr(sal), k, hw, step, _ptr(ws), n_ws, _ptr(t), _stream(sal.device)), "mirx_insdel_steps")
    return t


def blur2d_same(x, kernel2d):
    """[HIP] mirx_blur2d_same: x [n, c, h, w] CUDA fp32, kernel2d [klen, klen] -> the zero-padded correlation of every plane."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4):
        raise ValueError("blur2d_same: x must be a [n, c, h, w] float32 CUDA tensor")
    if kernel2d.dim() != 2 or kernel2d.shape[0] != kernel2d.shape[1] or kernel2d.shape[0] % 2 == 0 or \
            kernel2d.shape[0] > BLUR_MAX_KLEN:
        raise ValueError(f"blur2d_same: the kernel must be [klen, klen], klen odd and <= {BLUR_MAX_KLEN} "
                         f"(got {tuple(kernel2d.shape)})")
    n, c, h, w = x.shape
    if c < 1 or h < 1 or w < 1:
        raise ValueError(f"blur2d_same: empty planes (got {tuple(x.shape)})")
    if n == 0:
        return torch.empty_like(x)
    lib = _lib.load()
    x = x.contiguous()
    kern = kernel2d.detach().to(device=x.device, dtype=torch.float32).contiguous()
    y = torch.empty_like(x)
    with torch.cuda.device(x.device):
        _lib.check(lib.mirx_blur2d_same(_ptr(x), n, c, h, w, _ptr(kern), kern.shape[0], _ptr(y), _stream(x.device)),
                   "mirx_blur2d_same")
    return y


def insdel_compose(t, bank, start, finish, row, n_steps, g0, n, out=None):
    """[HIP] mirx_insdel_compose: images [g0, g0 + n) of the job -> [n, 3, hw] (t int32 [K, hw], bank fp32 [n_bank, 3, hw],
    start / finish / row int32 [curves] on the device, -1 = the all-zero image)."""
    if not (t.is_cuda and t.dtype == torch.int32 and t.dim() == 2 and t.is_contiguous()):
        raise ValueError("insdel_compose: t must be a contiguous [K, hw] int32 CUDA tensor")
    hw = t.shape[1]
    if not (bank.is_cuda and bank.dtype == torch.float32 and bank.dim() == 3 and bank.shape[1:] == (3, hw) and bank.is_contiguous()
            and bank.shape[0] >= 1):
        raise ValueError(f"insdel_compose: bank must be a contiguous [n_bank >= 1, 3, {hw}] float32 CUDA tensor")
    curves = start.numel()
    for a in (start, finish, row):
        if not (a.is_cuda and a.dtype == torch.int32 and a.dim() == 1 and a.numel() == curves and a.is_contiguous()):
            raise ValueError("insdel_compose: start, finish and row must be int32 CUDA vectors of one length")
    g0, n, n_steps = int(g0), int(n), int(n_steps)
    if curves < 1 or n_steps < 1 or g0 < 0 or n < 0 or g0 + n > curves * (n_steps + 1):
        raise ValueError(f"insdel_compose: [g0, g0 + n) = [{g0}, {g0 + n}) outside the job's {curves} x {n_steps + 1} images")
    if out is None:
        out = torch.empty((n, 3, hw), dtype=torch.float32, device=t.device)
    elif out.numel() != n * 3 * hw or out.dtype != torch.float32 or not out.is_contiguous() or out.device != t.device:
        raise ValueError(f"insdel_compose: out must be a contiguous float32 tensor of {n} x 3 x {hw} elements on {t.device}")
    if n == 0:
        return out
    lib = _lib.load()
    with torch.cuda.device(t.device):
        _lib.check(lib.mirx_insdel_compose(_ptr(t), t.shape[0], hw, _ptr(bank), bank.shape[0], _ptr(start), _ptr(finish), _ptr(row),
                                           curves, n_steps, g0, n, _ptr(out), _stream(t.device)), "mirx_insdel_compose")
    return out


def insdel_scores(q_feat, r_feats, curves, n_steps):
    """[HIP] mirx_insdel_curves: q_feat [1, D], r_feats [curves * (n_steps + 1), D] CUDA fp32 -> (scores fp64 [curves,
    n_steps + 1], auc fp64 [curves], zero_counter int64 [curves]) on the device."""
    curves, n_steps = int(curves), int(n_steps)
    for a in (q_feat, r_feats):
        if not (a.is_cuda and a.dtype == torch.float32 and a.dim() == 2):
            raise ValueError("insdel_scores: the embeddings must be 2-d float32 CUDA tensors")
    d = q_feat.shape[1]
    if curves < 1 or n_steps < 1 or d < 1 or q_feat.shape[0] != 1 or tuple(r_feats.shape) != (curves * (n_steps + 1), d):
        raise ValueError(f"insdel_scores: needs q_feat [1, D] and r_feats [{curves} * ({n_steps} + 1), D] "
                         f"(got {tuple(q_feat.shape)}, {tuple(r_feats.shape)})")
    lib = _lib.load()
    q_feat, r_feats = q_feat.contiguous(), r_feats.contiguous()
    dev = q_feat.device
    scores = torch.empty((curves, n_steps + 1), dtype=torch.float64, device=dev)
    auc = torch.empty((curves,), dtype=torch.float64, device=dev)
    zero = torch.empty((curves,), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.mirx_insdel_curves(_ptr(q_feat), _ptr(r_feats), curves, n_steps, d, _ptr(scores), _ptr(auc), _ptr(zero),
                                          _stream(dev)), "mirx_insdel_curves")
    return scores, auc, zero


# ---- substrates -----------------------------------------------------------------------------------------------------------
class GaussianBlur:
    """Callable substrate: every channel blurred with gkern(klen, nsig)[0, 0] (`.kernel2d`), zero padding klen // 2 -- what
    conv2d(x, gkern(klen, nsig), padding=klen // 2) computes.  Native (mirx_blur2d_same) on CUDA float32 input with an odd klen up
    to 63; elsewhere the conv2d form."""

    def __init__(self, klen=51, nsig=math.sqrt(50)):
        self.klen, self.nsig = int(klen), float(nsig)
        if self.klen < 1:
            raise ValueError(f"GaussianBlur: klen must be >= 1 (got {klen})")
        self.kernel2d = _xai().gkern(self.klen, self.nsig)[0, 0].contiguous()
        self.last_native = False
        self._on = {}

    def _kernel_on(self, device):
        k = self._on.get(device)
        if k is None:
            k = self._on[device] = self.kernel2d.to(device)
        return k

    def __call__(self, x):
        if x.dim() != 4:
            raise ValueError(f"GaussianBlur: x must be [n, c, h, w] (got {tuple(x.shape)})")
        k = self._kernel_on(x.device)
        self.last_native = bool(x.is_cuda and x.dtype == torch.float32 and self.klen % 2 == 1 and self.klen <= BLUR_MAX_KLEN
                                and x.numel() > 0)
        if self.last_native:
            return blur2d_same(x, k)
        c = x.shape[1]
        return F.conv2d(x, k.to(x.dtype).expand(c, 1, self.klen, self.klen), padding=self.klen // 2, groups=c)


# ---- the job ------------------------------------------------------------------------------------------------------------
class InsDelResult:
    """auc [K, M] float64, scores [K, M, n_steps + 1] float64, zero_counter [K, M] int64 (numpy; M follows `modes`),
    last_native: whether the HIP path ran."""

    def __init__(self, auc, scores, zero_counter, modes, n_steps, last_native):
        self.auc, self.scores, self.zero_counter = auc, scores, zero_counter
        self.modes, self.n_steps, self.last_native = tuple(modes), int(n_steps), bool(last_native)

    def __repr__(self):
        return f"InsDelResult(K={self.auc.shape[0]}, modes={self.modes}, n_steps={self.n_steps}, last_native={self.last_native})"


def stable_steps(sal, step):
    """The torch restatement of mirx_insdel_steps: sal [K, hw] float32 tensor -> int64 [K, hw] on its device."""
    k, hw = sal.shape
    # stable descending sort of the reversed row: equal values keep the reversed (= descending index) order; torch orders a NaN
    # above every number and -0.0 == +0.0
    order = (hw - 1) - torch.sort(sal.flip(1), dim=1, descending=True, stable=True).indices
    rank = torch.empty_like(order)
    rank.scatter_(1, order, torch.arange(hw, device=sal.device).expand(k, hw))
    return rank // int(step)


def _check_images(x_q, x_r, input_size):
    if not (torch.is_tensor(x_q) and torch.is_tensor(x_r)):
        raise ValueError("insdel_curves: x_q and x_r must be tensors")
    if x_q.dim() != 4 or x_q.shape[0] != 1 or x_q.shape[1] != 3 or x_q.shape[2] != x_q.shape[3]:
        raise ValueError(f"insdel_curves: x_q must be [1, 3, S, S] (got {tuple(x_q.shape)})")
    if x_r.dim() != 4 or x_r.shape[0] < 1 or x_r.shape[1:] != x_q.shape[1:]:
        raise ValueError(f"insdel_curves: x_r must be [K >= 1, 3, S, S] with the query's S (got {tuple(x_r.shape)})")
    if x_r.device != x_q.device or x_r.dtype != x_q.dtype:
        raise ValueError("insdel_curves: x_q and x_r must share device and dtype")
    s = x_q.shape[2]
    if input_size is not None and int(input_size) != s:
        raise ValueError(f"insdel_curves: input_size = {input_size} but the images are {s} x {s}")
    if not 1 <= s * s <= INSDEL_MAX_HW:
        raise ValueError(f"insdel_curves: S * S must be in [1, 2^20] (got S = {s})")
    if x_r.shape[0] > INSDEL_MAX_K:
        raise ValueError(f"insdel_curves: at most {INSDEL_MAX_K} hits per call (got {x_r.shape[0]})")
    return x_r.shape[0], s


def _substrate_images(fn, x_r):
    """fn applied to the hits: ours in one call (a blurred pixel's bits do not depend on the batch), any other callable per hit,
    the way CausalMetric calls it.  None = the all-zero image, which needs no bank entry."""
    if fn is torch.zeros_like:
        return None
    if isinstance(fn, GaussianBlur):
        out = fn(x_r)
    else:
        out = torch.cat([fn(x_r[k:k + 1]) for k in range(x_r.shape[0])])
    if not torch.is_tensor(out) or out.shape != x_r.shape:
        raise ValueError(f"insdel_curves: a substrate must return a tensor of its input's shape (got "
                         f"{tuple(out.shape) if torch.is_tensor(out) else type(out)})")
    return out.to(device=x_r.device, dtype=x_r.dtype)


def insdel_curves(model, x_q, x_r, saliency, step, modes=("del", "ins"), substrates=None, input_size=None, max_batch=1024):
    """All insertion / deletion curves of one query: x_q [1, 3, S, S], x_r [K, 3, S, S], saliency [K, S, S] (numpy or tensor,
    host or device; ranked as float32) -> InsDelResult.  Curve (k, mode) is CausalMetric(model, mode, step, substrates[mode])
    .evaluate(x_q, x_r[k:k+1], saliency[k]) under the stable tie rule: "del" goes from the hit to its substrate, "ins" from the
    substrate to the hit.  substrates: {"del": torch.zeros_like, "ins": GaussianBlur(51, sqrt(50))} unless given; any callable
    on [1, 3, S, S] works.  Native when the images are CUDA float32; only one `max_batch` chunk of step images exists at a time."""
    k, s = _check_images(x_q, x_r, input_size)
    hw = s * s
    try:
        step_i, max_batch_i = int(step), int(max_batch)
    except (TypeError, ValueError):
        raise ValueError("insdel_curves: step and max_batch must be integers") from None
    if step_i < 1 or step_i != step or max_batch_i < 1:
        raise ValueError(f"insdel_curves: step and max_batch must be integers >= 1 (got {step}, {max_batch})")
    modes = tuple(modes)
    if not modes or any(m not in _MODES for m in modes) or len(set(modes)) != len(modes):
        raise ValueError(f"insdel_curves: modes must be a non-empty selection of {_MODES} without repeats (got {modes})")
    subs = {"del": torch.zeros_like, "ins": None}
    if substrates is not None:
        if not isinstance(substrates, dict) or any(m not in _MODES for m in substrates) or \
                any(not callable(f) for f in substrates.values()):
            raise ValueError("insdel_curves: substrates must map 'del' / 'ins' to callables")
        subs.update(substrates)
    if "ins" in modes and subs["ins"] is None:
        subs["ins"] = GaussianBlur(51, math.sqrt(50))
    sal = torch.as_tensor(np.ascontiguousarray(saliency) if isinstance(saliency, np.ndarray) else saliency)
    if sal.numel() != k * hw or (sal.dim() > 1 and sal.shape[0] != k):
        raise ValueError(f"insdel_curves: saliency must be [K = {k}, {s}, {s}] (got {tuple(sal.shape)})")
    sal = sal.detach().to(device=x_r.device, dtype=torch.float32).reshape(k, hw)

    m_n = len(modes)
    curves = k * m_n
    n_steps = (hw + step_i - 1) // step_i
    per = n_steps + 1
    total = curves * per
    native = bool(x_r.is_cuda and x_r.dtype == torch.float32)
    embed = _xai().CausalMetric._embed
    dev = x_r.device
    with torch.no_grad():
        q_feat = embed(model, x_q)
        # the bank: the hits, then every mode's substrate images; curve j = k * M + m
        bank = [x_r.reshape(k, 3, hw)]
        start = np.empty((k, m_n), dtype=np.int32)
        finish = np.empty((k, m_n), dtype=np.int32)
        for mi, mode in enumerate(modes):
            img = _substrate_images(subs[mode], x_r)
            if img is None:
                sub_idx = np.full(k, -1, dtype=np.int32)
            else:
                sub_idx = np.arange(k, dtype=np.int32) + sum(b.shape[0] for b in bank)
                bank.append(img.reshape(k, 3, hw))
            hit_idx = np.arange(k, dtype=np.int32)
            start[:, mi], finish[:, mi] = (hit_idx, sub_idx) if mode == "del" else (sub_idx, hit_idx)
        bank = torch.cat(bank).contiguous() if len(bank) > 1 else bank[0].contiguous()
        row = np.repeat(np.arange(k, dtype=np.int32), m_n)
        start_d = torch.from_numpy(start.reshape(-1)).to(dev)
        finish_d = torch.from_numpy(finish.reshape(-1)).to(dev)
        row_d = torch.from_numpy(row).to(dev)

        feats = None
        if native:
            t = insdel_steps(sal, step_i)
            buf = torch.empty((min(max_batch_i, total), 3, s, s), dtype=torch.float32, device=dev)
        else:
            t = stable_steps(sal, step_i)
            zero_img = torch.zeros((1, 3, hw), dtype=bank.dtype, device=dev)
            bank_z = torch.cat([bank, zero_img])                     # index -1 reads the all-zero image
        for g0 in range(0, total, max_batch_i):
            n = min(max_batch_i, total - g0)
            if native:
                imgs = buf[:n]
                insdel_compose(t, bank, start_d, finish_d, row_d, n_steps, g0, n, out=imgs)
            else:
                g = torch.arange(g0, g0 + n, device=dev)
                j, st = g // per, g % per
                mask = t[row_d.long()[j]][:, None, :] < st[:, None, None]
                imgs = torch.where(mask, bank_z[finish_d.long()[j]], bank_z[start_d.long()[j]]).reshape(n, 3, s, s)
            f = embed(model, imgs)
            f = f.reshape(n, -1)
            if feats is None:
                feats = torch.empty((total, f.shape[1]), dtype=f.dtype, device=f.device)
            feats[g0:g0 + n] = f

        q2 = q_feat.reshape(1, -1)
        if q2.shape[1] != feats.shape[1]:
            raise ValueError(f"insdel_curves: the query embeds to {q2.shape[1]} features, the step images to {feats.shape[1]}")
        if native and feats.is_cuda and feats.dtype == torch.float32 and q2.dtype == torch.float32:
            scores, auc, zero = insdel_scores(q2, feats, curves, n_steps)
            scores, auc, zero = scores.cpu().numpy(), auc.cpu().numpy(), zero.cpu().numpy()
        else:
            native = False
            q64, r64 = q2.double(), feats.double()
            cos = (r64 @ q64[0]) / (q64.norm().clamp_min(1e-8) * r64.norm(dim=1).clamp_min(1e-8))
            cos = cos.cpu().numpy().reshape(curves, per)
            zero = np.count_nonzero(cos < 0, axis=1).astype(np.int64)
            scores = np.where(cos < 0, 0.0, cos)
            total_sum = np.cumsum(scores, axis=1)[:, -1]             # index order, as the kernel sums
            auc = (total_sum - scores[:, 0] / 2 - scores[:, -1] / 2) / n_steps
    return InsDelResult(auc.reshape(k, m_n), scores.reshape(k, m_n, per), zero.reshape(k, m_n), modes, n_steps, native)


class InsDel:
    """evaluate_saliency.py:33-91: deletion onto zeros and insertion from the gkern(51, sqrt(50)) blur, `input_size` pixels per
    step, with the reference's return orders.  `forward` runs all hits in one insdel_curves call."""

    def __init__(self, model, device="cuda", input_size=224, max_batch=1024):
        self.model = model
        self.device = device
        self.input_size = int(input_size)
        self.max_batch = int(max_batch)
        self.substrates = {"del": torch.zeros_like, "ins": GaussianBlur(51, math.sqrt(50))}
        self.last_native = False

    def load_query(self, query_image):
        self.q_image = query_image

    def _curves(self, sal_maps, ret_images):
        x_r = torch.cat([r.reshape(1, *r.shape[-3:]) for r in ret_images]).to(self.device)
        sal = np.stack([np.asarray(m.detach().cpu() if torch.is_tensor(m) else m, dtype=np.float32) for m in sal_maps])
        x_q = self.q_image.to(self.device)
        res = insdel_curves(self.model, x_q.reshape(1, *x_q.shape[-3:]), x_r, sal.reshape(len(sal_maps), -1), self.input_size,
                            modes=("del", "ins"), substrates=self.substrates, input_size=self.input_size, max_batch=self.max_batch)
        self.last_native = res.last_native
        return res

    def evaluate(self, new_sal, ret_image):
        """-> (score_del, score_ins, zero_cnt_ins, zero_cnt_del).  As in the reference the counter names are swapped: the third
        value is the DELETION run's count of negative similarities, the fourth the insertion run's."""
        res = self._curves([new_sal], [ret_image])
        return float(res.auc[0, 0]), float(res.auc[0, 1]), int(res.zero_counter[0, 0]), int(res.zero_counter[0, 1])

    def forward(self, q_image, ret_dict, sal_dict):
        """-> (ins_avg, del_avg, z_ins_list, z_del_list): per hit, in sal_dict's order; z_ins_list holds evaluate's third values."""
        self.load_query(q_image)
        n = len(sal_dict)
        if n == 0:
            return [], [], [], []
        res = self._curves([sal_dict[i] for i in range(n)], [ret_dict[i] for i in range(n)])
        ins_avg = [float(v) for v in res.auc[:, 1]]
        del_avg = [float(v) for v in res.auc[:, 0]]
        z_ins_list = [int(v) for v in res.zero_counter[:, 0]]
        z_del_list = [int(v) for v in res.zero_counter[:, 1]]
        return ins_avg, del_avg, z_ins_list, z_del_list

    __call__ = forward
