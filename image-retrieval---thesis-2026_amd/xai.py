"""Batched forwards for the insertion / deletion metric.

Mirrors (paths into /root/reference):
  gkern, auc                      evaluation.py:11-25, 41-43
  CausalMetric(...).evaluate      evaluate_test_dataset_milvus.py:32-85 (the variant the milvus
                                  evaluation runs; evaluation.py:46-138 `single_run` is its older twin)

The reference modifies `step` pixels, runs ONE B=1 forward, and repeats n_steps + 1 times (52 sequential
forwards per query-hit pair at step 1000 on 224x224), each of them ~190 kernel launches on a GPU that
is almost idle at B=1.  The images of all steps are known up front: pixel p changes after step
t(p) = rank of p in decreasing saliency // step, so image i is `where(t < i, finish, start)`.  This
class builds them on the device in one pass and pushes them through the embedder as large batches
(`max_batch`), so the whole curve costs a handful of full-occupancy forwards.  Same scores up to the
embedder's batch-size invariance (fp32, 1e-6), same return values.
"""
import numpy as np
import torch
import torch.nn.functional as F


def gkern(klen, nsig):
    """Gaussian blur kernel [3,3,klen,klen] (evaluation.py:11-25): a smoothed dirac per channel."""
    from scipy.ndimage import gaussian_filter
    inp = np.zeros((klen, klen))
    inp[klen // 2, klen // 2] = 1
    k = gaussian_filter(inp, nsig)
    kern = np.zeros((3, 3, klen, klen))
    for c in range(3):
        kern[c, c] = k
    return torch.from_numpy(kern.astype("float32"))


def auc(arr):
    """Normalised area under the curve (evaluation.py:41-43)."""
    return (arr.sum() - arr[0] / 2 - arr[-1] / 2) / (arr.shape[0] - 1)


class CausalMetric:
    def __init__(self, model, mode, step, substrate_fn, input_size=224, max_batch=256):
        assert mode in ["del", "ins"]
        self.model = model
        self.mode = mode
        self.step = step
        self.substrate_fn = substrate_fn
        self.hw = input_size * input_size
        self.max_batch = int(max_batch)

    @staticmethod
    def _embed(model, x):
        out = model(x)
        if isinstance(out, dict):
            out = out["embedding"]
        elif isinstance(out, tuple):
            out = out[0]
        return out

    def change_step(self, explanation, device):
        """t[p] = the step after which pixel p has been replaced: its rank in decreasing saliency
        (np.flip(np.argsort(...)), ties in that order) // step."""
        order = np.flip(np.argsort(np.asarray(explanation).flatten())).copy()
        rank = np.empty(self.hw, dtype=np.int64)
        rank[order] = np.arange(self.hw)
        return torch.from_numpy(rank // self.step).to(device)

    def evaluate(self, img_tensor, retrieved_tensor, explanation):
        """-> (auc, scores [n_steps + 1] float64, zero_counter) like the reference."""
        device = img_tensor.device
        n_steps = (self.hw + self.step - 1) // self.step
        side = int(self.hw ** 0.5)
        with torch.no_grad():
            q_feat = self._embed(self.model, img_tensor)
            if self.mode == "del":
                start, finish = retrieved_tensor.clone(), self.substrate_fn(retrieved_tensor)
            else:
                start, finish = self.substrate_fn(retrieved_tensor), retrieved_tensor.clone()
            start = start.reshape(1, 3, self.hw)
            finish = finish.reshape(1, 3, self.hw)
            t = self.change_step(explanation, device).view(1, 1, self.hw)
            sims = []
            for lo in range(0, n_steps + 1, self.max_batch):
                idx = torch.arange(lo, min(lo + self.max_batch, n_steps + 1), device=device).view(-1, 1, 1)
                imgs = torch.where(t < idx, finish, start).reshape(-1, 3, side, side)
                sims.append(F.cosine_similarity(q_feat, self._embed(self.model, imgs)))
            sims = torch.cat(sims).double().cpu().numpy()
        zero_counter = int(np.count_nonzero(sims < 0))
        scores = np.where(sims < 0, 0.0, sims)          # the reference clamps only negative values
        return auc(scores), scores, zero_counter


# ---- explanations.py:15-152 (SBSM / SBSMBatch: sliding-window occlusion saliency) ---------------------------
def sliding_window_masks(input_size, window_size, stride):
    """explanations.py:36-63: uint8 [N, 1, H, W], 1 outside the window, 0 inside; windows start at
    stride - window_size and step by stride (clipped at the borders)."""
    h, w = input_size
    rows = np.arange(stride - window_size, h, stride)
    cols = np.arange(stride - window_size, w, stride)
    masks = np.ones((len(rows) * len(cols), h, w), dtype=np.uint8)
    i = 0
    for r in rows:
        for c in cols:
            masks[i, max(r, 0):min(r + window_size, h), max(c, 0):min(c + window_size, w)] = 0
            i += 1
    return masks.reshape(-1, 1, h, w)


class SBSMBatch:
    """Same constructor / generate_masks / load_masks / call as explanations.py:15-152 (`SBSMBatch(model,
    input_size, gpu_batch)`, `explainer(x_q, x)` or `explainer(x)` for self-similarity) -> saliency [B, H, W]
    ([Q * B, H, W] for pairs).

    MI355X design: the masks of a sliding-window set are the outer product of row and column
    intervals, so the explainer keeps two small int32 arrays instead of the reference's uint8 [N, 1, H, W]
    tensor.  On 4-d CUDA float32 images and 2-d CUDA float32 embeddings the call is native (sbsm.py,
    csrc/k_sbsm.hip): masked images are composed `gpu_batch` at a time from the n-major list -- the reference's
    chunks exactly -- the gains are fp64 distances of the fp32 embeddings and the map is the fp64 sum over the
    covering windows.  Every other input (the CPU, other dtypes, a mask file that is not a window grid) takes
    the torch path: masked images `gpu_batch // B` whole masks at a time, the saliency as the matrix product
    sal[b] = (1 - masks)^T [HW x N] . gain[b] [N] / count.  `last_native` says which one ran.  Distances are
    Euclidean on the embedder's outputs like `torch.cdist` / `torch.norm` there."""

    def __init__(self, model, input_size, gpu_batch=100):
        self.model = model
        self.input_size = tuple(input_size)
        self.gpu_batch = int(gpu_batch)
        self.last_native = False
        self._clear()

    def _clear(self):
        self._intervals = None          # (row_iv, col_iv) numpy int32 when the masks are a window grid
        self._masks_np = None           # the mask array itself when they are not
        self._on = {}                   # device -> (row_iv, col_iv) tensors
        self._masks_t = self._inv_t = self._count = None        # the torch path's tensors, built on first use

    def _device(self):
        p = next(iter(self.model.parameters()), None) if hasattr(self.model, "parameters") else None
        return p.device if p is not None else torch.device("cpu")

    def _set_masks(self, masks):
        self._clear()
        self._masks_np = np.ascontiguousarray(masks)
        self.N = self._masks_np.shape[0]

    def _set_intervals(self, row_iv, col_iv):
        from . import sbsm
        sbsm.check_intervals(row_iv, col_iv, self.input_size)
        self._clear()
        self._intervals = (np.ascontiguousarray(row_iv), np.ascontiguousarray(col_iv))
        self.N = row_iv.shape[0] * col_iv.shape[0]

    def _masks_on(self, device):
        """The uint8 [N, 1, H, W] masks as a tensor on `device` (built once; the native path never asks)."""
        if self._masks_t is None or self._masks_t.device != torch.device(device):
            from . import sbsm
            m = self._masks_np if self._masks_np is not None else sbsm.masks_from_intervals(*self._intervals, self.input_size)
            self._masks_t = torch.from_numpy(m).to(device)
            self._inv_t = self._count = None
        return self._masks_t

    @property
    def masks(self):
        if self._intervals is None and self._masks_np is None:
            return None
        return self._masks_t if self._masks_t is not None else self._masks_on(self._device())

    def generate_masks(self, window_size, stride, savepath="masks.npy"):
        from . import sbsm
        row_iv, col_iv = sbsm.window_intervals(self.input_size, window_size, stride)
        if savepath:
            np.save(savepath, sliding_window_masks(self.input_size, window_size, stride))
        if max(row_iv.shape[0], col_iv.shape[0]) <= sbsm.SBSM_MAX_WINDOWS:
            self._set_intervals(row_iv, col_iv)
        else:
            self._set_masks(sliding_window_masks(self.input_size, window_size, stride))
        self.window_size, self.stride = window_size, stride

    def load_masks(self, filepath):
        from . import sbsm
        masks = np.load(filepath)
        grid = sbsm.grid_of_masks(masks) if tuple(masks.shape[-2:]) == self.input_size else None
        if grid is not None:
            self._set_intervals(*grid)
        else:
            self._set_masks(masks)

    def _embed_masked(self, x):
        """Embeddings of mask n applied to image b, n-major like the reference's stack: row n * B + b."""
        b, c, h, w = x.shape
        out = []
        masks = self._masks_on(x.device)
        per = max(1, self.gpu_batch // b)                                   # masks per chunk
        for n0 in range(0, self.N, per):
            m = masks[n0:n0 + per].to(x.dtype)                              # [n, 1, H, W]
            chunk = (m[:, None] * x[None]).reshape(-1, c, h, w)             # [n * B, C, H, W]
            out.append(CausalMetric._embed(self.model, chunk))
        return torch.cat(out)

    def __call__(self, x_q, x=None):
        return self.forward(x_q, x)

    def _native_inputs(self, x_q, x):
        from . import sbsm
        return bool(self._intervals is not None and all(
            torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 and t.device == x.device
            and tuple(t.shape[2:]) == self.input_size and t.shape[0] >= 1 and t.shape[1] >= 1 for t in (x_q, x))
            and x[0, 0].numel() <= sbsm.SBSM_MAX_HW and x[0].numel() <= 1 << 30)                 # the kernels' limits

    @staticmethod
    def _native_rows(e):
        from . import sbsm
        return bool(torch.is_tensor(e) and e.is_cuda and e.dtype == torch.float32 and e.dim() == 2 and e.shape[0] >= 1
                    and 1 <= e.shape[1] <= sbsm.SBSM_MAX_D)

    def forward(self, x_q, x=None):
        self_sim = x is None
        if self_sim:
            x = x_q
        with torch.no_grad():
            e_q = CausalMetric._embed(self.model, x_q)
            if self._native_inputs(x_q, x) and self._native_rows(e_q):
                sal = self._forward_native(x, e_q, self_sim)
                if sal is not None:
                    self.last_native = True
                    return sal
            self.last_native = False
            return self._forward_torch(x, e_q, self_sim)

    def _forward_native(self, x, e_q, self_sim):
        """-> the saliency, or None when the model's outputs are not 2-d CUDA float32 rows (the torch path then serves)."""
        from . import sbsm
        b = x.shape[0]
        dev = x.device
        e_r = None
        if not self_sim:
            e_r = CausalMetric._embed(self.model, x)
            if not self._native_rows(e_r):
                return None
        if dev not in self._on:
            self._on[dev] = tuple(torch.from_numpy(iv).to(dev) for iv in self._intervals)
        row_iv, col_iv = self._on[dev]
        x = x.contiguous()
        total = self.N * b
        step = max(1, self.gpu_batch)
        buf = torch.empty((min(step, total),) + tuple(x.shape[1:]), dtype=torch.float32, device=dev)
        e_m = None
        for g0 in range(0, total, step):                                    # the reference's chunks [i, i + gpu_batch)
            n = min(step, total - g0)
            f = CausalMetric._embed(self.model, sbsm.sbsm_compose(x, row_iv, col_iv, g0, n, out=buf[:n]))
            if not self._native_rows(f) or f.shape[0] != n:
                return None
            if e_m is None:
                e_m = torch.empty((total, f.shape[1]), dtype=torch.float32, device=f.device)
            e_m[g0:g0 + n] = f
        e_q = e_q.contiguous()
        gain = sbsm.sbsm_gain(e_q, e_m, None if self_sim else e_r.contiguous())
        return sbsm.sbsm_accumulate(gain, row_iv.to(gain.device), col_iv.to(gain.device), self.input_size)

    def _forward_torch(self, x, e_q, self_sim):
        b = x.shape[0]
        h, w = self.input_size
        e_m = self._embed_masked(x).reshape(self.N, b, -1)                  # [N, B, D]
        if self._inv_t is None:
            inv = (1 - self._masks_t.reshape(self.N, -1)).float()           # [N, HW]: 1 inside the window
            self._inv_t = inv.t().contiguous()                              # [HW, N]
            self._count = inv.sum(dim=0)                                    # windows covering each pixel
        if self_sim:
            gain = torch.linalg.vector_norm(e_q[None] - e_m, dim=2).t()                 # [B, N]
        else:
            e_r = CausalMetric._embed(self.model, x)
            o_dist = torch.cdist(e_q, e_r).reshape(-1, 1)                               # [Q * B, 1]
            m_dist = torch.cdist(e_q, e_m.reshape(self.N * b, -1))                      # [Q, N * B]
            m_dist = m_dist.reshape(-1, self.N, b).permute(0, 2, 1).reshape(-1, self.N)
            gain = (m_dist - o_dist).clamp(min=0)                                       # [Q * B, N]
        sal = (gain.float() @ self._inv_t.t()) / self._count                            # [., HW]
        return sal.reshape(-1, h, w)


# SimCAM similarity saliency (explanations.py:664-976), native on the retrieval backbones: simcam.py
from .simcam import SimCAM, SimCAM_Densenet121, SimCAM_MedSigLIP  # noqa: E402,F401
# attention rollout (explanations.py:979-1147), native on MedSigLIP: rollout.py
from .rollout import AttentionRolloutMedSigLIP  # noqa: E402,F401
# Grad-CAM retrieval saliency (medsiglip_saliency.py:137-269), native on MedSigLIP: siglip_gradcam.py
from .siglip_gradcam import _compute_single_gradcam, compute_gradcam_saliency  # noqa: E402,F401
# SimAtt similarity-attention saliency (explanations.py:605-661), native on DenseNet121's flattened Sequential: simatt.py
from .simatt import SimAtt, simatt_maps, simatt_pairs  # noqa: E402,F401
# insertion / deletion curves of one query as one device job (evaluate_saliency.py:33-91), native on CUDA float32 images: insdel.py
from .insdel import GaussianBlur, InsDel, InsDelResult, insdel_curves  # noqa: E402,F401
# SBSM occlusion saliency on interval-described window sets (explanations.py:15-152), native on CUDA float32 images: sbsm.py
from .sbsm import grid_of_masks, sbsm_accumulate, sbsm_compose, sbsm_gain, window_intervals  # noqa: E402,F401


def get_transforms_medsiglip(img_size=224):
    """(None, val_transform) of compute_saliency.py:131-148 / evaluate_saliency.py:13-31, so the drivers'
    `_, tf = get_transforms_medsiglip(...)` runs as written: Resize(img_size + 32, BICUBIC) + CenterCrop(img_size) + ToTensor().
    (u / 255 - 0) / 1 is u / 255 bit for bit, so ToTensor alone is default_transform with mean 0 and std 1; batches are
    resized on the device (tf.batch).  The training transform is out of scope."""
    from .retriever import default_transform
    return None, default_transform(img_size, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), resize=img_size + 32, interpolation="bicubic")
