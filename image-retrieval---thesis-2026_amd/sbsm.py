"""SBSM sliding-window occlusion saliency on interval-described window sets.

Mirrors (paths into the reference):
  SBSM.generate_masks             explanations.py:22-68 (the window geometry)
  SBSM.weighted_avg               explanations.py:75-79
  SBSMBatch.forward               explanations.py:105-152

The reference keeps its N masks as a uint8 [N, 1, H, W] tensor, multiplies all of them into a [N * B, C, H, W] stack and sums an
[H, W, B, N] tensor.  The masks of a sliding-window set are the outer product of nr row intervals and nc column intervals, so two
small int32 arrays describe them: mask n = i * nc + j zeroes row_iv[i] x col_iv[j].  The three kernels of csrc/k_sbsm.hip work
from those arrays: mirx_sbsm_compose writes a chunk of the masked images, mirx_sbsm_gain turns embeddings into fp64 distance
gains, mirx_sbsm_accumulate sums the gains of the windows that cover each pixel.  `mirx.xai.SBSMBatch` drives them.
"""
import numpy as np
import torch

from . import _lib

SBSM_MAX_HW = 1 << 20          # include/mirx.h MIRX_SBSM_MAX_HW
SBSM_MAX_WINDOWS = 4096        # MIRX_SBSM_MAX_WINDOWS: nr and nc, each
SBSM_MAX_D = 16384             # MIRX_SBSM_MAX_D


def _ptr(t):
    import ctypes
    return ctypes.c_void_p(t.data_ptr() if t is not None else None)


def _stream(dev):
    import ctypes
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


# ---- window geometry (host) -------------------------------------------------------------------------------------------------
def window_intervals(input_size, window_size, stride):
    """explanations.py:36-63 as intervals: windows start at stride - window_size and step by stride, clipped at the borders.
    -> (row_iv [nr, 2], col_iv [nc, 2]) numpy int32, half-open; mask i * nc + j zeroes row_iv[i] x col_iv[j]."""
    h, w = (int(v) for v in input_size)
    window_size, stride = int(window_size), int(stride)
    if h < 1 or w < 1 or window_size < 1 or stride < 1:
        raise ValueError(f"window_intervals: input_size, window_size and stride must be >= 1 (got {input_size}, {window_size}, "
                         f"{stride})")

    def axis(size):
        start = np.arange(stride - window_size, size, stride)
        return np.stack([np.maximum(start, 0), np.minimum(start + window_size, size)], axis=1).astype(np.int32)
    return axis(h), axis(w)


def masks_from_intervals(row_iv, col_iv, input_size):
    """The uint8 [N, 1, H, W] masks the intervals stand for (1 outside the window, 0 inside)."""
    h, w = input_size
    rin = (np.arange(h)[None] >= row_iv[:, :1]) & (np.arange(h)[None] < row_iv[:, 1:])       # [nr, H]
    cin = (np.arange(w)[None] >= col_iv[:, :1]) & (np.arange(w)[None] < col_iv[:, 1:])       # [nc, W]
    inside = rin[:, None, :, None] & cin[None, :, None, :]                                    # [nr, nc, H, W]
    return (~inside).astype(np.uint8).reshape(-1, 1, h, w)


def check_intervals(row_iv, col_iv, input_size):
    """Raise ValueError unless both arrays are int32 [n, 2] with 1 <= n <= 4096 and every interval is non-empty and inside
    the image.  (The entry points cannot check this: they never read the device arrays.)"""
    h, w = input_size
    for name, iv, size in (("row_iv", row_iv, h), ("col_iv", col_iv, w)):
        iv = np.asarray(iv)
        if iv.dtype != np.int32 or iv.ndim != 2 or iv.shape[1] != 2 or not 1 <= iv.shape[0] <= SBSM_MAX_WINDOWS:
            raise ValueError(f"sbsm: {name} must be int32 [n, 2] with 1 <= n <= {SBSM_MAX_WINDOWS} (got {iv.dtype} {iv.shape})")
        if (iv[:, 0] < 0).any() or (iv[:, 1] > size).any() or (iv[:, 0] >= iv[:, 1]).any():
            raise ValueError(f"sbsm: every {name} interval must be non-empty and inside [0, {size})")


def grid_of_masks(masks):
    """The intervals of a mask array ([N, 1, H, W] or [N, H, W], values 0 / 1) when it is a window grid, else None.  A grid:
    N = nr * nc and mask i * nc + j equals 1 - outer(row interval i, column interval j), both non-empty; nr, nc <= 4096."""
    m = np.asarray(masks)
    if m.ndim == 4 and m.shape[1] == 1:
        m = m[:, 0]
    if m.ndim != 3 or m.shape[0] < 1 or m.shape[1] < 1 or m.shape[2] < 1 or m.dtype.kind not in "biu":
        return None
    n, h, w = m.shape
    if m.dtype.kind != "b" and (m.max() > 1 or m.min() < 0):
        return None
    zero = m == 0
    rows_any, cols_any = zero.any(axis=2), zero.any(axis=1)                     # [N, H], [N, W]
    area = zero.sum(axis=(1, 2), dtype=np.int64)
    iv = []
    for hit, size in ((rows_any, h), (cols_any, w)):
        lo = hit.argmax(axis=1)
        hi = size - hit[:, ::-1].argmax(axis=1)
        if not hit.any(axis=1).all() or (hit.sum(axis=1) != hi - lo).any():     # empty, or not one run
            return None
        iv.append(np.stack([lo, hi], axis=1).astype(np.int32))
    riv, civ = iv
    # a zero set inside its bounding box with the box's area is the box
    if (area != (riv[:, 1] - riv[:, 0]).astype(np.int64) * (civ[:, 1] - civ[:, 0])).any():
        return None
    for nc in range(1, n + 1):
        if n % nc:
            continue
        nr = n // nc
        if nr > SBSM_MAX_WINDOWS or nc > SBSM_MAX_WINDOWS:
            continue
        r3, c3 = riv.reshape(nr, nc, 2), civ.reshape(nr, nc, 2)
        if (r3 == r3[:, :1]).all() and (c3 == c3[:1]).all():
            return np.ascontiguousarray(r3[:, 0]), np.ascontiguousarray(c3[0])
    return None


# ---- kernel wrappers --------------------------------------------------------------------------------------------------------
# Arguments are checked in a fixed order -- type, dtype, rank, layout, sizes, ranges and only then the device -- so that every
# rule but the last can be exercised without a GPU; nothing is loaded or launched before all of them hold.
_DT = {torch.float32: "float32", torch.float64: "float64", torch.int32: "int32"}


def _check_tensor(what, name, t, dtype, rank):
    if not torch.is_tensor(t):
        raise ValueError(f"{what}: {name} must be a tensor (got {type(t).__name__})")
    if t.dtype != dtype:
        raise ValueError(f"{what}: {name} must be {_DT[dtype]} (got {t.dtype})")
    if t.dim() != rank:
        raise ValueError(f"{what}: {name} must be {rank}-d (got {tuple(t.shape)})")
    if not t.is_contiguous():
        raise ValueError(f"{what}: {name} must be contiguous")


def _check_iv(what, row_iv, col_iv):
    for name, iv in (("row_iv", row_iv), ("col_iv", col_iv)):
        _check_tensor(what, name, iv, torch.int32, 2)
        if iv.shape[1] != 2 or not 1 <= iv.shape[0] <= SBSM_MAX_WINDOWS:
            raise ValueError(f"{what}: {name} must be [n, 2] with 1 <= n <= {SBSM_MAX_WINDOWS} (got {tuple(iv.shape)})")
    return row_iv.shape[0], col_iv.shape[0]


def _check_device(what, *tensors):
    """Last rule: CUDA tensors on one device."""
    if not all(t.is_cuda for t in tensors):
        raise ValueError(f"{what}: the tensors must be CUDA tensors (there is no CPU path)")
    if any(t.device != tensors[0].device for t in tensors):
        raise ValueError(f"{what}: the tensors must be on one device")


def sbsm_compose(x, row_iv, col_iv, g0, n, out=None):
    """[HIP] mirx_sbsm_compose: x [B, C, H, W] CUDA fp32 -> images [g0, g0 + n) of the n-major job list (image g = mask g // B on
    image g % B) as [n, C, H, W]; bit-identical to masks.float() * x."""
    _check_tensor("sbsm_compose", "x", x, torch.float32, 4)
    nr, nc = _check_iv("sbsm_compose", row_iv, col_iv)
    b, c, h, w = x.shape
    if b < 1 or c < 1 or not 1 <= h * w <= SBSM_MAX_HW or c * h * w > 1 << 30:
        raise ValueError(f"sbsm_compose: needs B, C >= 1, 1 <= H * W <= 2^20 and C * H * W <= 2^30 (got {tuple(x.shape)})")
    try:
        g0, n = int(g0), int(n)
    except (TypeError, ValueError):
        raise ValueError("sbsm_compose: g0 and n must be integers") from None
    if g0 < 0 or n < 0 or g0 + n > nr * nc * b:
        raise ValueError(f"sbsm_compose: [g0, g0 + n) = [{g0}, {g0 + n}) outside the job's {nr * nc} x {b} images")
    if out is not None:
        _check_tensor("sbsm_compose", "out", out, torch.float32, out.dim() if torch.is_tensor(out) else 4)
        if out.numel() != n * c * h * w:
            raise ValueError(f"sbsm_compose: out must hold {n} x {c} x {h} x {w} elements (got {tuple(out.shape)})")
    _check_device("sbsm_compose", x, row_iv, col_iv, *(() if out is None else (out,)))
    if out is None:
        out = torch.empty((n, c, h, w), dtype=torch.float32, device=x.device)
    if n == 0:
        return out
    lib = _lib.load()
    with torch.cuda.device(x.device):
        _lib.check(lib.mirx_sbsm_compose(_ptr(x), b, c, h, w, _ptr(row_iv), nr, _ptr(col_iv), nc, g0, n, _ptr(out), _stream(x.device)),
                   "mirx_sbsm_compose")
    return out


def sbsm_gain(e_q, e_m, e_r=None):
    """[HIP] mirx_sbsm_gain: e_q [Q, D], e_m [N * B, D] (row n * B + b), e_r [B, D] or None, CUDA fp32 -> gain fp64 [rows, N].
    e_r None (self-similarity, B = Q): gain[b, n] = |e_q[b] - e_m[n B + b]|; else gain[q B + b, n] = max(|e_q[q] - e_m[n B + b]|
    - |e_q[q] - e_r[b]|, 0).  fp64 throughout."""
    rows_in = (("e_q", e_q), ("e_m", e_m)) + ((("e_r", e_r),) if e_r is not None else ())
    for name, a in rows_in:
        _check_tensor("sbsm_gain", name, a, torch.float32, 2)
    q, d = e_q.shape
    if any(a.shape[1] != d for _, a in rows_in):
        raise ValueError(f"sbsm_gain: the embeddings must share their width (got {[tuple(a.shape) for _, a in rows_in]})")
    b = q if e_r is None else e_r.shape[0]
    if not 1 <= d <= SBSM_MAX_D or q < 1 or b < 1 or e_m.shape[0] < b or e_m.shape[0] % b:
        raise ValueError(f"sbsm_gain: needs 1 <= D <= {SBSM_MAX_D}, Q, B >= 1 and e_m [N * B, D] with N >= 1 (got e_q "
                         f"{tuple(e_q.shape)}, e_m {tuple(e_m.shape)}, B = {b})")
    n_masks = e_m.shape[0] // b
    rows = b if e_r is None else q * b
    if rows * n_masks > 1 << 30 or e_m.shape[0] > 1 << 30:
        raise ValueError(f"sbsm_gain: rows * N and N * B must be <= 2^30 (got rows = {rows}, N = {n_masks}, B = {b})")
    _check_device("sbsm_gain", *(a for _, a in rows_in))
    lib = _lib.load()
    gain = torch.empty((rows, n_masks), dtype=torch.float64, device=e_q.device)
    with torch.cuda.device(e_q.device):
        _lib.check(lib.mirx_sbsm_gain(_ptr(e_q), q, _ptr(e_m), n_masks, b, _ptr(e_r), d, _ptr(gain), _stream(e_q.device)),
                   "mirx_sbsm_gain")
    return gain


def sbsm_accumulate(gain, row_iv, col_iv, input_size):
    """[HIP] mirx_sbsm_accumulate: gain fp64 [rows, nr * nc] CUDA -> sal fp32 [rows, H, W]: per pixel the mean gain of the windows
    that cover it (fp64 sums in a fixed order, one rounding); NaN where none does."""
    _check_tensor("sbsm_accumulate", "gain", gain, torch.float64, 2)
    nr, nc = _check_iv("sbsm_accumulate", row_iv, col_iv)
    try:
        h, w = (int(v) for v in input_size)
    except (TypeError, ValueError):
        raise ValueError("sbsm_accumulate: input_size must be (H, W)") from None
    if h < 1 or w < 1 or h * w > SBSM_MAX_HW:
        raise ValueError(f"sbsm_accumulate: needs 1 <= H * W <= 2^20 (got {h} x {w})")
    rows = gain.shape[0]
    if rows < 1 or gain.shape[1] != nr * nc or rows * nr * nc > 1 << 30:
        raise ValueError(f"sbsm_accumulate: gain must be [rows >= 1, {nr} * {nc}] with rows * N <= 2^30 (got {tuple(gain.shape)})")
    _check_device("sbsm_accumulate", gain, row_iv, col_iv)
    lib = _lib.load()
    n_ws = lib.mirx_sbsm_workspace_bytes(rows, nr, w)
    if n_ws < 0:
        _lib.check(int(n_ws), "mirx_sbsm_workspace_bytes")
    with torch.cuda.device(gain.device):
        ws = torch.empty((n_ws // 8,), dtype=torch.float64, device=gain.device)
        sal = torch.empty((rows, h, w), dtype=torch.float32, device=gain.device)
        _lib.check(lib.mirx_sbsm_accumulate(_ptr(gain), rows, _ptr(row_iv), nr, _ptr(col_iv), nc, h, w, _ptr(ws), n_ws, _ptr(sal),
                                            _stream(gain.device)), "mirx_sbsm_accumulate")
    return sal
