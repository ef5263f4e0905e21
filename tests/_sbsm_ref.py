"""float64 numpy restatement of the reference's SBSM saliency (explanations.py:75-79 weighted_avg, 105-152 SBSMBatch.forward),
taken from given embeddings.  It keeps the reference's K-tensor form: the mask tensor (1 - masks) times the gains, summed over
the masks (an einsum, evaluated in blocks of masks so that the float64 copy of the masks stays small), divided by the count
N - masks.sum(0).  Shared by tests/test_sbsm_cpu.py and tests/test_sbsm_gpu.py; it touches no mirx code."""
import numpy as np

GEOMETRIES = [                   # (H, W, window, stride), the smallest at which each hazard shows
    (21, 27, 8, 3),              # H * W odd: unaligned image bases; clipped at all four borders; N = 99
    (32, 40, 24, 5),             # the drivers' window / stride ratio, non-square; N = 132
    (22, 30, 5, 7),              # stride > window: 1080 uncovered pixels are NaN; N = 12
    (9, 50, 24, 16),             # window taller than the image; N = 8
]


def sliding_window_masks(input_size, window_size, stride):
    """explanations.py:36-63: uint8 [N, 1, H, W], 1 outside the window, 0 inside."""
    h, w = input_size
    rows = np.arange(0 + stride - window_size, h, stride)
    cols = np.arange(0 + stride - window_size, w, stride)
    masks = np.ones((len(rows) * len(cols), h, w), dtype=np.uint8)
    i = 0
    for r in rows:
        for c in cols:
            masks[i, max(r, 0):min(r + window_size, h), max(c, 0):min(c + window_size, w)] = 0
            i += 1
    return masks.reshape(-1, 1, h, w)


def masks_of_intervals(row_iv, col_iv, input_size):
    """uint8 [nr * nc, 1, H, W] from half-open intervals: mask i * nc + j is 0 on rows row_iv[i] x columns col_iv[j], 1 elsewhere."""
    h, w = input_size
    masks = np.ones((len(row_iv) * len(col_iv), h, w), dtype=np.uint8)
    n = 0
    for r0, r1 in np.asarray(row_iv):
        for c0, c1 in np.asarray(col_iv):
            masks[n, r0:r1, c0:c1] = 0
            n += 1
    return masks.reshape(-1, 1, h, w)


def cdist(a, b):
    """Euclidean distances [len(a), len(b)] in float64, the direct form."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.sqrt(((a[:, None, :] - b[None, :, :]) ** 2).sum(axis=2))


def gain(e_q, e_m, e_r=None):
    """explanations.py:136-149 up to the product with the masks: e_q [Q, D], e_m [N * B, D] (row n * B + b), e_r [B, D] or
    None -> float64 [B, N] (self-similarity) or [Q * B, N]."""
    e_q, e_m = np.asarray(e_q, dtype=np.float64), np.asarray(e_m, dtype=np.float64)
    if e_r is None:
        b = e_q.shape[0]
        m = e_m.reshape(-1, b, e_q.shape[1]).transpose(1, 0, 2)                       # [B, N, D]
        return np.sqrt(((e_q[:, None, :] - m) ** 2).sum(axis=2))
    b = np.asarray(e_r).shape[0]
    n = e_m.shape[0] // b
    o_dist = cdist(e_q, e_r).reshape(-1, 1)
    m_dist = cdist(e_q, e_m).reshape(-1, n, b).transpose(0, 2, 1).reshape(-1, n)
    return np.maximum(m_dist - o_dist, 0.0)                                             # clamp(min=0): a NaN stays


def weighted_avg(masks, g, block=128):
    """K = (1 - masks) * gain summed over the masks, over count = N - masks.sum(0): masks uint8 [N, 1, H, W], g float64
    [rows, N] -> float64 [rows, H, W]; 0 / 0 = NaN where no window covers."""
    m = np.asarray(masks).reshape(masks.shape[0], *masks.shape[-2:])
    n = m.shape[0]
    g = np.asarray(g, dtype=np.float64)
    total = np.zeros((g.shape[0],) + m.shape[1:], dtype=np.float64)
    for n0 in range(0, n, block):
        inv = 1.0 - m[n0:n0 + block].astype(np.float64)
        total += np.einsum("rn,nhw->rhw", g[:, n0:n0 + block], inv)
    count = n - m.sum(axis=0, dtype=np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return total / count


def saliency(masks, e_q, e_m, e_r=None):
    return weighted_avg(masks, gain(e_q, e_m, e_r))


def ulp_diff32(a, b):
    """Largest distance in float32 units in the last place between two float32 arrays of finite values of one sign pattern
    (monotone integer images of the bit patterns)."""
    def key(v):
        i = np.ascontiguousarray(v, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return int(np.abs(key(a) - key(b)).max()) if np.size(a) else 0
