"""float64 / numpy restatement of the insertion / deletion job (mirx.insdel), shared by tests/test_insdel_cpu.py and
tests/test_insdel_gpu.py.  Nothing here imports the code under test.

The tie rule is the documented one: pixels in the order np.flip(np.argsort(sal, kind="stable")) of the float32 map."""
import numpy as np
import torch
import torch.nn.functional as F

ULP32 = 2.0 ** -23


def steps_ref(sal, step):
    """sal [K, hw] float32 -> int32 [K, hw]: rank under the stable rule // step."""
    sal = np.asarray(sal, dtype=np.float32)
    k, hw = sal.shape
    order = np.flip(np.argsort(sal, axis=1, kind="stable"), axis=1)      # row by row, as np.flip(np.argsort(sal[i], kind="stable"))
    rank = np.empty((k, hw), dtype=np.int64)
    np.put_along_axis(rank, order, np.broadcast_to(np.arange(hw), (k, hw)), axis=1)
    return (rank // int(step)).astype(np.int32)


def saliency_maps(k, hw, seed):
    """name -> [k, hw] float32 tensor, different rows: random with a few ties, half tied at 0 (with a -0.0), a NaN and infinities,
    all equal."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    a = torch.rand(k, hw, generator=g)
    if hw > 2:
        a[:, hw // 3] = a[:, 0]
    out["random"] = a
    b = torch.rand(k, hw, generator=g)
    b[:, ::2] = 0.0
    b[:, (hw // 2) // 2 * 2] = -0.0
    out["half_zero"] = b
    c = torch.randn(k, hw, generator=g)
    c[:, hw // 2] = float("nan")
    if hw > 4:
        c[:, 1], c[:, 2], c[:, hw - 1] = float("inf"), -float("inf"), -float("nan")
    out["nan"] = c
    out["all_equal"] = torch.full((k, hw), 0.5) * torch.arange(1, k + 1)[:, None]
    return out


def tie_free(sal):
    sal = np.asarray(sal, dtype=np.float32)
    return all(np.unique(row).size == row.size and not np.isnan(row).any() for row in sal.reshape(sal.shape[0], -1))


def distinct_saliency(k, hw, seed):
    """[k, hw] float32 without two equal values in a row: a permutation of 0 .. hw - 1, scaled (hw < 2^24)."""
    g = torch.Generator().manual_seed(seed)
    sal = torch.stack([torch.randperm(hw, generator=g) for _ in range(k)]).float().numpy() / np.float32(hw)
    assert tie_free(sal)
    return sal


def compose_ref(t, bank, start, finish, row, n_steps, g0, n):
    """torch.where restatement of mirx_insdel_compose on the tensors' device: -> [n, 3, hw]."""
    hw = t.shape[1]
    bank_z = torch.cat([bank, torch.zeros((1, 3, hw), dtype=bank.dtype, device=bank.device)])     # index -1
    g = torch.arange(g0, g0 + n, device=t.device)
    j, s = g // (n_steps + 1), g % (n_steps + 1)
    mask = t[row.long()[j]][:, None, :] < s[:, None, None]
    return torch.where(mask, bank_z[finish.long()[j]], bank_z[start.long()[j]])


def blur_f64(x, kernel2d):
    """Zero-padded cross-correlation of every plane of x [n, c, h, w] with kernel2d, in float64 (CPU)."""
    x64 = x.detach().cpu().double()
    k = kernel2d.detach().cpu().double()
    klen, pad = k.shape[0], k.shape[0] // 2
    h, w = x64.shape[2:]
    xp = F.pad(x64, (pad, pad, pad, pad))
    acc = torch.zeros_like(x64)
    for ky in range(klen):                                  # the definition, tap by tap in (ky, kx) order: klen^2 whole-image
        for kx in range(klen):                              # updates, many times faster on a CPU than a float64 F.conv2d
            acc.add_(xp[:, :, ky:ky + h, kx:kx + w], alpha=float(k[ky, kx]))
    return acc


def ulp32_of(v):
    """The spacing of float32 at |v| for float64 v (numpy): 2^(floor(log2 |v|) - 23), the subnormal spacing 2^-149 below 2^-126.
    Taken from the float64 value itself, so a value just under a power of two keeps the smaller spacing."""
    v = np.abs(np.asarray(v, dtype=np.float64))
    _, e = np.frexp(v)                                                    # |v| = m * 2^e with m in [0.5, 1)
    return np.ldexp(1.0, np.where(v == 0.0, -149, np.maximum(e - 24, -149)))


def blur_pixel_bound(x, kernel2d, exp64):
    """Per pixel, what "the correctly rounded sum up to klen^2 * 2^-53"  allows between the kernel and blur_f64:
    0.5 ulp32(f64 value) + 2 * klen^2 * 2^-53 * (|k| * |x|), the last factor the float64 correlation of the absolute values.
    Either float64 sum of klen^2 exact products is within klen^2 * 2^-53 * sum|k x| of the true value whatever its order
    (hence the 2); the rounding to float32 adds half a float32 ulp.  No measured number enters.  -> float64 tensor like exp64."""
    klen = kernel2d.shape[0]
    mag = blur_f64(x.detach().cpu().abs(), kernel2d.detach().cpu().abs())
    return 0.5 * torch.from_numpy(ulp32_of(exp64.numpy())) + 2.0 * klen * klen * 2.0 ** -53 * mag


def blur_pixel_excess(got, x, kernel2d, exp64):
    """max over the pixels of |got - f64| / blur_pixel_bound (<= 1 passes), and the flat index of that pixel."""
    ratio = (got.detach().cpu().double() - exp64).abs() / blur_pixel_bound(x, kernel2d, exp64)
    return float(ratio.max()), int(ratio.argmax())


def image_errors(got, exp64):
    """max|got - f64| / max|f64| per image."""
    got, exp64 = got.detach().cpu().double(), exp64.detach().cpu().double()
    return [float((got[i] - exp64[i]).abs().max() / exp64[i].abs().max()) for i in range(exp64.shape[0])]


def curves_ref(q, r, curves, n_steps):
    """numpy float64: cosine with each norm clamped at 1e-8, negatives counted and zeroed, auc."""
    q = np.asarray(q, dtype=np.float64).reshape(-1)
    r = np.asarray(r, dtype=np.float64)
    cos = (r @ q) / (max(np.linalg.norm(q), 1e-8) * np.maximum(np.linalg.norm(r, axis=1), 1e-8))
    cos = cos.reshape(curves, n_steps + 1)
    zero = np.count_nonzero(cos < 0, axis=1).astype(np.int64)
    scores = np.where(cos < 0, 0.0, cos)
    auc = (scores.sum(axis=1) - scores[:, 0] / 2 - scores[:, -1] / 2) / n_steps
    return scores, auc, zero


def insdel_ref(embed, x_q, x_r, saliency, step, modes, substrates, max_batch):
    """The whole job restated: embed = tensor -> [n, D] tensor; images are built in numpy, embedded in chunks of max_batch flat
    images (the chunking the code under test documents) and scored in float64.
    -> auc [K, M], scores [K, M, n_steps + 1], zero_counter [K, M]."""
    k, _, s, _ = x_r.shape
    hw = s * s
    n_steps = (hw + step - 1) // step
    per = n_steps + 1
    t = steps_ref(np.asarray(saliency, dtype=np.float32).reshape(k, hw), step)
    imgs = []
    for i in range(k):
        hit = x_r[i:i + 1]
        for mode in modes:
            sub = substrates[mode](hit)
            start, finish = (hit, sub) if mode == "del" else (sub, hit)
            start, finish = start.reshape(3, hw).numpy(), finish.reshape(3, hw).numpy()
            for st in range(per):
                imgs.append(np.where(t[i][None, :] < st, finish, start))
    imgs = torch.from_numpy(np.stack(imgs)).reshape(-1, 3, s, s).to(x_r.dtype)
    with torch.no_grad():
        q = embed(x_q)
        r = torch.cat([embed(imgs[lo:lo + max_batch]) for lo in range(0, imgs.shape[0], max_batch)])
    scores, auc, zero = curves_ref(q.numpy(), r.numpy(), k * len(modes), n_steps)
    m = len(modes)
    return auc.reshape(k, m), scores.reshape(k, m, per), zero.reshape(k, m)
