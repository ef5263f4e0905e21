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
    t = np.empty((k, hw), dtype=np.int64)
    for i in range(k):
        order = np.flip(np.argsort(sal[i], kind="stable"))
        rank = np.empty(hw, dtype=np.int64)
        rank[order] = np.arange(hw)
        t[i] = rank // int(step)
    return t.astype(np.int32)


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
    c = x64.shape[1]
    k = kernel2d.detach().cpu().double()
    return F.conv2d(x64, k.expand(c, 1, *k.shape).contiguous(), padding=k.shape[0] // 2, groups=c)


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
