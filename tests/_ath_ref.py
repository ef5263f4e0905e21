"""Float64 restatement of the reference's ATHNet (ath_model.py there) on a state dict, and the Hamming ranking oracle.

`forward(sd, x)` reads nothing but the state dict (eval-mode BatchNorm) and runs F.conv2d / F.max_pool2d / F.avg_pool2d / F.linear
in float64.  `hamming_topk(q, g, k, exclude)` is a stable sort of (distance, id) on the CPU: ties go to the lowest id.
`fixture_state_dict` / `fixture_images` decode the compact storage of tests/golden/ath_ref.npz (make_golden_ath.py)."""
import numpy as np
import torch
import torch.nn.functional as F


def _bn(sd, p, x):
    return F.batch_norm(x, sd[p + ".running_mean"].double(), sd[p + ".running_var"].double(), sd[p + ".weight"].double(),
                        sd[p + ".bias"].double(), False, 0.0, 1e-5)


def _resblock(sd, p, x, stride):
    w = lambda k: sd[f"{p}.{k}.weight"].double()      # noqa: E731
    h = F.relu(_bn(sd, p + ".net.1", F.conv2d(x, w("net.0"), stride=stride, padding=1)))
    h = _bn(sd, p + ".net.4", F.conv2d(h, w("net.3"), padding=1))
    d = _bn(sd, p + ".downsample.1", F.conv2d(x, w("downsample.0"), stride=stride, padding=1))
    return F.relu(h + d)


def forward(sd, x):
    """-> (hash codes, logits) in float64."""
    sd = {k: torch.as_tensor(v) for k, v in sd.items()}
    x = torch.as_tensor(x).double()
    x = F.max_pool2d(_resblock(sd, "net1.0", x, 2), 3, stride=1, padding=1)
    s = torch.cat([x.mean(dim=1, keepdim=True), x.max(dim=1, keepdim=True)[0]], dim=1)
    x = torch.sigmoid(F.conv2d(s, sd["sa.conv.weight"].double(), padding=1)) * x
    x = F.avg_pool2d(_resblock(sd, "net2.0", x, 2), 3, stride=1, padding=1, count_include_pad=True)
    x = _resblock(sd, "dense", x, 2).flatten(1)
    return (F.linear(x, sd["hashlayer.weight"].double(), sd["hashlayer.bias"].double()),
            F.linear(x, sd["typelayer.weight"].double(), sd["typelayer.bias"].double()))


def hamming_topk(q, g, k, exclude=None):
    """q [Q, bits], g [N, bits] 0/1 -> (dist int32 [Q, k], ids int64 [Q, k]) by (distance, id)."""
    q = np.asarray(q).astype(np.uint8)
    g = np.asarray(g).astype(np.uint8)
    qp, gp = np.packbits(q, axis=1), np.packbits(g, axis=1)
    table = np.array([bin(i).count("1") for i in range(256)], dtype=np.int32)
    dist = np.empty((q.shape[0], k), dtype=np.int32)
    ids = np.empty((q.shape[0], k), dtype=np.int64)
    for i in range(q.shape[0]):
        d = table[np.bitwise_xor(gp, qp[i][None, :])].sum(axis=1)
        order = np.argsort(d, kind="stable")
        if exclude is not None:
            order = order[order != int(exclude[i])]
        dist[i], ids[i] = d[order[:k]], order[:k]
    return dist, ids


SD_SCALE = 4096.0          # floating state-dict entries are stored as int16 multiples of 2^-12 (exact in float32 and float64)


def fixture_state_dict(z, m):
    """State dict of fixture model m (float64 tensors, integer buffers as stored)."""
    p = f"{m}__sd__"
    out = {}
    for k in z.files:
        if k.startswith(p):
            v = z[k]
            out[k[len(p):]] = torch.from_numpy(v.astype(np.float64) / SD_SCALE if v.dtype == np.int16 else v)
    return out


def fixture_images(z, m):
    """Images of fixture model m as float32 [B, 3, S, S]: 16 levels v / 15, stored two pixels per byte (low nibble first)."""
    packed = z[f"{m}_x4"]
    v = np.empty(packed.shape[:-1] + (2 * packed.shape[-1],), dtype=np.uint8)
    v[..., 0::2] = packed & 15
    v[..., 1::2] = packed >> 4
    return torch.from_numpy(v.astype(np.float32) / np.float32(15))
