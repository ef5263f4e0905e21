"""float64 restatement of ResNet-50 (torchvision layout: stride on conv2, eval BatchNorm) for the ResNet50 tests, written
with F.conv2d / F.batch_norm / F.max_pool2d from the published definition -- independent of mirx.model's module tree."""
import torch
import torch.nn.functional as F

LAYERS = (3, 4, 6, 3)


def bn(x, sd, pre):
    return F.batch_norm(x, sd[pre + ".running_mean"].double(), sd[pre + ".running_var"].double(), sd[pre + ".weight"].double(),
                        sd[pre + ".bias"].double(), training=False, eps=1e-5)


def features(x, sd):
    """x [B, 3, H, W] -> [B, 2048] (global average pool of layer4, before any fc / normalisation), float64."""
    sd = {k: v.detach().cpu() for k, v in sd.items()}
    x = x.double().cpu()
    x = F.conv2d(x, sd["resnet50.0.weight"].double(), stride=2, padding=3)
    x = F.relu(bn(x, sd, "resnet50.1"))
    x = F.max_pool2d(x, 3, stride=2, padding=1)
    for li, nb in enumerate(LAYERS):
        for j in range(nb):
            p = f"resnet50.{4 + li}.{j}"
            s = 2 if (li > 0 and j == 0) else 1
            y = F.relu(bn(F.conv2d(x, sd[p + ".conv1.weight"].double()), sd, p + ".bn1"))
            y = F.relu(bn(F.conv2d(y, sd[p + ".conv2.weight"].double(), stride=s, padding=1), sd, p + ".bn2"))
            y = bn(F.conv2d(y, sd[p + ".conv3.weight"].double()), sd, p + ".bn3")
            if p + ".downsample.0.weight" in sd:
                idt = bn(F.conv2d(x, sd[p + ".downsample.0.weight"].double(), stride=s), sd, p + ".downsample.1")
            else:
                idt = x
            x = F.relu(y + idt)
    return x.mean(dim=(2, 3))


def embed(x, sd):
    """The reference forward(): features -> (fc) -> F.normalize, float64."""
    f = features(x, sd)
    if "fc.weight" in sd:
        f = f @ sd["fc.weight"].detach().cpu().double().t() + sd["fc.bias"].detach().cpu().double()
    return F.normalize(f, dim=1)
