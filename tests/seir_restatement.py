"""CPU restatement of the SE-IR ResNet-101 encoder (IRBlock 3-4-23-3 with squeeze-and-excitation, 112 x 112 input) in
torch.nn.functional, on a state_dict with the reference's key names.  Shared by the host and GPU tests of the encoder."""
import torch
import torch.nn.functional as F

LAYERS = ((64, 3, 1), (128, 4, 2), (256, 23, 2), (512, 3, 2))


def _bn(sd, p, x):
    return F.batch_norm(x, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"], False, 0.0, 1e-5)


def se_gate(sd, p, t):
    """sigmoid(W2 . prelu(W1 . mean_hw(t) + b1) + b2) of one block, (N,C)."""
    y = t.mean(dim=(2, 3))
    y = F.prelu(F.linear(y, sd[p + ".fc.0.weight"], sd[p + ".fc.0.bias"]), sd[p + ".fc.1.weight"])
    return torch.sigmoid(F.linear(y, sd[p + ".fc.2.weight"], sd[p + ".fc.2.bias"]))


def seir101_forward(sd, x, taps=None, gates_one=False):
    """(N,3,112,112) -> (N,512) unit rows; `taps` (a dict) receives conv1 (before the pool), stem (after it),
    layer1..layer4 and bn3 (before the normalisation).  gates_one: every SE gate forced to 1 (the network without SE)."""
    sd = {k: torch.as_tensor(v) for k, v in sd.items()}
    keep = taps if taps is not None else {}
    with torch.no_grad():
        x = keep["conv1"] = F.prelu(_bn(sd, "bn1", F.conv2d(x, sd["conv1.weight"])), sd["prelu.weight"])
        x = keep["stem"] = F.max_pool2d(x, kernel_size=2, stride=2)
        for li, (planes, nblk, stride) in enumerate(LAYERS, start=1):
            for b in range(nblk):
                p = "layer%d.%d" % (li, b)
                st = stride if b == 0 else 1
                out = F.conv2d(_bn(sd, p + ".bn0", x), sd[p + ".conv1.weight"], padding=1)
                out = F.prelu(_bn(sd, p + ".bn1", out), sd[p + ".prelu.weight"])
                out = _bn(sd, p + ".bn2", F.conv2d(out, sd[p + ".conv2.weight"], stride=st, padding=1))
                if not gates_one:
                    out = out * se_gate(sd, p + ".se", out)[:, :, None, None]
                res = x
                if (p + ".downsample.0.weight") in sd:
                    res = _bn(sd, p + ".downsample.1", F.conv2d(x, sd[p + ".downsample.0.weight"], stride=st))
                x = F.prelu(out + res, sd[p + ".prelu.weight"])
            keep["layer%d" % li] = x
        x = _bn(sd, "bn2", x)
        x = F.linear(x.reshape(x.size(0), -1), sd["fc.weight"], sd["fc.bias"])
        x = keep["bn3"] = F.batch_norm(x, sd["bn3.running_mean"], sd["bn3.running_var"], sd["bn3.weight"], sd["bn3.bias"],
                                       False, 0.0, 1e-5)
        return F.normalize(x, p=2, dim=1)
