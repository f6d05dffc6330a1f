"""CPU restatement of the emotion network (ResNet-50 Bottleneck 3-4-6-3 with the fc and proj heads) in
torch.nn.functional, on a state_dict with the reference's key names.  Shared by the host and GPU emotion tests."""
import torch
import torch.nn.functional as F

LAYERS = ((64, 3, 1), (128, 4, 2), (256, 6, 2), (512, 3, 2))


def _bn(sd, p, x):
    return F.batch_norm(x, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"], False, 0.0, 1e-5)


def rn50_2b_forward(sd, x, taps=None):
    """(x_cls, x_proj); `taps` (a dict) receives stem, maxpool, layer1..layer4 and avgpool."""
    sd = {k: torch.as_tensor(v) for k, v in sd.items()}
    keep = taps if taps is not None else {}
    with torch.no_grad():
        x = keep["stem"] = F.relu(_bn(sd, "bn1", F.conv2d(x, sd["conv1.weight"], stride=2, padding=3)))
        x = keep["maxpool"] = F.max_pool2d(x, kernel_size=3, stride=2, padding=1)
        for li, (planes, nblk, stride) in enumerate(LAYERS, start=1):
            for b in range(nblk):
                p = "layer%d.%d" % (li, b)
                st = stride if b == 0 else 1
                out = F.relu(_bn(sd, p + ".bn1", F.conv2d(x, sd[p + ".conv1.weight"])))
                out = F.relu(_bn(sd, p + ".bn2", F.conv2d(out, sd[p + ".conv2.weight"], stride=st, padding=1)))
                out = _bn(sd, p + ".bn3", F.conv2d(out, sd[p + ".conv3.weight"]))
                res = x
                if b == 0:
                    res = _bn(sd, p + ".downsample.1", F.conv2d(x, sd[p + ".downsample.0.weight"], stride=st))
                x = F.relu(out + res)
            keep["layer%d" % li] = x
        x = keep["avgpool"] = F.avg_pool2d(x, 7, stride=1)
        x = x.view(x.size(0), -1)
        return F.linear(x, sd["fc.weight"], sd["fc.bias"]), F.linear(x, sd["proj.weight"], sd["proj.bias"])
