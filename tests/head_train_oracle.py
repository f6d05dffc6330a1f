"""Shared by tests/test_gpu_head_train.py: the float64 CPU oracle of one head-training run -- what the reference calls
for iresnet100(freeze_weights=True) under ClassificationTrainer (trainer/classification_trainer.py:13-21): nn.Linear(512, C)
+ F.log_softmax + F.nll_loss + torch.optim.Adam -- and the seeded inputs of the step-parity cases."""
import torch
import torch.nn.functional as F

CASES = ((7, 1), (7, 3), (17, 5), (1020, 37), (1020, 64))    # (C, B): below one class tile, below one K step, both tails, the reference's size
STEPS = 6
LR, WEIGHT_DECAY = 1e-3, 1e-4
SEED = 0          # chosen on the CPU: the first seed at which every oracle row's top-two logit gap exceeds MIN_GAP in all of CASES
MIN_GAP = 1e-4


def case_inputs(c, b, seed=SEED, steps=STEPS):
    """(W (C,512), bias (C), [(features (B,512), target (B,))] * steps), fp32 / int64, from ONE generator in this order."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(c, 512, generator=g) * 0.04
    bias = torch.randn(c, generator=g) * 0.04
    batches = []
    for _ in range(steps):
        f = torch.randn(b, 512, generator=g)
        batches.append((f, torch.randint(0, c, (b,), generator=g)))
    return w, bias, batches


def oracle_run(w, bias, batches, lr=LR, weight_decay=WEIGHT_DECAY, betas=(0.9, 0.999), eps=1e-8):
    """Train on `batches` in float64.  Returns dict(loss [per step], hits [per step], gap (smallest top-two logit gap of
    any row), weight, bias, exp_avg_sq_weight, exp_avg_sq_bias) -- tensors float64."""
    lin = torch.nn.Linear(512, w.shape[0]).double()
    with torch.no_grad():
        lin.weight.copy_(w.double())
        lin.bias.copy_(bias.double())
    opt = torch.optim.Adam(lin.parameters(), lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
    losses, hits, gap = [], [], float("inf")
    for f, t in batches:
        opt.zero_grad()
        z = lin(f.double())
        loss = F.nll_loss(F.log_softmax(z, dim=1), t)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
        hits.append(int((z.argmax(dim=1) == t).sum()))
        if z.shape[1] > 1:
            top = torch.topk(z.detach(), 2, dim=1).values
            gap = min(gap, float((top[:, 0] - top[:, 1]).min()))
    return {"loss": losses, "hits": hits, "gap": gap, "weight": lin.weight.detach().clone(), "bias": lin.bias.detach().clone(),
            "exp_avg_sq_weight": opt.state[lin.weight]["exp_avg_sq"].clone(), "exp_avg_sq_bias": opt.state[lin.bias]["exp_avg_sq"].clone()}
