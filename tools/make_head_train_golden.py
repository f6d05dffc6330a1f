#!/usr/bin/env python3
"""Generate tests/golden/head_train_ref.json by RUNNING THE REFERENCE (the checkout tools/make_golden.py's REF names),
through the import shim tools/make_heads_golden.py uses.  The tests read only the written file.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_head_train_golden.py

The reference's head-training case (cfg/train_cfg_img_classify.json, some_models[0]): iresnet100(n_classes=12,
freeze_weights=True) under torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-4), one optimisation step of
trainer/classification_trainer.py:13-21 on a batch of 2 on the CPU, then the checkpoint dict BaseTrainer.save_checkpoint
(trainer/base_trainer.py:83-105) would write.  Recorded: the number of parameters in the optimizer's group, the indices
that carry state, the keys of a state entry, of the group and of the checkpoint, and the model's type name -- the
layout trainer.TrainableHead writes.  Only those names and counts are written: no weights, no reference text."""
import importlib
import json
import os
import sys
import types
from pathlib import Path

import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

from make_golden import OUT, REF, install_shim, ref, seeded_normal  # noqa: E402


def main():
    install_shim()
    torch.manual_seed(0)
    model = ref("iresnet_encoder").iresnet100(pretrained=False, n_classes=12, freeze_weights=True)
    optimizer = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-4)
    model.train()                                         # classification_trainer.py:10
    optimizer.zero_grad()
    loss = F.nll_loss(model(seeded_normal((2, 3, 112, 112), 5000)), torch.tensor([3, 7]))
    loss.backward()
    optimizer.step()
    osd = optimizer.state_dict()
    names = [n for n, _ in model.named_parameters()]
    # the checkpoint dict, from the reference's own save_checkpoint with torch.save intercepted (260 MB are not written)
    for name in ("matplotlib", "matplotlib.pyplot"):      # utils imports them, never used on this path
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.path.insert(0, REF)
    pkg = types.ModuleType("trainer")                     # bypass the package __init__ (torchvision models / imgaug)
    pkg.__path__ = [os.path.join(REF, "trainer")]
    sys.modules["trainer"] = pkg
    base = importlib.import_module("trainer.base_trainer").BaseTrainer
    saved = {}
    stub = types.SimpleNamespace(model=model, optimizer=optimizer, mnt_best=float(loss.detach()), config={}, save_dir=Path("."),
                                 logger=types.SimpleNamespace(info=lambda *a, **k: None))
    keep, torch.save = torch.save, lambda state, path: saved.update(state)
    try:
        base.save_checkpoint(stub, 1, False)
    finally:
        torch.save = keep
    state_idx = sorted(int(k) for k in osd["state"])
    out = {
        "model": "iresnet100(n_classes=12, freeze_weights=True)",
        "arch": saved["arch"], "type_name": type(model).__name__,
        "P": len(osd["param_groups"][0]["params"]), "params_are_range": osd["param_groups"][0]["params"] == list(range(len(names))),
        "state_indices": state_idx, "state_names": [names[i] for i in state_idx],
        "state_entry_keys": sorted(osd["state"][state_idx[0]]),
        "group_keys": sorted(osd["param_groups"][0]),
        "checkpoint_keys": list(saved),
        "n_state_dict_keys": len(saved["state_dict"]),
    }
    with open(os.path.join(OUT, "head_train_ref.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(out)


if __name__ == "__main__":
    main()
