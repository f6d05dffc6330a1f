#!/usr/bin/env python3
"""Generate tests/golden/heads_ref.npz and tests/golden/eval_ref.json by RUNNING THE REFERENCE in the build container
(like tools/make_golden.py, whose import shim, seeded inputs and toy training case it reuses; /root/reference does not
exist on the GPU box).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_heads_golden.py [heads] [eval]

  heads  the reference's encoders WITH their classification head on this repository's generator weights (strict load),
         two seeded images each:
           irv1_7       InceptionResnetV1(pretrained=None, classify=True, num_classes=7)
           irv1_8631    InceptionResnetV1(pretrained=None, classify=True, num_classes=8631)   (the vggface2 width)
           ir100_1020   iresnet100(n_classes=1020, freeze_weights=True)
         The input seed of a case is the first for which, in every row, the two largest log-probabilities are >= 1e-2
         apart (a hundred times the parity gate), so the tests may ask for the identical argmax.
  eval   the reference's own ClassificationTrainer.eval(save_result=True) (trainer/base_trainer.py:177-200) on the toy
         embedding case of make_golden.mlp_train_case with the generator's MLP weights (the first weight seed with at
         least four rows right and four wrong): the logged loss and accuracy and the rows of result.csv (the file
         names without their scratch directory).

Only outputs are written: no weights, no reference text."""
import importlib
import json
import os
import shutil
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

from make_golden import OUT, REF, install_shim, ref, seeded_normal, write_mlp_train_case  # noqa: E402
from vn_celeb_face_recognition_amd.weights import generate_state_dict  # noqa: E402

MIN_GAP = 1e-2


def _separated(model, shape):
    for seed in range(64):
        x = seeded_normal(shape, 4000 + seed)
        with torch.no_grad():
            lp = model(x)
        top2 = torch.topk(lp, min(2, lp.shape[1]), dim=1).values
        gaps = (top2[:, 0] - top2[:, -1]) if lp.shape[1] > 1 else torch.full((lp.shape[0],), float("inf"))
        if bool((gaps >= MIN_GAP).all()):
            return 4000 + seed, lp, gaps
    raise AssertionError("no input seed with separated top-2 log-probabilities")


def golden_heads():
    import warnings
    warnings.filterwarnings("ignore", message="Implicit dimension choice")   # inception_resnet_v1.py:300 F.log_softmax(x)
    out = {}
    cases = []
    irv1 = ref("inception_resnet_v1").InceptionResnetV1
    for c in (7, 8631):
        m = irv1(pretrained=None, classify=True, num_classes=c).eval()
        m.load_state_dict(generate_state_dict("irv1", seed=0, as_torch=True, num_classes=c), strict=True)
        cases.append(("irv1_%d" % c, m, (2, 3, 160, 160)))
    m = ref("iresnet_encoder").iresnet100(pretrained=False, n_classes=1020, freeze_weights=True).eval()
    m.load_state_dict(generate_state_dict("iresnet100", seed=0, as_torch=True, n_classes=1020), strict=True)
    cases.append(("ir100_1020", m, (2, 3, 112, 112)))
    for key, m, shape in cases:
        seed, lp, gaps = _separated(m, shape)
        amax = lp.argmax(dim=1)
        out[key + "/input_seed"] = np.int64(seed)
        out[key + "/logp"] = lp.numpy()
        out[key + "/argmax"] = amax.numpy().astype(np.int32)
        out[key + "/prob"] = lp.gather(1, amax[:, None])[:, 0].exp().numpy()
        print("heads:", key, "input seed", seed, "top-2 gaps", gaps.tolist(), "max |logp| %.2f" % float(lp.abs().max()),
              "argmax", amax.tolist())
    np.savez_compressed(os.path.join(OUT, "heads_ref.npz"), **out)
    print("heads: wrote", os.path.getsize(os.path.join(OUT, "heads_ref.npz")), "bytes")


def golden_eval():
    import torch.optim as otpm
    from torch.utils.data import DataLoader
    for name in ("matplotlib", "matplotlib.pyplot", "imgaug", "imgaug.augmenters"):      # imported, never used on this path
        sys.modules.setdefault(name, types.ModuleType(name))
    tv = sys.modules["torchvision"]
    tv.transforms.Compose = tv.transforms.Lambda = tv.transforms.ToTensor = lambda *a, **k: None
    sys.path.insert(0, REF)
    cwd = os.getcwd()
    root = tempfile.mkdtemp(prefix="vnf_eval_")
    cfg = write_mlp_train_case(root)
    cfg["trainer"]["save_result"] = True
    os.chdir(root)                                    # the reference trainer logs relative to the working directory
    try:
        for pkg in ("trainer", "data_loader"):        # bypass the package __init__ files (torchvision models / imgaug pipelines)
            m = types.ModuleType(pkg)
            m.__path__ = [os.path.join(REF, pkg)]
            sys.modules[pkg] = m
        import losses as loss_md
        cls_tr = importlib.import_module("trainer.classification_trainer").ClassificationTrainer
        ds_cls = importlib.import_module("data_loader.vn_celeb_emb_dataset").VNCelebEmbDataset
        torch.manual_seed(123)                        # eval.py:15-20
        np.random.seed(123)
        val_ds = ds_cls(**cfg["val_dataset"]["args"], transforms=None)
        val_loader = DataLoader(dataset=val_ds, **cfg["val_data_loader"]["args"])
        # the generator's weights know nothing of the labels: take the first weight seed that gets some rows right and
        # some wrong, so that the hit count is checked on both kinds
        labels = torch.tensor(val_ds.labels)
        embs = torch.stack([val_ds[i][0] for i in range(len(val_ds))])
        for mlp_seed in range(64):
            model = ref("mlp_model").MLPModel(**cfg["model"]["args"]).eval()
            model.load_state_dict(generate_state_dict("mlp", seed=mlp_seed, as_torch=True, **cfg["model"]["args"]), strict=True)
            with torch.no_grad():
                right = int((model(embs).argmax(dim=1) == labels).sum())
            if 4 <= right <= len(val_ds) - 4:
                break
        assert 4 <= right <= len(val_ds) - 4, "no MLP weight seed with a mixed result"
        criterion = getattr(loss_md, cfg["loss"])
        metrics = [getattr(loss_md, x) for x in cfg["metrics"]]
        optimizer = getattr(otpm, cfg["optimizer"]["name"])(model.parameters(), **cfg["optimizer"]["args"])
        sched = getattr(otpm.lr_scheduler, cfg["lr_scheduler"]["name"])(optimizer, **cfg["lr_scheduler"]["args"])
        tr = cls_tr(cfg, model, criterion, metrics, optimizer, sched)
        tr.setup_loader(None, val_loader)
        logged = {}
        orig = tr._validate_epoch

        def wrapped(epoch, save_result=False):        # eval() only logs the two figures: keep them
            r = orig(epoch, save_result)
            logged.update({k: float(v) for k, v in (r[0] if save_result else r).items()})
            return r
        tr._validate_epoch = wrapped
        tr.eval(cfg["trainer"]["save_result"])
        text = open(os.path.join(str(tr.save_dir), "result.csv")).read()
    finally:
        os.chdir(cwd)
    lines = text.splitlines()
    emb_dir = os.path.join(root, "emb")
    rows = []
    for ln in lines[1:]:
        pth, tgt, pred, prob = ln.rsplit(",", 3)
        assert os.path.dirname(pth) == emb_dir, pth
        rows.append([os.path.basename(pth), int(tgt), int(pred), float(prob)])
    out = {"header": lines[0], "val_neg_log_llhood": logged["val_neg_log_llhood"], "val_accuracy": logged["val_accuracy"],
           "batch_size": cfg["val_data_loader"]["args"]["batch_size"], "mlp_seed": mlp_seed, "rows": rows}
    with open(os.path.join(OUT, "eval_ref.json"), "w") as f:
        json.dump(out, f, indent=0)
    shutil.rmtree(root, ignore_errors=True)
    print("eval:", lines[0], len(rows), "rows", out["val_neg_log_llhood"], out["val_accuracy"], rows[:2])


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    install_shim()
    torch.manual_seed(0)
    for w in (sys.argv[1:] or ["heads", "eval"]):
        globals()["golden_" + w]()
