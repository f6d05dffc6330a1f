"""Shared by tests/test_augment_host.py and tests/test_gpu_augment.py: the golden cases of tests/golden/facenet_aug_ref.npz
(tools/make_aug_golden.py) and a small image data set in the reference's on-disk form (class -> file names json + image
files, data_loader/vn_celeb_dataset.py:12-47) cut from the pictures under tests/golden/images."""
import json
import os

import numpy as np

from conftest import GOLDEN, load_image

PNGS = ("041bc30432964f95871d4c223eba8f7c.png", "318c7ec3b94b451c813a5665cfcfbda3.png", "33f2891da9694198a67aabd1660517c3.png")


def load_cases():
    """[(face (S,S,3) u8, s, t, angle, i, j, flip, expected (t,t,3) u8)]"""
    g = np.load(os.path.join(GOLDEN, "facenet_aug_ref.npz"))
    cases = []
    for k in range(len(g["s"])):
        s, t = int(g["s"][k]), int(g["t"][k])
        top, left = (int(v) for v in g["origin"][k])
        face = np.ascontiguousarray(load_image(str(g["picture"][k]))[top:top + s, left:left + s])
        cases.append((face, s, t, float(g["angle"][k]), int(g["i"][k]), int(g["j"][k]), int(g["flip"][k]), g["out_%d" % k]))
    return cases


def write_face_dataset(root, size=160, n_cls=12, per_cls_train=4, per_cls_val=2):
    """n_cls classes of size x size PNG crops (distinct windows of the three 181x181 face pictures) under <root>/img,
    plus <root>/train.json and <root>/val.json.  Returns (train dict, val dict)."""
    from PIL import Image
    os.makedirs(os.path.join(root, "img"), exist_ok=True)
    pics = [load_image(p) for p in PNGS]
    span = pics[0].shape[0] - size + 1
    train, val = {}, {}
    for c in range(n_cls):
        for k in range(per_cls_train + per_cls_val):
            q = c * (per_cls_train + per_cls_val) + k
            top, left = (q * 7) % span, (q * 11 + 3) % span
            name = "c%02d_%02d.png" % (c, per_cls_train + per_cls_val - 1 - k)      # written out of sorted order on purpose
            Image.fromarray(np.ascontiguousarray(pics[c % 3][top:top + size, left:left + size])).save(os.path.join(root, "img", name))
            (train if k < per_cls_train else val).setdefault(str(c), []).append(name)
    for fn, d in (("train.json", train), ("val.json", val)):
        with open(os.path.join(root, fn), "w") as f:
            json.dump(d, f)
    return train, val


def aug_train_config(root, transforms="facenet_aug", epochs=2, n_cls=12):
    return {
        "name": "aug train test", "data_path": "data",
        "train_dataset": {"name": "VNCelebDataset", "args": {"data_dir": os.path.join(root, "img"), "label_file": os.path.join(root, "train.json")}},
        "train_data_loader": {"name": "train", "args": {"batch_size": 16, "shuffle": True, "num_workers": 0}},
        "val_dataset": {"name": "VNCelebDataset", "args": {"data_dir": os.path.join(root, "img"), "label_file": os.path.join(root, "val.json")}},
        "val_data_loader": {"name": "val", "args": {"batch_size": 16, "shuffle": False, "num_workers": 0}},
        "transforms": {"name": transforms, "resize": False, "encoder_img_size": 160},
        "metrics": ["accuracy"], "loss": "neg_log_llhood",
        "model": {"name": "MLPModel", "args": {"input_dim": 512, "num_classes": n_cls}},
        "trainer": {"name": "AugClassificationTrainer", "resume_path": "", "save_dir": os.path.join(root, "saved"), "device": "GPU",
                    "log_step": 30, "do_validation": True, "validation_step": 1, "epochs": epochs,
                    "tracked_metric": ["val_neg_log_llhood", "min"], "patience": 10, "save_period": 1, "save_result": False,
                    "track4plot": True, "chosen_idx_enc": 0,
                    "encoders": [{"name": "InceptionResnetV1", "args": {"pretrained": None, "max_batch": 32}}]},
        "optimizer": {"name": "Adam", "args": {"lr": 0.002, "weight_decay": 1e-04}},
        "lr_scheduler": {"name": "ReduceLROnPlateau", "args": {"mode": "min", "threshold": 0.5, "factor": 0.5, "patience": 1,
                                                               "min_lr": 1e-05, "threshold_mode": "rel"}},
    }
