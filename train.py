#!/usr/bin/env python3
"""Train the MLP identity classifier, or the `logits` head of a frozen encoder: drop-in for the reference's train.py
(22-76) with the keys of cfg/train_cfg_emb_classify.json (precomputed embeddings), cfg/train_cfg_aug_emb_classify.json
(face images, augmented and embedded inside the loop) or cfg/train_cfg_img_classify.json (face images, the encoder's own
head).  The optimisation step runs in libvnface.so (csrc/mlp_train.hip, csrc/head_train.hip), the augmentation in
csrc/augment.hip; checkpoints are the reference's dict (trainer/base_trainer.py:83-105), readable by demo_image.py /
demo_video.py (-m) and, for a head, by eval.py (trainer.resume_path).

    python train.py -c cfg/train_cfg_emb_classify.json -d GPU
    python train.py -c cfg/train_cfg_aug_emb_classify.json -d GPU
    python train.py -c cfg/train_cfg_img_classify.json -d GPU

Only the embedding-classifier training of the README workflow (readme.md:16-34) is covered: model MLPModel, loss
neg_log_llhood, metric accuracy, Adam + ReduceLROnPlateau, and either
  - dataset VNCelebEmbDataset with trainer ClassificationTrainer ("transforms": "none"), or
  - dataset VNCelebDataset with trainer AugClassificationTrainer and transforms "default" | "facenet_aug" (resize false).
The third route trains one layer of an image classifier: model iresnet100 (n_classes, freeze_weights: true) or
InceptionResnetV1 (classify: true, freeze_weights: true -- this build's flag: the reference would fine-tune every layer),
dataset VNCelebDataset, trainer ClassificationTrainer, the same transforms.  Nothing runs backward through a backbone."""
import argparse
import json

import numpy as np
import torch
from torch.utils.data import DataLoader

from vn_celeb_face_recognition_amd.trainer import (AugClassificationTrainer, ClassificationTrainer, ReduceLROnPlateau,
                                                   TrainableHead, TrainableMLP, VNCelebDataset, VNCelebEmbDataset)

SEED = 123   # train.py:16-20


def aug_config(config):
    """Is this the image configuration (train_cfg_aug_emb_classify.json)?  Exits on the combinations this build refuses."""
    if config["train_dataset"]["name"] != "VNCelebDataset" and config["trainer"].get("name") != "AugClassificationTrainer":
        return False
    if config["model"]["name"] != "MLPModel":
        raise SystemExit("this build trains MLPModel only (SURVEY.md 8 f-4, f-6)")
    if config["train_dataset"]["name"] != "VNCelebDataset" or config["val_dataset"]["name"] != "VNCelebDataset" \
            or config["trainer"].get("name") != "AugClassificationTrainer":
        raise SystemExit("VNCelebDataset (train and val) goes with trainer AugClassificationTrainer and the other way round: got "
                         "%s / %s / %s" % (config["train_dataset"]["name"], config["val_dataset"]["name"], config["trainer"].get("name")))
    tf = config.get("transforms")
    name = tf.get("name") if isinstance(tf, dict) else tf
    if name == "rank1_aug":
        raise SystemExit("transforms rank1_aug (imgaug on the host, data_loader/__init__.py:10-25) is not built: use facenet_aug "
                         "or default (DESIGN.md 8)")
    if name not in ("default", "facenet_aug"):
        raise SystemExit("AugClassificationTrainer needs transforms.name default or facenet_aug, got %r" % (name,))
    if tf.get("resize"):
        raise SystemExit("transforms.resize is not built: the images must already have the encoder's input size (DESIGN.md 8)")
    tc = config["trainer"]
    if not isinstance(tc.get("encoders"), list) or not 0 <= tc.get("chosen_idx_enc", -1) < len(tc["encoders"]):
        raise SystemExit("trainer.encoders / trainer.chosen_idx_enc do not name an encoder (online_aug_trainer.py:9-13)")
    return True


def head_config(config):
    """Is this the head-training configuration (train_cfg_img_classify.json): an encoder whose `logits` layer alone
    trains, on face images, under ClassificationTrainer?  Exits on the transforms this build refuses."""
    model, args = config["model"]["name"], config["model"].get("args", {})
    frozen = args.get("freeze_weights") is True
    if not ((model == "iresnet100" and args.get("n_classes") is not None and frozen)
            or (model == "InceptionResnetV1" and args.get("classify") and frozen)):
        return False
    if config["train_dataset"]["name"] != "VNCelebDataset" or config.get("val_dataset", {}).get("name") != "VNCelebDataset" \
            or config["trainer"].get("name", "ClassificationTrainer") != "ClassificationTrainer":
        return False
    tf = config.get("transforms")
    name = tf.get("name") if isinstance(tf, dict) else tf
    if name == "rank1_aug":
        raise SystemExit("transforms rank1_aug (imgaug on the host, data_loader/__init__.py:10-25) is not built: use facenet_aug "
                         "or default (DESIGN.md 8)")
    if name not in ("default", "facenet_aug"):
        raise SystemExit("head training needs transforms.name default or facenet_aug, got %r" % (name,))
    if tf.get("resize"):
        raise SystemExit("transforms.resize is not built: the images must already have the encoder's input size (DESIGN.md 8)")
    return True


def head_model(config, max_batch, device):
    """The frozen encoder of config.model on `device` and the trainer of its head."""
    from vn_celeb_face_recognition_amd import models
    margs = dict(config["model"].get("args", {}))
    margs.setdefault("max_batch", min(256, max_batch))
    net = getattr(models, config["model"]["name"])(**margs)
    net.to(device)
    oargs = dict(config["optimizer"]["args"])
    return TrainableHead(net, lr=oargs.get("lr", 1e-3), betas=oargs.get("betas", (0.9, 0.999)), eps=oargs.get("eps", 1e-8),
                         weight_decay=oargs.get("weight_decay", 0.0), max_batch=max_batch)


def main(config, run_id=None, device="cuda:0"):
    torch.manual_seed(SEED)
    np.random.seed(SEED)
    head = head_config(config)
    aug = not head and aug_config(config)
    if not head and not aug:
        if config["trainer"].get("name", "ClassificationTrainer") != "ClassificationTrainer":
            raise SystemExit("trainer %s is not built: ClassificationTrainer or AugClassificationTrainer" % config["trainer"]["name"])
        if config["model"]["name"] != "MLPModel" or config["train_dataset"]["name"] != "VNCelebEmbDataset":
            raise SystemExit("this build trains MLPModel on VNCelebEmbDataset only (SURVEY.md 8 f-4)")
    if config["optimizer"]["name"] != "Adam" or config["lr_scheduler"]["name"] != "ReduceLROnPlateau":
        raise SystemExit("optimizer Adam + lr_scheduler ReduceLROnPlateau only (cfg/train_cfg_emb_classify.json)")
    if config["trainer"].get("device", "GPU") != "GPU":
        raise SystemExit("this build runs on MI355X only: trainer.device must be GPU (there is no CPU path)")
    if (aug or head) and not torch.cuda.is_available():
        raise SystemExit("this build runs on MI355X only: no GPU is visible (there is no CPU path)")
    dataset_cls = VNCelebDataset if aug or head else VNCelebEmbDataset
    trainer_cls = AugClassificationTrainer if aug else ClassificationTrainer
    train_dataset = dataset_cls(**config["train_dataset"]["args"], transforms=None)
    train_loader = DataLoader(dataset=train_dataset, **config["train_data_loader"]["args"])
    val_dataset = dataset_cls(**config["val_dataset"]["args"], transforms=None)
    val_loader = DataLoader(dataset=val_dataset, **config["val_data_loader"]["args"])
    oargs = dict(config["optimizer"]["args"])
    bs = max(config["train_data_loader"]["args"]["batch_size"], config["val_data_loader"]["args"]["batch_size"])
    if head:
        model = head_model(config, bs, device)
        for ds in (train_dataset, val_dataset):
            if len(ds) and ds.size != model.input_size:
                raise SystemExit("the images are %dx%d but %s takes %dx%d: transforms.resize is not built (DESIGN.md 8)"
                                 % (ds.size, ds.size, config["model"]["name"], model.input_size, model.input_size))
    else:
        model = TrainableMLP(**config["model"]["args"], lr=oargs.get("lr", 1e-3), betas=oargs.get("betas", (0.9, 0.999)),
                             eps=oargs.get("eps", 1e-8), weight_decay=oargs.get("weight_decay", 0.0), max_batch=bs, device=device)
    sargs = {k: v for k, v in config["lr_scheduler"]["args"].items() if k != "verbose"}
    trainer = trainer_cls(config, model, ReduceLROnPlateau(model, **sargs), run_id=run_id)
    trainer.setup_loader(train_loader, val_loader)
    trainer.train(config["trainer"]["track4plot"])
    return trainer


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description="VNCeleb - Face Recognition")
    ap.add_argument("-c", "--config", default=None, type=str, help="Path of config file")
    ap.add_argument("-d", "--device", default=None, type=str, help="Indices of GPUs")
    args = ap.parse_args()
    with open(args.config) as fp:
        main(json.load(fp))
