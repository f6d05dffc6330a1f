#!/usr/bin/env python3
"""Train the MLP identity classifier: drop-in for /root/reference/train.py (22-76) with the keys of
cfg/train_cfg_emb_classify.json (precomputed embeddings) or cfg/train_cfg_aug_emb_classify.json (face images, augmented
and embedded inside the loop).  The optimisation step runs in libvnface.so (csrc/mlp_train.hip), the augmentation in
csrc/augment.hip; checkpoints are the reference's dict (trainer/base_trainer.py:83-105), readable by demo_image.py /
demo_video.py (-m).

    python train.py -c cfg/train_cfg_emb_classify.json -d GPU
    python train.py -c cfg/train_cfg_aug_emb_classify.json -d GPU

Only the embedding-classifier training of the README workflow (readme.md:16-34) is covered: model MLPModel, loss
neg_log_llhood, metric accuracy, Adam + ReduceLROnPlateau, and either
  - dataset VNCelebEmbDataset with trainer ClassificationTrainer ("transforms": "none"), or
  - dataset VNCelebDataset with trainer AugClassificationTrainer and transforms "default" | "facenet_aug" (resize false)."""
import argparse
import json

import numpy as np
import torch
from torch.utils.data import DataLoader

from vn_celeb_face_recognition_amd.trainer import (AugClassificationTrainer, ClassificationTrainer, ReduceLROnPlateau,
                                                   TrainableMLP, VNCelebDataset, VNCelebEmbDataset)

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


def main(config, run_id=None, device="cuda:0"):
    torch.manual_seed(SEED)
    np.random.seed(SEED)
    aug = aug_config(config)
    if not aug and config["trainer"].get("name", "ClassificationTrainer") != "ClassificationTrainer":
        raise SystemExit("trainer %s is not built: ClassificationTrainer or AugClassificationTrainer" % config["trainer"]["name"])
    if not aug and (config["model"]["name"] != "MLPModel" or config["train_dataset"]["name"] != "VNCelebEmbDataset"):
        raise SystemExit("this build trains MLPModel on VNCelebEmbDataset only (SURVEY.md 8 f-4)")
    if config["optimizer"]["name"] != "Adam" or config["lr_scheduler"]["name"] != "ReduceLROnPlateau":
        raise SystemExit("optimizer Adam + lr_scheduler ReduceLROnPlateau only (cfg/train_cfg_emb_classify.json)")
    if config["trainer"].get("device", "GPU") != "GPU":
        raise SystemExit("this build runs on MI355X only: trainer.device must be GPU (there is no CPU path)")
    if aug and not torch.cuda.is_available():
        raise SystemExit("this build runs on MI355X only: no GPU is visible (there is no CPU path)")
    dataset_cls, trainer_cls = (VNCelebDataset, AugClassificationTrainer) if aug else (VNCelebEmbDataset, ClassificationTrainer)
    train_dataset = dataset_cls(**config["train_dataset"]["args"], transforms=None)
    train_loader = DataLoader(dataset=train_dataset, **config["train_data_loader"]["args"])
    val_dataset = dataset_cls(**config["val_dataset"]["args"], transforms=None)
    val_loader = DataLoader(dataset=val_dataset, **config["val_data_loader"]["args"])
    oargs = dict(config["optimizer"]["args"])
    bs = max(config["train_data_loader"]["args"]["batch_size"], config["val_data_loader"]["args"]["batch_size"])
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
