#!/usr/bin/env python3
"""Evaluate a trained model on val_dataset: drop-in for /root/reference/eval.py (22-68) + BaseTrainer.eval
(trainer/base_trainer.py:177-200).  Logs val_neg_log_llhood and val_accuracy and, with trainer.save_result, writes
<save_dir>/models/<run_id>/result.csv (Path,Target,Prediction,Probability).  The model runs in libvnface.so; the loss,
accuracy, prediction and probability of every row come from one kernel (csrc/head_eval.hip).

    python eval.py -c cfg/train_cfg_emb_classify.json -d GPU        # (a) MLPModel on precomputed embeddings
    python eval.py -c cfg/train_cfg_aug_emb_classify.json -d GPU    # (b) MLPModel behind a frozen encoder, on face images
    python eval.py -c cfg/eval_cfg_img_classify.json -d GPU         # (c) an encoder with its own logits head, on face images

Three configurations are built; every other one is refused with its reason:
  (a) model MLPModel, val_dataset VNCelebEmbDataset, trainer ClassificationTrainer;
  (b) model MLPModel, val_dataset VNCelebDataset, trainer AugClassificationTrainer (trainer.encoders[chosen_idx_enc] embeds
      the images; validation always takes the default transform, eval.py:24-40);
  (c) model InceptionResnetV1 (classify) or iresnet100 (n_classes), val_dataset VNCelebDataset, trainer
      ClassificationTrainer, default transform.
The weights are those of trainer.resume_path (a train.py checkpoint); in (c) model.args may name them instead."""
import argparse
import json

import numpy as np
import torch
from torch.utils.data import DataLoader

SEED = 123   # eval.py:15-20

ENCODERS = ("InceptionResnetV1", "iresnet100")


def plan(config):
    """Which of the three configurations `config` is: "emb", "aug" or "img".  Exits on everything else."""
    model, trainer = config["model"]["name"], config["trainer"].get("name", "ClassificationTrainer")
    dataset = config["val_dataset"]["name"]
    if model not in ("MLPModel",) + ENCODERS:
        raise SystemExit("model %s is not built: MLPModel, InceptionResnetV1 (classify) or iresnet100 (n_classes)" % model)
    if trainer not in ("ClassificationTrainer", "AugClassificationTrainer"):
        raise SystemExit("trainer %s is not built: ClassificationTrainer or AugClassificationTrainer" % trainer)
    if dataset not in ("VNCelebEmbDataset", "VNCelebDataset"):
        raise SystemExit("val_dataset %s is not built: VNCelebEmbDataset or VNCelebDataset" % dataset)
    if config["loss"] != "neg_log_llhood" or list(config["metrics"]) != ["accuracy"]:
        raise SystemExit("loss neg_log_llhood and metrics [accuracy] only: that is what the evaluation kernel computes, got %s / %s"
                         % (config["loss"], list(config["metrics"])))
    if config["trainer"].get("device", "GPU") != "GPU":
        raise SystemExit("this build runs on MI355X only: trainer.device must be GPU (there is no CPU path)")
    tf = config.get("transforms")
    if isinstance(tf, dict) and tf.get("resize"):
        raise SystemExit("transforms.resize is not built: the images must already have the encoder's input size (DESIGN.md 8)")
    if model == "MLPModel":
        if dataset == "VNCelebEmbDataset" and trainer == "ClassificationTrainer":
            kind = "emb"
        elif dataset == "VNCelebDataset" and trainer == "AugClassificationTrainer":
            tc = config["trainer"]
            if not isinstance(tc.get("encoders"), list) or not 0 <= tc.get("chosen_idx_enc", -1) < len(tc["encoders"]):
                raise SystemExit("trainer.encoders / trainer.chosen_idx_enc do not name an encoder (online_aug_trainer.py:9-13)")
            name = tf.get("name") if isinstance(tf, dict) else tf
            if name not in ("default", "facenet_aug"):
                raise SystemExit("AugClassificationTrainer needs transforms.name default or facenet_aug, got %r (rank1_aug is not "
                                 "built, DESIGN.md 8); validation itself always takes the default transform" % (name,))
            kind = "aug"
        else:
            raise SystemExit("MLPModel is evaluated on VNCelebEmbDataset with ClassificationTrainer or on VNCelebDataset with "
                             "AugClassificationTrainer: got %s / %s" % (dataset, trainer))
        if not config["trainer"].get("resume_path"):
            raise SystemExit("trainer.resume_path names no checkpoint: there is no trained MLPModel to evaluate")
        return kind
    if dataset != "VNCelebDataset" or trainer != "ClassificationTrainer":
        raise SystemExit("%s classifies face images: val_dataset VNCelebDataset with trainer ClassificationTrainer, got %s / %s"
                         % (model, dataset, trainer))
    args = config["model"].get("args", {})
    if model == "InceptionResnetV1" and not args.get("classify"):
        raise SystemExit("InceptionResnetV1 without classify=true returns embeddings, not class probabilities: nothing to evaluate")
    if model == "iresnet100" and args.get("n_classes") is None:
        raise SystemExit("iresnet100 without n_classes returns embeddings, not class probabilities: nothing to evaluate")
    return "img"


def main(config, run_id=None, device="cuda:0"):
    torch.manual_seed(SEED)
    np.random.seed(SEED)
    kind = plan(config)
    if not torch.cuda.is_available():
        raise SystemExit("this build runs on MI355X only: no GPU is visible (there is no CPU path)")
    from vn_celeb_face_recognition_amd import models
    from vn_celeb_face_recognition_amd.trainer import (AugClassificationTrainer, ClassificationTrainer, EvalModel, VNCelebDataset,
                                                       VNCelebEmbDataset)
    dataset_cls = VNCelebEmbDataset if kind == "emb" else VNCelebDataset
    val_dataset = dataset_cls(**config["val_dataset"]["args"], transforms=None)
    val_loader = DataLoader(dataset=val_dataset, **config["val_data_loader"]["args"])
    bs = int(config["val_data_loader"]["args"].get("batch_size", 1))
    margs = dict(config["model"].get("args", {}))
    if kind == "img":
        margs.setdefault("max_batch", min(256, bs))
        net = getattr(models, config["model"]["name"])(**margs)
        num_classes = net.head_classes
    else:
        net = models.MLPModel(**margs, max_batch=bs)
        num_classes = net.num_classes
    model = EvalModel(net, num_classes, device=device)
    trainer_cls = AugClassificationTrainer if kind == "aug" else ClassificationTrainer
    trainer = trainer_cls(config, model, None, run_id=run_id)
    trainer.setup_loader(None, val_loader)
    trainer.eval(bool(config["trainer"].get("save_result", False)))
    return trainer


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description="VNCeleb - Face Recognition")
    ap.add_argument("-c", "--config", default=None, type=str, help="Path of config file")
    ap.add_argument("-d", "--device", default=None, type=str, help="Indices of GPUs")
    args = ap.parse_args()
    with open(args.config) as fp:
        main(json.load(fp))
