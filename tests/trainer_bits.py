"""Shared by tests/test_gpu_trainer_bits.py and tools/make_trainer_bits.py: one seeded run of each on-device trainer
(trainer.TrainableMLP, trainer.TrainableHead), recorded as the SHA-256 of every parameter and Adam moment, the hex of
every loss, the hit counts and the step counter.  Only `_get`, `_set` (through load_state_dict), `_step_count` and `step`
are used, so the same run can be recorded on one commit and replayed on another."""
import hashlib
import subprocess
from collections import OrderedDict

import numpy as np
import torch

DEV = "cuda:0"
LR, WEIGHT_DECAY, SCALE = 1e-3, 1e-4, 0.04
# head (C, b): below one class tile and below one K step of 4 rows; both tails.
# mlp (D, C, b): D no multiple of the GEMM's K step of 16 with C and b below one 64-tile; the golden case's shape.
CASES = (("head", (7, 3)), ("head", (17, 5)), ("mlp", (20, 7, 5)), ("mlp", (512, 12, 64)))
STEPS = 5          # three training steps, one evaluation step, one training step after the checkpoint round trip


def case_id(kind, shape):
    return "%s-%s" % (kind, "x".join(str(s) for s in shape))


def case_seed(kind, shape):
    return 1000 * CASES.index((kind, shape)) + 17


class _HeadOnly:
    """What TrainableHead asks of an encoder, without a backbone: a `logits` layer behind one frozen tensor."""
    arch_name, input_size, compute_dtype, max_batch = "HeadOnly", 112, "f32", 8

    def __init__(self, c):
        self.device = torch.device(DEV)
        self.head_classes = c
        self._sd = OrderedDict([("stem.weight", torch.arange(4.0)), ("logits.weight", torch.zeros(c, 512)), ("logits.bias", torch.zeros(c))])

    def eval(self):
        return self

    def _spec(self):
        return [(k, tuple(v.shape), "conv") for k, v in self._sd.items()]

    def state_dict(self):
        return OrderedDict(self._sd)

    def load_state_dict(self, sd):
        self._sd = OrderedDict((k, sd[k]) for k in self._sd)


def _model(kind, shape):
    from vn_celeb_face_recognition_amd.trainer import HEAD_PARAMS, PARAMS, TrainableHead, TrainableMLP
    b = shape[-1]
    if kind == "head":
        return TrainableHead(_HeadOnly(shape[0]), lr=LR, weight_decay=WEIGHT_DECAY, max_batch=b), HEAD_PARAMS
    return TrainableMLP(shape[0], shape[1], lr=LR, weight_decay=WEIGHT_DECAY, max_batch=b), PARAMS


def _inputs(kind, shape):
    """(state_dict, [(x (b,width), target (b,))] * STEPS) from ONE RandomState, parameters first, in state_dict order."""
    rs = np.random.RandomState(case_seed(kind, shape))
    c, b = shape[-2], shape[-1]
    if kind == "head":
        shapes, width = OrderedDict([("logits.weight", (c, 512)), ("logits.bias", (c,))]), 512
    else:
        d = shape[0]
        shapes, width = OrderedDict([("dense_1.weight", (2048, d)), ("dense_1.bias", (2048,)), ("dense_2.weight", (c, 2048)),
                                     ("dense_2.bias", (c,))]), d
    sd = OrderedDict((k, torch.from_numpy((rs.standard_normal(s) * SCALE).astype(np.float32))) for k, s in shapes.items())
    batches = [(torch.from_numpy(rs.standard_normal((b, width)).astype(np.float32)), torch.from_numpy(rs.randint(0, c, b).astype(np.int64)))
               for _ in range(STEPS)]
    return sd, batches


def state_hashes(model, names):
    """{"<name>/<kind>": sha256 of the tensor's raw bytes} for kind 0 (parameter), 1 (exp_avg), 2 (exp_avg_sq)."""
    return {"%s/%d" % (k, kind): hashlib.sha256(model._get(k, kind).numpy().tobytes()).hexdigest() for k in names for kind in (0, 1, 2)}


def _step(model, kind, shape, i, batch, train):
    if kind == "mlp":
        torch.manual_seed(case_seed(kind, shape) + i)       # the dropout draw of this step
    loss, hits = model.step(batch[0].to(DEV), batch[1], train=train)
    return float(loss).hex(), int(hits)


def run_case(kind, shape):
    """The recorded sequence.  `after_eval` and the `resumed_*` entries are a second view of state the record already
    holds (the test asserts that they are equal to it); they are kept in the record so that both sides can be compared
    against the recording as well."""
    sd, batches = _inputs(kind, shape)
    model, names = _model(kind, shape)
    if kind == "head":
        sd = OrderedDict([("stem.weight", torch.arange(4.0))] + list(sd.items()))
    model.load_state_dict(sd)
    steps = [_step(model, kind, shape, i, batches[i], True) for i in range(3)]
    after3, count3 = state_hashes(model, names), model._step_count()
    steps.append(_step(model, kind, shape, 3, batches[3], False))
    after_eval, count_eval = state_hashes(model, names), model._step_count()
    fresh, _ = _model(kind, shape)
    fresh.load_state_dict(model.state_dict())
    fresh.load_optimizer_state_dict(model.optimizer_state_dict())
    steps.append(_step(model, kind, shape, 4, batches[4], True))
    resumed_step = _step(fresh, kind, shape, 4, batches[4], True)
    return {"loss": [s[0] for s in steps], "hits": [s[1] for s in steps],
            "after_step3": after3, "step_count_after_step3": count3,
            "after_eval": after_eval, "step_count_after_eval": count_eval,
            "after_step4": state_hashes(model, names), "step_count_after_step4": model._step_count(),
            "resumed_loss": resumed_step[0], "resumed_hits": resumed_step[1],
            "resumed_after_step4": state_hashes(fresh, names), "resumed_step_count": fresh._step_count()}


def versions():
    """The toolchain a record was made under / a test runs under: torch and the hipcc that builds the library."""
    from vn_celeb_face_recognition_amd.build import HIPCC
    try:
        hipcc = subprocess.run([HIPCC, "--version"], capture_output=True, text=True).stdout.strip()
    except OSError as e:
        hipcc = "unavailable: %s" % e
    return {"torch": torch.__version__, "hipcc": hipcc}
