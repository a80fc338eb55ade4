"""SHA-256 digests of both engines' state after the initial draw and after five training steps on fixed synthetic input: what two
checkouts over one library must print identically when a change is meant to leave every result alone
(profiles/engine_core_refactor.txt).  1-D engine: siamese contrastive steps in f16 and f32 and one classifier sequence (step 1 is
enqueued eagerly, step 2 recorded, steps 3-5 replayed); 2-D engine: siamese contrastive steps in f16 and f32.

    python tools/engine_digest.py            one line per (engine, storage, stage)
"""
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from voicemap_amd.engine import HipEncoderEngine  # noqa: E402
from voicemap_amd.spectro_engine import HipSpectrogramEncoderEngine  # noqa: E402

SEED, STEPS, PAIRS = 1234, 5, 4
BLOCKS = [(32, 16, 4), (3, 32, 2), (3, 48, 2), (3, 64, 2)]


def digest(eng, loss=None):
    torch.cuda.synchronize()
    parts = []
    for name in ("P", "M", "V", "NT", "ZD"):
        parts.append("%s %s" % (name, hashlib.sha256(getattr(eng, name).cpu().numpy().tobytes()).hexdigest()[:24]))
    if loss is not None:
        parts.append("loss %s" % hashlib.sha256(loss.cpu().numpy().tobytes()).hexdigest()[:24])
    parts.append("loss_scale %r iterations %d" % (float(eng.loss_scale), eng.iterations))
    return "  ".join(parts)


def main():
    r = np.random.default_rng(SEED)
    x1 = r.normal(0, 0.05, (PAIRS, 8000, 1)).astype(np.float32)
    x2 = r.normal(0, 0.05, (PAIRS, 8000, 1)).astype(np.float32)
    y = np.array([[0.0], [1.0]] * (PAIRS // 2), dtype=np.float32)
    labels = np.arange(2 * PAIRS, dtype=np.int32) % 5
    for dtype in ("f16", "f32"):
        eng = HipEncoderEngine(BLOCKS, 32, dropout=0.05, head="uniform_euclidean", dtype=dtype, seed=SEED)
        print("1-D siamese    %s draw    %s" % (dtype, digest(eng)))
        for _ in range(STEPS):
            pl = eng.siamese_train_step(x1, x2, y, loss="contrastive", preprocessed=False, downsampling=4, whitening=True)
        print("1-D siamese    %s 5 steps %s" % (dtype, digest(eng, pl["loss_acc"])))
    eng = HipEncoderEngine(BLOCKS, 32, dropout=0.05, head="classifier", num_classes=5, dtype="f16", seed=SEED)
    print("1-D classifier f16 draw    %s" % digest(eng))
    for _ in range(STEPS):
        pl = eng.classifier_train_step(np.concatenate([x1, x2]), labels, preprocessed=False, downsampling=4, whitening=True)
    print("1-D classifier f16 5 steps %s" % digest(eng, pl["loss_acc"]))
    for dtype in ("f16", "f32"):
        eng = HipSpectrogramEncoderEngine(32, 64, dropout=0.05, head="weighted_l1", dtype=dtype, seed=SEED)
        print("2-D siamese    %s draw    %s" % (dtype, digest(eng)))
        for _ in range(STEPS):
            pl = eng.siamese_train_step(x1, x2, y, loss="contrastive")
        print("2-D siamese    %s 5 steps %s" % (dtype, digest(eng, pl["loss_acc"])))


if __name__ == "__main__":
    main()
