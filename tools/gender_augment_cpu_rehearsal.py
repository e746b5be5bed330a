#!/usr/bin/env python3
"""CPU rehearsal of gender_classifier_train.py --synthetic N --augment true: the same data, seed, plan stream
(augment.TrainAugment's host generator, reseeded per epoch, draw_plan on the loader's lengths) and budget through
restatements only -- the fp64 restatement of the augmentation in tests/test_augment_gpu.py (``reference``),
oracle.features (Fbank, global InputNormalization updated on every training batch), oracle.xvector trained by torch
autograd (mean NLL over the doubled batch, Adam, clipping at 5.0, the recipe's ReduceLROnPlateau), the model of the
epoch with the lowest validation error evaluated on the test set.  No GPU, no kernel of this repository.  The white
noise comes from a CPU generator with the seed of the recipe's device generator: the same distribution, other
values.  Its test error is the constant E_CPU of tests/test_augment_gpu.py::test_recipe_learns_with_augmentation
(DESIGN section 12).  Prints one JSON line."""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import speech_anonymization_amd  # noqa: E402,F401  (registers the package name; host code only is used)
from speech_anonymization_amd import augment, data, gender  # noqa: E402
from oracle import features as OF, xvector as OX  # noqa: E402
from tests.test_augment_gpu import reference  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--synthetic", type=int, default=96)
    ap.add_argument("--batch_size", type=int, default=16)
    ap.add_argument("--number_of_epochs", type=int, default=4)
    ap.add_argument("--seed", type=int, default=1986)
    a = ap.parse_args()
    torch.manual_seed(a.seed)
    fbank, norm = OF.Fbank(), OF.InputNormalization()
    emb, cl = OX.Xvector(), OX.Classifier()
    params = list(emb.parameters()) + list(cl.parameters())
    opt = torch.optim.Adam(params, lr=1e-3)
    sched = gender.ReduceLROnPlateau(factor=0.5, patience=2, dont_halve_until_epoch=2)
    aug = augment.TrainAugment(seed=a.seed)
    noise_gen = torch.Generator()
    bs, n, seed = a.batch_size, a.synthetic, a.seed
    held = max(bs, n // 4)

    def log_probs(batch, train):
        wavs, lens, label = batch.sig[0], batch.sig[1], batch.gender
        norm.training = train
        with torch.no_grad():
            if train:
                plan = augment.draw_plan(aug.gen, lens, wavs.shape[1], aug.cfg)
                noise = torch.randn(wavs.shape, generator=noise_gen)
                wavs = reference(wavs, lens, plan, noise)[0].float()
                lens, label = lens.repeat(2), label.repeat(2)
            feats = norm(fbank(wavs), lens)
        return cl(emb(feats, lens)).squeeze(1), label

    def evaluate(batches):
        emb.eval(); cl.eval()
        err = cnt = 0
        loss = []
        with torch.no_grad():
            for b in batches:
                lp, label = log_probs(b, False)
                loss.append(float(F.nll_loss(lp, label)))
                err += int((lp.argmax(-1) != label).sum())
                cnt += int(label.numel())
        return sum(loss) / len(loss), err / cnt

    best, log = None, []
    for epoch in range(1, a.number_of_epochs + 1):
        emb.train(); cl.train()
        aug.reseed(epoch)
        noise_gen.manual_seed(aug._seed_now)
        tl = []
        for b in data.synthetic_gender_dataset(n, bs, seed=seed + 1000 * epoch):
            lp, label = log_probs(b, True)
            loss = F.nll_loss(lp, label)
            opt.zero_grad()
            loss.backward()
            torch.nn.utils.clip_grad_norm_(params, 5.0)
            opt.step()
            tl.append(float(loss.detach()))
        vloss, verr = evaluate(data.synthetic_gender_dataset(held, bs, seed=seed + 1))
        _, new_lr = sched([opt], epoch, vloss)
        gender.update_learning_rate(opt, new_lr)
        log.append({"epoch": epoch, "train_loss": sum(tl) / len(tl), "valid_loss": vloss, "valid_error": verr})
        if best is None or verr <= best[0]:                 # the most recent of equally good epochs
            best = (verr, epoch, copy.deepcopy(emb.state_dict()), copy.deepcopy(cl.state_dict()),
                    (norm.count, norm.glob_mean.clone(), norm.glob_std.clone()))
    emb.load_state_dict(best[2]); cl.load_state_dict(best[3])
    norm.count, norm.glob_mean, norm.glob_std = best[4]
    tloss, terr = evaluate(data.synthetic_gender_dataset(held, bs, seed=seed + 2))
    print(json.dumps({"synthetic": n, "batch_size": bs, "number_of_epochs": a.number_of_epochs, "seed": seed,
                      "best_epoch": best[1], "test_loss": tloss, "test_error": terr, "epochs": log}))


if __name__ == "__main__":
    main()
