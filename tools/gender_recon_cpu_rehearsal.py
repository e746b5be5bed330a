#!/usr/bin/env python3
"""CPU rehearsal of gender_classifier_train_recon.py --model_type fcae --synthetic N: the same data, seeds and
budget through restatements only -- oracle.features (Fbank, global InputNormalization updated on every training
batch), tests/fcae_ref.py with the trained weights of tests/golden/fcae_trained.npz for the reconstruction
(decoder(encoder(x)) under no_grad), oracle.xvector trained by torch autograd (mean NLL, Adam, clipping at 5.0,
the recipe's ReduceLROnPlateau), the model of the epoch with the lowest validation error evaluated on the test
set.  No GPU, no kernel of this repository.  Its test error is the constant E_CPU of
tests/test_reconstruct_gpu.py::test_recipe_end_to_end_fcae.  Prints one JSON line."""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import speech_anonymization_amd  # noqa: E402,F401  (registers the package name; host code only is used)
from speech_anonymization_amd import data, gender  # noqa: E402
from oracle import features as OF, xvector as OX  # noqa: E402
from tests import fcae_ref  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--synthetic", type=int, default=64)
    ap.add_argument("--batch_size", type=int, default=8)
    ap.add_argument("--number_of_epochs", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1986)
    a = ap.parse_args()
    torch.manual_seed(a.seed)
    z = np.load(os.path.join(ROOT, "tests", "golden", "fcae_trained.npz"))
    anon = fcae_ref.FullyConnectedAutoencoder(80, a.batch_size)
    anon.load_state_dict({k[len("ckpt/0."):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("ckpt/0.")})
    anon.train()                                            # as Brain.fit leaves it; decoder(encoder(x)) has no mode
    fbank, norm = OF.Fbank(), OF.InputNormalization()
    emb, cl = OX.Xvector(), OX.Classifier()
    params = list(emb.parameters()) + list(cl.parameters())
    opt = torch.optim.Adam(params, lr=1e-3)
    sched = gender.ReduceLROnPlateau(factor=0.5, patience=2, dont_halve_until_epoch=2)
    bs, n, seed = a.batch_size, a.synthetic, a.seed
    held = max(bs, n // 4)

    def log_probs(batch, train):
        norm.training = train
        with torch.no_grad():
            feats = norm(fbank(batch.sig[0]), batch.sig[1])
            recon = anon.decoder(anon.encoder(feats))
        return cl(emb(recon, batch.sig[1])).squeeze(1)

    def evaluate(batches):
        emb.eval(); cl.eval()
        err = cnt = 0
        loss = []
        with torch.no_grad():
            for b in batches:
                lp = log_probs(b, False)
                loss.append(float(F.nll_loss(lp, b.gender)))
                err += int((lp.argmax(-1) != b.gender).sum())
                cnt += int(b.gender.numel())
        return sum(loss) / len(loss), err / cnt

    best, log = None, []
    for epoch in range(1, a.number_of_epochs + 1):
        emb.train(); cl.train()
        tl = []
        for b in data.synthetic_gender_dataset(n, bs, seed=seed + 1000 * epoch):
            loss = F.nll_loss(log_probs(b, True), b.gender)
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
