"""Generate tests/golden/fcae_S.npz and tests/golden/fcae_trained.npz from the REFERENCE's own
FullyConnectedAutoencoder (models/FullyConnected.py).  Runs where a checkout of the reference exists
(REFERENCE_ROOT, default oracle.gen_golden.REF); never on the GPU box, and no test reads that checkout.

  1. oracle.gen_golden.install_shim() stands in for the two speechbrain symbols the reference imports;
  2. tests/fcae_ref.py in fp32 must reproduce the reference class BIT FOR BIT, train and eval mode, outputs
     and all 30 gradients (asserted here);
  3. fcae_S.npz: seeded weights and feats at B = 3, T = 100 with outputs, loss, gradients (subsampled like
     gen_golden.sub where large) and running statistics;
  4. fcae_trained.npz: parameters and buffers of the reference's trained checkpoint results/5_5_fc (read with
     weights_only=True; its keys carry the ModuleList index "0.") and the reference class's eval outputs on
     seeded feats.

Usage:  python tools/gen_fcae_golden.py        (from the repository root)
"""
import glob
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden")

from oracle import gen_golden as G                               # noqa: E402
from tests import fcae_ref as R                                  # noqa: E402

REF = os.environ.get("REFERENCE_ROOT", G.REF)


def seeded(B, T, seed):
    g = torch.Generator().manual_seed(seed)
    feats = torch.randn(B, T, 80, generator=g)
    feats = feats * (0.5 + torch.rand(1, 1, 80, generator=g)) + 0.3 * torch.randn(1, 1, 80, generator=g)
    return feats, torch.arange(B) % 2


def same(a, b, what):
    assert torch.equal(a, b), f"tests/fcae_ref.py != reference on {what}"


def fixture_S():
    from models.FullyConnected import FullyConnectedAutoencoder as RefFC
    B, T = 3, 100
    torch.manual_seed(8886)
    ref = RefFC(80, B)
    ours = R.FullyConnectedAutoencoder(80, B)
    ours.load_state_dict(ref.state_dict())
    init = {k: v.detach().clone() for k, v in ref.state_dict().items()}
    feats, gender = seeded(B, T, 1)
    tr = R.run_step(ref, feats, gender, True)
    tr2 = R.run_step(ours, feats, gender, True)
    for k in ("recon", "logp", "loss"):
        same(tr[k], tr2[k], k)
    assert len(tr["grads"]) == 30
    for k in tr["grads"]:
        same(tr["grads"][k], tr2["grads"][k], f"gradient {k}")
    for k in tr["buffers"]:
        same(tr["buffers"][k], tr2["buffers"][k], f"buffer {k}")
    ev, ev2 = R.run_step(ref, feats, gender, False), R.run_step(ours, feats, gender, False)
    for k in ("recon", "logp", "loss"):
        same(ev[k], ev2[k], k + " (eval)")
    d = dict(feats=feats.numpy(), gender=gender.numpy(), recon=tr["recon"].numpy(), logp=tr["logp"].numpy(),
             loss=tr["loss"].numpy(), eval_recon_sub=G.sub(ev["recon"]), eval_logp=ev["logp"].numpy())
    for k, v in init.items():
        d["init/" + k] = v.numpy()
    for k, g in tr["grads"].items():
        d["grad_sub/" + k] = G.sub(g)
        d["grad_stat/" + k] = np.array([float(g.double().sum()), float(g.double().norm())])
    for k, v in tr["buffers"].items():
        d["buffer/" + k] = v.numpy()
    np.savez_compressed(os.path.join(OUT, "fcae_S.npz"), **d)
    print(f"fcae_S: loss={float(tr['loss']):.6f} (tests/fcae_ref.py == reference: bit-exact, train and eval)")


def fixture_trained():
    from models.FullyConnected import FullyConnectedAutoencoder as RefFC
    ck = sorted(glob.glob(os.path.join(REF, "results", "5_5_fc", "8886", "save", "CKPT*", "model.ckpt")))[-1]
    sd = torch.load(ck, weights_only=True, map_location="cpu")
    assert all(k.startswith("0.") for k in sd)
    ref = RefFC(80, 3)
    ref.load_state_dict({k[2:]: v for k, v in sd.items()})
    ours = R.FullyConnectedAutoencoder(80, 3)
    ours.load_state_dict(ref.state_dict())
    feats, gender = seeded(3, 150, 2)
    ev, ev2 = R.run_step(ref, feats, gender, False), R.run_step(ours, feats, gender, False)
    for k in ("recon", "logp"):
        same(ev[k], ev2[k], k + " (trained, eval)")
    d = dict(feats=feats.numpy(), eval_recon=ev["recon"].numpy(), eval_logp=ev["logp"].numpy(),
             source=np.array(os.path.relpath(ck, REF)))
    for k, v in sd.items():
        d["ckpt/" + k] = v.numpy()
    np.savez_compressed(os.path.join(OUT, "fcae_trained.npz"), **d)
    print(f"fcae_trained: {len(sd)} tensors of {os.path.relpath(ck, REF)}")


if __name__ == "__main__":
    G.install_shim()
    sys.path.insert(0, REF)
    torch.set_num_threads(1)                                     # deterministic CPU reductions
    fixture_S()
    fixture_trained()
