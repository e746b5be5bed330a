#!/usr/bin/env python3
"""Times the frozen (eval-mode) x-vector gender classifier at B = 32, T = 1008: the no-grad forward
(classify_batch_feats) and EncoderClassifier.forward plus backward to the features, which is how
the `endtoend` training graph runs it (the only user of sa_tdnn_bwd_kernel).

Device events around each iteration after a warm-up; the median of --iters iterations.  Prints one
JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def median_ms(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--T", type=int, default=1008)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    assert a.iters >= 20, "the median of at least 20 iterations"
    from speech_anonymization_amd import xvector as HX
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    enc = HX.EncoderClassifier(HX.Xvector(pooling_noise=None), HX.Classifier(input_shape=[None, None, 128]))
    enc.to(dev).eval()
    feats = torch.randn(a.B, a.T, 80, device=dev)
    lens = torch.ones(a.B, device=dev)
    d_logp = torch.randn(a.B, 2, device=dev)

    def fwd():
        enc.classify_batch_feats(feats, lens)

    def fwd_bwd():
        x = feats.clone().requires_grad_(True)
        enc(x, lens)[0].backward(d_logp)

    print(json.dumps({"B": a.B, "T": a.T, "iters": a.iters,
                      "fwd_ms": round(median_ms(fwd, a.warmup, a.iters), 4),
                      "fwd_bwd_ms": round(median_ms(fwd_bwd, a.warmup, a.iters), 4)}))


if __name__ == "__main__":
    main()
