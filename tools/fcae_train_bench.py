#!/usr/bin/env python3
"""Times one train step of model_type fcae (forward, 0.5 MSE + 0.5 NLL, backward, gradient clipping at 5.0,
Adam) at B = 32, T = 1008 and at the reference's B = 3 on the HIP path (speech_anonymization_amd.fcae), and
torch's own fp32 autograd step of tests/fcae_ref.py moved to the GPU as a yardstick in the same run.

Device events around each step after a warm-up; the median of --steps steps.  Launches per step are the
device kernels torch.profiler sees in one step (model, losses, clip and Adam together).  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

MFLOP_PER_FRAME = 2 * 18400 * 3 / 1e6          # forward + data gradients + weight gradients of the per-frame Linears


def time_steps(step, warmup, steps):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        step()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def launches(step):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
                   and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())
    except Exception:                                            # no profiler in this build: the count is optional
        return None


def make_step(model, feats, label, fused_clip):
    params = list(model.parameters())
    opt = torch.optim.Adam(params, lr=1e-3, fused=True)
    B = feats.shape[0]

    def step():
        recon, logp = model(feats)
        loss = 0.5 * F.mse_loss(recon.view(B, -1), feats.view(B, -1)) + 0.5 * F.nll_loss(logp, label)
        loss.backward()
        flats = getattr(model, "_last_flats", None) if fused_clip else None
        if flats:
            from speech_anonymization_amd import ops
            ops.clip_flats(flats, 5.0)                           # what Brain.check_gradients does on the flat bucket
        else:
            torch.nn.utils.clip_grad_norm_(params, 5.0)
        opt.step()
        opt.zero_grad()
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=1008)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch fp32 yardstick")
    a = ap.parse_args()
    assert a.steps >= 20, "the median of at least 20 steps"
    dev = torch.device("cuda:0")
    from speech_anonymization_amd import fcae
    from tests import fcae_ref
    out = {"T": a.T, "steps": a.steps, "torch_allow_tf32": torch.backends.cuda.matmul.allow_tf32}
    for B in (32, 3):
        torch.manual_seed(0)
        feats = torch.randn(B, a.T, 80, device=dev)
        label = torch.arange(B, device=dev) % 2
        ref = fcae_ref.FullyConnectedAutoencoder(80, B)
        hip = fcae.FullyConnectedAutoencoder(80, B, pooling_noise=False)
        hip.load_state_dict(ref.state_dict())
        step = make_step(hip.to(dev).train(), feats, label, True)
        ms = time_steps(step, a.warmup, a.steps)
        rec = {"ms_per_step": round(ms, 4), "launches_per_step": launches(step),
               "frames_per_s": round(B * a.T / ms * 1e3, 1),
               "gflop_per_step": round(MFLOP_PER_FRAME * B * a.T / 1e3, 3)}
        if not a.no_torch:
            tstep = make_step(ref.to(dev).train(), feats, label, False)
            tms = time_steps(tstep, a.warmup, a.steps)
            rec.update({"torch_fp32_ms_per_step": round(tms, 4), "torch_launches_per_step": launches(tstep),
                        "speedup_vs_torch_fp32": round(tms / ms, 3)})
        out[f"B{B}"] = rec
    print(json.dumps(out))


if __name__ == "__main__":
    main()
