#!/usr/bin/env python3
"""bench.py -- throughput of the ConvAE + gender-adversarial train step on MI355X.

  python bench.py --gpus N --steps K --warmup W          (N = 1 default; N > 1 without a torchrun
                                                          environment launches its own N ranks)
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
         --master-port P bench.py --gpus N --steps K --warmup W
  python bench.py ... --full                            (+ B = 10 point, roofline, CPU baseline)
  python bench.py ... --dump-outputs DIR                (+ the last timed step's results as DIR/*.npy)

One "step" = SexAnonymizationTraining.fit_batch on one synthetic 16 kHz batch per rank (weak
scaling): Fbank x2 + InputNormalization x2 + ConvAutoencoder fwd + L1 recon / NLL losses +
backward + clip_grad_norm_(5.0) + Adam + Noam (+ SyncBN statistic and gradient all-reduce on
N > 1).  Workload = BASELINE.json configs[1]: recon 0.1 + sex 0.9 adversarial, shape M of
SURVEY.md 8(d): B utterances of 161 120 samples -> T = 1008 frames each (B = 32 is `value`).
Inputs are resident in HBM when the timed region starts.  Prints ONE JSON line on rank 0.

A plain run measures `value` and nothing else.  --full adds what takes measurements of its own:
the B = 10 point of the same config (config.b10), the HIP-event roofline of the dominant kernel
family (roofline, roofline_family) and the CPU oracle baseline (cpu_baseline).
"""
import argparse
import json
import os
import socket
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0            # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.29 TB/s measured copy)
MFMA_PEAK_TFLOPS = {"bf16": 2500.0, "bf16x3": 2500.0, "f32": 157.3, "fp8": 5000.0}
MFMA_PER_FLOP = {"bf16": 1, "bf16x3": 3, "f32": 1, "fp8": 1}      # executed MFMA flops per algorithmic flop
N_SAMPLES = 161120               # -> T = 1 + N // 160 = 1008 frames (already a multiple of 36)
BYTES_PER_FRAME = {"f32": 862400, "bf16x3": 862400, "bf16": 431200, "fp8": 215600}
SETUP_STEPS = 8                  # un-timed, before the contract's W warm-up steps (see run_config)
KERNEL_T = {"bf16": "bf16", "bf16x3": "bf16x3_t", "f32": "float", "fp8": "fp8_t"}


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32,
                    help="utterances per GPU of shape M (BASELINE.md config 2: B 10 and B 32)")
    ap.add_argument("--dtype", default=os.environ.get("SA_BENCH_DTYPE", "bf16x3"),
                    choices=["bf16x3", "bf16", "f32", "fp8"],
                    help="bf16x3 (default): fp32 storage + split-bf16 operands on the bf16 MFMA, "
                         "the mode that passes the 1e-4 parity tests; bf16: bf16 storage, single MFMA")
    ap.add_argument("--samples", type=int, default=N_SAMPLES,
                    help="waveform samples per utterance (default 161120 = shape M; 480000 = the 30 s shape XL)")
    ap.add_argument("--full", action="store_true",
                    help="also measure config.b10, the roofline of the dominant kernel family and cpu_baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the last timed step's loss terms and the model state it "
                         "updated (parameters, buffers, normaliser statistics) as DIR/<name>.npy, float32")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip cpu_baseline")
    ap.add_argument("--no-b10", action="store_true", help="with --full: skip the secondary B = 10 measurement")
    ap.add_argument("--plumbing-only", action="store_true",
                    help="launcher / rendezvous / max-over-ranks timing / JSON relay with the train step "
                         "replaced by a sleep (CPU test of the N > 1 path; the line says so, it is NOT a measurement)")
    ap.add_argument("--graph", action="store_true",
                    help="replay the captured hipGraph of the step instead of launching eagerly (N = 1 only). "
                         "GPU time is the same (B = 32: 9.12-9.14 vs 9.04-9.10 ms); what differs is the host: "
                         "~190 launches per step cost 4-8 ms of host time depending on the box, 0.15 ms as a "
                         "replay.  Default: B = 32 eager (with --full its kernels are timed live with HIP "
                         "events), replay only if the eager region turns out host-bound on this box; the B = 10 "
                         "block of --full, which eager cannot keep GPU-bound (3.8 ms of GPU work per step), as a "
                         "replay")
    ap.add_argument("--no-graph", action="store_true", help="never replay a hipGraph (eager everywhere)")
    ap.add_argument("--dp-graph", action="store_true",
                    help="allow the hipGraph replay with more than one rank too (the RCCL all-reduces are "
                         "captured with the step; rehearsed on one rank only, hence opt-in here)")
    ap.add_argument("--master-port", type=int, default=0)
    ap.add_argument("--conv-impl", default="default", choices=["default", "one-tile", "pingpong"],
                    help="A/B timing of the conv kernels (default: weight-stationary where it covers)")
    ap.add_argument("--tile-rows", type=int, default=0, choices=[0, 64, 128],
                    help="A/B knob: output rows per workgroup of the one-tile conv kernel (0 = per-shape policy)")
    return ap.parse_args(argv)


# ------------------------------------------------------------------------------------------------
# N > 1 without a torchrun environment: start the ranks ourselves.  Nothing here touches the GPU
# (no HIP call, no torch.cuda.is_available()): the children are separate processes, never an exec
# of a process that initialised the device.
# ------------------------------------------------------------------------------------------------
def self_launch(args, argv):
    port = args.master_port
    if not port:
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + list(argv)
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "4")
    p = subprocess.Popen(cmd, stdout=subprocess.PIPE, env=env, text=True)
    line = None
    for ln in p.stdout:                     # relay rank 0's JSON line (and anything else) as it comes
        sys.stdout.write(ln)
        sys.stdout.flush()
        if ln.lstrip().startswith("{") and '"metric"' in ln:
            line = ln
    rc = p.wait()
    if rc != 0:
        raise SystemExit(rc)
    if line is None:
        raise SystemExit("bench.py: the ranks exited without printing a result line")
    return 0


def build_brain(device, dtype_name, batch, hip_graph=False):
    import functools
    import torch
    import speech_anonymization_amd as pkg
    from speech_anonymization_amd import brain as B, convae, losses
    torch.manual_seed(8886)
    model = convae.ConvAutoencoder(precision=dtype_name)
    hparams = dict(
        model_type="convae", compute_features=pkg.Fbank(16000, 400, 80).to(device),
        epoch_counter=B.EpochCounter(500),
        loss_reconstruction=losses.L1Loss(), loss_sex_classification=losses.NLLLoss(),
        loss_confusion=losses.ConfusionLoss(),
        recon_loss_weight=0.1, sex_loss_weight=0.9, utility_loss_weight=0.0,
        confusion_loss_weight=0.0, gradient_accumulation=1,
        noam_annealing=B.NoamScheduler(1.0, 25000, 768))
    hparams["epoch_counter"].current = 1
    adam_kw = dict(lr=0.001, betas=(0.9, 0.98), eps=1e-9)
    brain = B.SexAnonymizationTraining(
        modules={"normalize": pkg.InputNormalization("global", update_until_epoch=4)},
        opt_class=functools.partial(torch.optim.Adam, **adam_kw), hparams=hparams,
        run_opts={"device": str(device), "max_grad_norm": 5.0, "hip_graph": hip_graph})
    brain.modules["ConvAE"] = model.to(device)
    brain.on_fit_start()
    brain.modules.train()
    return brain


def synthetic_batch(batch, rank, device, n_samples=None):
    """0.1*randn + 220 Hz / 1 kHz / 3.4 kHz sinusoids, clipped, seed 8886+rank."""
    import torch
    from speech_anonymization_amd.brain import Batch
    g = torch.Generator(device="cpu").manual_seed(8886 + rank)
    n_samples = n_samples or N_SAMPLES
    t = torch.arange(n_samples, dtype=torch.float64) / 16000.0
    w = 0.1 * torch.randn(batch, n_samples, generator=g, dtype=torch.float64)
    for f, a in ((220.0, 0.2), (1000.0, 0.1), (3400.0, 0.05)):
        w += a * torch.sin(2 * torch.pi * f * t)[None, :]
    # utterances differ (amplitude / spectral tilt) like real batches do
    w *= torch.linspace(0.5, 1.5, batch, dtype=torch.float64)[:, None]
    wav = w.clamp(-1, 1).float().to(device)
    lens = torch.ones(batch, device=device)
    gender = (torch.arange(batch) % 2).to(device)
    return Batch(wav, lens, gender)


def cpu_model():
    try:
        for ln in open("/proc/cpuinfo"):
            if ln.startswith("model name"):
                return ln.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def usable_cores():
    """cores this process may really use: the affinity mask, capped by the cgroup CPU quota (the
    GPU box hands a 1-GPU job a 16-CPU share of a much larger host: an OpenMP pool sized by the
    affinity mask alone oversubscribes it many times over) and by 16."""
    n = len(os.sched_getaffinity(0))
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return max(1, min(n, 16))


def note(msg):
    """progress on stderr (stdout carries exactly one JSON line)"""
    print(f"[bench] {msg}", file=sys.stderr, flush=True)


def cpu_baseline():
    """the oracle (CPU restatement of the reference step, the same ATen CPU
    kernels the reference executes) at shape M, B = 10, every core this process may use, 2 warm-up
    steps + the median of 5 timed steps.  ~30 s of CPU work."""
    import torch
    from oracle.train_step import OracleTrainer
    from oracle.features import synthetic_wave
    threads = usable_cores()
    Bc, warm, steps = 10, 2, 5
    note(f"cpu baseline: oracle step, B={Bc}, {threads} threads, {warm}+{steps} steps")
    tr = OracleTrainer(threads=threads)
    wav = synthetic_wave(Bc, N_SAMPLES, seed=8886)
    lens, gender = torch.ones(Bc), torch.arange(Bc) % 2
    for _ in range(warm):
        tr.fit_batch(wav, lens, gender)
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        tr.fit_batch(wav, lens, gender)
        ts.append(time.perf_counter() - t0)
        note(f"cpu baseline step {ts[-1]:.2f} s")
    dt = statistics.median(ts)
    return {"value": Bc * 1008 / dt, "unit": "frames/s", "cores": threads, "kind": "port",
            "cpu_model": cpu_model(), "s_per_step": dt, "cores_in_affinity_mask": len(os.sched_getaffinity(0)),
            "sample": f"oracle train step (torch CPU fp32, {threads} threads), shape M: B={Bc} x T=1008 "
                      f"frames, {warm} warm-up + median of {steps} timed steps"}


def step_outputs(brain, loss):
    """what a caller of fit_batch holds after the last step: the loss it returned, the loss's two
    terms, and the state the step updated (every parameter and buffer of the modules, the
    normaliser's running statistics included), as float32 host arrays keyed by name (~2 MB)"""
    out = {"loss": loss, "recon_loss": brain.last_losses["recon"], "sex_loss": brain.last_losses["sex"]}
    out.update(brain.modules.named_parameters())
    out.update(brain.modules.named_buffers())
    return {k: t.detach().float().cpu().numpy() for k, t in out.items()}


def write_outputs(outputs, path):
    import numpy as np
    os.makedirs(path, exist_ok=True)
    for name, a in outputs.items():
        np.save(os.path.join(path, name + ".npy"), a)
    note(f"{len(outputs)} arrays ({sum(a.nbytes for a in outputs.values()) / 1e6:.1f} MB) written to {path}")


def run_config(args, batch_size, rank, world, device, profile_key=None, graph=None, dump=False):
    """SETUP_STEPS + args.warmup un-timed steps, then EXACTLY args.steps timed steps between
    barrier + synchronize on both sides; returns (elapsed max over ranks, last loss, profile of the
    dominant kernel, graph mode, host time spent issuing one step, step_outputs of the last timed
    step if `dump` else None)."""
    import torch
    from speech_anonymization_amd import ops
    ops.conv_impl(pingpong=args.conv_impl == "pingpong", ws=args.conv_impl == "default",
                  tile_rows=args.tile_rows)
    graph = (world == 1 or args.dp_graph) and (args.graph if graph is None else graph)
    brain = build_brain(device, args.dtype, batch_size, hip_graph=graph)
    batch = synthetic_batch(batch_size, rank, device, args.samples)

    def sync_all():
        if world > 1:
            torch.distributed.barrier()
        torch.cuda.synchronize()

    # set-up, before the W warm-up steps of the contract: the first steps of a process pay one-time
    # costs (code-object upload of ~60 kernels, allocator pools, operand-image tables, clock ramp).
    # Reported as "setup_steps"; not part of the timed region.
    for _ in range(SETUP_STEPS + args.warmup):
        brain.step += 1
        brain.fit_batch(batch)
    # what Brain.fit does after its first steps: without it the interpreter's first full garbage
    # collection (~100 ms of host time, ~60 steps into the process) lands wherever the step count
    # puts it -- possibly inside the timed region, where it would cost ten steps' worth of idle GPU
    from speech_anonymization_amd.brain import settle_python_heap
    settle_python_heap()
    sync_all()
    if profile_key and not graph:
        ops.PROFILE.enable(profile_key)               # dominant kernel: timed live with HIP events
    t0 = time.perf_counter()
    for _ in range(args.steps):
        brain.step += 1
        loss = brain.fit_batch(batch)
    host_issue = time.perf_counter() - t0            # the host has ISSUED all steps (no wait in the loop)
    sync_all()
    elapsed = time.perf_counter() - t0
    host_ms = host_issue / args.steps * 1e3
    outputs = step_outputs(brain, loss) if dump else None      # before any un-timed step below
    prof = ops.PROFILE.collect() if profile_key and not graph else None
    loss = float(loss)
    if profile_key and graph:
        # HIP events cannot be read back from inside a replayed hipGraph: the dominant kernel is
        # timed over the same number of EAGER steps right after the timed region (same kernels,
        # same shapes, same stream; the launches themselves are identical)
        brain.hip_graph = False
        brain.optimizer.zero_grad(set_to_none=True)
        for _ in range(2):
            brain.step += 1
            brain.fit_batch(batch)
        sync_all()
        ops.PROFILE.enable(profile_key)
        for _ in range(args.steps):
            brain.step += 1
            brain.fit_batch(batch)
        sync_all()
        prof = ops.PROFILE.collect()
        for p_ in prof:
            p_["timed_in"] = "eager steps after the timed region (events are not readable inside a replayed hipGraph)"
    if world > 1:
        tt = torch.tensor([elapsed], device=device, dtype=torch.float64)
        torch.distributed.all_reduce(tt, op=torch.distributed.ReduceOp.MAX)
        elapsed = float(tt)
    return elapsed, loss, prof, graph, host_ms, outputs


def roofline_of(prof, dtype):
    """SURVEY 8(d) accounting for one device kernel of the dominant family (sa_conv_gemm 128->128:
    encoder.11, decoder.0, the three TDNN convolutions and their five data gradients; the forward
    launches run on the weight-stationary kernel, the fused data gradients on the one-tile kernel):
      algorithmic bytes = input rows + output rows once each (fp32 storage: 2 560 + 2 560 elements
        per frame x 4 B) + on the data-gradient launches the stored forward tensor their fused
        norm/activation-backward epilogue re-reads (8(d)'s "norm/act-bwd re-read");
      algorithmic flops = 2 x MAC; the bf16x3 mode EXECUTES 3 MFMA flops per algorithmic flop.
    frac_hbm = algorithmic bytes / launch time / 8 TB/s; frac_mfma = executed flops / launch time /
    dense MFMA peak.  The binding roof is the one whose minimum time is larger; `frac` is the
    fraction of THAT roof.  designed_bytes = what the kernel is built to move (adds the bf16
    operand cache it writes and the second tensor of the fused apply prologue) -- informational."""
    if not prof or not prof["launches"]:
        return None
    n = prof["launches"]
    avg_s = prof["ms"] * 1e-3 / n
    alg_b, des_b, flops = prof["alg_bytes"] / n, prof["bytes"] / n, prof["flops"] / n
    mult = MFMA_PER_FLOP[dtype]
    peak_tf = MFMA_PEAK_TFLOPS[dtype]
    frac_hbm = alg_b / avg_s / 1e9 / HBM_PEAK_GBS
    frac_mfma = flops * mult / avg_s / 1e12 / peak_tf
    t_hbm, t_mfma = alg_b / (HBM_PEAK_GBS * 1e9), flops * mult / (peak_tf * 1e12)
    if t_hbm >= t_mfma:
        roof = {"bound": "hbm", "achieved": alg_b / avg_s / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": frac_hbm}
    else:
        roof = {"bound": "mfma", "achieved": flops * mult / avg_s / 1e12, "peak": peak_tf,
                "unit": "TFLOP/s", "frac": frac_mfma}
    roof.update({
        "traffic": None, "kernel": prof["kernel"],
        "launches_timed": n, "avg_us": avg_s * 1e6,
        "timed_in": prof.get("timed_in", "the timed region (HIP events on the launch stream)"),
        "algorithmic_bytes": alg_b, "algorithmic_flops": flops, "designed_bytes": des_b,
        "frac_hbm": frac_hbm, "frac_mfma": frac_mfma,
        "roof_time_us": {"hbm": t_hbm * 1e6, "mfma": t_mfma * 1e6},
        "mfma_flops_executed_per_algorithmic_flop": mult,
        "hbm_gbs": alg_b / avg_s / 1e9, "tflops_algorithmic": flops / avg_s / 1e12,
        "tflops_executed": flops * mult / avg_s / 1e12})
    return roof


def attach_pmc_traffic(roof, dtype, batch):
    """HBM bytes per launch of the same kernel from the rocprofv3 --pmc passes of this config
    (tools/pmc_traffic.py writes profiles/pmc_traffic.json; FETCH_SIZE x2 correction, WRITE_SIZE).
    A separate profiled run, not this process: the source is named beside the number."""
    try:
        pm = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json")))
        key = "%s:B%d:%s" % (dtype, batch, roof["kernel"])
        if key in pm:
            roof["traffic"] = pm[key]["total_bytes"]
            roof["traffic_source"] = pm[key].get("source", "profiles/pmc_traffic.json (rocprofv3 --pmc, separate run)")
            roof["traffic_over_algorithmic"] = pm[key]["total_bytes"] / roof["algorithmic_bytes"]
    except Exception:
        pass


def step_traffic(dtype, batch, T):
    """HBM bytes of ONE train step summed over every kernel, from the rocprofv3 --pmc passes of this
    configuration (profiles/pmc_traffic.json "<dtype>:B<batch>:step", written by tools/pmc_traffic.py
    --json; a separate profiled run: `source` names it), beside the algorithmic figure of SURVEY 8(d)."""
    try:
        pm = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json")))
        e = pm["%s:B%d:step" % (dtype, batch)]
        alg = BYTES_PER_FRAME[dtype] * batch * T
        return {"bytes": e["total_bytes"], "read_bytes": e["read_bytes"], "write_bytes": e["write_bytes"],
                "algorithmic_bytes": alg, "over_algorithmic": e["total_bytes"] / alg, "source": e.get("source")}
    except Exception:
        return None


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    args = parse_args(argv)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return self_launch(args, argv)

    import torch
    from speech_anonymization_amd import distributed as sdist
    rank, local_rank, world = sdist.ddp_init_group()
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    dp = sdist.dp_active()           # world > 1, or the one-rank RCCL rehearsal (SA_FORCE_DP=1)
    backend = ("sa_comm (library-owned RCCL communicator)" if sdist.lib_comm_active()
               else torch.distributed.get_backend() if dp else "none")
    ranks_seen = torch.distributed.get_world_size() if dp else 1
    T = 1 + args.samples // 160
    T += (-T) % 36                                  # frames entering the ConvAE (padded to 36)

    if args.plumbing_only:
        # the N > 1 path without the GPU step: rendezvous, barriers, max-over-ranks, JSON on rank 0
        torch.distributed.barrier() if world > 1 else None
        t0 = time.perf_counter()
        time.sleep(0.01 * args.steps * (1 + rank))          # ranks differ: MAX must pick the slowest
        torch.distributed.barrier() if world > 1 else None
        elapsed = time.perf_counter() - t0
        if world > 1:
            tt = torch.tensor([elapsed], dtype=torch.float64)
            torch.distributed.all_reduce(tt, op=torch.distributed.ReduceOp.MAX)
            elapsed = float(tt)
        if rank == 0:
            print(json.dumps({"metric": "audio frames/sec (node), ConvAE+gender-adv train step",
                              "value": None, "plumbing_only": True, "n_gpus": world, "steps": args.steps,
                              "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3,
                              "ranks_seen": ranks_seen, "backend": backend}), flush=True)
        if world > 1:
            torch.distributed.barrier()
            torch.distributed.destroy_process_group()
        return 0

    device = torch.device("cuda", local_rank)
    torch.cuda.set_device(device)

    dump = args.dump_outputs is not None and rank == 0
    elapsed, loss, prof, graph, host_b, outputs = run_config(
        args, args.batch, rank, world, device, profile_key="conv_gemm(128,128,1,1)" if args.full else None,
        dump=dump)
    eager_ms = None
    if (world == 1 and not graph and not args.no_graph
            and host_b > 0.9 * elapsed / args.steps * 1e3):
        # this box's host cannot issue ~190 launches per step as fast as the GPU retires them: the
        # timed region above measured the host.  Same K steps as a hipGraph replay (run_opts
        # hip_graph, the product's answer to exactly this); the dominant kernel's HIP-event timing
        # stays the one taken live in the eager region (its duration does not depend on who issued it)
        note(f"eager region host-bound ({host_b:.2f} ms issue / {elapsed / args.steps * 1e3:.2f} ms step): replaying as hipGraph")
        try:
            e2, l2, _, _, h2, o2 = run_config(args, args.batch, rank, world, device, graph=True, dump=dump)
        except Exception as exc:                      # the eager measurement above stands
            note(f"hipGraph replay failed ({type(exc).__name__}: {exc}); keeping the eager region")
            e2 = float("inf")
        if e2 < elapsed:
            eager_ms, elapsed, loss, graph, host_b, outputs = elapsed / args.steps * 1e3, e2, l2, True, h2, o2
    frames = world * args.batch * T * args.steps
    value = frames / elapsed
    if rank == 0:
        note(f"B={args.batch}: {value:.4g} frames/s, {elapsed / args.steps * 1e3:.3f} ms/step")
    if dump:
        write_outputs(outputs, args.dump_outputs)
    b10 = None
    if args.full and not args.no_b10 and args.batch != 10 and args.samples == N_SAMPLES:
        g10_want = False if args.no_graph else (True if (world == 1 or args.dp_graph) else None)
        try:
            e10, l10, _, g10, host10, _ = run_config(args, 10, rank, world, device, graph=g10_want)
        except Exception as exc:
            if not g10_want:
                raise
            note(f"hipGraph replay failed at B=10 ({type(exc).__name__}: {exc}); eager")
            e10, l10, _, g10, host10, _ = run_config(args, 10, rank, world, device, graph=False)
        b10 = {"batch_per_gpu": 10, "value": world * 10 * T * args.steps / e10, "unit": "frames/s",
               "ms_per_step": e10 / args.steps * 1e3, "host_issue_ms_per_step": host10,
               "hip_graph": bool(g10), "loss": l10}

    if rank == 0:
        # one record per device kernel of the family, largest total time first: `roofline` is the
        # dominant one, `roofline_family` lists all of them (same accounting)
        roofs = [r for r in (roofline_of(p, args.dtype) for p in (prof or [])) if r]
        for r in roofs:
            attach_pmc_traffic(r, args.dtype, args.batch)
        roof = roofs[0] if roofs else None
        out = {
            "metric": "audio frames/sec (node), ConvAE+gender-adv train step", "value": value,
            "unit": "frames/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "setup_steps": SETUP_STEPS,
            "ms_per_step": elapsed / args.steps * 1e3, "host_issue_ms_per_step": host_b, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": args.dtype, "data": "synthetic", "full": args.full,
            "ranks_seen": ranks_seen, "backend": backend, "hip_graph": graph,
            "eager_ms_per_step": eager_ms,     # set when the eager region was host-bound and the K steps were re-timed as a replay
            "config": {"workload": "ConvAE recon0.1+sex0.9 adversarial train step (L1 recon + NLL), "
                                   f"shape {'M' if args.samples == N_SAMPLES else 'custom'}: {args.batch} utt/GPU x "
                                   f"{args.samples} samples (T={T} frames), "
                                   "Fbank x2 + norm + fwd + bwd + clip + Adam + Noam",
                       "batch_per_gpu": args.batch, "frames_per_utt": T, "parallelism": f"dp{world}",
                       "loss": loss, "b10": b10},
            "step_hbm_roofline_frac": value * BYTES_PER_FRAME[args.dtype] / (world * HBM_PEAK_GBS * 1e9),
            "step_traffic": step_traffic(args.dtype, args.batch, T),
            "roofline": roof,
            "roofline_family": [{k: r[k] for k in ("kernel", "launches_timed", "avg_us", "bound", "frac", "frac_hbm",
                                                   "frac_mfma", "algorithmic_bytes", "algorithmic_flops", "traffic")}
                                for r in roofs],
        }
        if args.full and world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline()
        print(json.dumps(out), flush=True)
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
