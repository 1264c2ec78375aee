"""Headline benchmark: training images/s of the Onet twin 256x256 pass on N MI355X
(BASELINE.json metric), one process per GPU, weak scaling (per-GPU batch fixed).

    python bench.py --gpus 1 --steps 5 --warmup 2
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...
    python bench.py --gpus N          # N > 1 without a launcher: starts the line above itself, as a CHILD process

A step = zero_grad + twin forward + JSD loss + backward + [RCCL all-reduce] + fused Adam on one
synthetic K-distributed clutter batch already resident in HBM (TS:209-219 order).  Prints ONE JSON
line on rank 0.  A plain run sets up, warms up, times --steps steps and prints the headline (`value`,
`ms_per_step`); --dump-outputs DIR also writes what the last timed step computed (dump_outputs).

--full adds everything else, each part measured after the headline's timed region: `roofline` (dominant
MFMA kernel, HIP-event timed inside the timed region, plus a fully bracketed breakdown loop),
`f32_mfma_only`, `reference_loop`, for N > 1 the with / without-overlap `comm` curve, and, at N=1,
`cpu_baseline` (the CPU oracle timed on the host cores on the SAME batch) and `secondary` (BASELINE
configs[2]: the bf16 MFMA conv path at B=256, run in a child process of its own so that it starts from a
fresh allocator).

Nothing in this file touches the GPU (no torch / onet_amd import) before `_self_launch` has had its chance:
a process that has initialised HIP must not be replaced or forked into ranks."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
torch = dist = None          # imported by main(), after the launcher decision

FP32_MFMA_PEAK_TFLOPS = 157.3      # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 = fp32 vector rate
BF16_MFMA_PEAK_TFLOPS = 2500.0     # MI355X_MICROARCH.md: dense bf16 MFMA (no sparsity)
HBM_PEAK_GBPS = 8000.0             # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.29 TB/s measured float4 copy)
PMC_JSON = os.path.join(ROOT, "profiles", "pmc_bench_latest.json")   # written by tools/pmc_parse.py


def pmc_traffic(kernel_prefix, bf16=False, batch=32):
    """HBM bytes per launch of the dominant kernel from the committed rocprofv3 --pmc passes of THIS
    command (FETCH_SIZE and WRITE_SIZE in separate passes, FETCH_SIZE doubled per the gfx950
    correction).  PMC counters cannot be collected inside the timed run, so the number comes from
    profiles/ (the default fp32 B=32 run: pmc_bench_latest.json; other configurations:
    pmc_bench_<f32|bf16>_b<batch>_latest.json); None if the file is absent."""
    path = PMC_JSON if (not bf16 and batch == 32) else os.path.join(
        ROOT, "profiles", "pmc_bench_%s_b%d_latest.json" % ("bf16" if bf16 else "f32", batch))
    try:
        d = json.load(open(path))
    except Exception:
        return None
    # bench.py names a kernel FAMILY by the label its Python wrapper times it under; since round 5 a family has two device kernels
    # (the v_mfma_f32_16x16x32 forms) and the profile's keys are device kernel names
    prefixes = {"conv3x3_split_pre_kernel": ("conv3x3_split_pre_kernel", "conv3x3_pre16_kernel"),
                "conv3x3_split_wgrad_pre_kernel": ("conv3x3_split_wgrad_pre_kernel", "conv3x3_wgrad_pre16_kernel")}.get(kernel_prefix, (kernel_prefix,))
    tot_b = tot_n = 0
    for k, v in d.items():
        if k.startswith(prefixes) and "hbm_bytes_per_launch" in v:
            n = v["FETCH_SIZE"]["launches"]
            tot_b += v["hbm_bytes_per_launch"] * n
            tot_n += n
    return (tot_b / tot_n) if tot_n else None


def _cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def _host_cores():
    """Cores this process may actually use: the affinity mask, capped by the cgroup CPU quota (a GPU box hands each job a
    share of the host; os.cpu_count() reports the whole machine and 128 threads on a 16-core share run 3x slower than 16)."""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            n = max(1, min(n, int(float(quota) / float(period) + 0.5)))
    except (OSError, ValueError):
        pass
    return n


def cpu_baseline(X_cpu, seconds_budget):
    """fwd + loss + bwd + Adam of the CPU oracle (PyTorch CPU fp32: the same ATen / oneDNN kernels the reference runs
    on CPU) on the host cores of this box, for n = all cores and n = 8 threads.  The sample is the first
    B_s images of the SAME synthetic batch, B_s = the largest power of two <= the benchmark batch of which two timed steps
    fit a thread setting's share of the budget (estimated from a B=2 warm-up step); up to 3 steps are timed while they fit.
    At the default budget that is the WHOLE configs[1] batch (32 / 32 images)."""
    from oracle import onet_oracle as orc
    ncores = _host_cores()
    settings = [ncores] + ([8] if ncores > 8 else [])
    per_setting = seconds_budget / len(settings)
    by_threads, sample, nsteps = {}, {}, {}
    for n in settings:
        torch.set_num_threads(n)
        top = orc.clone_state(orc.det_state_dict(X_cpu.shape[1], 1981, randomize_running=False))
        params = [v for v in top.values() if v.requires_grad]
        opt = torch.optim.Adam(params, lr=5e-6, betas=(0.9, 0.999), eps=1e-8)

        def step(xs):
            t0 = time.perf_counter()
            opt.zero_grad()
            orc.train_mode_step(xs, top)
            opt.step()
            return time.perf_counter() - t0

        t_warm = step(X_cpu[:2].contiguous())                 # warm-up (allocator, oneDNN primitive cache) + estimate
        bs = 2
        while bs * 2 <= X_cpu.shape[0] and 2 * t_warm * (bs * 2) / 2 <= per_setting - t_warm:
            bs *= 2
        if bs * 2 > X_cpu.shape[0] and 2 * t_warm * X_cpu.shape[0] / 2 <= per_setting - t_warm:
            bs = X_cpu.shape[0]                               # a batch that is not a power of two: all of it
        xs = X_cpu[:bs].contiguous()
        times, t_begin = [], time.perf_counter()
        for _ in range(3):
            if times and (time.perf_counter() - t_begin) + max(times) > per_setting:
                break
            times.append(step(xs))
            sys.stderr.write("[cpu_baseline] n=%d B=%d step %.2f s\n" % (n, bs, times[-1]))
            sys.stderr.flush()
        by_threads[str(n)] = round(bs / (sum(times) / len(times)), 4)
        sample[str(n)], nsteps[str(n)] = bs, len(times)
    torch.set_num_threads(ncores)
    n0 = str(settings[0])
    B = X_cpu.shape[0]
    return {"value": by_threads[n0], "unit": "images/s", "cores": settings[0], "kind": "port",
            "cpu_model": _cpu_model(), "host_cpus": os.cpu_count(), "by_threads": by_threads,
            "sample": "%s of the %d images (n=%s threads) of the same %dx%dx%d K-clutter batch the GPU ran; per thread setting 1 "
                      "warm-up step at B=2 + %s timed full training steps (zero_grad+fwd+loss+bwd+Adam) of the CPU oracle"
                      % ("/".join(str(sample[k]) for k in by_threads), B, "/".join(by_threads), X_cpu.shape[1],
                         X_cpu.shape[2], X_cpu.shape[3], "/".join(str(nsteps[k]) for k in by_threads))}


def comm_curve(onet, opt, X, train_step, barrier, dev, nsteps, overlap, bucket_mb):
    """SURVEY 8e's with / without-overlap curve, measured behind the timed region on the same replicas: the same step with
    (a) ONE all-reduce of the flat gradient after backward, (b) the bucketed all-reduces overlapped with backward (the headline's
    --bucket-mb), (c) NO all-reduce at all (compute only; the replicas drift apart, which is why this runs last and why the
    caller reads the loss BEFORE calling this).  Max over ranks of each; allreduce_exposed_ms = the headline's ms/step - (c).
    The mode the headline ran is not timed twice, and the optimizer is handed back in the headline's mode."""
    import torch.distributed as dist

    def timed():
        for _ in range(2):
            train_step(onet, opt, X)
        barrier()
        t0 = time.perf_counter()
        for _ in range(nsteps):
            train_step(onet, opt, X)
        barrier()
        t = torch.tensor([time.perf_counter() - t0], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return round(float(t.item()) / nsteps * 1e3, 3)

    out = {"steps": nsteps, "bucket_mb": bucket_mb}
    if overlap:
        opt.disable_overlap()
        out["no_overlap_ms"] = timed()
    else:
        opt.enable_overlap(bucket_mb)
        out["overlap_ms"] = timed()
        opt.disable_overlap()
    opt.skip_allreduce = True
    out["no_allreduce_ms"] = timed()
    opt.skip_allreduce = False
    if overlap:                      # back to the headline's mode
        opt.enable_overlap(bucket_mb)
    return out


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _relay_child(cmd, env=None):
    """Run `cmd` as a child process; stderr is inherited (progress stays visible), stdout is returned.  -> (rc, stdout)."""
    proc = subprocess.Popen(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, text=True)
    out, _ = proc.communicate()
    return proc.returncode, out or ""


def _visible_gpu_count():
    """GPUs this process tree will see, WITHOUT touching the HIP runtime (the launcher parent must stay GPU-free: it starts the
    ranks as children): KFD topology nodes with compute units (/sys/class/kfd/kfd/topology/nodes/*/properties: simd_count > 0),
    narrowed by ROCR_VISIBLE_DEVICES / HIP_VISIBLE_DEVICES / CUDA_VISIBLE_DEVICES when they list indices.  -> 0 without a KFD driver,
    None if the topology exists but cannot be read (then nothing is checked here; the ranks check for themselves)."""
    root = "/sys/class/kfd/kfd/topology/nodes"
    if not os.path.isdir("/sys/class/kfd"):
        return 0                  # no KFD driver on this host: no AMD GPU for any process
    try:
        n = 0
        for node in os.listdir(root):
            try:
                props = dict(ln.split()[:2] for ln in open(os.path.join(root, node, "properties")) if len(ln.split()) >= 2)
            except OSError:
                continue
            if int(props.get("simd_count", "0")) > 0:
                n += 1
    except OSError:
        return None
    for var in ("ROCR_VISIBLE_DEVICES", "HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        v = os.environ.get(var)
        if v is not None:
            ids = [t for t in v.split(",") if t.strip() != ""]
            n = min(n, len(ids))
    return n


def _preflight(n_gpus, local=None, in_rank=False):
    """A clear message BEFORE any rank is started / any collective is entered when the node has fewer GPUs than --gpus asks for.
    The launcher parent counts KFD topology nodes (no HIP call: it must not initialise the runtime it then spawns ranks under);
    a rank (in_rank) asks torch.cuda.device_count(), which is what it will actually be able to open.  ONET_FORCE_LOCAL_RANK (the
    one-GPU rehearsal: N ranks sharing cuda:0 over gloo) waives the check."""
    if "ONET_FORCE_LOCAL_RANK" in os.environ:
        return
    if in_rank:
        import torch as _t
        have, how = _t.cuda.device_count(), "torch.cuda.device_count()"
    else:
        have, how = _visible_gpu_count(), "KFD topology + *_VISIBLE_DEVICES"
        if have is None:
            return
    if have < n_gpus or (local is not None and local >= have):
        sys.stderr.write("[bench] --gpus %d, but this node exposes %d GPU(s) to the process (%s; check "
                         "HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES): nothing was launched\n" % (n_gpus, have, how))
        sys.stderr.flush()
        raise SystemExit(2)


def _self_launch(args, argv):
    """`python bench.py --gpus N` (N > 1) outside a launcher: THIS process (which has not imported torch / onet_amd and
    makes no GPU call: the preflight reads sysfs) starts `python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py <same arguments>`
    as a child, relays rank 0's JSON line and exits with the child's code.  No exec, no retry."""
    _preflight(args.gpus)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)] + list(argv)
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")          # dmabuf IPC: RCCL across processes needs it on this image
    env.setdefault("OMP_NUM_THREADS", "1")
    sys.stderr.write("[bench] --gpus %d without a launcher: starting %s\n" % (args.gpus, " ".join(cmd)))
    sys.stderr.flush()
    rc, out = _relay_child(cmd, env)
    for ln in out.splitlines():
        if ln.startswith("{"):
            print(ln, flush=True)
        elif ln.strip():
            sys.stderr.write(ln + "\n")
    return rc


SECONDARY_ARGS = ["--gpus", "1", "--conv", "bf16", "--batch", "256", "--warmup", "8", "--steps", "5", "--full",
                  "--no-cpu-baseline", "--no-secondary", "--no-reference-loop"]
DUMP_SAMPLE = 1 << 22      # values of the flat parameter / gradient vectors written by --dump-outputs (16 MiB each in fp32)


def dump_outputs(path, model, loss):
    """--dump-outputs: what the last timed step handed its caller -- the loss, the updated parameters, their gradients and the
    BatchNorm running statistics -- as float32 .npy files under `path`.  Parameters and gradients (31 M values each) are a
    fixed sample: the same DUMP_SAMPLE positions of the flat vectors (model.parameters() order) in every run."""
    import numpy as np
    params = list(model.parameters())
    flat_p = torch.cat([p.detach().reshape(-1) for p in params])
    flat_g = torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).detach().reshape(-1) for p in params])
    n = flat_p.numel()
    idx = np.sort(np.random.default_rng(1981).choice(n, min(n, DUMP_SAMPLE), replace=False))
    idx = torch.from_numpy(idx).to(flat_p.device)
    arrays = {"loss": loss.detach().reshape(1), "params_sample": flat_p[idx], "grads_sample": flat_g[idx],
              "bn_running_stats": torch.cat([b.detach().reshape(-1) for k, b in model.named_buffers()
                                             if k.endswith(("running_mean", "running_var"))])}
    os.makedirs(path, exist_ok=True)
    for name, t in arrays.items():
        np.save(os.path.join(path, name + ".npy"), t.float().cpu().numpy())


def secondary_config2():
    """BASELINE configs[2] (B=256 1x256x256, bf16 MFMA conv path, one GPU) measured by the same program in a child process,
    after the headline's timed region and with the parent's HBM released.  -> the object attached as
    out["secondary"]["configs[2]"]; a failure is reported in the object, it does not fail the headline line."""
    cmd = [sys.executable, os.path.abspath(__file__)] + SECONDARY_ARGS
    t0 = time.perf_counter()
    try:
        rc, out = _relay_child(cmd)
    except Exception as e:      # noqa: BLE001
        return {"error": "could not start the child: %r" % (e,), "cmd": " ".join(cmd[1:])}
    lines = [ln for ln in out.splitlines() if ln.startswith("{")]
    if rc != 0 or len(lines) != 1:
        return {"error": "child exited %d with %d JSON lines" % (rc, len(lines)), "cmd": " ".join(cmd[1:])}
    d = json.loads(lines[0])
    r = d.get("roofline", {})
    keep = ("kernel", "bound", "achieved", "peak", "unit", "frac", "mfma_frac", "hbm_frac", "traffic", "traffic_unit",
            "compulsory_bytes_per_launch", "launches_timed", "avg_launch_ms", "algorithm", "kernels", "step")
    sec = {k: d[k] for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "dtype", "precision", "data",
                             "config", "loss", "hbm_peak_gb", "device_allocs_per_timed_step") if k in d}
    sec["roofline"] = {k: r[k] for k in keep if k in r}
    if "streaming" in r:
        sec["roofline"]["streaming"] = {k: v for k, v in r["streaming"].items() if k != "kernels"}
    sec["cmd"] = "python bench.py " + " ".join(SECONDARY_ARGS)
    sec["child_wall_s"] = round(time.perf_counter() - t0, 1)
    return sec


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32, help="images per GPU (weak scaling)")
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--chans", type=int, default=1)
    ap.add_argument("--conv", default=None, choices=["auto", "split", "bf16", "winograd4", "winograd", "direct"],
                    help="ops.CONV_ALGO for this run (default: ONET_CONV_ALGO or auto = the fp32 kernels); bf16 = BASELINE "
                         "config 3's bf16-operand MFMA path for forward / input gradient")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--mfma-events-only", action="store_true",
                    help="timed region: HIP-event brackets around every MFMA launch (default: around the dominant kernel's launches only)")
    ap.add_argument("--bracket-all", action="store_true",
                    help="timed region: HIP-event brackets around EVERY launch of the library (costs ~1 ms/step at B=32; default: the "
                         "dominant kernel's launches only, and the whole-step breakdown from a separate bracketed loop after the timed region)")
    ap.add_argument("--cpu-seconds", type=float, default=200.0,
                    help="budget of the CPU-oracle baseline (split over the thread settings n = all cores and n = 8); the "
                         "default fits the whole configs[1] batch (B=32, ~28 s per step on 16 cores)")
    ap.add_argument("--no-f32-mfma-only", action="store_true",
                    help="skip the extra loop with the fp32-MFMA kernels only (profiling runs: keeps the kernel trace to the headline's kernels)")
    ap.add_argument("--no-reference-loop", action="store_true",
                    help="skip the extra loop that restores TS:211's per-step host-to-device copy and TS:219's per-step loss.item()")
    ap.add_argument("--no-secondary", action="store_true",
                    help="do not attach BASELINE configs[2] (bf16, B=256) as `secondary` (default at N=1 with the headline "
                         "configuration: attached)")
    ap.add_argument("--torch-adam", action="store_true", help="use torch.optim.Adam instead of the fused flat Adam")
    ap.add_argument("--no-overlap", action="store_true",
                    help="one gradient all-reduce after backward instead of bucketed all-reduces overlapped with it")
    ap.add_argument("--bucket-mb", type=float, default=32.0)
    ap.add_argument("--host-data", action="store_true", help="synthesise the batch with the NumPy generator on the host")
    ap.add_argument("--no-comm-curve", action="store_true",
                    help="N > 1: skip the two extra loops (single all-reduce after backward; no all-reduce) behind the timed region")
    ap.add_argument("--full", action="store_true",
                    help="also measure everything beyond the headline: roofline and per-kernel tables, f32_mfma_only, reference_loop, "
                         "the N > 1 comm curve, cpu_baseline and secondary (the --no-* options above leave parts out)")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write what the last timed step computed (loss, sampled parameters and gradients, BatchNorm running "
                         "statistics) as float32 DIR/<name>.npy")
    args = ap.parse_args(argv)
    if (args.bracket_all or args.mfma_events_only) and not args.full:
        ap.error("--bracket-all / --mfma-events-only choose the roofline's HIP-event brackets: they need --full")
    return args


def main(args):
    global torch, dist
    import torch
    import torch.distributed as dist
    from onet_amd import Onet, _lib, ops
    from onet_amd import data as odata
    from onet_amd.trainer import FlatAdam, init_distributed, train_step
    _lib.load()                      # fail loudly without the HIP library
    conv = args.conv or ops.CONV_ALGO
    bf16 = conv == "bf16"

    if int(os.environ.get("WORLD_SIZE", "1")) != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%s" % (args.gpus, os.environ.get("WORLD_SIZE", "1")))
    _preflight(args.gpus, int(os.environ.get("LOCAL_RANK", "0")), in_rank=True)
    rank, world, local = init_distributed("nccl")
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)

    torch.manual_seed(1981)
    onet = Onet(in_chns=args.chans, binit=True, bshare=True).to(dev)
    # the model carries its switches (no process globals).  The loop owns the optimizer step: the loss's NaN assertion (OV:234)
    # is evaluated by FlatAdam.step() before the update instead of by a device synchronisation between forward and backward
    onet.settings = ops.Settings(conv=conv, lazy_nan=not args.torch_adam)
    opt = (torch.optim.Adam(onet.parameters(), lr=5e-6, betas=(0.9, 0.999), eps=1e-8) if args.torch_adam
           else FlatAdam(onet, lr=5e-6, world_size=world))
    if not args.torch_adam:
        opt.broadcast_params(0)
    distributed = dist.is_available() and dist.is_initialized()
    overlap = distributed and not args.torch_adam and not args.no_overlap
    if overlap:
        opt.enable_overlap(args.bucket_mb)
    onet.train()

    # the rank's shard of the synthetic batch, made ON its GPU (csrc/clutter.hip: frames depend on (seed, frame index) only, so
    # seed + rank gives every rank its own frames without N hosts' worth of SciPy gammaincinv before the first barrier); shapes the
    # GPU generator does not cover (3-channel 512 x 512 tiles) keep the NumPy statement of the same recipe
    if args.chans == 1 and max(args.size, args.size) <= odata.FRAME and not args.host_data:
        X = odata.make_clutter_batch_gpu(args.batch, args.size, args.size, seed=1981 + rank, device=dev)
        data_src = "synthetic K-clutter generated on the GPU (onet_clutter_generate, seed 1981 + rank)"
    else:
        X = torch.from_numpy(odata.make_clutter_batch(args.batch, args.size, args.size, seed=1981 + rank,
                                                      channels=args.chans)).to(dev)
        data_src = "synthetic K-clutter generated on the host (NumPy statement of the same recipe, seed 1981 + rank)"
    X = X.contiguous()               # inputs resident in HBM before the timed region

    def barrier():
        if distributed:
            dist.barrier()
        torch.cuda.synchronize()

    loss = X_cpu = None
    # the warm-up steps also say which MFMA kernel dominates the step: the timed region then brackets THAT kernel's launches only
    # (HIP events on the launch stream) -- bracketing all ~300 launches of a step costs ~1 ms of it
    if args.full and args.warmup > 0:
        ops.profile_start(everything=False)
    for _ in range(args.warmup):
        loss = train_step(onet, opt, X)      # (held like in the timed loop: the caching allocator sees the same liveness pattern)
    barrier()
    dom_kind = None
    if args.full and args.warmup > 0:
        wprof, _ = ops.profile_stop()
        if wprof:
            dom_kind = max(wprof, key=lambda k: sum(r[1].elapsed_time(r[2]) for r in wprof[k]))
        del wprof
    if args.full and args.bracket_all:
        ops.profile_start(everything=True)
    elif args.full:
        ops.profile_start(everything=False, only=None if (dom_kind is None or args.mfma_events_only) else {dom_kind})
    dev_allocs0 = int(torch.cuda.memory_stats(dev).get("num_device_alloc", 0))
    t0 = time.perf_counter()
    allocs_per_step = []
    for _ in range(args.steps):
        loss = train_step(onet, opt, X)
        allocs_per_step.append(int(torch.cuda.memory_stats(dev).get("num_device_alloc", 0)))     # host-side counter, no sync
    barrier()
    elapsed = time.perf_counter() - t0
    prof, prof_all = ops.profile_stop()
    if args.dump_outputs and rank == 0:      # before any loop below trains the model further
        dump_outputs(args.dump_outputs, onet, loss)
    # whole-step breakdown (every launch bracketed): its own short loop AFTER the timed region, same model, same batch
    prof_b, n_break, wall_b = prof, args.steps, elapsed / args.steps * 1e3
    if args.full and not args.bracket_all:
        n_break = 3
        ops.profile_start(everything=True)
        barrier()
        tb0 = time.perf_counter()
        for _ in range(n_break):
            loss = train_step(onet, opt, X)
        barrier()
        wall_b = (time.perf_counter() - tb0) / n_break * 1e3
        prof_b, prof_all = ops.profile_stop()
    # the same loop with the fp32-MFMA kernels only (Winograd F(4x4) / direct), for the record next to
    # the headline, whose 3x3 convolutions run on the bf16 matrix pipe by operand splitting (same fp32 tensors and results)
    f32_mfma_only = None
    if args.full and world == 1 and not bf16 and conv in ("auto", "split") and ops.SPLIT_AUTO and not args.torch_adam and not args.no_f32_mfma_only:
        keep = onet.settings
        onet.settings = keep.replace(conv="auto", split=False)
        for _ in range(3):
            loss2 = train_step(onet, opt, X)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        n2 = max(5, args.steps // 2)
        for _ in range(n2):
            loss2 = train_step(onet, opt, X)
        torch.cuda.synchronize()
        e2 = time.perf_counter() - t1
        f32_mfma_only = {"value": round(args.batch * n2 / e2, 3), "unit": "images/s", "ms_per_step": round(e2 / n2 * 1e3, 3), "steps": n2,
                         "warmup": 3, "kernels": "fp32 MFMA only: Winograd F(4x4,3x3) / direct (Settings(split=False))"}
        del loss2
        onet.settings = keep
    per_rank_ms, comm, per_rank, replicas_identical = None, None, None, None
    loss_val = float(loss.item())            # (before the comm loops below: their last mode lets the replicas drift apart)
    hbm_peak_gb = round(torch.cuda.max_memory_allocated(dev) / 2 ** 30, 2)
    if distributed:
        # one record per rank: elapsed seconds, loss, HBM peak, and a checksum of the flat parameter buffer (data-parallel
        # replicas that saw the same reduced gradients hold the same bits: sum and sum of squares in fp64 must agree exactly)
        flat = opt.flat.double() if not args.torch_adam else torch.cat([p.detach().reshape(-1) for p in onet.parameters()]).double()
        mine = torch.tensor([elapsed, loss_val, hbm_peak_gb, float(flat.sum().item()), float((flat * flat).sum().item())],
                            device=dev, dtype=torch.float64)
        del flat
        every = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(every, mine)
        every = [[float(v) for v in t.tolist()] for t in every]
        per_rank_ms = [round(r[0] / args.steps * 1e3, 3) for r in every]
        per_rank = {"loss": [r[1] for r in every], "hbm_peak_gb": [r[2] for r in every]}
        replicas_identical = all(r[3] == every[0][3] and r[4] == every[0][4] for r in every)
        elapsed = max(r[0] for r in every)
        bad = [i for i, r in enumerate(every) if not (r[1] == r[1] and abs(r[1]) != float("inf"))]
        if bad:                              # every rank sees the same record: every rank leaves with the same code
            raise SystemExit("[bench] non-finite loss on rank(s) %s: %s" % (bad, per_rank["loss"]))
        if "ONET_FORCE_LOCAL_RANK" not in os.environ and (dist.get_backend() != "nccl" or dist.get_world_size() != args.gpus):
            raise SystemExit("[bench] --gpus %d but the process group is %s with %d rank(s): not an RCCL run of the requested size"
                             % (args.gpus, dist.get_backend(), dist.get_world_size()))
        if args.full and not args.torch_adam and not args.no_comm_curve:
            comm = comm_curve(onet, opt, X, train_step, barrier, dev, max(3, args.steps // 2), overlap, args.bucket_mb)
            comm["overlap_ms" if overlap else "no_overlap_ms"] = round(elapsed / args.steps * 1e3, 3)
            if "no_allreduce_ms" in comm:
                comm["allreduce_exposed_ms"] = round(comm["overlap_ms" if overlap else "no_overlap_ms"] - comm["no_allreduce_ms"], 3)
    # the reference's own loop shape (TS:209-219), for the record next to the headline: the same steps with the batch copied from
    # pinned host memory every step (TS:211 X.to(device)) and loss.item() every step (TS:219)
    reference_loop = None
    if args.full and world == 1 and not args.no_reference_loop:
        Xh = X.cpu().pin_memory()
        for _ in range(2):
            float(train_step(onet, opt, Xh.to(dev, non_blocking=False)).item())
        torch.cuda.synchronize()
        tr0 = time.perf_counter()
        for _ in range(args.steps):
            float(train_step(onet, opt, Xh.to(dev, non_blocking=False)).item())
        torch.cuda.synchronize()
        er = time.perf_counter() - tr0
        reference_loop = {"value": round(args.batch * args.steps / er, 3), "unit": "images/s", "ms_per_step": round(er / args.steps * 1e3, 3),
                          "steps": args.steps, "warmup": 2,
                          "what": "the headline's step with TS:211's per-step X.to(device) (from pinned host memory, %.1f MB) and TS:219's "
                                  "per-step loss.item() restored; the headline omits both (config.inputs_resident / per_step_host_sync)"
                                  % (Xh.numel() * 4 / 2 ** 20)}
        del Xh

    roofline = None
    if rank == 0 and args.full:
        # multiplies the algorithm issues relative to direct convolution: F(4x4,3x3) 36 per 16 outputs x 9 taps -> 1/4 (the
        # weight-gradient kernel F(3x3,4x4) likewise); the split kernels issue THREE 16-bit MFMAs per product term of the direct
        # algorithm: 1/3
        REDUCTION = {"conv_wino4_kernel": 4.0,
                     "conv_wino4_wgrad_kernel": 4.0, "conv3x3_split_kernel": 1.0 / 3.0, "conv3x3_split_wgrad_kernel": 1.0 / 3.0,
                     "conv3x3_split_pre_kernel": 1.0 / 3.0, "conv3x3_split_wgrad_pre_kernel": 1.0 / 3.0}
        BF16 = ("conv3x3_split_kernel", "conv3x3_split_wgrad_kernel",
                "conv3x3_split_pre_kernel", "conv3x3_split_wgrad_pre_kernel")
        if bf16 and ops.CONVT_BF16:     # the ConvTranspose2d GEMMs take bf16 operands too (priced against the bf16 peak)
            BF16 += ("convt_gemm_kernel", "convt_wgrad_gemm_kernel")
        with ops.using(onet.settings):
            convt_split = ops.convt_operand_bf16(2 * args.batch, args.size // 2, args.size // 2, 64) == 2     # the last Up block's GEMM
            # (round 5: on slot operands -- fp16 hi | mid parts, three MFMAs per term -- wherever the input was written pre-split)
            convt_split = convt_split or (not bf16 and ops.presplit() and bool(ops.CONVT_SLOTS))
        if bf16:                        # conv == "bf16" through the pre-split kernels with ONE part: one MFMA per product term
            REDUCTION.update({"conv3x3_split_pre_kernel": 1.0, "conv3x3_split_wgrad_pre_kernel": 1.0})
        if convt_split:                 # ... or split bf16 operands (three bf16 MFMAs per term, fp32-level results)
            BF16 += ("convt_gemm_kernel", "convt_wgrad_gemm_kernel")
            REDUCTION.update({"convt_gemm_kernel": 1.0 / 3.0, "convt_wgrad_gemm_kernel": 1.0 / 3.0})
        ALGO = {"conv_wino4_kernel": "Winograd F(4x4,3x3) on fp32 MFMA (fwd + dgrad; BatchNorm statistics / backward-reduce "
                                     "epilogues)",
                "conv_wino4_wgrad_kernel": "Winograd F(3x3,4x4) weight gradient on fp32 MFMA, deterministic split-K",
                "conv3x3_split_kernel": "fp32 convolution (fwd + dgrad) on the 16-bit matrix cores by operand splitting: x = hi + mid, "
                                        "w = hi + mid (forward: fp16 parts, input gradient: bf16 parts), 3 x v_mfma_f32_32x32x16_{f16,bf16} "
                                        "per term, fp32 accumulate; error <= the fp32 Winograd F(4x4) kernel's (forward: the direct kernel's)",
                "conv3x3_split_wgrad_kernel": "fp32 weight gradient on the bf16 matrix cores by operand splitting, deterministic split-K",
                "conv3x3_split_pre_kernel": "fp32-level convolution (fwd + dgrad) on the 16-bit matrix cores, operands PRE-SPLIT by their producers "
                                            "(fp16 hi | mid slots [C/8][H][part][W][8]; under --conv bf16: one part of plain bf16): staging is an "
                                            "LDS-DMA copy, 3 x v_mfma_f32_32x32x16_f16 per term (plain bf16: 1), f32 accumulate, BatchNorm "
                                            "statistics from the accumulators; round 5: the forward launches with statistics, the input "
                                            "gradients with the BatchNorm-backward reduce in their epilogue and every plain-bf16 launch run "
                                            "the v_mfma_f32_16x16x32 form (K-packed hi | mid operands)",
                "conv3x3_split_wgrad_pre_kernel": "weight gradient from pre-split x and dz: LDS-DMA staging, fragments by ds_read_b64_tr_b16 "
                                                  "(transposing LDS read), 3 x v_mfma_f32_16x16x32_f16 per term (plain bf16: 1), deterministic split-K",
                "conv_fwd_kernel": "direct implicit GEMM on fp32 MFMA (stem, tiny maps)",
                "conv_wgrad_kernel": "direct split-K weight gradient on fp32 MFMA (stem, tiny maps)",
                "stem_conv_stats_kernel": "stem convolution (Cin = n_channels) + BatchNorm statistics, one streaming VALU pass "
                                          "(bound by writing z: see hbm_frac)",
                "convt_gemm_kernel": "ConvTranspose2d forward / input-gradient GEMMs on SLOT operands (round 5: x pre-split by the block below, "
                                     "the up-sampled half of the concat gradient pre-split by the 3x3 input gradient that produces it, weights in "
                                     "K-slot packs; fp16 hi | mid parts, 3 x v_mfma_f32_32x32x16_f16 per term, every fragment one ds_read_b128 of a "
                                     "DMA-copied slot; one part of plain bf16 under --conv bf16); 128x128 tiles, 4 blocks per CU; fp32 operands "
                                     "(split or rounded in registers) where the slot path does not apply",
                "convt_wgrad_gemm_kernel": "ConvTranspose2d weight-gradient GEMM on slot operands (transposing LDS reads ds_read_b64_tr_b16, "
                                           "256x256 tiles of 8 waves where Cin % 256 == 0, split-K, bias gradient as a row of ones in the same "
                                           "launch); fp32 operands where the slot path does not apply"}
        def kernel_table(records, where):
            tab = {}
            for kind, recs in records.items():
                ms = sum(r[1].elapsed_time(r[2]) for r in recs)
                fl = sum(r[0] for r in recs)
                by = sum(r[3] for r in recs)
                peak = BF16_MFMA_PEAK_TFLOPS if kind in BF16 else FP32_MFMA_PEAK_TFLOPS
                issued = fl / REDUCTION.get(kind, 1.0)
                tab[kind] = {"launches": len(recs), "ms_total": round(ms, 3), "avg_ms": round(ms / len(recs), 4),
                             "direct_equivalent_tflops": round(fl / (ms * 1e-3) / 1e12, 2),
                             "issued_mfma_tflops": round(issued / (ms * 1e-3) / 1e12, 2),
                             "mfma_frac": round(issued / (ms * 1e-3) / 1e12 / peak, 4),
                             "compulsory_gbps": round(by / (ms * 1e-3) / 1e9, 1),
                             "hbm_frac": round(by / (ms * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4), "measured_in": where}
            return tab

        kern_t = kernel_table(prof, "timed region (%d steps)" % args.steps)
        kern_b = kern_t if args.bracket_all else kernel_table(prof_b, "breakdown loop (%d steps after the timed region, every launch bracketed)" % n_break)
        # the dominant kernel: by HIP-event time over the TIMED region (the other MFMA kernels' rows come from the breakdown loop)
        dom = dom_kind if (dom_kind in kern_t) else max(kern_t, key=lambda k: kern_t[k]["ms_total"])
        kern = dict(kern_b)
        kern.update(kern_t)
        d = kern[dom]
        traffic = pmc_traffic(dom, bf16, args.batch)
        SPLIT = ("conv3x3_split_kernel", "conv3x3_split_wgrad_kernel", "conv3x3_split_pre_kernel", "conv3x3_split_wgrad_pre_kernel")
        if dom in SPLIT and not bf16:
            # fp32 tensors, fp32-level results, computed on the bf16 matrix pipe by operand splitting: MFMA-bound, priced against
            # the DENSE bf16 MFMA peak with the FLOPs the kernel issues (three bf16 MFMAs per product term of the direct algorithm)
            roofline = {"kernel": dom, "bound": "mfma", "achieved": d["issued_mfma_tflops"], "peak": BF16_MFMA_PEAK_TFLOPS,
                        "unit": "TFLOP/s", "frac": d["mfma_frac"], "hbm_frac": d["hbm_frac"],
                        "fp32_mfma_peak_equivalent": round(d["direct_equivalent_tflops"] / FP32_MFMA_PEAK_TFLOPS, 3)}
        elif dom in BF16:
            # in bf16 the 64- and 128-channel layers sit below the ridge (312 FLOP/B): the launch is priced
            # against HBM; `achieved` = compulsory bytes (operands once + result once, fp32 storage) / time
            roofline = {"kernel": dom, "bound": "hbm", "achieved": d["compulsory_gbps"], "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                        "frac": d["hbm_frac"], "mfma_frac": d["mfma_frac"]}
        else:
            # fp32: every dense layer is far above the ridge (19.7 FLOP/B): priced against the fp32 MFMA peak with the MFMA
            # FLOPs the kernel ISSUES (Winograd issues 4x / 2.25x fewer than the direct algorithm performs)
            roofline = {"kernel": dom, "bound": "mfma", "achieved": d["issued_mfma_tflops"], "peak": FP32_MFMA_PEAK_TFLOPS,
                        "unit": "TFLOP/s", "frac": d["mfma_frac"], "hbm_frac": d["hbm_frac"]}
        roofline.update({"traffic": traffic, "traffic_unit": "HBM bytes per launch (rocprofv3 --pmc, profiles/)",
                         "compulsory_bytes_per_launch": round(d["compulsory_gbps"] * 1e9 * d["avg_ms"] * 1e-3),
                         "direct_equivalent_tflops": d["direct_equivalent_tflops"],
                         "mfma_flop_reduction": REDUCTION.get(dom, 1.0), "launches_timed": d["launches"],
                         "avg_launch_ms": d["avg_ms"], "algorithm": ALGO.get(dom, dom), "kernels": kern})
        if prof_all:
            stream = {}
            for name, recs in prof_all.items():
                ms = sum(r[1].elapsed_time(r[2]) for r in recs)
                by = sum(r[0] for r in recs if r[0])
                stream[name] = {"launches": len(recs), "ms_total": round(ms, 3), "avg_ms": round(ms / len(recs), 4),
                                "gbps": round(by / (ms * 1e-3) / 1e9, 1) if by else None}
            priced = {k: v for k, v in stream.items() if v["gbps"]}
            sdom = max(priced, key=lambda k: priced[k]["ms_total"])
            roofline["streaming"] = {"kernel": sdom, "bound": "hbm", "achieved": priced[sdom]["gbps"], "peak": HBM_PEAK_GBPS,
                                     "unit": "GB/s", "frac": round(priced[sdom]["gbps"] / HBM_PEAK_GBPS, 4),
                                     "launches_timed": priced[sdom]["launches"], "avg_launch_ms": priced[sdom]["avg_ms"],
                                     "kernels": dict(sorted(stream.items(), key=lambda kv: -kv[1]["ms_total"])[:12])}
            mfma_ms = sum(v["ms_total"] for v in kern_b.values()) / n_break
            hbm_ms = sum(v["ms_total"] for v in priced.values()) / n_break
            small_ms = sum(v["ms_total"] for k, v in stream.items() if k not in priced) / n_break
            wall = wall_b
            roofline["step"] = {"wall_ms": round(wall, 3), "mfma_kernels_ms": round(mfma_ms, 3),
                                "hbm_kernels_ms": round(hbm_ms, 3), "small_kernels_ms": round(small_ms, 3),
                                "unattributed_ms": round(wall - mfma_ms - hbm_ms - small_ms, 3),
                                "mfma_share": round(mfma_ms / wall, 4), "hbm_share": round(hbm_ms / wall, 4),
                                "timed_region_ms_per_step": round(elapsed / args.steps * 1e3, 3),
                                "note": ("per-launch HIP-event brackets on the launch stream, inside the timed region; " if args.bracket_all else
                                         "per-launch HIP-event brackets on the launch stream around EVERY launch, in a loop of %d steps run after "
                                         "the timed region (which brackets the dominant kernel only: bracketing everything costs the "
                                         "difference between wall_ms and timed_region_ms_per_step); " % n_break) +
                                        "unattributed = torch glue kernels, event overhead and launch gaps"}
    if rank == 0:
        imgs = args.batch * world * args.steps
        if args.size == 256 and args.chans == 1:
            cfg_name = "configs[2]" if bf16 else ("configs[3]" if world > 1 and args.batch * world == 256 else "configs[1]")
        elif args.size == 512 and args.chans == 3:
            cfg_name = "configs[4]-shaped (3x512x512 tiles)"
        else:
            cfg_name = "non-BASELINE shape"
        out = {"metric": "training images/sec (twin %dx%d pass)" % (args.size, args.size), "value": round(imgs / elapsed, 3),
               "unit": "images/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
               "ms_per_step": round(elapsed / args.steps * 1e3, 3), "higher_is_better": True, "scaling": "weak",
               "vs_baseline": None,
               "dtype": "bf16" if bf16 else "f32",
               "precision": ("bf16 MFMA operands (3x3 conv fwd/dgrad/wgrad: written as bf16 slots by their producers, round to nearest even; "
                             "ConvTranspose2d GEMMs), f32 accumulation; conv outputs z of those layers STORED as bf16 (rounded once in the "
                             "conv epilogue, as torch.autocast(bfloat16) stores an nn.Conv2d output; BatchNorm statistics from the f32 "
                             "accumulators); BatchNorm arithmetic, activation gradients, loss, master weights and optimizer in f32") if bf16 else
                            ("f32 master tensors (inputs, outputs, conv outputs z, activation gradients, weights, optimizer) and f32-level results; "
                             "the 3x3 convolutions on maps >= 16 px wide (all but the Cin=1 stem) run on the 16-bit matrix pipe by operand splitting (each operand = hi + mid "
                             "fp16 parts of a power-of-two-scaled value: 22-bit operands, 3 MFMAs per term, f32 accumulate; error vs fp64 5e-8..1.5e-7 "
                             "rms of the output scale forward, 3e-7 max on the weight gradient), their operands stored PRE-SPLIT by the producing "
                             "BatchNorm / pooling / ConvTranspose2d kernels (same values as the fp32 passes: forward bit-identical to fp32 storage); "
                             "ConvTranspose2d GEMMs on the same kind of slots in all three directions (22-bit operands; round 4: bf16 parts split in "
                             "registers); every gradient element within 2e-4 of the "
                             "fp64 oracle under the run's own decisions incl. this B=32 dispatch (tests/test_gpu_gradients.py: 9.5e-5; the "
                             "fp32-MFMA-only dispatch: 4.6e-5 on the comparable case); Settings(split=False) keeps the fp32-MFMA Winograd kernels "
                             "(timed in f32_mfma_only under --full)") if (conv in ("auto", "split") and ops.split_enabled()) else "f32 throughout (fp32 MFMA)",
               "data": "synthetic",
               "data_source": data_src,
               "config": {"workload": "%s: batch=%d/GPU %dx%dx%d synthetic K-clutter, %s, twin U-Net "
                                      "fwd+JSD loss+bwd+Adam" % (cfg_name, args.batch, args.chans,
                                                                 args.size, args.size, "bf16 MFMA conv path" if bf16 else "fp32"),
                          "global_batch": args.batch * world, "parallelism": "dp%d" % world,
                          "optimizer": "torch.optim.Adam" if args.torch_adam else "fused flat Adam (HIP)",
                          "grad_allreduce": ("none (1 process)" if not distributed else
                                             "%g MB buckets overlapped with backward" % args.bucket_mb if overlap
                                             else "single all-reduce after backward"),
                          # where the timed step differs from the reference loop TS:209-219, stated in the line itself:
                          "per_step_host_sync": False,      # TS:219's loss.item() every step is NOT in the timed loop (the
                                                            # loss's NaN verdict, OV:234, travels behind an event instead)
                          "inputs_resident": True},         # TS:211's per-step X.to(device) is not in the timed loop

               "loss": loss_val, "hbm_peak_gb": hbm_peak_gb,
               "hbm_reserved_gb": round(torch.cuda.max_memory_reserved(dev) / 2 ** 30, 2),
               "alloc_retries": int(torch.cuda.memory_stats(dev).get("num_alloc_retries", 0)),
               "device_allocs_in_timed_steps": int(torch.cuda.memory_stats(dev).get("num_device_alloc", 0)) - dev_allocs0,
               "device_allocs_per_timed_step": [b - a for a, b in zip([dev_allocs0] + allocs_per_step, allocs_per_step)]}
        if roofline is not None:
            out["roofline"] = roofline
        if distributed:
            out["rccl_world"] = world if dist.get_backend() == "nccl" else 0
            out["dist_backend"] = dist.get_backend()
            try:
                out["nccl_version"] = ".".join(str(v) for v in torch.cuda.nccl.version())
            except Exception:      # noqa: BLE001
                out["nccl_version"] = None
            out["per_rank_ms"] = per_rank_ms
            out["per_rank"] = per_rank
            out["replicas_identical"] = replicas_identical
            if comm is not None:
                out["comm"] = comm
        if f32_mfma_only is not None:
            out["f32_mfma_only"] = f32_mfma_only
        if reference_loop is not None:
            out["reference_loop"] = reference_loop
        headline = world == 1 and not bf16 and args.size == 256 and args.chans == 1 and args.batch == 32 and not args.torch_adam
        if args.full and headline and not args.no_secondary:
            # BASELINE configs[2] in the same driver-run line: release this process's HBM first (the child peaks at ~150 GB)
            X_cpu = X.cpu()
            del loss, opt, onet, X, prof, prof_all, prof_b
            import gc
            gc.collect()
            ops._WS.clear()
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            out["secondary"] = {"configs[2]": secondary_config2()}
        if args.full and world == 1 and not args.no_cpu_baseline:
            if X_cpu is None:
                X_cpu = X.cpu()
            out["cpu_baseline"] = cpu_baseline(X_cpu, args.cpu_seconds)
        print(json.dumps(out), flush=True)
    if distributed:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    _args = parse_args()
    if _args.gpus > 1 and "RANK" not in os.environ:
        sys.exit(_self_launch(_args, sys.argv[1:]))      # before any GPU call: the ranks are children of a GPU-free parent
    try:
        main(_args)
    except BaseException as e:      # noqa: BLE001 -- any failure (RCCL included) ends THIS rank at once with a non-zero code:
        if isinstance(e, SystemExit) and e.code in (0, None):      # no in-process retry, no waiting in a collective's
            raise                                                  # destructor; the launcher then stops the other ranks
        import traceback
        traceback.print_exc()
        sys.stderr.flush()
        os._exit(1)
