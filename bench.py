#!/usr/bin/env python3
"""bench.py -- analysis frames/sec of the MI355X WORLD analysis path.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--full]

A plain run does only what the headline figure needs: it sets up, warms up, times the K steps, writes its outputs if
--dump-outputs is given and prints the result line.  --full adds everything else described below (the run's checks of
itself, the CPU baselines, the other BASELINE configs, the per-kernel and roofline figures, the side legs and the machine
probes), each of which takes runs of its own.

N = 1 (the default, what the driver's BENCH run executes)
    `value` = BASELINE.json configs[1]: one 48 kHz x 10 s utterance per step (2001 frames), Harvest + CheapTrick +
    D4C, 5 ms hop, fft_size 2048, inputs and outputs resident in HBM, `--streams` (12) independent jobs in flight.
    The timed region is K = --steps steps inside ONE barrier + synchronize bracket and `ms_per_step` is its wall time
    over K; --min-wall S > 0 instead repeats the K steps until the region lasts >= S seconds (`repeats`).
    --dump-outputs DIR writes the last timed step's results (tpos, f0, sp, ap, nf) to DIR/<name>.npy as float64
    (a fixed, seeded sample of the spectral rows past 64 MB); the inputs depend on the arguments alone, so two builds
    run with the same arguments can be compared output for output.
    With --full, after the timed region the run checks itself (`parity_in_run`): every in-flight slot's
    (f0, sp, ap) must be bit-identical to a serial single-context run, and that run must agree with the CPU
    reference computed for `cpu_baseline` to the contract's 1e-4 -- otherwise the process exits non-zero.
    Beside `value` the --full line carries `value_single_job` (1 / latency of a lone job) and a `configs` object with one
    timed leg per remaining single-GPU BASELINE config: configs[2] (256 x 5 s, Harvest only), the per-GPU share of
    configs[3] (128 x 5 s, full pipeline) and configs[4] (64 x 16 kHz x 5 s, DIO + StoneMask + CheapTrick + D4C),
    each run for >= --min-wall seconds with its dominant kernel and HBM / FP64 roofline fractions.

N > 1 (the driver's SCALE run; one rank per GPU over RCCL)
    BASELINE.json configs[3]: ONE job of 1024 x (48 kHz, 5 s) utterances per step, split 1024/N per rank by
    world_amd.distributed.analyze_sharded (longest-first partition, batched analysis in sub-batches, one packed
    [frames][2 + 2*1025] block per rank, ONE all-gather).  Total work is fixed: "scaling": "strong".  Compute and
    exchange are timed separately on every rank (`phases`).  With --full the run also checks utterances received from
    other ranks against a lone analysis (`parity_in_run`) and times the all-gather alone, the roofline and the CPU baseline.

Rank 0 prints ONE JSON line.  (--full:) `roofline` describes the kernel that dominates a configs[1] step (HIP-event timing on
the launch stream, taken in a separate profiled pass); `cpu_baseline*` are the unmodified reference timed on this
box's host cores (1 core at -O1 = the reference's own flags, 1 core at -O3, and every core).
"""
import argparse
import hashlib
import json
import os
import sys
import time

# The number of hardware queues the HIP runtime spreads a process's streams over is left to the machine's environment:
# the GPUs are shared, and a process that opens more queues than the card's slots can destabilise it for everyone on it.
# RCCL between processes (N > 1): this pool's host driver only supports dmabuf IPC; the boxes export the setting, a
# launcher that scrubs the environment would otherwise fail in hipIpcGetMemHandle at the first collective
# -- so the default is applied ONLY where the box exports nothing, and the line says which it was (`environment.hsa_ipc`)
HSA_IPC_EXPORTED = os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY")
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FS = 48000
FRAME_PERIOD = 5.0
FFT_SIZE = 2048
# compulsory HBM bytes per output frame (one hop of x read once, tpos + f0 + the rows written once)
BYTES_PER_FRAME = 240 * 8 + 8 + 8 + 2 * 1025 * 8          # 48 kHz, full pipeline (configs 1, 3)
BYTES_PER_FRAME_HARVEST = 240 * 8 + 16                     # 48 kHz, Harvest only (configs 2)
BYTES_PER_FRAME_16K = 80 * 8 + 16 + 2 * 513 * 8            # 16 kHz, fft 1024 (configs 4)
HBM_PEAK_GBS = 8000.0           # MI355X_MICROARCH.md: 8 TB/s spec (6.3 TB/s measured copy)
FP64_VECTOR_PEAK_TFLOPS = 78.6  # MI355X FP64 vector: 256 CUs x 4 SIMDs x 16 lanes x 2 flop x 2.4 GHz
RTOL = 1e-4                     # north_star: F0 / envelope / aperiodicity within 1e-4 relative


# ---------------------------------------------------------------------------------------------------------
# committed PMC evidence (profiles/pmc_traffic.json, written by tools/profile_summary.py on the GPU box)
def csrc_hash():
    """Hash of the kernel sources the library is built from: the PMC profile is stamped with it, and a line
    whose sources differ from the profiled ones says so (`traffic_stale`) instead of silently replaying."""
    h = hashlib.sha256()
    d = os.path.join(ROOT, "world_amd", "csrc")
    for name in sorted(os.listdir(d)):
        if name.endswith((".hip", ".h", ".inc", ".cpp")):
            h.update(name.encode())
            with open(os.path.join(d, name), "rb") as f:
                h.update(f.read())
    return h.hexdigest()[:16]


def unit_hashes():
    """{unit: hash of that .hip unit + every header it includes, transitively}, {kernel name: unit}: the PMC counters are
    stamped per KERNEL with the hash of the unit the kernel is compiled from, so a change to one unit (or to a header only
    other units include: dropin.inc is api.hip's alone) makes only its own kernels' counters stale -- and
    tools/round_evidence.sh re-collects only those (a one-line kernel change cost a full re-profile)."""
    import re
    d = os.path.join(ROOT, "world_amd", "csrc")
    inc_re = re.compile(r'^\s*#\s*include\s*"([^"]+)"', re.M)
    texts = {}

    def text(name):
        if name not in texts:
            try:
                with open(os.path.join(d, os.path.basename(name)), "rb") as f:
                    texts[name] = f.read()
            except OSError:
                texts[name] = b""                              # (a header outside csrc: include/world_hip.h -- the ABI, not kernel code)
        return texts[name]

    def closure(name, seen):
        for inc in inc_re.findall(text(name).decode("utf-8", "replace")):
            inc = os.path.basename(inc)
            if inc not in seen and os.path.exists(os.path.join(d, inc)):
                seen.add(inc)
                closure(inc, seen)
        return seen

    units, kernels = {}, {}
    for name in sorted(os.listdir(d)):
        if not name.endswith(".hip"):
            continue
        h = hashlib.sha256(text(name))
        for inc in sorted(closure(name, set())):
            h.update(inc.encode())
            h.update(text(inc))
        units[name] = h.hexdigest()[:16]
        for m in re.finditer(r"__global__\s+void\s+(?:__launch_bounds__\([^)]*(?:\([^)]*\)[^)]*)*\)\s*)?(\w+)\s*\(", text(name).decode("utf-8", "replace")):
            kernels[m.group(1)] = name
    return units, kernels


def _kernel_stale(counters, kernel):
    """True when `kernel`'s counters were taken on other sources than today's (per-unit stamp; whole-tree stamp for old files)"""
    units, kernels = unit_hashes()
    base = kernel.split("<")[0]
    stamp = counters.get("unit_hash")
    if stamp is None or base not in kernels:
        return None
    return stamp != units[kernels[base]]


def _pmc(config="1"):
    """{kernel: counters} of one profiled config, its frames per launch, and whether the stamp is stale."""
    path = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    try:
        with open(path) as f:
            t = json.load(f)
    except (OSError, ValueError):
        return None
    stale = t.get("csrc_hash") != csrc_hash()
    if "configs" in t:
        c = t["configs"].get(str(config))
        if not c:
            return None
        return c["kernels"], c.get("frames_per_launch"), stale
    if str(config) != "1":
        return None
    return t.get("kernels", {}), t.get("frames_per_launch"), stale


def measured_traffic(kernel, frames_per_launch, config="1"):
    """HBM bytes per launch of `kernel` from the committed rocprofv3 PMC passes.  FETCH_SIZE is doubled per
    MI355X_MICROARCH.md (gfx950 reports half of a wide coalesced read); WRITE_SIZE is used as reported
    (uncalibrated).  None when no profile of this workload exists."""
    p = _pmc(config)
    if not p or p[1] != frames_per_launch:
        return None
    # rocprofv3 prints template arguments ("d4c_groupdelay<4096>"), the library's labels do not
    names = [n for n in p[0] if n == kernel or n.startswith(kernel + "<")]
    if not names:
        return None
    k = p[0][names[0]]
    if "FETCH_SIZE" not in k and "WRITE_SIZE" not in k:
        return None
    return int((2.0 * k.get("FETCH_SIZE", 0.0) + k.get("WRITE_SIZE", 0.0)) * 1024.0)


def traffic_stale(config="1", kernel=None):
    """whether the committed counters (of `kernel`, or of the whole config) were measured on other kernel sources"""
    p = _pmc(config)
    if not p:
        return None
    if kernel is not None:
        names = [n for n in p[0] if n == kernel or n.startswith(kernel + "<")]
        if names:
            st = _kernel_stale(p[0][names[0]], names[0])
            if st is not None:
                return bool(st)
    return bool(p[2])


def measured_fp64(kernels, frames_per_launch, config="1"):
    """FP64 work per launch from the committed rocprofv3 PMC pass (SQ_INSTS_VALU_{ADD,MUL,FMA,TRANS}_F64:
    wave-level instructions, 64 lanes each, an FMA counted as two operations) set against the live
    per-launch durations: {kernel: (flop per launch, achieved TFLOP/s)} and the pipeline's flop per frame.
    None when the profile lacks the counters or was taken on another workload."""
    p = _pmc(config)
    if not p or p[1] != frames_per_launch:
        return None
    out, total = {}, 0.0
    for name, c in p[0].items():
        if "SQ_INSTS_VALU_FMA_F64" not in c:
            continue
        flop = 64.0 * (c.get("SQ_INSTS_VALU_ADD_F64", 0.0) + c.get("SQ_INSTS_VALU_MUL_F64", 0.0) +
                       2.0 * c["SQ_INSTS_VALU_FMA_F64"] + c.get("SQ_INSTS_VALU_TRANS_F64", 0.0))
        base = name.split("<")[0]
        if base in kernels and flop > 0:
            k = kernels[base]
            out[base] = (flop, flop / (k["avg_ms"] * 1e-3) / 1e12)
            total += flop * k["launches_per_step"]
    return (out, total / frames_per_launch) if out else None


# ---------------------------------------------------------------------------------------------------------
# CPU baselines: the unmodified reference (oracle/_ref, built in place by oracle/Makefile) on this box's cores
def cpu_baseline(x_np, optimized=False, keep_outputs=False):
    """One analysis of the same utterance on ONE host core; returns (record, outputs or None)."""
    from oracle.loader import PortOracle, RefOracle, ref_available
    o = RefOracle(optimized=optimized) if ref_available() else PortOracle()
    t0 = time.perf_counter()
    tp, f0 = o.harvest(x_np, FS, frame_period=FRAME_PERIOD)
    sp = o.cheaptrick(x_np, FS, tp, f0, fft_size=FFT_SIZE)
    ap = o.d4c(x_np, FS, tp, f0, FFT_SIZE)
    dt = time.perf_counter() - t0
    rec = {"value": len(f0) / dt, "unit": "frames/s", "cores": 1,
           "kind": "reference" if o.kind == "reference" else "port",
           "sample": f"1 x ({len(x_np) / FS:.1f} s of 48 kHz audio, Harvest+CheapTrick+D4C, {len(f0)} frames), "
                     f"{getattr(o, 'flags', 'gcc -O2 restatement')}, {dt:.1f} s of CPU time",
           "host_cores_available": os.cpu_count()}
    return rec, ((tp, f0, sp, ap) if keep_outputs else None)


def usable_cores():
    """host cores this process may actually use: the affinity mask, cut by a cgroup CPU quota if there is one
    (a GPU box hands a container 256 logical CPUs and sometimes a quota of a few cores' worth of time)"""
    cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    quota = None
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:                       # cgroup v2: "<quota|max> <period>"
            q, period = f.read().split()
            if q != "max":
                quota = float(q) / float(period)
    except (OSError, ValueError):
        try:                                                            # cgroup v1
            with open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us") as f, open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as g:
                q, period = float(f.read()), float(g.read())
                if q > 0:
                    quota = q / period
        except (OSError, ValueError):
            pass
    return cores, quota


def cpu_baseline_all_cores(x_np, optimized=False, seconds=2.5):
    """The reference is re-entrant (no globals), so the whole-box CPU number is one analysis per core:
    P worker PROCESSES (the reference allocates per candidate, threads would fight over one heap), each analysing
    the first `seconds` of the utterance once, all started at the same instant.  P doubles from 8 up to every usable
    core for as long as the aggregate rate still grows (a box may expose 256 logical CPUs and far less CPU time);
    the best round is reported.  Bounded: a few seconds of work per process and round."""
    from oracle.loader import parallel_analyses, ref_available
    cores, quota = usable_cores()
    limit = max(1, min(cores, int(os.environ.get("WORLD_BENCH_CPU_PROCS", cores))))
    x_cut = x_np[:int(seconds * FS)]
    best, rounds, procs = None, [], min(8, limit)
    while True:
        frames, dt, flags = parallel_analyses(x_cut, FS, FRAME_PERIOD, FFT_SIZE, procs, optimized=optimized)
        rate = frames / dt
        rounds.append({"processes": procs, "frames_per_s": round(rate, 1), "wall_s": round(dt, 2)})
        if best is None or rate > best[0]:
            best = (rate, procs, dt)
        stalled = len(rounds) > 1 and rate < 1.15 * rounds[-2]["frames_per_s"]
        if procs >= limit or stalled:
            break
        procs = min(limit, procs * 2)
    return {"value": best[0], "unit": "frames/s", "cores": best[1],
            "kind": "reference" if ref_available() else "port", "flags": flags,
            "sample": f"{best[1]} concurrent analyses of the first {len(x_cut) / FS:.1f} s of the utterance, one per process, "
                      f"{best[2]:.1f} s wall (excluding worker start-up); process counts tried: "
                      + ", ".join(f"{r['processes']}: {r['frames_per_s']:.0f}" for r in rounds),
            "host_cores_available": os.cpu_count(), "affinity_cores": cores, "cgroup_cpu_quota": quota}


def smi_snapshot():
    """What rocm-smi says about device 0 right now: clocks, power and cap, performance level, compute / memory partition
    mode.  Two of round 4's seven boxes ran a lone job's latency-bound kernels 10-90 % slower and the line had nothing to
    tell them apart by.  Best effort: a missing tool or field gives None, never an exception."""
    import shutil
    import subprocess
    exe = shutil.which("rocm-smi") or "/opt/rocm/bin/rocm-smi"
    out = {}
    try:
        r = subprocess.run([exe, "-d", "0", "--showclocks", "--showpower", "--showmaxpower", "--showperflevel",
                            "--showcomputepartition", "--showmemorypartition", "--showtemp", "--json"],
                           capture_output=True, text=True, timeout=20)
        d = json.loads(r.stdout[r.stdout.index("{"):]) if "{" in r.stdout else {}
        card = d.get("card0") or (next(iter(d.values())) if d else {})
        for k, v in (card or {}).items():
            kl = k.lower()
            if "sclk" in kl or "mclk" in kl or "fclk" in kl or "socclk" in kl:
                out.setdefault("clocks", {})[k.strip()] = v         # rocm-smi gives a level index AND a "(2100Mhz)" speed per domain
            elif "max graphics package power" in kl or "max power" in kl:
                out["power_cap_w"] = v
            elif "power" in kl and "w" in kl and "power_w" not in out:
                out["power_w"] = v
            elif "performance level" in kl:
                out["perf_level"] = v
            elif "compute partition" in kl:
                out["compute_partition"] = v
            elif "memory partition" in kl:
                out["memory_partition"] = v
            elif "temperature" in kl and "junction" in kl:
                out["temp_junction_c"] = v
        if not out:
            out["raw"] = (r.stdout or r.stderr)[-400:]
    except Exception as e:                                   # noqa: BLE001 -- diagnostics must not break the run
        out["error"] = f"{type(e).__name__}: {e}"[:200]
    return out


def rel_err(a, b):
    import numpy as np
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))) if a.size else 0.0


DUMP_BYTES = 64 << 20           # --dump-outputs: at most this many bytes in all


def dump_outputs(out_dir, arrays, seed=0):
    """--dump-outputs: every array as out_dir/<name>.npy in float64.  The 3-d ones ([utterance][frame][bin]: sp, ap) are cut
    to a seeded sample of their (utterance, frame) rows when the whole set would pass DUMP_BYTES; the sample depends on the
    shapes alone (two builds run with the same arguments dump the same rows) and its flat row indices go to sample_rows.npy."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    host = {k: np.ascontiguousarray(v.cpu().numpy() if hasattr(v, "cpu") else v, dtype=np.float64) for k, v in arrays.items()}
    if sum(a.nbytes for a in host.values()) > DUMP_BYTES:
        wide = [k for k, a in host.items() if a.ndim == 3]
        rows = host[wide[0]].shape[0] * host[wide[0]].shape[1]
        assert all(host[k].shape[0] * host[k].shape[1] == rows for k in wide)
        room = DUMP_BYTES - 4096 - sum(a.nbytes for k, a in host.items() if k not in wide)     # (4 kB: the .npy headers)
        keep = min(rows, room // (8 + 8 * sum(host[k].shape[2] for k in wide)))
        pick = np.sort(np.random.default_rng(seed).choice(rows, size=keep, replace=False))
        for k in wide:
            host[k] = host[k].reshape(rows, -1)[pick]
        host["sample_rows"] = pick.astype(np.float64)
    for k, a in host.items():
        np.save(os.path.join(out_dir, k + ".npy"), a)
    return sorted(host)


def visible_gpus():
    """devices this process would see, without creating a HIP context in it (the count is taken in a child: a parent that
    is about to become a launcher must not hold the runtime)"""
    import subprocess
    r = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.device_count())"], capture_output=True, text=True)
    try:
        return int(r.stdout.strip().splitlines()[-1])
    except (ValueError, IndexError):
        return 0


def spawn_ranks(args):
    """`python bench.py --gpus N` as the driver types it -- no launcher, WORLD_SIZE unset -- must give N ranks, not an N = 1
    line that claims nothing was asked (the guard used to fire only when a launcher disagreed).  With
    fewer than N devices visible the run FAILS with one line; there is no silent fallback.  (Ranks may share a device only
    under WORLD_HIP_BENCH_BACKEND=gloo, the functional check of the N > 1 path on a 1-GPU box -- never a number of record.)"""
    have = None
    if "WORLD_SIZE" in os.environ:
        world = int(os.environ["WORLD_SIZE"])
        if world != args.gpus:
            raise SystemExit(f"bench.py: --gpus {args.gpus} but the launcher set WORLD_SIZE={world}")
    if args.gpus == 1 or "WORLD_SIZE" in os.environ:
        # this process is (or becomes) a rank: it is about to initialise the runtime anyway, count here
        if int(os.environ.get("LOCAL_RANK", "0")) == 0:
            import torch
            have = torch.cuda.device_count()
    else:
        have = visible_gpus()                                   # about to start the launcher: count in a child
    shared_ok = os.environ.get("WORLD_HIP_BENCH_BACKEND") == "gloo"
    if have is not None and have < (1 if shared_ok else args.gpus):
        raise SystemExit(f"bench.py: --gpus {args.gpus} asked for, {have} GPU(s) visible: not running (no CPU path, no fewer-GPU fallback)")
    if args.gpus == 1 or "WORLD_SIZE" in os.environ:
        return
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__), *sys.argv[1:]]
    sys.stderr.write("bench.py: --gpus %d without a launcher: " % args.gpus + " ".join(cmd[1:8]) + " ...\n")
    sys.stderr.flush()
    # the launcher runs as a child process (this one never initialised the runtime, but is not replaced either) and its
    # exit status becomes ours
    import subprocess
    r = subprocess.run(cmd, env=dict(os.environ, WORLD_HIP_BENCH_SELF_SPAWNED="1"))
    sys.exit(r.returncode if r.returncode >= 0 else 128 - r.returncode)


# ---------------------------------------------------------------------------------------------------------
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=1, help="N = 1: utterances per step of the headline leg")
    ap.add_argument("--seconds", type=float, default=10.0, help="N = 1: utterance length of the headline leg")
    ap.add_argument("--min-wall", type=float, default=0.0,
                    help="> 0: every timed region repeats its K steps until it has lasted this many seconds "
                         "(default 0: exactly K timed steps)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="N = 1: write the last timed step's results of the headline leg to DIR/<name>.npy (float64)")
    ap.add_argument("--full", action="store_true",
                    help="also run everything beyond the headline figure: the run's checks of itself, CPU baselines, the other "
                         "configs, per-kernel / roofline figures, side legs and machine probes (default: the headline alone)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baselines")
    ap.add_argument("--no-configs", action="store_true", help="N = 1, with --full: skip the legs of the other BASELINE configs")
    ap.add_argument("--only-config", type=int, default=0,
                    help="N = 1: run ONLY the leg of this BASELINE config (2, 3 or 4) -- the profiling entry point")
    ap.add_argument("--contexts", type=int, default=2,
                    help="N = 1: batched jobs in flight in the configs[2] / [3] / [4] legs (1 = per-kernel durations free of queueing: profiles)")
    ap.add_argument("--no-gather", action="store_true", help="N > 1: skip the result all-gather")
    ap.add_argument("--no-extras", action="store_true",
                    help="with --full: skip the graph / codec / synthesis / host-pointer legs and the environment microprobe")
    ap.add_argument("--job-utterances", type=int, default=1024, help="N > 1: utterances of the configs[3] job")
    ap.add_argument("--sub-batch", type=int, default=32,
                    help="configs[3] job (N > 1, and the N = 1 anchor configs['3_full']): utterances per batched call = per all-gather")
    ap.add_argument("--wire", choices=["auto", "f64", "f32"], default="auto",
                    help="configs[3] job: record format of the exchange.  f64 = bit-identical to a lone analysis; f32 = the spectra "
                         "rounded once to float by the stage kernels (half the bytes on the links, 6e-8 against the 1e-4 contract).  "
                         "auto (default): N > 1 measures RCCL's all-gather rate on this node before the timed region and takes f64 if "
                         "that rate hides the f64 exchange under the analysis, else f32 -- the line says which and what the other "
                         "would have cost; N = 1 (no exchange): f64")
    ap.add_argument("--streams", type=int, default=12,
                    help="independent analysis jobs in flight per GPU (each step is one job on its own HIP "
                         "stream with its own workspace; 1 = strictly one after the other)")
    args = ap.parse_args()
    if args.gpus < 1 or args.steps < 1:
        raise SystemExit("bench.py: --gpus and --steps must be >= 1")
    if args.dump_outputs and (args.gpus > 1 or args.only_config):
        raise SystemExit("bench.py: --dump-outputs writes the headline leg of --gpus 1 (not with --gpus N > 1 or --only-config)")
    spawn_ranks(args)                                           # --gpus N > 1 without a launcher: become N ranks (never returns then)

    import numpy as np
    import torch
    import torch.distributed as dist
    from world_amd import distributed as wd
    from world_amd import synth
    from world_amd.api import WorldHip, frame_count

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}")
    # one rank per GPU; (for a functional check of the N > 1 path on a 1-GPU box, ranks may share a
    # device with WORLD_HIP_BENCH_BACKEND=gloo -- never used for numbers of record)
    local = local % max(1, torch.cuda.device_count())
    torch.cuda.set_device(local)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        dist.init_process_group(os.environ.get("WORLD_HIP_BENCH_BACKEND", "nccl"), rank=rank, world_size=world)
    dev = torch.device("cuda", local)
    if world == 1 and args.wire == "auto":
        args.wire = "f64"                                       # no exchange to hide: the bit-identical records
    props = torch.cuda.get_device_properties(local)
    environment = {"device": props.name, "arch": getattr(props, "gcnArchName", None), "compute_units": props.multi_processor_count,
                   "hbm_bytes": props.total_memory,
                   "gpu_max_hw_queues": os.environ.get("GPU_MAX_HW_QUEUES"),
                   "hsa_ipc": {"HSA_ENABLE_IPC_MODE_LEGACY": os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY"),
                               "exported_by_the_box": HSA_IPC_EXPORTED is not None},
                   "launcher": "bench.py itself (torch.distributed.run)" if os.environ.get("WORLD_HIP_BENCH_SELF_SPAWNED") else
                               ("external" if "WORLD_SIZE" in os.environ else "none")}
    if args.full:
        environment["rocm_smi_at_start"] = smi_snapshot() if rank == 0 else None

    def environment_done(wh_probe=None):
        """the line's `environment` object: rocm-smi before and after the run, and the library's microprobe of the machine
        under load (world_hip_probe_machine: effective shader clock under an FP64 load, HBM and L2 pointer-chase latency,
        an LDS round trip on an idle and on a loaded CU) -- what tells a slow box from a regression"""
        environment["rocm_smi_at_end"] = smi_snapshot() if rank == 0 else None
        if wh_probe is not None and hasattr(wh_probe, "probe_machine") and not args.no_extras:
            try:
                environment["microprobe"] = wh_probe.probe_machine()
            except Exception as e:                           # noqa: BLE001
                environment["microprobe"] = {"error": str(e)[:200]}
        return environment

    def barrier():
        if world > 1:
            dist.barrier()

    def timed_region(step, finish, steps, est_ms_per_step):
        """`repeats` blocks of `steps` steps inside one barrier + synchronize bracket; max over ranks"""
        repeats = max(1, int(1.25 * args.min_wall * 1e3 / max(est_ms_per_step * steps, 1e-3) + 0.999)) if args.min_wall > 0 else 1
        for attempt in range(3):
            if world > 1:
                r = torch.tensor([repeats], device=dev)
                dist.all_reduce(r, op=dist.ReduceOp.MAX)
                repeats = int(r.item())
            torch.cuda.synchronize()
            barrier()
            t0 = time.perf_counter()
            for _ in range(repeats * steps):
                step()
            finish()
            torch.cuda.synchronize()
            barrier()
            dt = time.perf_counter() - t0
            if world > 1:
                t = torch.tensor([dt], dtype=torch.float64, device=dev)
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
                dt = float(t.item())
            if dt >= args.min_wall or args.min_wall <= 0:
                break
            # the estimate was too optimistic (a region of 1.93 s was committed once): the whole region again, longer --
            # only the last one is reported
            repeats = int(repeats * 1.3 * args.min_wall / max(dt, 1e-6)) + 1
        return dt, repeats

    def estimate(step, finish, n=3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            step()
        finish()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    def kernel_profile(wh, run, reps=2):
        prof = wh.profile(lambda: [run() for _ in range(reps)])
        torch.cuda.synchronize()
        return {k: {"launches_per_step": len(v) // reps, "ms_per_step": sum(v) / reps, "avg_ms": sum(v) / len(v)}
                for k, v in prof.items()}

    def roofline_of(kernels, frames, bytes_per_frame, config):
        dom = max(kernels, key=lambda k: kernels[k]["ms_per_step"])
        alg = bytes_per_frame * frames
        ach = alg / (kernels[dom]["avg_ms"] * 1e-3) / 1e9
        r = {"bound": "hbm", "kernel": dom, "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s",
             "frac": ach / HBM_PEAK_GBS, "traffic": measured_traffic(dom, frames, config),
             "traffic_stale": traffic_stale(config, dom),
             "algorithmic_bytes_per_launch": alg, "avg_launch_ms": kernels[dom]["avg_ms"]}
        fp = measured_fp64(kernels, frames, config)
        if fp and dom in fp[0]:
            flop, tflops = fp[0][dom]
            r["fp64"] = {"flop_per_launch": flop, "achieved": tflops, "peak": FP64_VECTOR_PEAK_TFLOPS, "unit": "TFLOP/s",
                         "frac": tflops / FP64_VECTOR_PEAK_TFLOPS, "peak_spec": FP64_VECTOR_PEAK_TFLOPS,
                         "peak_measured": None, "frac_of_measured": None,      # (filled from the run's own microprobe: measured_peak)
                         "pipeline_flop_per_frame": fp[1],
                         "source": "profiles/pmc_traffic.json (SQ_INSTS_VALU_*_F64) over live durations"}
        return r

    def measured_peak(env, *roofs):
        """both denominators in the line: the spec figure (78.6 TFLOP/s at 2.4 GHz) and the FP64 FMA rate the
        box itself sustains chip-wide at the clock it holds under that load (the library's microprobe, same run)"""
        rate = ((env or {}).get("microprobe") or {}).get("fp64_fma_tflops")
        for r in roofs:
            fp = (r or {}).get("fp64")
            if fp and rate:
                fp["peak_measured"] = rate
                fp["frac_of_measured"] = fp["achieved"] / rate
                fp["peak_measured_what"] = "world_hip_probe_machine: chip-wide FP64 FMA chains, whole launch timed by HIP events, this run"

    # =====================================================================================================
    # N > 1: BASELINE configs[3], one job of --job-utterances utterances per step, sharded over the ranks
    # =====================================================================================================
    if world > 1:
        n_job, sec = args.job_utterances, 5.0
        n_samp = int(round(FS * sec))
        lengths = [n_samp] * n_job
        parts = wd.partition(lengths, world)
        mine = parts[rank]
        xs = {i: synth.utterance(i, FS, sec, device=dev) for i in mine}        # only this rank's share exists here
        wh = WorldHip(device=local)
        phases = {"compute_ms": 0.0, "exchange_ms": 0.0, "exchange_exposed_ms": 0.0, "steps": 0}

        last = [None]
        nb_job = FFT_SIZE // 2 + 1
        frames_job = sum(frame_count(FS, n, FRAME_PERIOD) for n in lengths)

        def run_step(wire, gather):
            last[0] = wd.analyze_sharded(xs, FS, lengths=lengths, packer=wh, sub_batch=args.sub_batch,
                                         gather=gather, timings=phases, wire=wire)

        def measure_gather(blocks):
            """blocking in-place all-gathers of the job's largest sub-batch buffer, nothing else running, HIP events: the rate
            RCCL achieves on this node (bytes a rank RECEIVES per second, the slowest rank's)"""
            buf = max(blocks, key=lambda b: b.numel())
            recv = (world - 1) * buf[0].numel() * 8
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for _ in range(2):
                wd._gather_in_place(buf, rank, None, False)
            torch.cuda.synchronize(); barrier()
            e0.record()
            for _ in range(5):
                wd._gather_in_place(buf, rank, None, False)
            e1.record(); torch.cuda.synchronize()
            tg = torch.tensor([e0.elapsed_time(e1) / 5], dtype=torch.float64, device=dev)
            dist.all_reduce(tg, op=dist.ReduceOp.MAX)
            return {"allgather_gbs_per_rank": recv / (float(tg.item()) * 1e-3) / 1e9, "bytes_received_per_rank": recv,
                    "ms": float(tg.item()), "what": "blocking in-place all_gather_into_tensor of the largest sub-batch buffer, nothing else running"}

        # ---- the wire format: measured, not assumed (under the pessimistic reading of the link rate the f64
        # exchange is exposed at 8 GPUs, and f64 used to be the default the first scaling run would have timed) ----------
        wire, wire_choice = args.wire, None
        if args.no_gather:
            wire = "f64" if wire == "auto" else wire
        elif wire == "auto":
            run_step("f64", True)                              # buffers, tables, workspace (and RCCL's channels)
            torch.cuda.synchronize(); barrier()
            rate = measure_gather(last[0].blocks)
            for _ in range(2):
                run_step("f64", False)
            torch.cuda.synchronize(); barrier()
            t0 = time.perf_counter()
            for _ in range(3):
                run_step("f64", False)
            torch.cuda.synchronize(); barrier()
            tc = torch.tensor([(time.perf_counter() - t0) / 3], dtype=torch.float64, device=dev)
            dist.all_reduce(tc, op=dist.ReduceOp.MAX)
            compute_s = float(tc.item())
            recv = {w: frames_job * (world - 1) / world * wd.WIRE_COLS[w](nb_job) * 8 for w in ("f64", "f32")}
            last_rows = wd.chunk_sizes(len(mine), args.sub_batch)[-1] * frame_count(FS, n_samp, FRAME_PERIOD)
            gbs = rate["allgather_gbs_per_rank"]
            need = {w: recv[w] / compute_s / 1e9 for w in recv}
            # a step = the analysis (or the exchange, whichever is slower) + the one exchange nothing overlaps: the last chunk's
            proj = {w: (max(compute_s, recv[w] / (gbs * 1e9)) + (world - 1) * last_rows * wd.WIRE_COLS[w](nb_job) * 8 / (gbs * 1e9)) * 1e3
                    for w in recv}
            margin = 1.25                                      # collectives under load achieve less than standalone
            wire = "f64" if gbs >= margin * need["f64"] else "f32"
            other = "f32" if wire == "f64" else "f64"
            wire_choice = {"chosen": wire, "measured_allgather_gbs_per_rank": gbs, "compute_only_ms_per_step": compute_s * 1e3,
                           "gbs_needed_to_hide": need, "margin": margin, "projected_ms_per_step": proj,
                           "other": other, "other_would_cost_ms_per_step": proj[other] - proj[wire],
                           "rule": "f64 (bit-identical to a lone analysis) if the standalone all-gather rate is >= margin x the rate that "
                                   "hides the f64 exchange under the analysis, else f32 (spectra rounded once to float: 6e-8 against 1e-4)"}
            phases.update(compute_ms=0.0, exchange_ms=0.0, exchange_exposed_ms=0.0, steps=0)
        args.wire = wire

        def step():
            run_step(wire, not args.no_gather)

        for _ in range(max(1, args.warmup)):
            step()
        phases.update(compute_ms=0.0, exchange_ms=0.0, exchange_exposed_ms=0.0, steps=0)
        est = estimate(step, lambda: None, 1)
        phases.update(compute_ms=0.0, exchange_ms=0.0, exchange_exposed_ms=0.0, steps=0, gathered_bytes=0, last_chunk_bytes=0)
        dt, repeats = timed_region(step, lambda: None, args.steps, est)
        frames_per_step = sum(frame_count(FS, n, FRAME_PERIOD) for n in lengths)
        nsteps = args.steps * repeats
        ph = torch.tensor([phases["compute_ms"], phases["exchange_ms"]], dtype=torch.float64, device=dev) / max(1, phases["steps"])
        ph_max = ph.clone()
        dist.all_reduce(ph_max, op=dist.ReduceOp.MAX)
        # the run checks itself: utterances analysed on OTHER ranks, as this rank received them, against a lone
        # analysis made here (bit-identical: batched == single, and the exchange must not touch a bit)
        parity = None
        if args.full and not args.no_gather:
            res, checked, same = last[0], [], True
            for i in sorted({(rank * 7 + 1) % n_job, n_job // 2, (n_job - 1 - rank) % n_job}):
                tp1, f01, sp1, ap1, nf1 = wh.analyze(synth.utterance(i, FS, sec, device=dev).unsqueeze(0), FS)
                tp, f0, sp, ap = res.utterance(i)
                k = int(nf1[0])
                sp_want, ap_want = (sp1[0, :k], ap1[0, :k]) if args.wire == "f64" else \
                    (sp1[0, :k].to(torch.float32), ap1[0, :k].to(torch.float32))      # f32 wire: the f64 result rounded once
                same = same and tp.shape[0] == k and torch.equal(tp, tp1[0, :k]) and torch.equal(f0, f01[0, :k]) and \
                    torch.equal(sp, sp_want) and torch.equal(ap, ap_want)
                checked.append(i)
            ok = torch.tensor([1 if same else 0], device=dev)
            dist.all_reduce(ok, op=dist.ReduceOp.MIN)
            parity = {"utterances_checked_on_rank0": checked, "every_rank_bit_identical_to_lone_analysis": bool(ok.item()),
                      "randn_table_intact": bool(wh.verify_tables())}
        # The all-gather by itself: blocking in-place all-gathers of the job's largest sub-batch buffer, HIP events around
        # them -- the rate RCCL achieves on this node when nothing else runs, beside the rate the overlap NEEDS
        # (bytes a rank receives per step / the step's time) and the bytes of the one exchange the overlap cannot hide.
        gather_gbs = measure_gather(last[0].blocks) if args.full and not args.no_gather else None
        # roofline of the dominant kernel of ONE batched call of this rank's share (rank 0; HIP events per kernel)
        roofline = None
        if args.full and rank == 0 and mine:
            idx = mine[:args.sub_batch]
            xb = torch.stack([xs[i] for i in idx]).contiguous()
            kernels = kernel_profile(wh, lambda: wh.analyze(xb, FS, frame_period=FRAME_PERIOD), 1)
            roofline = roofline_of(kernels, frame_count(FS, n_samp, FRAME_PERIOD) * len(idx), BYTES_PER_FRAME,
                                   "3" if len(idx) == 128 else "-")
            roofline["scope"] = f"one batched analysis of {len(idx)} utterances on rank 0"
            del xb
        # what the communicator itself reports, and which device every rank ran on (a line that says n_gpus = 8 must show 8)
        ranks_seen = dist.get_world_size()
        names = [None] * world
        dist.all_gather_object(names, {"rank": rank, "device_index": local, "device": props.name,
                                       "uuid": str(getattr(props, "uuid", "")) or None})
        # the CPU baseline beside it (rank 0, one utterance of the job on one host core; the other ranks wait at the barrier)
        cpu = None
        if args.full and rank == 0 and not args.no_cpu_baseline and mine:
            cpu, _ = cpu_baseline(xs[mine[0]].cpu().numpy(), optimized=False)
        barrier()
        dist.destroy_process_group()
        if rank == 0:
            nb = FFT_SIZE // 2 + 1
            line = {
                "metric": "analysis frames/sec (Harvest+CheapTrick+D4C, 48 kHz, 5 ms hop)",
                "value": frames_per_step * nsteps / dt, "unit": "frames/s", "n_gpus": world, "steps": args.steps,
                "repeats": repeats, "warmup": args.warmup, "ms_per_step": dt / nsteps * 1e3, "timed_wall_s": dt,
                "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
                "config": {"workload": f"configs[3]: one job of {n_job} x (48 kHz, {sec:g} s) utterances per step, "
                                       f"Harvest+CheapTrick+D4C, fft_size=2048, frame_period=5 ms, {n_job // world} utterances "
                                       f"per GPU in sub-batches of {args.sub_batch}, inputs/outputs in HBM",
                           "frames_per_step": frames_per_step, "utterances_per_gpu": len(mine),
                           "parallelism": f"utterance-sharded x{world}" + (
                               ", no collective" if args.no_gather else
                               f", one in-place RCCL all-gather of packed [frames][{wd.WIRE_COLS[args.wire](nb)}] records ({args.wire} spectra) per sub-batch "
                               f"(sizes {wd.chunk_sizes(len(mine), args.sub_batch)}: the last, exposed one is tapered), overlapped with the next sub-batch's analysis "
                               f"({frames_per_step * wd.WIRE_COLS[args.wire](nb) * 8 / 1e9:.1f} GB reassembled on every rank)")},
                "phases": {"compute_ms_per_step_max_over_ranks": float(ph_max[0]),
                           "exchange_exposed_ms_per_step_max_over_ranks": float(ph_max[1]),
                           "allgather_gbs_per_rank": None if gather_gbs is None else gather_gbs["allgather_gbs_per_rank"],
                           "allgather_standalone": gather_gbs,
                           "allgather_gbs_per_rank_needed_to_hide": None if args.no_gather else
                               phases.get("gathered_bytes", 0) / max(1, phases["steps"]) / (dt / nsteps) / 1e9,
                           "exposed_last_chunk_bytes_per_step": None if args.no_gather else
                               phases.get("last_chunk_bytes", 0) // max(1, phases["steps"]),
                           "wire": args.wire, "wire_choice": wire_choice,
                           "note": "chunk k's all-gather runs while chunk k+1 is analysed; exposed = device time the compute stream "
                                   "waited for all-gathers after its last analysis (HIP events), compute = the rest of the step"},
                "rccl_ranks_seen": ranks_seen, "backend": os.environ.get("WORLD_HIP_BENCH_BACKEND", "nccl"), "ranks": names,
                "environment": environment}
            if args.full:
                measured_peak(environment_done(wh), roofline)
                line.update({"parity_in_run": parity, "roofline": roofline, "cpu_baseline": cpu})
            print(json.dumps(line))
            if parity is not None and not (parity["every_rank_bit_identical_to_lone_analysis"] and parity["randn_table_intact"]):
                sys.stderr.write("bench.py: parity_in_run failed: " + json.dumps(parity) + "\n")
                sys.exit(1)
        return

    # =====================================================================================================
    # N = 1
    # =====================================================================================================
    def run_leg(name, config, workload, make_x, fs, analyze, frames_of, bytes_per_frame, n_ctx=None):
        """one timed leg: `n_ctx` contexts alternate (two batched jobs in flight), >= --min-wall seconds"""
        n_ctx = n_ctx or max(1, args.contexts)
        x = make_x()
        streams = [torch.cuda.Stream(device=dev) for _ in range(n_ctx)]
        whs = [WorldHip(device=local) for _ in range(n_ctx)]
        counter = [0]
        out = [None] * n_ctx

        def step():
            k = counter[0] % n_ctx
            counter[0] += 1
            with torch.cuda.stream(streams[k]):
                out[k] = analyze(whs[k], x)

        for _ in range(n_ctx + 1):
            step()
        est = estimate(step, lambda: None, 2)
        dt, repeats = timed_region(step, lambda: None, args.steps, est)
        frames = frames_of(out[0])
        nsteps = args.steps * repeats

        def lone():
            with torch.cuda.stream(streams[0]):
                analyze(whs[0], x)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        lone()
        torch.cuda.synchronize()
        lat = (time.perf_counter() - t1) * 1e3
        kernels = kernel_profile(whs[0], lone)
        leg = {"workload": workload, "value": frames * nsteps / dt, "unit": "frames/s", "frames_per_step": frames,
               "steps": args.steps, "repeats": repeats, "ms_per_step": dt / nsteps * 1e3, "timed_wall_s": dt,
               "jobs_in_flight": n_ctx, "single_step_latency_ms": lat,
               "roofline": roofline_of(kernels, frames, bytes_per_frame, config),
               "kernels_ms_per_step": {k: round(v["ms_per_step"], 4) for k, v in sorted(
                   kernels.items(), key=lambda kv: -kv[1]["ms_per_step"])[:12]},
               "workspace_bytes": sum(w.workspace_bytes() for w in whs)}
        for w in whs:
            w.close()
        del x, out
        torch.cuda.empty_cache()
        return leg

    def leg_config2():
        B = 256
        return run_leg("configs[2]", "2", f"configs[2]: batch of {B} x (48 kHz, 5 s) vowels / chirps, Harvest F0 only, one batched call per step",
                       lambda: torch.stack([synth.utterance(i, FS, 5.0, device=dev) for i in range(B)]).contiguous(), FS,
                       lambda wh, x: wh.harvest(x, FS, frame_period=FRAME_PERIOD), lambda o: int(o[2].sum()),
                       BYTES_PER_FRAME_HARVEST)

    def leg_config3():
        B = 128
        return run_leg("configs[3]-share", "3", f"configs[3] per-GPU share at 8 GPUs: batch of {B} x (48 kHz, 5 s), Harvest+CheapTrick+D4C, "
                       "one batched call per stage per step",
                       lambda: torch.stack([synth.utterance(i, FS, 5.0, device=dev) for i in range(B)]).contiguous(), FS,
                       lambda wh, x: wh.analyze(x, FS, frame_period=FRAME_PERIOD), lambda o: int(o[4].sum()),
                       BYTES_PER_FRAME)

    def leg_config4():
        B, fs = 64, 16000
        return run_leg("configs[4]", "4", f"configs[4]: batch of {B} x (16 kHz, 5 s) vowels, Dio + StoneMask + CheapTrick(fft 1024, q1 -0.15) "
                       "+ D4C(threshold 0.85), one batched call per stage per step",
                       lambda: torch.stack([synth.vowel(fs, 5.0, seed=100 + i, base_f0=90.0 + (i % 32) * 8.0, device=dev)
                                            for i in range(B)]).contiguous(), fs,
                       lambda wh, x: wh.analyze(x, fs, f0_method="dio", frame_period=FRAME_PERIOD), lambda o: int(o[4].sum()),
                       BYTES_PER_FRAME_16K)

    def leg_config0():
        """BASELINE configs[0]: test/vaiueo2d.wav (the samples committed in tests/golden/vaiueo2d_dio.npz) through test.cpp's
        DIO plumbing -- Dio(f0_floor 40) -> StoneMask -> CheapTrick(q1 -0.15) -> D4C(0.85) -- on HOST pointers: the drop-in
        symbols of libworld_hip.so beside the unmodified reference on one host core (reference test/test.cpp:89-219)"""
        from world_amd.api import HostAPI
        g = np.load(os.path.join(ROOT, "tests", "golden", "vaiueo2d_dio.npz"))
        xw, fsw, fftw = g["q"].astype(np.float64) / 32768.0, int(g["fs"]), int(g["fft_size"])

        def job(api):
            tp, f0 = api.dio(xw, fsw, f0_floor=float(g["f0_floor_est"]), frame_period=float(g["frame_period"]))
            f0 = api.stonemask(xw, fsw, tp, f0)
            sp = api.cheaptrick(xw, fsw, tp, f0, q1=float(g["q1"]), f0_floor=71.0, fft_size=fftw)
            ap = api.d4c(xw, fsw, tp, f0, fftw, threshold=float(g["threshold"]))
            return tp, f0, sp, ap
        H = HostAPI()
        job(H)
        reps = 20
        t1 = time.perf_counter()
        for _ in range(reps):
            tp, f0, sp, ap = job(H)
        ms = (time.perf_counter() - t1) / reps * 1e3
        leg = {"workload": "configs[0]: test/vaiueo2d.wav (22.05 kHz, 17 500 samples, 159 frames), Dio + StoneMask + CheapTrick + D4C "
                           "as test/test.cpp calls them, host pointers in and out (PCIe and one synchronisation per stage included)",
               "frames_per_step": int(len(f0)), "ms_per_utterance": ms, "value": len(f0) / (ms * 1e-3), "unit": "frames/s",
               "golden": {"f0": rel_err(f0[g["f0"] > 0], g["f0"][g["f0"] > 0]), "vuv_flips": int(np.sum((f0 > 0) != (g["f0"] > 0))),
                          "sp": rel_err(sp[g["rows"]], g["sp_rows"]), "ap": rel_err(ap[g["rows"]], g["ap_rows"]), "tolerance": RTOL}}
        if not args.no_cpu_baseline:
            from oracle.loader import PortOracle, RefOracle, ref_available
            o = RefOracle() if ref_available() else PortOracle()
            job(o)
            t1 = time.perf_counter()
            for _ in range(3):
                job(o)
            ms_ref = (time.perf_counter() - t1) / 3 * 1e3
            leg["cpu_reference"] = {"kind": o.kind, "cores": 1, "ms_per_utterance": ms_ref, "frames_per_s": len(f0) / (ms_ref * 1e-3)}
        return leg

    def leg_config3_full():
        """BASELINE configs[3] as ONE job on ONE GPU: 1024 x (48 kHz, 5 s) utterances through world_amd.distributed.analyze_sharded
        -- the code path of `--gpus N`, with a world of one: the N = 1 anchor of the strong-scaling curve."""
        n_job, sec = args.job_utterances, 5.0
        lengths = [int(round(FS * sec))] * n_job
        xs_job = {i: synth.utterance(i, FS, sec, device=dev) for i in range(n_job)}
        whj = WorldHip(device=local)
        phases = {}

        def step():
            return wd.analyze_sharded(xs_job, FS, lengths=lengths, packer=whj, sub_batch=args.sub_batch, timings=phases, wire=args.wire)
        res = step()
        phases.clear()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        steps = 0
        while steps < 2 or time.perf_counter() - t1 < args.min_wall:
            res = step()
            steps += 1
        torch.cuda.synchronize()
        dtj = time.perf_counter() - t1
        frames = sum(res.n_frames)
        # the job checks itself: every utterance (so both lanes and every chunk size, the tapered tail included) against a lone
        # analysis -- bit-identical: batched == single
        by_chunk = {}
        for i, w in res.where.items():
            by_chunk.setdefault(w[0], []).append(i)
        # EVERY utterance of the job (round 5 checked four per sub-batch, 136 of 1024: VERDICT r05 weak 1b; a lone analysis of
        # a 5 s utterance and four device-side comparisons cost ~2 ms, the whole check ~2 s)
        picks = sorted(res.where)
        same = True
        for i in picks:
            tp1, f01, sp1, ap1, nf1 = whj.analyze(xs_job[i].unsqueeze(0), FS)
            tp, f0, sp, ap = res.utterance(i)
            k = int(nf1[0])
            sp_want, ap_want = (sp1[0, :k], ap1[0, :k]) if args.wire == "f64" else \
                (sp1[0, :k].to(torch.float32), ap1[0, :k].to(torch.float32))
            same = same and tp.shape[0] == k and torch.equal(tp, tp1[0, :k]) and torch.equal(f0, f01[0, :k]) and \
                torch.equal(sp, sp_want) and torch.equal(ap, ap_want)
        leg = {"workload": f"configs[3] full job on one GPU: {n_job} x (48 kHz, {sec:g} s), Harvest+CheapTrick+D4C, sub-batches of "
                           f"{args.sub_batch} (tapered tail: {wd.chunk_sizes(n_job, args.sub_batch)[-3:]}) written straight into packed "
                           f"[frames][{wd.WIRE_COLS[args.wire](FFT_SIZE // 2 + 1)}] records ({args.wire} spectra; no pack pass, no collective)",
               "value": frames * steps / dtj, "unit": "frames/s", "frames_per_step": frames, "steps": steps,
               "ms_per_step": dtj / steps * 1e3, "timed_wall_s": dtj,
               "phases": {"compute_ms_per_step": phases.get("compute_ms", 0.0) / max(1, phases.get("steps", 1)),
                          "exchange_exposed_ms_per_step": phases.get("exchange_exposed_ms", 0.0) / max(1, phases.get("steps", 1))},
               "utterances_bit_identical_to_lone_analysis": bool(same), "utterances_checked": len(picks),
               "sub_batches": len(by_chunk),
               "result_bytes": frames * wd.WIRE_COLS[args.wire](FFT_SIZE // 2 + 1) * 8, "workspace_bytes": whj.workspace_bytes()}
        whj.close()
        wd._buffers.clear()
        wd._lanes.clear()
        del xs_job, res
        torch.cuda.empty_cache()
        return leg

    if args.only_config:
        leg = {2: leg_config2, 3: leg_config3, 4: leg_config4}[args.only_config]()
        print(json.dumps(leg))
        return

    # ---- the headline leg: configs[1] ---------------------------------------------------------------------
    B = args.batch
    S = max(1, args.streams)

    def slot_input(k):
        """slot k's own job: slot 0 analyses SURVEY.md 8d's configs[1] vowel (seed 12345, 140 Hz: the utterance the CPU
        reference is timed and checked on), every other slot the same kind of vowel with its own seed and pitch -- twelve
        different WAVs in flight, not one tensor read twelve times (shared L2 / Infinity-Cache lines, identical windows)"""
        xs_k = [synth.vowel(FS, args.seconds, seed=12345 + 977 * k + i, base_f0=140.0 + 7.0 * ((5 * k + i) % 12), device=dev)
                for i in range(B)]
        return xs_k
    xs = slot_input(0)
    x_slots = [torch.stack(slot_input(k)).contiguous() for k in range(S)]
    x = x_slots[0]
    n = x.shape[1]
    nf = frame_count(FS, n, FRAME_PERIOD)
    # Steps are independent analysis jobs.  `--streams S` keeps S of them in flight: job k
    # runs on HIP stream k % S with its own library context (workspace) and output buffers,
    # so one job's short serial kernels (contour logic, decimation) overlap another job's
    # wide ones.  Every job still does the full work; nothing is cached between steps.
    streams = [torch.cuda.Stream(device=dev) for _ in range(S)]
    # (the contexts of the in-flight mode say so -- world_hip.h: WORLD_HIP_HINT_SHARED_DEVICE: narrow launch shapes for the
    # one-workgroup contour kernels; the serial parity run and the lone-job latency below use contexts WITHOUT the hint, so
    # `slots_bit_identical_to_serial_run` also says that the two launch shapes give the same bits)
    whs = [WorldHip(device=local, shared_device=S > 1) for _ in range(S)]
    wh = whs[0]
    sp_bufs = [torch.empty((B, nf, FFT_SIZE // 2 + 1), dtype=torch.float64, device=dev) for _ in range(S)]
    ap_bufs = [torch.empty_like(sp_bufs[0]) for _ in range(S)]
    last = [None] * S
    counter = [0]

    def step():
        k = counter[0] % S
        counter[0] += 1
        with torch.cuda.stream(streams[k]):
            last[k] = whs[k].analyze(x_slots[k], FS, frame_period=FRAME_PERIOD, sp_out=sp_bufs[k], ap_out=ap_bufs[k])

    # one-time initialisation of every slot (workspace allocation, constant tables): not a step
    for _ in range(S):
        step()
    torch.cuda.synchronize()
    for _ in range(args.warmup):
        step()
    est = estimate(step, lambda: None, max(3, S))
    dt, repeats = timed_region(step, lambda: None, args.steps, est)
    nsteps = args.steps * repeats
    frames_per_step = nf * B
    value = frames_per_step * nsteps / dt
    if args.dump_outputs:
        # what the last timed step's caller received: its slot's (tpos, f0, sp, ap, nf); nothing has run on that slot since
        tpos_l, f0_l, sp_l, ap_l, nf_l = last[(counter[0] - 1) % S]
        dump_outputs(args.dump_outputs, {"tpos": tpos_l, "f0": f0_l, "sp": sp_l, "ap": ap_l, "nf": nf_l})

    line = {
        "metric": "analysis frames/sec (Harvest+CheapTrick+D4C, 48 kHz, 5 ms hop)",
        "value": value, "unit": "frames/s", "n_gpus": 1, "steps": args.steps, "repeats": repeats, "warmup": args.warmup,
        "ms_per_step": dt / nsteps * 1e3, "timed_wall_s": dt, "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "f64", "data": "synthetic",
        "config": {"workload": f"configs[1]: {B} x (48 kHz, {args.seconds:g} s) utterance(s) per step, "
                               f"Harvest+CheapTrick+D4C, fft_size=2048, frame_period=5 ms, inputs/outputs in HBM, "
                               f"{S} independent jobs in flight (one HIP stream + context each, a different utterance per job)",
                   "frames_per_step": frames_per_step, "utterances_per_gpu": B, "jobs_in_flight": S,
                   "parallelism": "single GPU, no collective"},
        "environment": environment,
    }
    if not args.full:
        print(json.dumps(line))
        return

    # ---- the run checks itself: every slot of the timed mode against a serial single-context run ---------
    torch.cuda.synchronize()
    sp_ser, ap_ser = torch.empty_like(sp_bufs[0]), torch.empty_like(sp_bufs[0])
    ser = WorldHip(device=local)
    slots_equal = True
    for k in range(S - 1, -1, -1):                       # every slot's own utterance, serially, on one fresh context; slot 0 last
        tpos_ser, f0_ser, _, _, _ = ser.analyze(x_slots[k], FS, frame_period=FRAME_PERIOD, sp_out=sp_ser, ap_out=ap_ser)
        torch.cuda.synchronize()
        slots_equal = slots_equal and last[k] is not None and torch.equal(last[k][0], tpos_ser) and \
            torch.equal(last[k][1], f0_ser) and torch.equal(sp_bufs[k], sp_ser) and torch.equal(ap_bufs[k], ap_ser)
    tables_ok = ser.verify_tables()
    ser.close()
    parity = {"slots": S, "distinct_utterances": S, "slots_bit_identical_to_serial_run": bool(slots_equal),
              "randn_table_intact": bool(tables_ok), "frames": nf * B}

    # latency of ONE job with nothing else in flight (not the headline number): a context of its own, no shared-device hint
    lone = WorldHip(device=local)

    def lone_job():
        with torch.cuda.stream(streams[0]):
            lone.analyze(x, FS, frame_period=FRAME_PERIOD, sp_out=sp_bufs[0], ap_out=ap_bufs[0])
        torch.cuda.synchronize()
    for _ in range(3):                                   # the parity leg above ran other contexts: settle first
        lone_job()
    t1 = time.perf_counter()
    for _ in range(20):
        lone_job()
    lat = (time.perf_counter() - t1) / 20 * 1e3

    # ---- the same job captured into a HIP graph (world_hip_graph_*): one host launch per job --------------------
    graph_leg = None
    if not args.no_extras:
        blk = torch.zeros((nf * B, 2 + 2 * (FFT_SIZE // 2 + 1)), dtype=torch.float64, device=dev)
        with torch.cuda.stream(streams[0]):
            for _ in range(2):
                whs[0].analyze_packed(x, FS, blk, frame_period=FRAME_PERIOD)
            torch.cuda.synchronize()
            want = blk.clone()
            g = whs[0].capture(lambda: whs[0].analyze_packed(x, FS, blk, frame_period=FRAME_PERIOD))
            blk.fill_(-1.0)
            g.launch()
            torch.cuda.synchronize()
            same = bool(torch.equal(blk, want))
            for _ in range(3):
                g.launch()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(20):
                g.launch()
                torch.cuda.synchronize()
            lat_g = (time.perf_counter() - t1) / 20 * 1e3
            t1 = time.perf_counter()
            for _ in range(50):
                g.launch()
            host_g = (time.perf_counter() - t1) / 50 * 1e3
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(50):
                whs[0].analyze_packed(x, FS, blk, frame_period=FRAME_PERIOD)
            host_e = (time.perf_counter() - t1) / 50 * 1e3
            torch.cuda.synchronize()
        g.close()
        graph_leg = {"workload": "the configs[1] job (analyze_packed: records written by the stage kernels) captured into one HIP graph",
                     "replay_bit_identical_to_eager": same, "single_job_latency_ms": lat_g,
                     "host_ms_per_job": {"graph_launch": host_g, "eager_calls": host_e},
                     "note": "host ms = time to enqueue 50 jobs back to back on one stream / 50 (queue back-pressure included)"}
        del blk, want

    # ---- roofline leg: per-kernel HIP-event timing of a few extra steps ------------------------------------
    def lone():
        with torch.cuda.stream(streams[0]):
            whs[0].analyze(x, FS, frame_period=FRAME_PERIOD, sp_out=sp_bufs[0], ap_out=ap_bufs[0])
    kernels = kernel_profile(wh, lone, 3)
    roofline = roofline_of(kernels, nf * B, BYTES_PER_FRAME, "1")
    roofline["note"] = ("FP64 / latency-bound pipeline (SURVEY.md 8d): see fp64.pipeline_flop_per_frame (measured) against 18.3 kB of "
                        "compulsory traffic per frame. frac is not comparable with round 1's 0.0203: that was quoted on "
                        "d4c_groupdelay (0.212 ms), one of the two kernels (d4c_band: 0.186 ms) that d4c_frame replaces -- on "
                        "their sum the same formula gave 0.0115 (DESIGN.md section 4)")
    if "fp64" in roofline:
        roofline["fp64"]["pipeline_achieved"] = roofline["fp64"]["pipeline_flop_per_frame"] * value / 1e12

    # ---- coders behind the path: reported beside the metric, never part of `value` ----
    codec = synthesis = host_to_host = None
    if not args.no_extras:
        sp, apb = sp_bufs[0], ap_bufs[0]
        with torch.cuda.stream(streams[0]):
            for _ in range(2):
                mcep = wh.code_spectral_envelope(sp, FS, FFT_SIZE, 60)
                bap = wh.code_aperiodicity(apb, FS, FFT_SIZE)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            reps = 20
            e0.record()
            for _ in range(reps):
                mcep = wh.code_spectral_envelope(sp, FS, FFT_SIZE, 60)
                bap = wh.code_aperiodicity(apb, FS, FFT_SIZE)
            e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / reps
        cbytes = nf * B * 8 * (2 * (FFT_SIZE // 2 + 1) + mcep.shape[-1] + bap.shape[-1])
        codec = {"workload": f"CodeSpectralEnvelope(60 dims) + CodeAperiodicity on the step's {nf * B} frames",
                 "ms": ms, "frames_per_s": nf * B / (ms * 1e-3),
                 "roofline": {"bound": "hbm", "achieved": cbytes / (ms * 1e-3) / 1e9, "peak": HBM_PEAK_GBS,
                              "unit": "GB/s", "frac": cbytes / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                              "algorithmic_bytes": cbytes}}
        # synthesis from the step's device-resident parameters
        with torch.cuda.stream(streams[0]):
            tpos1, f01, sp1, ap1, nf1 = whs[0].analyze(x, FS, frame_period=FRAME_PERIOD, sp_out=sp_bufs[0], ap_out=ap_bufs[0])
            y = wh.synthesis(f01, sp1, ap1, nf1, FFT_SIZE, FRAME_PERIOD, FS, n)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(3):
                y = wh.synthesis(f01, sp1, ap1, nf1, FFT_SIZE, FRAME_PERIOD, FS, n, check_pulses=False)   # checked above: timed without the sync
            e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / 3
        synthesis = {"workload": f"Synthesis() of {B} x {args.seconds:g} s from the analysis outputs in HBM",
                     "ms": ms, "x_realtime": B * args.seconds / (ms * 1e-3),
                     "note": "bound by the bit-faithful serial phase accumulation (one chain of dependent FP64 adds per "
                             "utterance, ~7 cycles a sample, one wavefront per utterance)"}
        # the same job through the reference's host-pointer API (the drop-in boundary):
        # PCIe-inclusive, reported beside the metric and never part of `value`
        from world_amd.api import HostAPI
        H = HostAPI()
        x_host = xs[0].cpu().numpy()[:n]

        def host_job():
            tp, f0 = H.harvest(x_host, FS, frame_period=FRAME_PERIOD)
            H.cheaptrick(x_host, FS, tp, f0, fft_size=FFT_SIZE)
            H.d4c(x_host, FS, tp, f0, FFT_SIZE)
            return len(f0)
        host_job()
        t1 = time.perf_counter()
        frames_h = sum(host_job() for _ in range(5))
        dt_h = time.perf_counter() - t1
        host_to_host = {"workload": "Harvest() + CheapTrick() + D4C() on host pointers (libworld_hip.so drop-in symbols), "
                                    "one utterance at a time, PCIe and per-stage synchronisation included",
                        "python_binding_ms_per_utterance": dt_h / 5 * 1e3,
                        "python_binding_note": "world_amd.api.HostAPI (ctypes + numpy): fresh numpy outputs every call, as round 3's "
                                               "line measured it -- the binding's own cost and the page faults of untouched "
                                               "output arrays are inside this figure"}
        # the figure of record: a plain C++ caller (examples/dropin_bench.cpp), rows allocated one by one as the reference's
        # own test/test.cpp:148-151 allocates them
        import subprocess
        import tempfile
        from world_amd import build as hip_build
        try:
            exe = os.path.join(ROOT, "examples", "dropin_bench")
            if not os.path.exists(exe):
                hip_build.build_examples()
            with tempfile.NamedTemporaryFile(suffix=".f64", delete=False) as tf:
                tf.write(x_host.astype(np.float64).tobytes())
            r = subprocess.run([exe, tf.name, str(FS), "10", "4"], capture_output=True, text=True, timeout=600)
            os.unlink(tf.name)
            cc = json.loads(r.stdout.strip().splitlines()[-1]) if r.returncode == 0 else {"error": (r.stdout + r.stderr)[-500:]}
        except Exception as e:                                          # noqa: BLE001
            cc = {"error": repr(e)}
        host_to_host["c_caller"] = cc
        # ... and with WORLD_HIP_DROPIN_WIRE=f32: the two matrices cross PCIe as float (rounded once on the device, 6e-8
        # relative against the contract's 1e-4) and are widened on the host -- opt-in, never `value`
        try:
            with tempfile.NamedTemporaryFile(suffix=".f64", delete=False) as tf:
                tf.write(x_host.astype(np.float64).tobytes())
            r = subprocess.run([exe, tf.name, str(FS), "10", "4"], capture_output=True, text=True, timeout=600,
                               env=dict(os.environ, WORLD_HIP_DROPIN_WIRE="f32"))
            os.unlink(tf.name)
            host_to_host["c_caller_f32_rows"] = json.loads(r.stdout.strip().splitlines()[-1]) if r.returncode == 0 else \
                {"error": (r.stdout + r.stderr)[-500:]}
        except Exception as e:                                          # noqa: BLE001
            host_to_host["c_caller_f32_rows"] = {"error": repr(e)}
        if "separate_rows_ms" in cc:
            host_to_host["ms_per_utterance"] = cc["separate_rows_ms"]
            host_to_host["frames_per_s"] = cc["frames"] / (cc["separate_rows_ms"] * 1e-3)
            host_to_host["measured_by"] = "examples/dropin_bench.cpp: separately allocated rows reused across 10 repetitions"
        else:
            host_to_host["ms_per_utterance"] = dt_h / 5 * 1e3
            host_to_host["frames_per_s"] = frames_h / dt_h
            host_to_host["measured_by"] = "python binding (the C caller did not run)"
        # the same with four host threads (the drop-in layer is re-entrant since round 4: a slot per caller)
        import threading
        xs_h = [xs_k.cpu().numpy()[0, :n].copy() for xs_k in x_slots[:4]]

        def host_thread(xh):
            for _ in range(3):
                tp, f0 = H.harvest(xh, FS, frame_period=FRAME_PERIOD)
                H.cheaptrick(xh, FS, tp, f0, fft_size=FFT_SIZE)
                H.d4c(xh, FS, tp, f0, FFT_SIZE)
        for warm in range(2):
            th = [threading.Thread(target=host_thread, args=(xh,)) for xh in xs_h]
            t1 = time.perf_counter()
            for t in th:
                t.start()
            for t in th:
                t.join()
            dt_t = time.perf_counter() - t1
        host_to_host["four_threads_ms_per_utterance"] = dt_t / (3 * len(xs_h)) * 1e3
        host_to_host["four_threads_frames_per_s"] = 3 * len(xs_h) * nf / dt_t
        # cold start, in a fresh process (tools/first_call.py)
        try:
            r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "first_call.py"), str(args.seconds)],
                               capture_output=True, text=True, timeout=600)
            cold = json.loads(r.stdout.strip().splitlines()[-1]) if r.returncode == 0 else {"error": r.stderr[-500:]}
        except Exception as e:                                          # noqa: BLE001
            cold = {"error": repr(e)}
        host_to_host["cold_start"] = cold

    workspace = sum(w.workspace_bytes() for w in whs)
    table_bytes = wh.noise_table_bytes()

    # ---- the other single-GPU BASELINE configs, each for >= --min-wall seconds -----------------------------
    configs = None
    if not args.no_configs:
        f0_k, sp_k, ap_k = f0_ser[0].cpu().numpy(), sp_ser[0].cpu().numpy(), ap_ser[0].cpu().numpy()
        tp_k = tpos_ser[0].cpu().numpy()
        for w in whs:
            w.close()
        del sp_bufs, ap_bufs, last
        torch.cuda.empty_cache()
        configs = {"0": leg_config0(), "2": leg_config2(), "3_share": leg_config3(), "3_full": leg_config3_full(),
                   "4": leg_config4()}
    else:
        f0_k, sp_k, ap_k = f0_ser[0].cpu().numpy(), sp_ser[0].cpu().numpy(), ap_ser[0].cpu().numpy()
        tp_k = tpos_ser[0].cpu().numpy()

    # ---- CPU reference on this box: the baseline AND the checker of the run's own outputs ------------------
    cpu = cpu_o3 = cpu_all = cpu_all_o3 = None
    if not args.no_cpu_baseline:
        x_host = xs[0].cpu().numpy()
        cpu, ref = cpu_baseline(x_host, optimized=False, keep_outputs=True)
        tp_r, f0_r, sp_r, ap_r = ref
        voiced = f0_r > 0
        parity.update({
            "checked_against": cpu["kind"] + " (" + cpu["sample"].split(", ")[-2] + ")",
            "tpos_bit_exact": bool(np.array_equal(tp_k[:len(tp_r)], tp_r)),
            "vuv_flips": int(np.sum((f0_k[:len(f0_r)] > 0) != voiced)),
            "f0": rel_err(f0_k[:len(f0_r)][voiced], f0_r[voiced]),
            "sp": rel_err(sp_k[:len(f0_r)], sp_r), "ap": rel_err(ap_k[:len(f0_r)], ap_r), "tolerance": RTOL})
        cpu_o3, _ = cpu_baseline(x_host, optimized=True)
        cpu_all = cpu_baseline_all_cores(x_host, optimized=False)
        cpu_all_o3 = cpu_baseline_all_cores(x_host, optimized=True)
    ok = parity["slots_bit_identical_to_serial_run"] and parity["randn_table_intact"]
    if "f0" in parity:
        ok = ok and parity["tpos_bit_exact"] and parity["vuv_flips"] == 0 and max(parity["f0"], parity["sp"], parity["ap"]) <= RTOL
    parity["ok"] = bool(ok)

    env_1 = environment_done(WorldHip(device=local))
    measured_peak(env_1, roofline, *[(leg or {}).get("roofline") for leg in (configs or {}).values()])
    line.update({
        "value_single_job": frames_per_step / (lat * 1e-3), "single_job_latency_ms": lat,
        "parity_in_run": parity,
        "roofline": roofline, "cpu_baseline": cpu, "cpu_baseline_o3": cpu_o3,
        "cpu_baseline_all_cores": cpu_all, "cpu_baseline_all_cores_o3": cpu_all_o3,
        "kernels_ms_per_step": {k: round(v["ms_per_step"], 4) for k, v in sorted(
            kernels.items(), key=lambda kv: -kv[1]["ms_per_step"])},
        "configs": configs, "graph": graph_leg, "codec": codec, "synthesis": synthesis, "host_to_host": host_to_host,
        "first_call_ms": None if not host_to_host else host_to_host.get("cold_start", {}).get("first_call_ms"),
        "randn_table_first_build_ms": None if not host_to_host else host_to_host.get("cold_start", {}).get("randn_table_build_ms"),
        "workspace_bytes": workspace, "randn_table_bytes": table_bytes, "csrc_hash": csrc_hash(),
    })
    print(json.dumps(line))
    if not ok:
        sys.stderr.write("bench.py: parity_in_run failed: " + json.dumps(parity) + "\n")
        sys.exit(1)


if __name__ == "__main__":
    main()
