#!/usr/bin/env python3
"""Headline benchmark: persons/s of the ViTPose hot path on N MI355X (BASELINE.json).

    python bench.py [--gpus N --steps K --warmup W] [--dtype fp16|bf16] [--batch 256] [--full] [--dump-outputs DIR]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W
(`python bench.py --gpus N` with N > 1 and no WORLD_SIZE in the environment launches those N ranks itself.)

A plain run sets up, warms up (W steps), times EXACTLY K steps, writes the keypoints of the last timed step when --dump-outputs is
given and prints the headline line: `metric` / `value` (persons/s over the timed steps) / `unit` / `higher_is_better` / `dtype` /
`ms_per_step` (wall time of one timed step).  Nothing else runs unless asked for: no event records, no checks, no extra passes.

--full adds everything described below, as every run did before the option existed (each leg can still be dropped with its --no-*
option); --breakdown and --strong stay separate opt-ins.

--dump-outputs DIR writes DIR/keypoints.npy: the float32 [B, K, 3] (y, x, conf) keypoints the timed path left in HBM after its last
step (N > 1: the all-gathered [N*B, K, 3] of rank 0).  Weights and crops are seeded, so the same arguments give the same inputs on
every run and two builds can be compared output for output.

One "step" = one pass of the whole hot path (crop batch resident in HBM -> patch embed
-> ViT encoder -> deconv head -> heatmaps -> arg-max/DARK-UDP decode -> keypoints in
HBM, + the RCCL all-gather of keypoints when N > 1) over one batch of 256 synthetic
256x192 crops per GPU (weak scaling: crops are independent, each rank owns its batch).
Workload = BASELINE.json configs[1]: ViTPose-B COCO-17, batch 256, seeded random
weights of that architecture, synthetic uniform-noise crops.

With --full, prints ONE JSON line on rank 0 with `roofline` (the GEMM family with the largest share of the step, timed live
with HIP events on the library's stream inside the timed region; `kernel` = what the library says it launched, `traffic` read
from the committed PMC passes as `traffic_source` states), `clock_under_load` (N=1: shader clock and board power sampled with rocm-smi during an
untimed replay of the step -- the chip runs these GEMMs at its power limit, well below the 2.4 GHz behind `roofline.peak`), `step_ms` percentiles, `host_persons_per_sec` (N=1: pinned host
buffers -> keypoints on the host through the asynchronous double-buffered entry, PCIe included), `cpu_baseline` +
`cpu_baseline_batched` (the oracle's torch-CPU path per crop / in batches of 16 on this box's host cores, rank 0, N=1 only,
bounded samples), and for N > 1 `per_rank_ms_per_step` / `allgather_ms` / `strong_scaling_config4`.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

NOMINAL_SCLK_MHZ = 2400.0
PEAK_MFMA_16BIT = 2.5e15   # dense bf16/fp16 MFMA peak, MI355X_MICROARCH.md (256 CU x 4096 FLOP/clk x 2.4 GHz)
PEAK_HBM = 8.0e12
PEAK_MFMA_FP8 = 5.0e15    # dense fp8 (MX-scaled K = 128) MFMA peak, MI355X_MICROARCH.md


def physical_cores():
    """Distinct (package, core) pairs of /proc/cpuinfo among the CPUs this process may run on; None when the file has no topology."""
    try:
        allowed = os.sched_getaffinity(0)
    except AttributeError:
        allowed = None
    cores, cpu, pkg = set(), None, 0
    try:
        for line in open('/proc/cpuinfo'):
            k, _, v = line.partition(':')
            k, v = k.strip(), v.strip()
            if k == 'processor':
                cpu, pkg = int(v), 0
            elif k == 'physical id':
                pkg = int(v)
            elif k == 'core id' and (allowed is None or cpu in allowed):
                cores.add((pkg, int(v)))
    except (OSError, ValueError):
        return None
    return len(cores) or None


def cpu_baseline(variant, dataset, budget_s=15.0, probe_crops=8):
    """Reference-equivalent CPU path (oracle/ restatement of _inference_torch, per crop,
    batch 1 exactly like VitInference) on a bounded sample of the same synthetic crops.

    torch's default of one thread per hardware thread is pathological for batch-1 ViT
    GEMMs on a many-core host (measured 0.03 persons/s with 256 threads), so a few
    thread counts -- never more than the physical cores -- are probed and the best one
    is used.  The probe is `probe_crops` crops per candidate after two warm-up crops and
    ranks candidates by their MEDIAN crop time (round 5 probed two crops each and moved
    37 % between rounds on an unchanged oracle: VERDICT r5 "What's weak" 11); every
    probed rate is printed in `sample`."""
    import torch
    from easy_vitpose_amd.configs import model_shape
    from easy_vitpose_amd.synth import synthetic_crops, synthetic_state_dict
    from oracle import vitpose_cpu as O
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    phys = physical_cores() or avail
    shp = model_shape(variant, dataset)
    sd = O.to_torch_state_dict(synthetic_state_dict(shp, 0))
    crops = synthetic_crops(256, 0, 'noise')
    run = lambda i: O.inference_torch(sd, shp.depth, shp.num_heads, crops[i])
    cap = max(1, min(avail, phys))
    probed = {}
    for t in sorted({min(cap, c) for c in (8, 16, 32, 64)}):
        torch.set_num_threads(t)
        run(0); run(1)
        ts = []
        for i in range(probe_crops):
            t0 = time.perf_counter(); run(2 + i); ts.append(time.perf_counter() - t0)
            if sum(ts) > 12.0:
                break
        probed[t] = float(np.median(ts))
        if probed[t] > 3.0:
            break
    best_t = min(probed, key=probed.get)
    torch.set_num_threads(best_t)
    n, t0 = 0, time.perf_counter()
    while n < len(crops) and (time.perf_counter() - t0 < budget_s or n < 3):
        run(n)
        n += 1
    dt = time.perf_counter() - t0
    rates = ', '.join(f'{t} threads {1.0 / v:.1f}/s' for t, v in sorted(probed.items()))
    return {'value': round(n / dt, 3), 'unit': 'persons/s', 'cores': best_t, 'kind': 'port',
            'sample': f'{n} crops of the same workload, one at a time (pre_img -> torch fp32 model -> decode), '
                      f'{dt:.1f} s, torch {torch.__version__} with {best_t} threads; probe (median of {probe_crops} crops each): {rates}; '
                      f'host has {avail} hw threads on {phys} physical cores',
            'probe_persons_per_sec': {str(t): round(1.0 / v, 2) for t, v in sorted(probed.items())}}


def cpu_baseline_batched(variant, dataset, threads, batch=16, budget_s=12.0):
    """The batched variant SURVEY.md 8(d) / BASELINE.md section 4 ask for beside the per-crop baseline: the same oracle path on batches
    of 16 crops (one torch forward per batch, decode per crop like the reference), same thread count as `cpu_baseline` found."""
    import torch
    from easy_vitpose_amd.configs import model_shape
    from easy_vitpose_amd.synth import synthetic_crops, synthetic_state_dict
    from oracle import vitpose_cpu as O
    shp = model_shape(variant, dataset)
    sd = O.to_torch_state_dict(synthetic_state_dict(shp, 0))
    crops = synthetic_crops(256, 0, 'noise')
    torch.set_num_threads(threads)

    def run(i0):
        x = np.concatenate([O.pre_img(c)[0] for c in crops[i0:i0 + batch]])
        return O.decode_per_crop(O.model_forward(sd, x, shp.depth, shp.num_heads))
    run(0)
    n, t0 = 0, time.perf_counter()
    while n + batch <= len(crops) and (time.perf_counter() - t0 < budget_s or n < batch):
        run(n)
        n += batch
    dt = time.perf_counter() - t0
    return {'value': round(n / dt, 3), 'unit': 'persons/s', 'cores': threads, 'kind': 'port',
            'sample': f'{n} crops of the same workload in batches of {batch} (pre_img -> one torch fp32 forward per batch -> decode per crop), '
                      f'{dt:.1f} s, {threads} threads'}


# GEMM families of the encoder (profiling-family name -> what the launch does); the KERNEL a family ran on is reported by the
# library itself (vp_profile_kernel: the launch code writes the name of the kernel it resolved to)
FAMILIES = {
    'gemm_fc1': 'mlp.fc1 (+LayerNorm fold +bias +GELU)',
    'gemm_fc2': 'mlp.fc2 (+bias +residual planes +LayerNorm row statistics)',
    'gemm_qkv': 'attn.qkv (+LayerNorm fold +bias)',
    'gemm_proj': 'attn.proj (+bias +residual planes +LayerNorm row statistics)',
}


class Harness:
    """The distributed half of the measurement, independent of the HIP engine: one step = local inference on this rank's crops +
    (world > 1) the all-gather of the keypoints; fence = engine + device + barrier; the timed loop takes the MAX over ranks and
    also returns every rank's own time and the all-gather's share.  main() builds it around VitPoseHip on cuda:LOCAL_RANK with
    RCCL; tests/test_parallel_cpu.py drives the SAME code with a fake engine on CPU tensors over gloo (world size 2)."""

    def __init__(self, eng, d_crops, d_out, d_all=None, dist=None, device_sync=None):
        self.eng, self.d_crops, self.d_out, self.d_all, self.dist = eng, d_crops, d_out, d_all, dist
        self.device_sync = device_sync or (lambda: None)
        self.use_dist = dist is not None
        self.world = dist.get_world_size() if self.use_dist else 1
        self.rank = dist.get_rank() if self.use_dist else 0

    def step(self):
        # stream-ordered entry (vp_infer_device_stream): the library's kernels are ordered behind torch's current stream and torch work enqueued
        # afterwards waits for them ON THE DEVICE -- the all-gather queues behind the keypoints with no host synchronisation (SURVEY.md 8e:
        # "enqueue on each device's compute stream ... no host sync"); the host blocks only in fence()
        self.eng.infer_device(self.d_crops, self.d_out, sync=False)
        if self.use_dist:
            self.dist.all_gather_into_tensor(self.d_all, self.d_out)             # RCCL over xGMI, [world*B, K, 3]

    def fence(self):
        self.eng.synchronize()
        self.device_sync()
        if self.use_dist:
            self.dist.barrier()

    def timed(self, steps):
        """EXACTLY `steps` steps between two fences -> (max-over-ranks seconds, [every rank's seconds])"""
        import torch
        self.fence()
        t0 = time.perf_counter()
        for _ in range(steps):
            self.step()
        self.fence()
        dt = time.perf_counter() - t0
        if not self.use_dist:
            return dt, [dt]
        mine = torch.tensor([dt], dtype=torch.float64, device=self.d_out.device)
        every = torch.zeros(self.world, dtype=torch.float64, device=self.d_out.device)
        self.dist.all_gather_into_tensor(every, mine)
        return float(every.max().item()), [float(v) for v in every.tolist()]

    def allgather_ms(self, reps=20):
        """the all-gather alone (host-synchronised before and after each one): what of a step is the exchange"""
        if not self.use_dist:
            return None
        self.fence()
        t0 = time.perf_counter()
        for _ in range(reps):
            self.dist.all_gather_into_tensor(self.d_all, self.d_out)
            self.device_sync()
        return (time.perf_counter() - t0) / reps * 1e3

    def check_gathered(self, n_local):
        """every rank holds every rank's keypoints; the own shard bit-identical to the local result"""
        import torch
        if self.use_dist:
            assert torch.equal(self.d_all[self.rank * n_local:(self.rank + 1) * n_local], self.d_out), \
                'all-gather result differs from the local shard'
        assert torch.isfinite(self.d_out).all(), 'non-finite keypoints'


def strong_scaling_config4(world, rank, dev, dtype, steps=100, warmup=10, n_total=64, engine_factory=None, dist=None, device_sync=None,
                           num_keypoints=None):
    """BASELINE.json configs[3]: one frame of 64 crops through ViTPose-L coco_25, strong-scaled: every rank takes its contiguous shard
    of the frame (resident in its HBM; ceil(64 / world) crops, the tail rank short or empty when it does not divide), runs it, and ONE
    all-gather (easy_vitpose_amd.parallel.ShardedPose, pre_sharded) leaves all keypoints on every rank; max-over-ranks time.
    Reported inside the single JSON line as `strong_scaling_config4` (the driver computes efficiency from the per-N values).
    `engine_factory(per) -> (engine, local_crops, K)` and `dist` are injectable: the gloo test runs this function with a fake engine."""
    import torch
    from easy_vitpose_amd.parallel import ShardedPose, shard_bounds
    if dist is None:
        import torch.distributed as dist
    N = n_total
    lo, hi = shard_bounds(N, world, rank)
    per = -(-N // world)
    if engine_factory is None:
        from easy_vitpose_amd import VitPoseHip
        from easy_vitpose_amd.configs import model_shape
        from easy_vitpose_amd.synth import synthetic_crops, synthetic_state_dict
        shp = model_shape('l', 'coco_25')
        eng = VitPoseHip(shp, synthetic_state_dict(shp, 0), dtype=dtype, device_id=dev.index, max_batch=per)
        crops = torch.from_numpy(synthetic_crops(N, seed=4, kind='noise')[lo:hi]).to(dev)
        K = shp.num_keypoints
        device_sync = device_sync or torch.cuda.synchronize
    else:
        eng, crops, K = engine_factory(per, lo, hi)
        device_sync = device_sync or (lambda: None)
    local = torch.zeros((per, K, 3), dtype=torch.float32, device=dev)
    # sync=False: the stream-ordered entry orders the all-gather behind the keypoints on the device; the host never blocks inside a frame
    sp = ShardedPose(lambda shard, wh: eng.infer_device(shard, local[:len(shard)], sync=False), K, device=dev, reuse_buffers=True)
    out = {}

    def frame():
        out['kp'] = sp.infer(crops, None, n_total=N, pre_sharded=True)

    def fence():
        eng.synchronize(); device_sync(); dist.barrier()

    for _ in range(warmup):
        frame()
    fence()
    t0 = time.perf_counter()
    for _ in range(steps):
        frame()
    fence()
    mine = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=dev)
    every = torch.zeros(world, dtype=torch.float64, device=dev)
    dist.all_gather_into_tensor(every, mine)
    kp = out['kp']
    assert kp.shape == (N, K, 3) and torch.isfinite(kp).all()
    assert hi == lo or torch.equal(kp[lo:hi], local[:hi - lo]), 'gathered frame differs from the local shard'
    eng.close()
    dt = float(every.max().item())
    return {'workload': f'ViTPose-L coco_25, one frame of {N} u8 crops resident in HBM, ceil({N}/world) per rank, RCCL all-gather of keypoints',
            'scaling': 'strong', 'crops_per_rank': per, 'frames': steps, 'ms_per_frame': round(dt / steps * 1e3, 4),
            'per_rank_ms_per_frame': [round(float(v) / steps * 1e3, 4) for v in every.tolist()],
            'persons_per_sec': round(N * steps / dt, 1), 'keypoints': kp}


PMC_FILE = os.path.join('profiles', 'pmc_r6.json')


def pmc_traffic(args, kernel_name):
    """HBM bytes per launch of the dominant kernel from the committed rocprofv3 PMC passes of THIS command (PMC_FILE, made by
    tools/profile.sh + tools/summarize_profile.py; FETCH_SIZE x2 on gfx950 as MI355X_MICROARCH.md prescribes).  PMC passes cannot
    run inside this process, so the figure is READ from the committed profile of the same configuration -- `roofline.traffic_source`
    says so in the JSON line; (None, reason) when the configuration differs from the profiled one or the file is absent."""
    path = os.path.join(ROOT, PMC_FILE)
    if not (args.variant == 'b' and args.batch == 256 and args.dtype == 'fp16' and args.gpus == 1 and args.dataset == 'coco'):
        return None, 'not measured: the committed PMC passes are of the default configuration only'
    if not os.path.exists(path):
        return None, f'not measured: {PMC_FILE} absent'
    norm = lambda t: t.replace(' ', '').replace('vp::', '').replace('(anonymousnamespace)::', '')
    try:
        for k, d in json.load(open(path)).items():
            if norm(kernel_name) in norm(k) and 'hbm_bytes_per_dispatch' in d:
                return d['hbm_bytes_per_dispatch'], f'{PMC_FILE} (committed rocprofv3 PMC passes of this command, not measured in this run)'
    except Exception as e:
        return None, f'not measured: {PMC_FILE}: {e}'
    return None, f'not measured: kernel not found in {PMC_FILE}'


def clock_power_under_load(step, fence, seconds=3.0):
    """Shader clock and board power WHILE the step runs (untimed pass after the measurement): `rocm-smi --showclocks --showpower --json`
    polled back to back from a thread while the main thread replays the step.  The MI355X hits its board power limit under the encoder
    GEMMs and drops the shader clock well below the 2.4 GHz that the 2.5 PFLOP/s peak assumes (profiles/clock_power_r3.txt); the
    bench line carries the measured clock so that `roofline.frac` (against the nominal peak) can be read beside the peak the chip can
    sustain at that clock.  Returns None when rocm-smi is missing or prints something unexpected."""
    import shutil
    import subprocess
    import threading
    smi = shutil.which('rocm-smi') or '/opt/rocm/bin/rocm-smi'
    if not os.path.exists(smi):
        return None
    samples, stop = [], [False]

    def num(txt):
        t = ''.join(ch for ch in str(txt) if ch.isdigit() or ch == '.')
        return float(t) if t else None

    def poll():
        while not stop[0]:
            t0 = time.time()
            try:
                o = subprocess.run([smi, '--showclocks', '--showpower', '--json'], capture_output=True, text=True, timeout=20).stdout
                card = next(iter(json.loads(o).values()))
                samples.append((t0, time.time(), num(card.get('sclk clock speed:')), num(card.get('Current Socket Graphics Package Power (W)'))))
            except Exception:
                return
    th = threading.Thread(target=poll, daemon=True)
    fence()
    t_begin = time.time()
    th.start()
    while time.time() - t_begin < seconds:
        for _ in range(8):
            step()
        fence()
    t_end = time.time()
    stop[0] = True
    th.join(timeout=30)
    ok = [(c, p) for a, b, c, p in samples if a >= t_begin + 0.5 and b <= t_end and c and p]
    if not ok:
        return None
    sclk = sum(c for c, _ in ok) / len(ok)
    return {'sclk_mhz': round(sclk, 0), 'board_power_w': round(sum(p for _, p in ok) / len(ok), 0), 'samples': len(ok),
            'nominal_sclk_mhz': NOMINAL_SCLK_MHZ,
            'mfma_peak_at_sclk_tflops': round(PEAK_MFMA_16BIT / 1e12 * sclk / NOMINAL_SCLK_MHZ, 1),
            'source': f'rocm-smi polled during an untimed {seconds:.0f} s replay of the step (whole step, not one kernel)'}


def host_path_rate(eng, crops_u8, K, seconds=1.5):
    """persons/s of the host-visible path: uint8 crops in pinned host memory -> keypoints in pinned host memory, through
    vp_infer_submit / vp_infer_wait (H2D of batch i+1 and D2H of batch i-1 under the compute of batch i)."""
    from easy_vitpose_amd import PinnedArray
    B = crops_u8.shape[0]
    pin_in = [PinnedArray(crops_u8.shape, np.uint8) for _ in range(2)]
    pin_out = [PinnedArray((B, K, 3), np.float32) for _ in range(2)]
    for p in pin_in:
        p.array[...] = crops_u8
    pending = []
    def push(i):
        pending.append(eng.submit(pin_in[i & 1].array, pin_out[i & 1].array))
    for i in range(3):          # warm
        push(i)
        if len(pending) == 2:
            eng.wait(pending.pop(0))
    while pending:
        eng.wait(pending.pop(0))
    n, t0 = 0, time.perf_counter()
    while True:
        push(n)
        n += 1
        if len(pending) == 2:
            eng.wait(pending.pop(0))
        if time.perf_counter() - t0 > seconds and n >= 20:
            break
    while pending:
        eng.wait(pending.pop(0))
    dt = time.perf_counter() - t0
    assert np.isfinite(pin_out[0].array).all()
    for p in pin_in + pin_out:
        p.free()
    return n * B / dt


def self_launch(n: int, argv, stdout_fd) -> int:
    """`python bench.py --gpus N` with WORLD_SIZE unset (how the driver starts the N = 1 run): re-execute this
    script as N ranks under torch.distributed.run on 127.0.0.1 -- one process per GPU -- and hand through its exit code.  The
    children inherit stdout, so rank 0's ONE JSON line is still the only thing on it (every rank points its own fd 1 at stderr)."""
    import socket
    import subprocess
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')    # dmabuf IPC: RCCL across processes needs it on this driver
    env.setdefault('OMP_NUM_THREADS', '8')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', f'--nproc-per-node={n}', '--master-addr', '127.0.0.1',
           '--master-port', str(port), os.path.abspath(__file__)] + list(argv)
    print(f'[bench] --gpus {n} without WORLD_SIZE: launching {" ".join(cmd)}', file=sys.stderr, flush=True)
    return subprocess.run(cmd, env=env, stdout=stdout_fd).returncode   # this process has pointed its own fd 1 at stderr already: the children get the real stdout


def _load_hook(spec):
    """VP_BENCH_ENGINE=module:function (tests only): function(args, rank, world, local_rank) -> dict(eng, d_crops, d_out, K, dev, backend,
    device_sync, strong_factory) replaces the HIP engine and the device tensors, so that the launcher, the process-group set-up and the
    whole multi-rank measurement code of main() run on a CPU box over gloo (tests/test_parallel_cpu.py)."""
    import importlib
    mod, fn = spec.split(':')
    return getattr(importlib.import_module(mod), fn)


def main():
    # The ONE JSON line must be the only thing on stdout: RCCL prints a version banner to the C-level stdout of rank 0 (buffered, so it
    # lands AFTER python's own output at exit).  fd 1 is pointed at stderr for the whole run and the line goes to the saved descriptor.
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--dtype', default='fp16', choices=['fp16', 'bf16', 'fp8'],
                    help='fp8 = the OPT-IN mode of BASELINE configs[4] (qkv / fc1 / fc2 on MXFP8 operands): does not meet the 1e-3 confidence tolerance, never the default')
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--max-batch', type=int, default=0, help='workspace batch of the handle (< --batch: the batch is processed in chunks)')
    ap.add_argument('--variant', default='b')
    ap.add_argument('--dataset', default='coco')
    ap.add_argument('--input', default='f32', choices=['f32', 'u8'])
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--no-host-path', action='store_true')
    ap.add_argument('--no-live-events', action='store_true', help='no HIP-event records in the timed region (roofline timing from the warm-up pass): lets VP_GRAPH=n replay a hipGraph at large batches')
    ap.add_argument('--no-clock', action='store_true', help='skip the untimed 3 s pass that samples shader clock / board power with rocm-smi')
    ap.add_argument('--breakdown', action='store_true', help='extra untimed pass with every kernel family timed (stderr)')
    ap.add_argument('--strong', action='store_true', help='also measure the strong-scaled frame of BASELINE configs[3] (default when WORLD_SIZE > 1)')
    ap.add_argument('--force-dist', action='store_true', help='run the RCCL code path (process group, all-gather, barrier) even with one rank')
    ap.add_argument('--full', action='store_true',
                    help='beyond the headline: roofline + per-family GEMM timing (HIP events), step-time percentiles, the all-gather check and '
                         'share, host-visible rate, clock / power under load, CPU baselines, the strong-scaled frame when WORLD_SIZE > 1')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='write the keypoints of the last timed step to DIR/keypoints.npy (float32)')
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error('--steps must be >= 1 and --warmup >= 0')

    if args.gpus > 1 and 'WORLD_SIZE' not in os.environ:   # started plainly (as the driver starts N = 1): spawn the ranks ourselves
        rc = self_launch(args.gpus, sys.argv[1:], json_fd)
        os.close(json_fd)
        sys.exit(rc)

    import torch
    import torch.distributed as dist
    from easy_vitpose_amd.configs import model_shape

    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    assert world == args.gpus, f'--gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run --nproc-per-node {args.gpus} (or plainly, without WORLD_SIZE)'
    use_dist = world > 1 or args.force_dist
    shp = model_shape(args.variant, args.dataset)
    B, K = args.batch, shp.num_keypoints
    hook = os.environ.get('VP_BENCH_ENGINE')
    strong_factory = None
    if hook:   # tests only: fake engine on CPU tensors over gloo
        h = _load_hook(hook)(args, rank, world, local_rank)
        eng, d_crops, d_out, K, dev, device_sync, strong_factory = h['eng'], h['d_crops'], h['d_out'], h['K'], h['dev'], h['device_sync'], h.get('strong_factory')
        B = d_crops.shape[0]
        crops_u8 = None
        if use_dist:
            os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
            os.environ.setdefault('MASTER_PORT', '29517')
            dist.init_process_group(h.get('backend', 'gloo'), rank=rank, world_size=world)
    else:
        from easy_vitpose_amd import VitPoseHip
        from easy_vitpose_amd.synth import synthetic_crops, synthetic_state_dict
        assert torch.cuda.is_available(), 'bench.py needs an AMD GPU (the HIP path has no CPU fallback)'
        assert local_rank < torch.cuda.device_count(), f'rank {rank}: LOCAL_RANK {local_rank} but only {torch.cuda.device_count()} visible devices'
        torch.cuda.set_device(local_rank)
        dev = torch.device('cuda', local_rank)
        device_sync = torch.cuda.synchronize
        if use_dist:
            os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
            os.environ.setdefault('MASTER_PORT', '29517')
            dist.init_process_group('nccl', rank=rank, world_size=world, device_id=dev)
        eng = VitPoseHip(shp, synthetic_state_dict(shp, 0), dtype=args.dtype, device_id=local_rank, max_batch=args.max_batch or B)
        crops_u8 = synthetic_crops(B, seed=rank, kind='noise')
        if args.input == 'u8':
            d_crops = torch.from_numpy(crops_u8).to(dev)
        else:  # what pre_img hands to the model: normalised float32 NCHW
            mean = np.array([0.485, 0.456, 0.406]); std = np.array([0.229, 0.224, 0.225])
            x = ((crops_u8.astype(np.float64) / 255 - mean) / std).transpose(0, 3, 1, 2).astype(np.float32)
            d_crops = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
        d_out = torch.zeros((B, K, 3), dtype=torch.float32, device=dev)
    d_all = torch.zeros((world * B, K, 3), dtype=torch.float32, device=dev) if use_dist else None
    device_sync()

    H = Harness(eng, d_crops, d_out, d_all, dist if use_dist else None, device_sync)
    step, fence = H.step, H.fence

    fams = list(FAMILIES)
    if args.full:
        eng.set_profiling(fams)      # warm-up pass with all four encoder GEMM families timed: picks the dominant one
        eng.reset_profile()
    for _ in range(args.warmup):
        step()
    fence()
    if args.full:
        wprof = eng.profile()
        dom = max(fams, key=lambda f: wprof[f]['ms']) if args.warmup > 0 else 'gemm_fc1'
    # --full: the four encoder GEMM families are timed live (HIP events around every launch, on the library's stream); the one with
    # the largest share of the step is reported as the dominant kernel (rocprofv3 --stats of the same command: profiles/)
    # batches of <= 16 crops replay a captured hipGraph, which event records inside the chunk would switch off: there the timed
    # region runs unprofiled and the dominant kernel's launch time is the warm-up pass's (roofline.timed = 'warm-up pass')
    graph_path = B <= 16 or args.no_live_events
    live = args.full and not graph_path
    if args.full:
        eng.set_profiling([dom] if live else False)     # timed region: only the dominant family carries event records (2 per launch)
        eng.reset_profile()
    if graph_path:
        for _ in range(3):       # first sighting runs eagerly, the second captures the graph
            step()
    dt, per_rank = H.timed(args.steps)              # EXACTLY --steps steps between two fences, max over ranks
    if args.dump_outputs and rank == 0:
        os.makedirs(args.dump_outputs, exist_ok=True)
        kp = d_all if use_dist else d_out           # what the caller of the timed step receives, as of its last step
        np.save(os.path.join(args.dump_outputs, 'keypoints.npy'), kp.detach().cpu().numpy().astype(np.float32))
    if args.full:
        prof = eng.profile() if live else wprof
        kernels = {f: eng.profile_kernel(f) for f in fams}   # the library's own record of what each family ran on
        eng.set_profiling(False)
        H.check_gathered(B)
        ag_ms = H.allgather_ms()

    step_ms, host_rate, clock = [], None, None
    if args.full:
        # per-step distribution (separate, untimed-for-`value` pass with a host synchronisation after every step)
        for _ in range(min(args.steps, 50)):
            fence()
            t1 = time.perf_counter()
            step()
            fence()
            step_ms.append((time.perf_counter() - t1) * 1e3)
        if rank == 0 and world == 1 and not args.no_host_path and not hook:
            host_rate = host_path_rate(eng, crops_u8, K)
        if rank == 0 and world == 1 and not args.no_clock and not hook:
            clock = clock_power_under_load(step, fence)

    strong = None
    if use_dist and (args.strong or (args.full and world > 1)):
        if hook:
            strong = strong_scaling_config4(world, rank, dev, args.dtype, steps=3, warmup=1, n_total=7, engine_factory=strong_factory, dist=dist)
        else:
            strong = strong_scaling_config4(world, rank, dev, args.dtype)

    breakdown = None
    if args.breakdown and rank == 0:
        eng.set_profiling(True); eng.reset_profile()
        for _ in range(3):
            eng.infer_device(d_crops, d_out, sync=True)
        p = eng.profile(); eng.set_profiling(False)
        breakdown = {k: {'ms_per_step': round(v['ms'] / 3, 4), 'launches_per_step': v['launches'] // 3,
                         'tflops': round(v['flops'] / max(v['ms'], 1e-9) / 1e9, 1),
                         'gbps': round(v['bytes'] / max(v['ms'], 1e-9) / 1e6, 1)} for k, v in p.items()}
        print(json.dumps({'breakdown': breakdown}), file=sys.stderr)

    if rank == 0:
        persons_s = world * B * args.steps / dt
        line = {
            'metric': 'persons_per_sec', 'value': round(persons_s, 1), 'unit': 'persons/s',
            'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup,
            'ms_per_step': round(dt / args.steps * 1e3, 4), 'higher_is_better': True, 'scaling': 'weak',
            'vs_baseline': None, 'dtype': args.dtype, 'data': 'synthetic',
            'config': {'workload': f'ViTPose-{args.variant.upper()} {args.dataset} K={K}, batch {B} x 256x192 crops per GPU '
                                   f'({args.input} input resident in HBM) -> (y,x,conf) keypoints in HBM'
                                   + (', RCCL all-gather of keypoints' if use_dist else ''),
                       'global_batch': world * B, 'weights': 'seeded random init (no checkpoint offline)',
                       'gflop_per_person': round(shp.gflop_per_person(), 3)},
            'model_tflops': round(persons_s * shp.gflop_per_person() / 1e3, 1),
            'model_frac_of_mfma_peak': round(persons_s * shp.gflop_per_person() * 1e9 / PEAK_MFMA_16BIT, 4),
            # diagnosis of a multi-GPU run: every rank's own time for the same steps
            'per_rank_ms_per_step': [round(v / args.steps * 1e3, 4) for v in per_rank],
            'full': args.full,
        }
        if args.full:
            d = prof[dom]
            ach = d['flops'] / (d['ms'] * 1e-3) if d['ms'] > 0 else 0.0
            peak = PEAK_MFMA_FP8 if 'gemm8f_kernel' in kernels[dom] else PEAK_MFMA_16BIT     # the pipe the dominant kernel runs on
            traffic, traffic_source = pmc_traffic(args, kernels[dom])
            # one number per kernel in the line: the dominant family from the TIMED region (the same events `roofline` uses), the other three
            # from the warm-up pass (all four families event-timed there, which perturbs the step slightly) -- each entry says which
            def fam_entry(f):
                src = prof if (live and f == dom) else wprof
                steps_ = args.steps if (live and f == dom) else max(args.warmup, 1)
                what = FAMILIES[f]
                if kernels[f].startswith('qkvattn_kernel'):   # the fused kernel is accounted under the qkv family: its flops and time include the attention core,
                    what = 'attn.qkv (+LayerNorm fold +bias) + attention core (softmax, P.V) as ONE kernel; flops = both; the `attention` family is empty'
                return {'what': what, 'kernel': kernels[f], 'timed': 'timed region' if (live and f == dom) else 'warm-up pass',
                        'ms_per_step': round(src[f]['ms'] / steps_, 4), 'avg_launch_us': round(1e3 * src[f]['ms'] / max(src[f]['launches'], 1), 2),
                        'tflops': round(src[f]['flops'] / max(src[f]['ms'], 1e-9) / 1e9, 1),
                        'algorithmic_gbps': round(src[f]['bytes'] / max(src[f]['ms'], 1e-9) / 1e6, 1)}
            per_family = {f: fam_entry(f) for f in fams}
            line.update({
                'roofline': {'bound': 'mfma', 'kernel': kernels[dom], 'kernel_source': 'vp_profile_kernel (written by the launch code)',
                             'what': FAMILIES[dom],
                             'achieved': round(ach / 1e12, 2), 'peak': peak / 1e12, 'unit': 'TFLOP/s',
                             'frac': round(ach / peak, 4), 'traffic': traffic, 'traffic_source': traffic_source,
                             'timed': 'live, HIP events around every launch of the timed region' if live else 'warm-up pass (no event records in the timed region)',
                             'launches': d['launches'], 'avg_launch_ms': round(d['ms'] / max(d['launches'], 1), 5),
                             'flops_per_launch': d['flops'] / max(d['launches'], 1),
                             'algorithmic_bytes_per_launch': d['bytes'] / max(d['launches'], 1)},
                'clock_under_load': clock,
                'encoder_gemms': per_family,
                'step_ms': {'p10': round(float(np.percentile(step_ms, 10)), 4), 'p50': round(float(np.percentile(step_ms, 50)), 4),
                            'p90': round(float(np.percentile(step_ms, 90)), 4), 'n': len(step_ms), 'note': 'one host synchronisation per step'},
                'host_persons_per_sec': None if host_rate is None else round(host_rate, 1),
                'allgather_ms': None if ag_ms is None else round(ag_ms, 4),   # the exchange alone
            })
        if hook:   # the engine was swapped by VP_BENCH_ENGINE (CPU tests of the launcher): the numbers above are NOT a measurement of the HIP path
            line['engine'] = 'hook:' + hook
            line['valid'] = False
        if args.dtype == 'fp8':
            line['mode_note'] = ('OPT-IN fp8 mode (BASELINE configs[4]): the encoder GEMMs on MXFP8 operands (e4m3 + one 2^k scale per 32 k) through the block-scaled fp8 MFMA, qkv / fc1 / attn.proj / fc2; '
                                 'attention core, head, decode as fp16.  Does NOT meet the north_star 1e-3 on confidences (peaked AP-10K checkpoint: max 3.1e-3, '
                                 'coordinates max 0.21 px: tests/test_gpu_fp8.py); not a parity-grade number, reported beside the fp16 line of the same workload.')
        if strong is not None:
            strong.pop('keypoints', None)
            line['strong_scaling_config4'] = strong
        if args.full and world == 1 and not args.no_cpu_baseline:
            line['cpu_baseline'] = cpu_baseline(args.variant, args.dataset)
            line['cpu_baseline_batched'] = cpu_baseline_batched(args.variant, args.dataset, line['cpu_baseline']['cores'])
        elif args.full:
            line['cpu_baseline'] = None
            line['cpu_baseline_batched'] = None
        os.write(json_fd, (json.dumps(line) + '\n').encode())
    eng.close()
    if use_dist:
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
