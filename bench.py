'''
bench.py -- FusionNet training throughput on MI355X (BASELINE.json metric).

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

Workload (BASELINE.json configs[1]): the published FusionNet (bash/train_fusionnet_nuscenes.sh:27-40), fp32,
per-GPU batch 8, 900x1600, 64-point synthetic radar maps; one step = forward + ground-truth outlier removal +
masked-L1 loss (w_lidar 2.0) + backward + Adam, training-mode BatchNorm -- the body of the reference's loop
(src/fusionnet_main.py:369-399).  Inputs are resident in HBM before the timed region.

N > 1: one process per GPU over RCCL, the same per-GPU batch (weak scaling), gradients all-reduced in buckets that
overlap the backward pass.  Started WITHOUT a launcher (`python bench.py --gpus N`, WORLD_SIZE unset) the parent starts
the N ranks itself as child processes -- before it touches the GPU, and it never execs -- and refuses (exit 2) when fewer
than N devices are visible; it never silently measures fewer GPUs than it was asked for.

Rank 0 prints ONE JSON line.  A plain run sets up, warms up (W steps, then the untimed pre-heat), times exactly K steps and prints
the line: `value`, `ms_per_step` and the configuration.  --dump-outputs DIR then also writes what the last timed step computed
(dump_outputs below).

--full adds everything else the benchmark measures or checks, after the timed steps.  `roofline`: every launch of the dominant
kernel family (the 3x3 stride-1 implicit-GEMM convolution, forward + input-gradient launches) is bracketed by events on the launch
stream; achieved = algorithmic FLOP / event time.  `cpu_baseline` (N = 1 only) times the CPU oracle on the host cores on a bounded
sample (2 warm-up + 5 timed training steps at batch 1, 900x1600, median; --cpu-baseline-batch8 adds a batch-8 leg).  The loss of the
first step is compared with the value the CPU oracle computed for the same seeds (tests/golden/bench_expected.json): a wrong step
exits 3.  At the default shape, `exact_tier` and `other_configs` time the other arithmetic tier and configurations.

Other legs (the driver's default run is the training metric):  --workload infer  (BASELINE.json configs[4]: eval-mode,
BatchNorm folded, batch 32, hipGraph-captured);  --workload radarnet  (configs[2]: RadarNet stage 1, 16 images x 4 points).
'''

import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

F32_MFMA_PEAK_TFLOPS = 157.3   # /opt/skills/guides/MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, 256 CUs x 2.4 GHz
BF16_MFMA_PEAK_TFLOPS = 2500.0  # same guide: dense bf16 MFMA peak (the 5 PF headline includes 2:1 sparsity)
HBM_PEAK_GBS = 8000.0
# what a loop of nothing but v_mfma_f32_32x32x16_bf16 on random operand bits sustains at the ~1.4 kW board limit
# (tools/probe/mfma_issue_probe.hip: 17.0 ns per MFMA per SIMD) -- reported next to `frac`, never instead of it
BF16_MFMA_SUSTAINED_TFLOPS = 1970.0
# partial products the split kernels execute per fp32 multiply-add, by arithmetic tier
SPLIT_PRODUCTS = {'f32': 3, 'f32_3plane': 6, 'bf16': 1}
SPLIT_PIPE = {
    'f32': 'fp16 MFMA (v_mfma_f32_32x32x16_f16): 3 partial products of two scaled fp16 planes per fp32 multiply, fp32 accumulate',
    'f32_3plane': 'bf16 MFMA: 6 exact partial products of three bf16 planes per fp32 multiply, fp32 accumulate',
    'bf16': 'bf16 MFMA, bf16 operands, fp32 accumulate'}
TIER_TEXT = {'f32': 'fp32 tensors, two scaled fp16 planes', 'f32_3plane': 'fp32 tensors, three bf16 planes', 'bf16': 'bf16 tensors and operands'}
TRAIN_GFLOP_PER_SAMPLE = 994.8  # forward + dgrad + wgrad of the reference's 9-tap convolutions at 900x1600
FWD_GFLOP_PER_SAMPLE = 333.09
KERNEL_NAMES = {
    0: 'conv_fwd_kernel 3x3 s1', 1: 'conv_fwd_kernel 3x3 s2', 2: 'conv_fwd_kernel 1x1', 3: 'conv_fwd_kernel 7x7 s2 stem',
    5: 'conv_split_kernel 3x3 s1', 6: 'conv_split_kernel 3x3 s2', 8: 'conv_split_kernel 4x4 stem on the space-to-depth image', 9: 'conv_split_kernel 2x2 phases',
    10: 'conv_wgrad_kernel 3x3 s1', 11: 'conv_wgrad_kernel 3x3 s2', 12: 'conv_wgrad_kernel 1x1', 13: 'conv_wgrad_kernel 7x7 s2 stem',
}


def decode_kernel_id(kid):
    '''rcf_conv_info.kernel_id / wgrad_kernel_id (csrc/rcf_conv_impl.h: rcf_conv2d_query) -> (kernel class, arithmetic it ran on).
    forward / input gradient: kind * 1000 + ... (+ 5000 split); weight gradient: 10000 + kind * 1000 + ... (+ 5000 split);
    + 20000: bf16 operands, + 40000: two scaled fp16 planes.'''
    tier = kid // 20000
    base = kid % 20000
    wgrad = base >= 10000
    b = base % 10000
    split = b >= 5000
    kind = (b - 5000) // 1000 if split else b // 1000
    kname = {0: '3x3 stride 1', 1: '3x3 stride 2', 2: '1x1', 3: '7x7 stride-2 stems', 4: '2x2 phases'}.get(kind, 'kind %d' % kind)
    if split:
        arith = {0: 'three bf16 planes, 6 products per multiply (bf16 MFMA)', 1: 'bf16 operands, 1 product (bf16 MFMA)',
                 2: 'two scaled fp16 planes, 3 products per multiply (fp16 MFMA)'}[tier]
    else:
        arith = 'f32 MFMA (exact fp32 products)'
    return kname + (' weight gradient' if wgrad else ' forward + input gradient'), arith


def arithmetic_of_step(table, n_steps):
    '''config.arithmetic: which arithmetic each class of convolution launches of the measured step ran on -- generated from the kernel
    ids the step LAUNCHED (engine -> ops.KernelTimer), not written by hand.  {class: {arithmetic: launches per step}} plus one line.'''
    by = {}
    for kid, (cnt, flops, ms) in table.items():
        k, a = decode_kernel_id(kid)
        r = by.setdefault(k, {}).setdefault(a, [0, 0.0])
        r[0] += cnt
        r[1] += ms
    out = {k: {a: {'launches_per_step': round(v[0] / float(n_steps), 1), 'ms_per_step': round(v[1] / n_steps, 3)} for a, v in d.items()}
           for k, d in sorted(by.items())}
    line = '; '.join('%s: %s' % (k, ' / '.join('%s x %g' % (a.split(',')[0], v['launches_per_step']) for a, v in d.items())) for k, d in out.items())
    return out, line


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=100, help='timed steps (default: ~7 s of GPU time at batch 8)')
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--workload', choices=('train', 'infer', 'radarnet'), default='train')
    ap.add_argument('--batch', type=int, default=0, help='per-GPU batch (default: 8 train, 32 infer, 16 radarnet images)')
    ap.add_argument('--height', type=int, default=900)
    ap.add_argument('--width', type=int, default=1600)
    ap.add_argument('--points', type=int, default=64)
    ap.add_argument('--dtype', choices=('f32', 'f32_3plane', 'bf16'), default=None,
                    help='f32: the reference arithmetic (the metric; default for train): fp32 tensors, fp32-accurate products -- the 3x3 / '
                         '2x2 split kernels on two scaled fp16 planes (three products per multiply; fp32-convolution-class error against '
                         'fp64, tests/test_hip_f16x2.py), the rest on the f32 MFMA.  f32_3plane (train only): the same with the split '
                         'kernels on three bf16 planes / six products (the previous rounds\' exact tier).  bf16: bf16 tensors in HBM and '
                         'bf16 MFMA operands, fp32 accumulate / master weights / BatchNorm statistics (BASELINE.json configs 2-4; default '
                         'for infer and radarnet)')
    ap.add_argument('--preheat-s', type=float, default=4.0,
                    help='untimed steps run for this many seconds after the W warm-up steps, so the timed steps see the clocks '
                         'of a board at its power limit and not the boost clocks of a cold one')
    ap.add_argument('--graph', type=int, default=-1, help='train: replay the step from one hipGraph / graph segments (1) or launch it '
                                                          'eagerly with per-launch events (0: the profiled form); default: eager '
                                                          'launches with the weight gradients on a side stream -- measured faster than '
                                                          'the replayed graph, which serialises the two branches (bitwise the same step)')
    ap.add_argument('--full', action='store_true',
                    help='after the timed steps, also measure and check everything beyond the headline: roofline and per-kernel events, '
                         'host enqueue time, the data-parallel overlap, the first-step loss against the CPU oracle, `cpu_baseline`, and at '
                         'the default shape `exact_tier` and `other_configs` (each of the last three can be skipped with its --no- option)')
    ap.add_argument('--dump-outputs', type=str, default='', metavar='DIR',
                    help='write what the last timed step computed to DIR/<name>.npy (float32, the loss float64; a fixed seeded sample '
                         'of an output larger than 4 Mi elements; at most 64 MB in all)')
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--side-leg', action='store_true', help='(accepted for older command lines: the legs below are part of --full)')
    ap.add_argument('--no-side-leg', action='store_true', help='--full: skip `exact_tier`: the same step on the three-plane bf16 split '
                                                               '(f32_3plane), 20 timed steps after the metric\'s timed region')
    ap.add_argument('--no-other-configs', action='store_true',
                    help='--full: skip `other_configs`: short legs (10 timed steps / replays each, after the metric\'s timed region, N = 1 '
                         'only) of BASELINE.json configs[3] per GPU (bf16 training), configs[4] (bf16 inference, batch 32, hipGraph) and '
                         'configs[2] (RadarNet bf16 training), each checked against the CPU oracle\'s recorded values')
    ap.add_argument('--leg-steps', type=int, default=10, help='timed steps of each `other_configs` leg (exact_tier: twice that)')
    ap.add_argument('--cpu-baseline-batch8', action='store_true', help='cpu_baseline: add a batch-8 leg (1 warm-up + 2 timed steps, ~3 min)')
    ap.add_argument('--kernel-table', type=str, default='', help='write the per-kernel event table (JSON) here')
    return ap.parse_args()


# ---------------------------------------------------------------------------------------------------------------- launcher
def spawn_ranks(args):
    '''`python bench.py --gpus N` without a launcher: start N ranks as children.  Runs before anything touches the GPU in this
    process (torch.cuda.device_count() does not initialise it on this image) and never execs.'''
    import socket
    import torch
    n_dev = torch.cuda.device_count()
    if os.environ.get('RCF_BENCH_SINGLE_DEVICE') and n_dev >= 1:   # tests on a 1-GPU box: every rank shares cuda:0 (gloo backend)
        n_dev = args.gpus
    if n_dev < args.gpus:
        sys.stderr.write('bench.py: --gpus %d but only %d device(s) visible; refusing to measure fewer GPUs than asked\n'
                         % (args.gpus, n_dev))
        return 2
    import tempfile
    RENDEZVOUS_ERRORS = ('EADDRINUSE', 'ddress already in use', 'failed to bind', 'server socket has failed', 'DistStoreError',
                         'DistNetworkError', 'connect() timed out', 'Connection refused', 'store timeout')
    rc = 0
    for attempt in range(2):
        # a free port, found by binding port 0 and closing the socket: another process can take it before the children bind it.  ONLY
        # that failure -- a rendezvous / bind error in a rank's stderr -- is retried, once, on a fresh port; any other early death (out of
        # memory, a HIP fault, an import error) is a real failure and is reported as what it is, once
        s = socket.socket()
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
        s.close()
        procs, logs = [], []
        for r in range(args.gpus):
            env = dict(os.environ)
            env.update({'RANK': str(r), 'LOCAL_RANK': str(r), 'WORLD_SIZE': str(args.gpus), 'LOCAL_WORLD_SIZE': str(args.gpus),
                        'MASTER_ADDR': '127.0.0.1', 'MASTER_PORT': str(port), 'HSA_ENABLE_IPC_MODE_LEGACY': '0',
                        'RCF_BENCH_SELF_SPAWNED': '1'})
            logs.append(tempfile.TemporaryFile(mode='w+'))
            procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env, stderr=logs[-1]))
        # fail fast: a rank that dies would leave the others waiting in a collective until the backend's (30-minute) timeout
        rc = 0
        live = list(procs)
        while live:
            for p in list(live):
                code = p.poll()
                if code is None:
                    continue
                live.remove(p)
                if code != 0 and rc == 0:
                    rc = code
                    sys.stderr.write('bench.py: a rank exited with code %d; stopping the other %d\n' % (code, len(live)))
                    for q in live:
                        q.terminate()
            if live:
                time.sleep(0.2)
        errs = []
        for f in logs:
            f.seek(0)
            errs.append(f.read())
            f.close()
        rendezvous = rc != 0 and any(sig in e for e in errs for sig in RENDEZVOUS_ERRORS)
        if not (rendezvous and attempt == 0):
            for e in errs:
                sys.stderr.write(e)
            break
        sys.stderr.write('bench.py: the ranks could not rendezvous on port %d (taken between probing and binding?); retrying once on a fresh port\n' % port)
    return rc


# ---------------------------------------------------------------------------------------------------------------- CPU baseline
def _cpu_model():
    try:
        for line in open('/proc/cpuinfo'):
            if line.startswith('model name'):
                return line.split(':', 1)[1].strip()
    except Exception:
        pass
    return 'unknown'


def _cpu_steps(model, opt, b, n_steps, torch):
    times = []
    for i in range(n_steps):
        t0 = time.time()
        out = model.forward(b['image'], b['input_depth'])
        loss = model.compute_loss(out, b['ground_truth'], b['lidar_map'], 2.0)[0]
        opt.zero_grad()
        loss.backward()
        opt.step()
        times.append(time.time() - t0)
        if i == 0 and times[0] > 60.0:   # a slow host: keep the run bounded, report the single step and say so
            break
    return times


def cpu_baseline(height, width, points, batch8=False):
    '''The CPU oracle (stock PyTorch fp32, oneDNN) on the host cores, SURVEY.md 8d's protocol: training steps at batch 1, 2 warm-up +
    5 timed, median (~50 s on the GPU box's host).  batch8=True adds the batch-8 leg (1 warm-up + 2 timed: ~3 min, behind a flag so
    the default run stays within minutes).'''
    import torch
    from rcf_amd import synth
    from oracle.fusionnet_oracle import FusionNetOracle
    # torch's default intra-op thread count (= physical cores): setting it to the logical-CPU count
    # (256 on the 2 x EPYC 9575F box) oversubscribes oneDNN and is ~25x slower
    model = FusionNetOracle(**synth.PUBLISHED)
    synth.fill_state_dict_([model.encoder, model.decoder], 1234)
    opt = torch.optim.Adam([{'params': model.parameters(), 'weight_decay': 0.0}], lr=1e-3)
    model.train()
    times = _cpu_steps(model, opt, synth.make_batch(1, height, width, points, seed=99), 7, torch)
    timed = sorted(times[2:]) if len(times) > 2 else times
    dt = timed[len(timed) // 2]
    rec = {'value': round(1.0 / dt, 5), 'unit': 'samples/s', 'cores': torch.get_num_threads(), 'kind': 'port',
           'cpu': _cpu_model(), 'logical_cpus': os.cpu_count(),
           'sample': '%s training steps (fwd+loss+bwd+Adam) at batch 1, %dx%d, published net, CPU oracle (stock PyTorch fp32, oneDNN); '
                     'step times %s s' % ('2 warm-up + median of %d timed' % len(timed) if len(times) > 2 else '1 cold', height, width,
                                          [round(t, 2) for t in times])}
    if batch8:
        t8 = _cpu_steps(model, opt, synth.make_batch(8, height, width, points, seed=1234), 3, torch)
        timed8 = sorted(t8[1:]) if len(t8) > 1 else t8
        rec['batch8'] = {'value': round(8.0 / timed8[len(timed8) // 2], 5), 'unit': 'samples/s',
                         'sample': '1 warm-up + median of %d timed training steps at batch 8; step times %s s' % (len(timed8), [round(t, 2) for t in t8])}
    return rec


# ---------------------------------------------------------------------------------------------------------------- helpers
def _csrc_sha():
    h = hashlib.sha256()
    for name in sorted(os.listdir(os.path.join(ROOT, 'radar-camera-fusion-depth_amd', 'csrc'))):
        if not name.endswith(('.h', '.hip')):
            continue      # (a stray cache directory is not a kernel source)
        h.update(open(os.path.join(ROOT, 'radar-camera-fusion-depth_amd', 'csrc', name), 'rb').read())
    return h.hexdigest()[:16]


def _pmc_traffic(kernel_name):
    '''HBM bytes per launch of the dominant kernel from the newest committed rocprofv3 --pmc passes of this same command
    (profiles/rNN_pmc_bench.json).  PMC counters cannot be read from inside the process, so this number comes from a profile run;
    it is reported only when that run profiled the kernels this tree builds (same csrc hash), else null with the reason.'''
    import glob
    cands = sorted(glob.glob(os.path.join(ROOT, 'profiles', 'r*_pmc_bench.json')))
    if not cands:
        return None, 'no PMC profile committed'
    path = cands[-1]
    try:
        pmc = json.load(open(path))
        row = pmc.get(kernel_name, {})
        val = round(row['hbm_bytes_per_launch'] / 1e9, 4)
    except Exception:
        return None, '%s has no row for this kernel' % os.path.basename(path)
    meta = pmc.get('_meta', {})
    src = 'profiles/%s (GB per launch, FETCH_SIZE x2 + WRITE_SIZE; collected at commit %s)' % (os.path.basename(path),
                                                                                               meta.get('head', 'of round 1'))
    if meta.get('csrc_sha') != _csrc_sha():
        return None, 'stale: ' + src + ' profiled other kernel sources than this tree (was %s GB)' % val
    return val, src


def _encoder_3x3(timer, ev_steps, dtype):
    flops = ms = 0.0
    n = 0
    for (kid, tag), (c, f, m) in getattr(timer, 'layers', {}).items():
        if tag.startswith('encoder ') and (' k3 ' in tag or ' k2 ' in tag):   # k2: the phase forms of the stride-2 layers' gradients
            flops += f; ms += m; n += c
    if ms <= 0.0:
        return None
    tf = flops / (ms * 1e-3) / 1e12
    prod = SPLIT_PRODUCTS[dtype]
    return {'launches_per_step': n // max(1, ev_steps), 'gflop_per_step': round(flops / max(1, ev_steps) / 1e9, 1),
            'ms_per_step': round(ms / max(1, ev_steps), 3), 'tflops_algorithmic': round(tf, 2),
            'tflops_executed': round(tf * prod, 1), 'frac_of_pipe_peak': round(tf * prod / BF16_MFMA_PEAK_TFLOPS, 4),
            'note': 'forward + input-gradient + weight-gradient launches of the encoder\'s 3x3 convolutions; executed = algorithmic x %d '
                    'partial products (the few stride-2 forward launches on the f32 MFMA are priced the same way)' % prod}


def _wgrad_3x3(timer, ev_steps, dtype):
    '''The 3x3 / 2x2 weight-gradient launches on the 16-bit matrix pipe (kernel ids 10000 + ... + 5000 split): round 6 rebuilt this family
    (csrc/rcf_conv_wgrad_tr.h, ids with the hundreds digit 3 / 7), so the driver's line carries its rate next to the forward family's.'''
    flops = ms = 0.0
    n = n_tr = 0
    for (kid, tag), (c, f, m) in getattr(timer, 'layers', {}).items():
        base = kid % 20000
        if base >= 15000 and (' k3 ' in tag or ' k2 ' in tag):      # a split weight-gradient kernel
            flops += f; ms += m; n += c
            if (kid // 100) % 10 in (3, 7):
                n_tr += c
    if ms <= 0.0:
        return None
    tf = flops / (ms * 1e-3) / 1e12
    prod = SPLIT_PRODUCTS[dtype]
    return {'launches_per_step': n // max(1, ev_steps), 'on_conv_wgrad_tr_kernel': n_tr // max(1, ev_steps),
            'gflop_per_step': round(flops / max(1, ev_steps) / 1e9, 1), 'ms_per_step': round(ms / max(1, ev_steps), 3),
            'tflops_algorithmic': round(tf, 2), 'tflops_executed': round(tf * prod, 1),
            'frac_of_pipe_peak': round(tf * prod / BF16_MFMA_PEAK_TFLOPS, 4),
            'note': 'kernel + reduction per launch, single-stream events; the family runs at 1.57-1.65 GHz at the 1400 W cap '
                    '(profiles/r06_power_bound.txt): frac_of_pipe_peak is against the 2.4 GHz peak'}


def _pmc_value(kernel_name, field):
    import glob
    cands = sorted(glob.glob(os.path.join(ROOT, 'profiles', 'r*_pmc_bench.json')))
    try:
        pmc = json.load(open(cands[-1]))
        if pmc.get('_meta', {}).get('csrc_sha') != _csrc_sha():
            return None
        return round(float(pmc[kernel_name][field]), 4)
    except Exception:
        return None


def _pmc_workload(workload, family, field):
    '''A value of the newest committed profiles/rNN_pmc_<workload>.json (tools/pmc_families.py), or (None, why): only when that profile
    was taken on the kernel sources this tree builds.'''
    import glob
    cands = sorted(glob.glob(os.path.join(ROOT, 'profiles', 'r[0-9][0-9]_pmc_%s.json' % workload)))
    if not cands:
        return None, 'no PMC profile of this workload committed'
    try:
        pmc = json.load(open(cands[-1]))
        meta = pmc.get('_meta', {})
        src = 'profiles/%s (rocprofv3 --pmc passes of this command, collected at commit %s)' % (os.path.basename(cands[-1]), meta.get('head'))
        if meta.get('csrc_sha') != _csrc_sha():
            return None, 'stale: ' + src + ' profiled other kernel sources than this tree'
        return float(pmc[family][field]), src
    except Exception:
        return None, '%s has no such row' % os.path.basename(cands[-1])


# an eager step whose enqueue takes more than this share of its GPU time is host-bound: fall back to the replayed graph (the environment
# override exists for the test that forces the fallback on a fast host)
HOST_BOUND_FRAC = float(os.environ.get('RCF_BENCH_HOST_BOUND_FRAC', '0.8'))


def _expected_first_loss(key, world=1, w_lidar=2.0):
    '''The CPU oracle's loss of the first step.  Under data parallelism the step computes the reference's ONE masked mean over the
    gathered batch (src/fusionnet_main.py:385, src/fusionnet_model.py:245-253): rank r trains on data seed 1234 + r, so the expected
    value is formed from the oracle's per-seed sums and valid counts (BatchNorm is per replica, so per-seed oracle runs at the
    per-GPU batch are exactly the replicas' forwards) -- NOT rank 0's own mean.'''
    path = os.path.join(ROOT, 'tests', 'golden', 'bench_expected.json')
    try:
        rec = json.load(open(path))[key]
        if world == 1:
            return float(rec['first_step_loss'])
        per = [rec['per_data_seed'][str(1234 + r)] for r in range(world)]
        sup = sum(p['sum_abs_gt'] for p in per) / sum(p['count_gt'] for p in per)
        lid = sum(p['sum_abs_lidar'] for p in per) / sum(p['count_lidar'] for p in per)
        return sup + w_lidar * lid
    except Exception:
        return None


DUMP_SAMPLE = 1 << 22           # elements written of a larger output (16 MB in float32)
DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(dirpath, arrays):
    '''--dump-outputs: {name: tensor} of the last timed step -> dirpath/<name>.npy, float64 tensors as float64 and everything else as
    float32, so that two builds can be compared output for output.  A tensor of more than DUMP_SAMPLE elements is written flattened as
    <name>_sample.npy: the elements at DUMP_SAMPLE distinct sorted indices drawn by a generator seeded with its element count, the same
    indices on every run and every build.'''
    import numpy as np
    import torch
    os.makedirs(dirpath, exist_ok=True)
    total = 0
    for name, t in arrays.items():
        t = t.detach()
        if t.numel() > DUMP_SAMPLE:
            idx = np.sort(np.random.default_rng(t.numel()).choice(t.numel(), DUMP_SAMPLE, replace=False))
            t = t.reshape(-1)[torch.from_numpy(idx).to(t.device)]
            name += '_sample'
        a = (t if t.dtype == torch.float64 else t.float()).cpu().numpy()     # (numpy has no bf16)
        total += a.nbytes
        if total > DUMP_LIMIT_BYTES:
            raise RuntimeError('--dump-outputs: more than %d bytes' % DUMP_LIMIT_BYTES)
        np.save(os.path.join(dirpath, name + '.npy'), a)


def _flat_parameters(model):
    import torch
    return torch.cat([p.detach().reshape(-1) for p in model.parameters()])


def _rollback_point(model, opt):
    '''--dump-outputs: the pre-heat runs for a time, not for a number of steps, so its training steps are rolled back (the model's
    own checkpoint round trip, in memory): the dumped step then follows the same number of steps on every run and every build.
    Returns the function that restores the training state of now.'''
    import io
    buf = io.BytesIO()
    model.save_model(buf, 0, opt)

    def restore():
        buf.seek(0)
        model.restore_model(buf, opt)
    return restore


# ---------------------------------------------------------------------------------------------------------------- rank body
def run_rank(args):
    import torch
    import torch.distributed as dist
    import rcf_amd  # noqa: F401
    from rcf_amd import ops, parallel, synth, train

    affinity = parallel.pin_rank_to_gpu_numa_node()     # before anything touches the GPU (also under a launcher: LOCAL_RANK from the env)
    rank, world, local_rank = parallel.init_from_env()
    if world != args.gpus:
        raise SystemExit('--gpus %d but WORLD_SIZE=%d' % (args.gpus, world))
    if not torch.cuda.is_available():
        raise SystemExit('bench.py needs a GPU: the hot path is HIP-only')
    single_dev = bool(os.environ.get('RCF_BENCH_SINGLE_DEVICE'))   # tests on a 1-GPU box (gloo backend): every rank shares cuda:0
    if world > 1 and not single_dev and torch.cuda.device_count() < world:
        raise SystemExit('--gpus %d but only %d device(s) visible' % (world, torch.cuda.device_count()))
    dev = torch.device('cuda', local_rank if (world > 1 and not single_dev) else 0)
    torch.cuda.set_device(dev)
    if args.workload != 'train':
        if args.dtype == 'f32_3plane':
            raise SystemExit('--dtype f32_3plane is a training leg')
        if world > 1:
            raise SystemExit('--workload %s is a single-GPU leg' % args.workload)
        return run_infer(args, dev) if args.workload == 'infer' else run_radarnet(args, dev)
    dtype = args.dtype or 'f32'
    batch = args.batch or 8

    model = train.build_model(synth.PUBLISHED, device=dev)
    synth.fill_state_dict_([model.encoder, model.decoder], 1234)   # seeded U(+-1/sqrt(fan_in)) weights, identical on every rank
    model.compute_dtype = {'bf16': 'bf16', 'f32_3plane': 'fp32_3plane'}.get(dtype, 'fp32')
    if world > 1:
        model.data_parallel()
    opt = train.make_optimizer(model, lr=1e-3)
    model.train()
    b = synth.make_batch(batch, args.height, args.width, args.points, seed=1234 + rank)
    image, input_depth = b['image'].to(dev), b['input_depth'].to(dev)
    gt, lidar = b['ground_truth'].to(dev), b['lidar_map'].to(dev)

    from rcf_amd.net_utils import OutlierRemoval
    outlier = OutlierRemoval(kernel_size=7, threshold=1.5)   # bash/train_fusionnet_nuscenes.sh:48-49
    last = {}     # --dump-outputs: the newest eager step's output depth (a replayed graph hands its caller the loss alone)

    def eager_step():
        loss, _, output_depth = train.train_step(model, opt, image, input_depth, gt, lidar, outlier_removal=outlier)
        if args.dump_outputs:
            last['output_depth'] = output_depth
        return loss

    step = eager_step
    first_loss = None
    # world > 1: graph segments between the exchange points -- over RCCL (stream-ordered collectives).  gloo (the 1-GPU test mode) blocks
    # the host in every collective and two processes time-slice the device: there the eager step is the faster one, measured
    use_graph = args.graph == 1 and hasattr(model, 'capture_training_step') and (world == 1 or dist.get_backend() == 'nccl')
    # the default: eager launches, weight gradients on the engine's side stream (Engine.wgrad_side), no per-launch events in the timed steps
    fast_eager = args.graph == -1 and bool(getattr(model._engine, 'wgrad_side', False))
    if args.graph == -1 and not fast_eager:   # side stream switched off (RCF_WGRAD_SIDE_STREAM=0): the captured step is the faster one
        use_graph = hasattr(model, 'capture_training_step') and (world == 1 or dist.get_backend() == 'nccl')
    graph_note = None
    n_pre = 0
    for i in range(max(args.warmup, 0)):
        loss = step()
        if i == 0:
            first_loss = float(loss.detach())
    probe = None
    if fast_eager and args.warmup > 0:
        # the eager default only holds while the host enqueues a step faster than the GPU runs it: on a slow or loaded host (or eight
        # ranks' Python threads on one host) fall back to the replayed graph / graph segments (same step, ~1 ms of host time) and say
        # so.  N ranks decide TOGETHER (one all-reduce): a step is a sequence of collectives, every rank must launch it the same way
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        th = time.time()
        loss = step()
        host_probe = time.time() - th
        torch.cuda.synchronize()
        gpu_probe = time.time() - th
        host_bound = host_probe > HOST_BOUND_FRAC * gpu_probe
        can_capture = hasattr(model, 'capture_training_step') and (world == 1 or dist.get_backend() == 'nccl')
        probe = {'host_ms': round(1000 * host_probe, 2), 'step_ms': round(1000 * gpu_probe, 2), 'host_bound': bool(host_bound)}
        if world > 1:
            t = torch.tensor([host_probe, gpu_probe, float(host_bound)], dtype=torch.float64, device=dev)
            gathered = [torch.zeros_like(t) for _ in range(world)]
            dist.all_gather(gathered, t)
            host_bound = any(float(g[2]) > 0 for g in gathered)
            probe = {'host_ms_by_rank': [round(1000 * float(g[0]), 2) for g in gathered],
                     'step_ms_by_rank': [round(1000 * float(g[1]), 2) for g in gathered],
                     'host_bound_by_rank': [bool(float(g[2]) > 0) for g in gathered], 'host_bound': bool(host_bound)}
        if host_bound and can_capture:
            fast_eager, use_graph = False, True
            graph_note = 'host-bound eager step (%.1f of %.1f ms on rank %d%s): %s instead' % (
                1000 * host_probe, 1000 * gpu_probe, rank, '' if world == 1 else '; decided over all ranks',
                'replayed graph' if world == 1 else 'graph segments between the exchange points')
        probe['decision'] = ('graph' if world == 1 else 'graph segments') if use_graph else (
            'eager (host-bound, but %s cannot be captured into segments: host-blocking collectives)' % dist.get_backend() if host_bound else 'eager')
    if use_graph:
        try:
            step = model.capture_training_step(opt, image, input_depth, gt, lidar, outlier_removal=outlier)
            last.clear()
        except Exception as e:   # a box whose runtime cannot capture: measure the eager step and say so
            use_graph, graph_note = False, 'eager launches (hipGraph capture failed: %s)' % str(e)[:120]
    if args.preheat_s > 0:   # untimed: board at its power limit, clocks settled
        restore = _rollback_point(model, opt) if args.dump_outputs else None
        torch.cuda.synchronize()
        t_pre = time.time()
        if world == 1:
            while time.time() - t_pre < args.preheat_s:
                loss = step()
                if first_loss is None:
                    first_loss = float(loss.detach())
                n_pre += 1
                torch.cuda.synchronize()
        else:
            # every rank must run the SAME number of steps (each step is a sequence of collectives): time one, agree on the count
            loss = step()
            if first_loss is None:
                first_loss = float(loss.detach())
            torch.cuda.synchronize()
            n_pre = 1
            n_more = int(min(2000, max(0, int(args.preheat_s / max(time.time() - t_pre, 1e-3)))))
            tn = torch.tensor([n_more], dtype=torch.int64, device=dev)
            dist.all_reduce(tn, op=dist.ReduceOp.MAX)
            for _ in range(int(tn.item())):
                loss = step()
                n_pre += 1
            torch.cuda.synchronize()
        if restore is not None:
            restore()
    timer = ops.KernelTimer()
    if not use_graph and not fast_eager:
        model._engine.prof = timer

    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.time()
    for _ in range(args.steps):
        loss = step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    dt = time.time() - t0
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {'loss': loss.detach().double(), **last, 'parameters': _flat_parameters(model)})
    last.clear()
    # host time of ENQUEUEING one step into an empty queue (untimed, after the timed region; inside the timed loop the host runs ahead
    # until the queue pushes back, so per-step host time there is just the GPU's time): what a step costs the host thread
    host_s = None
    if args.full and (use_graph or fast_eager):   # (--graph 0 runs -- the profiled ones -- keep exactly warm-up + timed steps)
        host_s = 1e9
        slow_backend = world > 1 and dist.get_backend() != 'nccl'   # gloo (1-GPU test mode): every collective goes through the host
        for _ in range(1 if slow_backend else 3):
            torch.cuda.synchronize()
            if world > 1:
                dist.barrier()
            th = time.time()
            loss = step()
            host_s = min(host_s, time.time() - th)
        torch.cuda.synchronize()
    model._engine.prof = None
    my_ms = 1000.0 * dt / args.steps
    final_loss = float(loss.detach())
    if first_loss is None:
        first_loss = final_loss if args.steps == 1 else None
    per_rank_ms = [my_ms]
    dp_info = None
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        gathered = [torch.zeros_like(t) for _ in range(world)]
        dist.all_gather(gathered, t)
        per_rank_ms = [round(1000.0 * float(g.item()) / args.steps, 3) for g in gathered]
        dt = max(float(g.item()) for g in gathered)
    if world > 1 and args.full:
        dp_info = measure_overlap(model, eager_step, dev, 1000.0 * dt / args.steps, reps=1 if dist.get_backend() != 'nccl' else max(1, min(5, args.steps)))
        dp_info['host_ms_per_step'] = None if host_s is None else round(1000.0 * host_s, 3)
        if host_s is not None:
            th_ = torch.tensor([host_s], dtype=torch.float64, device=dev)
            gh = [torch.zeros_like(th_) for _ in range(world)]
            dist.all_gather(gh, th_)
            dp_info['host_ms_per_step_by_rank'] = [round(1000.0 * float(g.item()), 3) for g in gh]
        dp_info['launch_probe'] = probe
        dp_info['launch'] = ('%d hipGraph segments + the RCCL calls between them per step' % len(step.segments)) if (use_graph and getattr(step, 'segments', None)) else ('eager launches, weight gradients and the depth branch on side streams' if fast_eager else 'eager launches')

    table = timer.collect()
    if (args.full or args.kernel_table) and (use_graph or fast_eager):
        # a replayed graph has no per-launch events, and the default's overlapped streams would time every kernel with its neighbour's
        # share of the board power: time the kernel families one at a time, on a few single-stream eager steps after the timed region
        side_was, branch_was = getattr(model._engine, 'wgrad_side', False), getattr(model._engine, 'branch_stream', False)
        model._engine.wgrad_side = model._engine.branch_stream = False
        model._engine.prof = timer
        for _ in range(3):
            eager_step()
        torch.cuda.synchronize()
        model._engine.prof = None
        model._engine.wgrad_side, model._engine.branch_stream = side_was, branch_was
        table = timer.collect()
    # aggregate kernel ids (kind*1000 + ck*10 + nt [+100 for the 16x16 tile]; wgrad ids are 10000 + ...) by kernel family
    fam = {}
    for kid, (cnt, flops, ms) in table.items():
        kid0 = kid % 20000        # + 20000: bf16 variant of the same kernel family, + 40000: two-plane fp16 variant
        f = (10 + (kid0 - 10000) // 1000) if kid0 >= 10000 else kid0 // 1000
        r = fam.setdefault(f, [0, 0.0, 0.0, 0.0])
        r[0] += cnt; r[1] += flops; r[2] += ms; r[3] += getattr(timer, 'bytes', {}).get(kid, 0.0)
    dom = max(fam, key=lambda f: fam[f][2]) if fam else None
    ev_steps = 3 if (use_graph or fast_eager) else args.steps
    arith_table, arith_line = arithmetic_of_step(table, ev_steps)

    side = None
    others = None
    is_default_run = dtype == 'f32' and world == 1 and (args.height, args.width, args.points, batch) == (900, 1600, 64, 8)
    if args.full and is_default_run and not (args.no_side_leg and args.no_other_configs):
        # everything the driver's one command should witness, AFTER the metric's timed region: the headline's model goes first (its
        # activations and the three streams' allocator pools are ~32 GB)
        del step
        model._engine.prof = None
        opt = model = None
        import gc
        gc.collect()
        torch.cuda.empty_cache()
        if not args.no_side_leg:
            try:    # the exact tier: the same step, same seeds, split kernels on three bf16 planes (six exact products per multiply)
                side = train_leg(args, dev, batch, 'f32_3plane', 2 * args.leg_steps)
            except Exception as e:
                side = {'error': str(e)[:200]}
        if not args.no_other_configs:
            others = other_configs(args, dev)
    if rank != 0:
        if world > 1:
            dist.destroy_process_group()
        return 0
    n_samples = world * batch * args.steps
    is_headline = (args.height, args.width, args.points, batch) == (900, 1600, 64, 8)
    rec = {
        'metric': 'FusionNet train samples/sec at 900x1600',
        'value': round(n_samples / dt, 4),
        'unit': 'samples/s',
        'n_gpus': world,
        'steps': args.steps,
        'warmup': args.warmup,
        'ms_per_step': round(1000.0 * dt / args.steps, 3),
        'higher_is_better': True,
        'scaling': 'weak',
        'vs_baseline': None,
        'dtype': dtype,
        'arithmetic_tier': {'f32': 'fp32 tensors; split convolutions on two scaled fp16 planes, 3 products per multiply (RCF_PREC_F16X2: fp32-class error vs fp64, not IEEE fp32 products)', 'f32_3plane': 'fp32 tensors; split convolutions on three bf16 planes, 6 products (exact)', 'bf16': 'bf16 tensors and operands'}[dtype],
        'data': 'synthetic',
        'config': {'workload': 'FusionNet %s training, per-GPU batch %d, %dx%d, %d-point radar maps (BASELINE.json %s)'
                               % ({'f32': 'fp32', 'f32_3plane': 'fp32 (split conv kernels on three bf16 planes)'}.get(
                                   dtype, 'bf16 (bf16 tensors in HBM + bf16 MFMA operands, fp32 accumulate / master weights / BN statistics)'),
                                  batch, args.height, args.width, args.points,
                                  'configs[1]' if dtype in ('f32', 'f32_3plane') else 'configs[3] on %d GPU(s)' % world),
                   'global_batch': world * batch, 'parallelism': 'dp%d' % world,
                   'step': 'forward + outlier removal + masked L1 + backward + Adam, train-mode BatchNorm',
                   'launch': (('one hipGraph replay per step (bitwise the eager step)' if world == 1 else 'hipGraph segments between the exchange points of the data-parallel step (bitwise the eager step)') if use_graph
                              else ('eager launches on three streams: the main chain, the weight gradients, the encoder\'s depth branch (bitwise the single-stream step; --graph 1 replays a hipGraph, whose branches the runtime serialises)' if fast_eager else (graph_note or 'eager launches'))),
                   'launch_note': graph_note if use_graph else None, 'launch_probe': probe,
                   'first_step_loss': None if first_loss is None else round(first_loss, 5), 'final_loss': round(final_loss, 5),
                   'preheat_steps': n_pre},
        'rccl_ranks': dist.get_world_size() if world > 1 else 1,
        'backend': dist.get_backend() if world > 1 else 'none',
        'per_rank_ms_per_step': per_rank_ms,
        'algorithmic_tflops': round(TRAIN_GFLOP_PER_SAMPLE * (args.height * args.width / 1.44e6) * n_samples / dt / 1e3, 2),
    }
    if args.full:
        rec['config'].update({
            'host_enqueue_ms_per_step': None if host_s is None else round(1000.0 * host_s, 3),
            'arithmetic': ('fp32 tensors' if dtype != 'bf16' else 'bf16 tensors') + ', fp32 accumulate, fp64 BatchNorm sums; convolution launches of the '
                          'measured step by the arithmetic they ran on (from their kernel ids): ' + arith_line,
            'arithmetic_by_kernel_class': arith_table})
    if dp_info is not None:
        dp_info['cpu_affinity_rank0'] = affinity
        rec['dp'] = dp_info
    if side is not None:
        rec['exact_tier'] = side
    if others is not None:
        rec['other_configs'] = others
    # the step that is being timed must be the right step: its first loss against the CPU oracle's value for these seeds
    loss_ok = True
    small = (args.height, args.width, args.points, batch) == (224, 384, 32, 2)   # the shape the 2-rank tests run
    if args.full and (is_headline or small) and first_loss is not None:
        want = _expected_first_loss('train_b8_900x1600_p64' if is_headline else 'train_b2_224x384_p32', world)
        if want is not None:
            tol = 3e-2 if dtype == 'bf16' else 1e-3
            relerr = abs(first_loss - want) / abs(want)
            loss_ok = relerr < tol
            rec['config']['loss_check'] = {'oracle_first_step_loss': round(want, 5), 'rel_err': float('%.3e' % relerr), 'tol': tol,
                                           'ok': loss_ok,
                                           'expected': 'CPU oracle, rank-local batch' if world == 1 else
                                           'CPU oracle: global masked mean over the %d ranks\' batches (per-seed sums / counts)' % world}
    if args.full and dom is not None:
        cnt, flops, ms, abytes = fam[dom]
        algorithmic = flops / (ms * 1e-3) / 1e12
        is_split = dom in (5, 6, 8, 9, 15, 19)
        # split kernels are bound by the bf16 matrix pipe: price them on the bf16 FLOPs they execute (6 per fp32 MAC)
        achieved = algorithmic * (SPLIT_PRODUCTS[dtype] if is_split else 1)
        peak = BF16_MFMA_PEAK_TFLOPS if is_split else F32_MFMA_PEAK_TFLOPS   # the guide's dense peak is the same for bf16 and fp16
        kname = KERNEL_NAMES.get(dom, str(dom))
        if dtype == 'f32':
            traffic, traffic_src = _pmc_traffic(kname)
            mfma_busy = _pmc_value(kname, 'mfma_busy_fraction')
        elif dtype == 'bf16':
            fam_key = kname.replace('conv_split_kernel', 'conv_b16_kernel')
            traffic, traffic_src = _pmc_workload('bf16_train', fam_key, 'hbm_bytes_per_launch')
            traffic = None if traffic is None else round(traffic / 1e9, 4)
            mfma_busy = _pmc_workload('bf16_train', fam_key, 'mfma_busy_fraction')[0]
            mfma_busy = None if mfma_busy is None else round(mfma_busy, 4)
        else:   # the committed PMC passes profile the default fp32 step
            traffic, traffic_src = None, 'the committed PMC passes (profiles/) were collected on the default fp32 step'
            mfma_busy = None
        if is_split:
            if dtype == 'bf16':
                kname = kname.replace('conv_split_kernel', 'conv_b16_kernel')   # the bf16-tensor twin of the family (LDS-DMA operands)
            kname += ' (%s)' % TIER_TEXT[dtype]
        conv_ms = sum(r[2] for r in fam.values())
        conv_flops = sum(r[1] for r in fam.values())
        rec['roofline'] = {
            'bound': 'mfma', 'kernel': kname,
            'achieved': round(achieved, 2), 'peak': peak, 'unit': 'TFLOP/s',
            'frac': round(achieved / peak, 4), 'algorithmic_fp32_tflops': round(algorithmic, 2),
            # the honest fraction: useful (algorithmic) FLOP/s over the peak of the pipe the kernel runs on -- `frac` above prices
            # the partial products of the split as work, this one does not
            'useful_frac': round(algorithmic / peak, 4),
            'useful_frac_of_f32_mfma_peak': round(algorithmic / F32_MFMA_PEAK_TFLOPS, 4),
            'frac_of_power_limited_peak': round(achieved / BF16_MFMA_SUSTAINED_TFLOPS, 4) if is_split else None,
            'pipe': SPLIT_PIPE[dtype] if is_split else 'f32 MFMA',
            'products_per_multiply': SPLIT_PRODUCTS[dtype] if is_split else 1,
            'events_from': ('%d single-stream eager steps after the timed region (every kernel timed alone: no per-launch events in a replayed '
                            'graph, and overlapped streams share the board power)' % ev_steps) if (use_graph or fast_eager)
                           else 'HIP events around every launch of the family inside the timed steps',
            'traffic': traffic, 'traffic_source': traffic_src,
            'mfma_busy_pmc': mfma_busy,   # SQ_VALU_MFMA_BUSY_CYCLES / (GRBM_GUI_ACTIVE / 8 XCDs x 1024 SIMDs) of the family, same committed passes
            'algorithmic_gbytes_per_launch': round(abytes / cnt / 1e9, 4),
            'launches_per_step': cnt // ev_steps, 'avg_launch_ms': round(ms / cnt, 4),
            'algorithmic_gflop_per_launch': round(flops / cnt / 1e9, 3),
            'share_of_step_time': round(ms / ev_steps / (1000.0 * dt / args.steps), 4),
            # the subset north_star's ">= 70 % MFMA utilisation" names: the encoder's 3x3 convolutions (ResNet blocks, both branches;
            # forward + input gradient + weight gradient launches), from the same events
            'encoder_3x3': dict(_encoder_3x3(timer, ev_steps, dtype) or {}, mfma_busy_pmc_of_its_kernels=(_pmc_value('kernels of the encoder 3x3 convolutions', 'mfma_busy_fraction') if dtype == 'f32' else None)),
            'weight_gradients': dict(_wgrad_3x3(timer, ev_steps, dtype) or {}, mfma_busy_pmc=(_pmc_value('conv_wgrad_tr_kernel', 'mfma_busy_fraction') if dtype == 'f32' else None)),
            'all_conv_kernels': {'achieved': round(conv_flops / (conv_ms * 1e-3) / 1e12, 2),
                                 'share_of_step_time': round(conv_ms / ev_steps / (1000.0 * dt / args.steps), 4),
                                 'gflop_per_sample': round(conv_flops / (batch * ev_steps) / 1e9, 2)},
        }
    if args.kernel_table:
        rows = [{'kernel_id': kid, 'launches': c, 'gflop': f / 1e9, 'ms': m, 'tflops': f / (m * 1e-3) / 1e12 if m > 0 else 0}
                for kid, (c, f, m) in sorted(table.items())]
        layers = [{'kernel_id': k[0], 'layer': k[1], 'launches': c, 'gflop': f / 1e9, 'ms': m,
                   'tflops': f / (m * 1e-3) / 1e12 if m > 0 else 0} for k, (c, f, m) in sorted(timer.layers.items(), key=lambda kv: -kv[1][2])]
        with open(args.kernel_table, 'w') as fh:
            json.dump({'steps': ev_steps, 'ms_per_step': 1000.0 * dt / args.steps, 'kernels': rows, 'layers': layers}, fh, indent=1)
    if args.full and world == 1 and not args.no_cpu_baseline:
        rec['cpu_baseline'] = cpu_baseline(args.height, args.width, args.points, batch8=args.cpu_baseline_batch8)
    print(json.dumps(rec), flush=True)
    if world > 1:
        dist.destroy_process_group()
    if not loss_ok:
        sys.stderr.write('bench.py: first-step loss %.6f disagrees with the CPU oracle (%s): the timed step is WRONG\n'
                         % (first_loss, rec['config']['loss_check']))
        return 3
    return 0


def _leg_args(args, steps, preheat_s=1.0, warmup=2):
    import copy
    a = copy.copy(args)
    a.steps, a.preheat_s, a.warmup, a.batch, a.dtype = steps, min(args.preheat_s, preheat_s), warmup, 0, None
    a.dump_outputs = ''      # the headline's step wrote the outputs
    return a


def family_roofline(timer, tier, ev_steps, step_ms):
    '''The dominant convolution family of a leg from its KernelTimer events (single-stream eager steps): compact form of the
    headline's `roofline` object -- achieved = executed FLOP/s of the family (algorithmic x partial products), priced on its pipe.'''
    fam = {}
    for kid, (cnt, flops, ms) in timer.collect().items():
        kid0 = kid % 20000
        f = (10 + (kid0 - 10000) // 1000) if kid0 >= 10000 else kid0 // 1000
        r = fam.setdefault(f, [0, 0.0, 0.0])
        r[0] += cnt; r[1] += flops; r[2] += ms
    if not fam:
        return None
    dom = max(fam, key=lambda f: fam[f][2])
    cnt, flops, ms = fam[dom]
    is_split = dom in (5, 6, 8, 9, 15, 19)
    algorithmic = flops / (ms * 1e-3) / 1e12
    achieved = algorithmic * (SPLIT_PRODUCTS[tier] if is_split else 1)
    peak = BF16_MFMA_PEAK_TFLOPS if is_split else F32_MFMA_PEAK_TFLOPS
    kname = KERNEL_NAMES.get(dom, str(dom))
    if is_split and tier == 'bf16':
        kname = kname.replace('conv_split_kernel', 'conv_b16_kernel')
    return {'bound': 'mfma', 'kernel': kname + (' (%s)' % TIER_TEXT[tier] if is_split else ''), 'achieved': round(achieved, 2), 'peak': peak,
            'unit': 'TFLOP/s', 'frac': round(achieved / peak, 4), 'algorithmic_fp32_tflops': round(algorithmic, 2),
            'products_per_multiply': SPLIT_PRODUCTS[tier] if is_split else 1, 'launches_per_step': cnt // ev_steps,
            'avg_launch_ms': round(ms / cnt, 4), 'share_of_step_time': round(ms / ev_steps / step_ms, 4),
            'events_from': '%d single-stream eager steps after the leg\'s timed steps' % ev_steps}


def train_leg(args, dev, batch, dtype, steps):
    '''The FusionNet training step of the metric, same weights and data seeds, under another arithmetic tier -- 'f32_3plane' (three bf16
    planes, six exact products per multiply: the exact fp32 tier) or 'bf16' (BASELINE.json configs[3], one GPU's share) -- reported
    BESIDE the metric, never as `value`.  Its own model, 3 warm-up steps, <= 1 s pre-heat, `steps` timed steps between synchronisations,
    launched like the headline (eager, three streams); the first step's loss is checked against the CPU oracle's recorded value.'''
    import torch
    from rcf_amd import ops, synth, train
    from rcf_amd.net_utils import OutlierRemoval
    model = train.build_model(synth.PUBLISHED, device=dev)
    synth.fill_state_dict_([model.encoder, model.decoder], 1234)
    model.compute_dtype = {'f32_3plane': 'fp32_3plane', 'bf16': 'bf16'}[dtype]
    opt = train.make_optimizer(model, lr=1e-3)
    model.train()
    b = synth.make_batch(batch, args.height, args.width, args.points, seed=1234)
    image, input_depth, gt, lidar = (b[k].to(dev) for k in ('image', 'input_depth', 'ground_truth', 'lidar_map'))
    outlier = OutlierRemoval(kernel_size=7, threshold=1.5)
    step = lambda: train.train_step(model, opt, image, input_depth, gt, lidar, outlier_removal=outlier)[0]
    eager = step
    first_loss = float(step().detach())
    for _ in range(2):
        step()
    # like the headline: eager launches on three streams unless this host cannot enqueue a step as fast as the GPU runs it (a bf16
    # step is ~23 ms of GPU time against 14-18 ms of Python) -- then the replayed graph, and the line says so
    torch.cuda.synchronize()
    th = time.time()
    step()
    host_probe = time.time() - th
    torch.cuda.synchronize()
    gpu_probe = time.time() - th
    launch = 'eager launches on three streams'
    if host_probe > HOST_BOUND_FRAC * gpu_probe and hasattr(model, 'capture_training_step'):
        try:
            step = model.capture_training_step(opt, image, input_depth, gt, lidar, outlier_removal=outlier)
            launch = 'one hipGraph replay per step (host-bound eager step: %.1f of %.1f ms)' % (1000 * host_probe, 1000 * gpu_probe)
        except Exception as e:
            launch += ' (host-bound, hipGraph capture failed: %s)' % str(e)[:80]
    torch.cuda.synchronize()
    t_pre = time.time()
    while time.time() - t_pre < min(args.preheat_s, 1.0):
        step()
        torch.cuda.synchronize()
    torch.cuda.synchronize()
    t0 = time.time()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    dt = time.time() - t0
    step = eager
    timer = ops.KernelTimer()
    eng = model._engine
    side_was, branch_was = eng.wgrad_side, eng.branch_stream
    eng.wgrad_side = eng.branch_stream = False
    eng.prof = timer
    for _ in range(2):
        step()
    torch.cuda.synchronize()
    eng.prof = None
    eng.wgrad_side, eng.branch_stream = side_was, branch_was
    want = _expected_first_loss('train_b8_900x1600_p64')
    tol = 3e-2 if dtype == 'bf16' else 1e-3
    relerr = None if want is None else abs(first_loss - want) / abs(want)
    rec = {'value': round(batch * steps / dt, 4), 'unit': 'samples/s', 'ms_per_step': round(1000.0 * dt / steps, 3), 'steps': steps,
           'dtype': dtype, 'workload': 'FusionNet %s training, batch %d, %dx%d (BASELINE.json %s)' % (
               {'f32_3plane': 'fp32 (split conv kernels on three bf16 planes, six exact products per multiply)', 'bf16': 'bf16'}[dtype],
               batch, args.height, args.width, 'configs[1], exact tier' if dtype == 'f32_3plane' else 'configs[3], one GPU\'s share'),
           'launch': launch,
           'algorithmic_tflops': round(TRAIN_GFLOP_PER_SAMPLE * batch * steps / dt / 1e3, 2),
           'roofline': family_roofline(timer, dtype, 2, 1000.0 * dt / steps),
           'check': {'first_step_loss': round(first_loss, 5), 'oracle_first_step_loss': None if want is None else round(want, 5),
                     'rel_err': None if relerr is None else float('%.3e' % relerr), 'tol': tol, 'ok': None if relerr is None else bool(relerr < tol)}}
    del step, model, opt
    return rec


def other_configs(args, dev):
    '''Short legs of the other BASELINE.json configurations on this one GPU, each with its own model, warm-up, <= 1 s pre-heat and
    `--leg-steps` timed steps / replays, each checked against values the CPU oracle recorded (tests/golden/bench_expected.json).'''
    import gc
    import torch
    out = {}
    legs = (('configs[3] FusionNet bf16 training, per-GPU batch 8', lambda: train_leg(args, dev, 8, 'bf16', args.leg_steps)),
            ('configs[4] FusionNet bf16 inference, batch 32, hipGraph', lambda: _compact(run_infer(_leg_args(args, args.leg_steps), dev, emit=False))),
            ('configs[2] RadarNet bf16 training, 16 images x 4 points', lambda: _compact(run_radarnet(_leg_args(args, args.leg_steps), dev, emit=False))))
    for name, fn in legs:
        try:
            out[name] = fn()
        except Exception as e:
            out[name] = {'error': '%s: %s' % (type(e).__name__, str(e)[:200])}
        gc.collect()
        torch.cuda.empty_cache()
    return out


def _compact(rec):
    r = rec.get('roofline') or {}
    return {'value': rec['value'], 'unit': rec['unit'], 'ms_per_step': rec['ms_per_step'], 'steps': rec['steps'], 'dtype': rec['dtype'],
            'workload': rec['config']['workload'], 'algorithmic_tflops': rec.get('algorithmic_tflops'),
            'roofline': {k: r.get(k) for k in ('bound', 'kernel', 'achieved', 'peak', 'unit', 'frac') if k in r},
            'check': rec['config'].get('check')}


def measure_overlap(model, step, dev, dp_ms, reps=5):
    '''After the timed region (untimed): the gradient buckets all-reduced alone, and the step with the exchange switched off, so
    the exposed communication time and the overlap fraction are numbers and not a design claim.'''
    import torch
    import torch.distributed as dist
    dp = model._dp
    torch.cuda.synchronize()
    dist.barrier()
    t0 = time.time()
    for _ in range(reps):
        hs = [dist.all_reduce(dp.garena[lo:hi], op=dist.ReduceOp.SUM, async_op=True) for lo, hi in dp.bounds]
        for h in hs:
            h.wait()
    torch.cuda.synchronize()
    comm_ms = 1000.0 * (time.time() - t0) / reps
    model._dp = None          # no loss-sum all-reduce, no buckets: the compute of one rank alone
    try:
        step()
        torch.cuda.synchronize()
        dist.barrier()
        t0 = time.time()
        for _ in range(reps):
            step()
        torch.cuda.synchronize()
        alone_ms = 1000.0 * (time.time() - t0) / reps
    finally:
        model._dp = dp
    t = torch.tensor([comm_ms, alone_ms], dtype=torch.float64, device=dev)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    comm_ms, alone_ms = float(t[0]), float(t[1])
    exposed = max(0.0, dp_ms - alone_ms)
    return {'gradient_bytes': int(sum(hi - lo for lo, hi in dp.bounds) * 4), 'buckets': len(dp.bounds),
            'all_reduce_alone_ms': round(comm_ms, 3), 'step_without_exchange_ms': round(alone_ms, 3),
            'exposed_exchange_ms': round(exposed, 3),
            'overlap_frac': round(min(1.0, max(0.0, 1.0 - exposed / comm_ms)), 4) if comm_ms > 0 else None}


# ---------------------------------------------------------------------------------------------------------------- other legs
def _time_steps(fn, args, torch, trained=None):
    '''trained: (model, optimizer) of a training step, whose pre-heat steps --dump-outputs rolls back.'''
    for _ in range(max(args.warmup, 1)):
        out = fn()
    n_pre = 0
    if args.preheat_s > 0:
        restore = _rollback_point(*trained) if (trained and args.dump_outputs) else None
        torch.cuda.synchronize()
        t_pre = time.time()
        while time.time() - t_pre < args.preheat_s:
            out = fn()
            n_pre += 1
            torch.cuda.synchronize()
        if restore is not None:
            restore()
    torch.cuda.synchronize()
    t0 = time.time()
    for _ in range(args.steps):
        out = fn()
    torch.cuda.synchronize()
    return time.time() - t0, out, n_pre


def run_infer(args, dev, emit=True):
    '''BASELINE.json configs[4]: FusionNet inference, batch 32, 900x1600, eval-mode BatchNorm folded into the convolutions, one
    hipGraph replay per batch (FusionNetModel.capture_inference; the reference loop is src/fusionnet_main.py:794-816).'''
    import torch
    from rcf_amd import synth, train
    dtype = args.dtype or 'bf16'
    batch = args.batch or 32
    model = train.build_model(synth.PUBLISHED, device=dev)
    synth.fill_state_dict_([model.encoder, model.decoder], 1234)
    model.compute_dtype = 'bf16' if dtype == 'bf16' else 'fp32'
    model.eval()
    b = synth.make_batch(batch, args.height, args.width, args.points, seed=1234)
    img, dep = b['image'].to(dev), b['input_depth'].to(dev)
    with torch.no_grad():
        use_graph = args.graph != 0
        fwd = model.capture_inference(img, dep, fold_once=True) if use_graph else model.forward
        dt, out, n_pre = _time_steps(lambda: fwd(img, dep), args, torch)
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, {'output_depth': out})
    n_samples = batch * args.steps
    rec = {'metric': 'FusionNet inference samples/sec at 900x1600', 'value': round(n_samples / dt, 3), 'unit': 'samples/s', 'n_gpus': 1,
           'steps': args.steps, 'warmup': args.warmup, 'ms_per_step': round(1000.0 * dt / args.steps, 3), 'higher_is_better': True,
           'scaling': 'weak', 'vs_baseline': None, 'dtype': dtype, 'data': 'synthetic',
           'config': {'workload': 'FusionNet %s inference, batch %d, %dx%d, eval-mode BatchNorm folded, %s (BASELINE.json configs[4])'
                                  % (dtype, batch, args.height, args.width, 'hipGraph-captured, weights folded and packed once before the recording' if use_graph else 'eager'),
                      'global_batch': batch, 'parallelism': 'dp1', 'preheat_steps': n_pre,
                      'output_mean_depth': round(float(out.float().mean()), 4)},
           'algorithmic_tflops': round(FWD_GFLOP_PER_SAMPLE * (args.height * args.width / 1.44e6) * n_samples / dt / 1e3, 2),
           'peak_memory_gb': round(torch.cuda.max_memory_allocated() / 1e9, 2)}
    if args.full:
        # forward minimum traffic: every conv input read once + every conv output written once
        gbytes = (2.80 if dtype == 'f32' else 1.40) * (args.height * args.width / 1.44e6)
        ach = gbytes * n_samples / dt
        traffic, traffic_src = _pmc_workload('bf16_infer' if dtype == 'bf16' else 'f32_infer', 'whole_step', 'hbm_bytes')
        conv_busy = _pmc_workload('bf16_infer' if dtype == 'bf16' else 'f32_infer', 'conv_b16_kernel 3x3 s1', 'mfma_busy_fraction')[0]
        rec['roofline'] = {'bound': 'hbm', 'achieved': round(ach, 1), 'peak': HBM_PEAK_GBS, 'unit': 'GB/s', 'frac': round(ach / HBM_PEAK_GBS, 4),
                           'traffic': None if traffic is None else round(traffic / 1e9, 3), 'traffic_source': traffic_src,
                           'traffic_unit': 'HBM GB per batch, all kernels of one forward (algorithmic: %.1f GB)' % (gbytes * batch),
                           'mfma_busy_pmc_3x3_kernels': None if conv_busy is None else round(conv_busy, 4), 'scope': 'whole forward: algorithmic conv input + output bytes per sample (%.2f GB) x samples / time; '
                                                     'the bf16 layers sit near the MFMA/HBM ridge (SURVEY.md 8d)' % gbytes,
                           'mfma_frac_of_bf16_peak': round(rec['algorithmic_tflops'] / BF16_MFMA_PEAK_TFLOPS, 4)}
        rec['config']['check'] = _infer_check(out, batch, args)
    if emit:
        print(json.dumps(rec), flush=True)
        return 0 if not args.full or rec['config']['check'].get('ok', True) else 3
    return rec


def _infer_check(out, batch, args):
    '''Rows 0 and 31 of the batch against the CPU oracle's eval-mode output of those samples alone (tests/golden/bench_expected.json,
    'infer_b32_900x1600_p64': mean depth and 64 seeded pixels each).  fp32: 1e-3 of the largest depth; bf16: 1.1e-2 (the bar of
    tests/test_configs_gpu.py).'''
    if (batch, args.height, args.width, args.points) != (32, 900, 1600, 64):
        return {'ok': None, 'why': 'recorded for batch 32, 900x1600, 64 points'}
    try:
        exp = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'bench_expected.json')))['infer_b32_900x1600_p64']
    except Exception:
        return {'ok': None, 'why': 'no recorded oracle values'}
    import torch
    idx = torch.tensor(exp['pixel_index'], device=out.device)
    worst, means = 0.0, {}
    for s_, r in exp['samples'].items():
        flat = out[int(s_)].reshape(-1).float()
        got = flat[idx].cpu()
        want = torch.tensor(r['pixels'])
        worst = max(worst, float((got - want).abs().max() / want.abs().max()))
        means[s_] = [round(float(flat.double().mean()), 4), round(r['mean_depth'], 4)]
    tol = 1.1e-2 if (args.dtype or 'bf16') == 'bf16' else 1e-3
    return {'ok': bool(worst < tol), 'max_rel_err_of_128_pixels': float('%.3e' % worst), 'tol': tol, 'mean_depth_got_vs_oracle': means,
            'expected': 'CPU oracle, eval mode, samples 0 and 31 of the batch'}


def run_radarnet(args, dev, emit=True):
    '''BASELINE.json configs[2]: RadarNet stage-1 training (src/radarnet_main.py:320-403), 16 images x 4 radar points = 64 crops of
    900x288 from 900x1888 edge-padded images; one step = forward + masked BCE + backward + Adam.'''
    import torch
    from rcf_amd import radarnet_model, synth
    dtype = args.dtype or 'bf16'
    n_img = args.batch or 16
    k = 4
    m = radarnet_model.RadarNetModel(device=dev, **synth.RADARNET_PUBLISHED)
    m.compute_dtype = 'bf16' if dtype == 'bf16' else 'fp32'
    synth.fill_state_dict_([m.encoder, m.decoder], 41)
    b = synth.make_radarnet_batch(7, n=n_img, k=k, h=args.height, w=args.width + 288, patch_w=288)
    b = {key: (v.to(dev) if isinstance(v, torch.Tensor) else [t.to(dev) for t in v]) for key, v in b.items()}
    opt = torch.optim.Adam([{'params': m.parameters(), 'weight_decay': 0.0}], lr=2e-4)
    m.train()

    last = {}

    def step():
        logits = m.forward(b['image'], b['point'], b['bounding_boxes'])
        loss, _ = m.compute_loss(logits, b['ground_truth'], b['validity_map'], w_positive_class=2.0)
        opt.zero_grad()
        loss.backward()
        opt.step()
        if args.dump_outputs:
            last['logits'] = logits
        return loss
    first_loss = float(step().detach())
    dt, loss, n_pre = _time_steps(step, args, torch, trained=(m, opt))
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, {'loss': loss.detach().double(), **last, 'parameters': _flat_parameters(m)})
    last.clear()
    n_samples = n_img * args.steps
    # the dominant conv family of this step, from HIP events around its launches on three more (untimed) steps
    from rcf_amd import ops
    timer = ops.KernelTimer()
    if args.full:
        m._engine.prof = timer
        side_was, branch_was = getattr(m._engine, 'wgrad_side', False), getattr(m._engine, 'branch_stream', False)
        m._engine.wgrad_side = m._engine.branch_stream = False   # single stream: every kernel timed alone (the timed steps overlap streams)
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        m._engine.prof = None
        m._engine.wgrad_side, m._engine.branch_stream = side_was, branch_was
    fam = {}
    for kid, (cnt, flops, ms) in timer.collect().items():
        kid0 = kid % 20000
        f = (10 + (kid0 - 10000) // 1000) if kid0 >= 10000 else kid0 // 1000
        r = fam.setdefault(f, [0, 0.0, 0.0])
        r[0] += cnt; r[1] += flops; r[2] += ms
    roofline = None
    if fam:
        dom = max(fam, key=lambda f: fam[f][2])
        cnt, flops, ms = fam[dom]
        tier = 'bf16' if dtype == 'bf16' else 'f32'
        is_split = dom in (5, 6, 8, 9, 15, 19)
        algorithmic = flops / (ms * 1e-3) / 1e12
        achieved = algorithmic * (SPLIT_PRODUCTS[tier] if is_split else 1)
        peak = BF16_MFMA_PEAK_TFLOPS if is_split else F32_MFMA_PEAK_TFLOPS
        conv_ms = sum(r[2] for r in fam.values())
        kname = KERNEL_NAMES.get(dom, str(dom))
        if is_split and tier == 'bf16':
            kname = kname.replace('conv_split_kernel', 'conv_b16_kernel')
        roofline = {'bound': 'mfma', 'kernel': kname + (' (%s)' % TIER_TEXT[tier] if is_split else ''),
                    'achieved': round(achieved, 2), 'peak': peak, 'unit': 'TFLOP/s', 'frac': round(achieved / peak, 4),
                    'algorithmic_fp32_tflops': round(algorithmic, 2), 'useful_frac': round(algorithmic / peak, 4),
                    'products_per_multiply': SPLIT_PRODUCTS[tier] if is_split else 1,
                    'traffic': (lambda v: None if v is None else round(v / 1e9, 4))(_pmc_workload('bf16_radarnet', kname, 'hbm_bytes_per_launch')[0]) if tier == 'bf16' else None,
                    'traffic_source': _pmc_workload('bf16_radarnet', kname, 'hbm_bytes_per_launch')[1] if tier == 'bf16' else 'no PMC profile of the fp32 RadarNet step',
                    'mfma_busy_pmc': (lambda v: None if v is None else round(v, 4))(_pmc_workload('bf16_radarnet', kname, 'mfma_busy_fraction')[0]) if tier == 'bf16' else None,
                    'events_from': '3 eager steps after the timed region', 'launches_per_step': cnt // 3,
                    'avg_launch_ms': round(ms / cnt, 4), 'share_of_step_time': round(ms / 3 / (1000.0 * dt / args.steps), 4),
                    'all_conv_kernels_share_of_step_time': round(conv_ms / 3 / (1000.0 * dt / args.steps), 4)}
    rec = {'metric': 'RadarNet stage-1 train images/sec at 900x1600', 'value': round(n_samples / dt, 3), 'unit': 'images/s', 'n_gpus': 1,
           'steps': args.steps, 'warmup': args.warmup, 'ms_per_step': round(1000.0 * dt / args.steps, 3), 'higher_is_better': True,
           'scaling': 'weak', 'vs_baseline': None, 'dtype': dtype, 'data': 'synthetic',
           'config': {'workload': 'RadarNet stage-1 %s training, %d images x %d points (crops 900x288 of 900x%d padded images) '
                                  '(BASELINE.json configs[2])' % (dtype, n_img, k, args.width + 288),
                      'global_batch': n_img, 'parallelism': 'dp1', 'preheat_steps': n_pre, 'final_loss': round(float(loss.detach()), 5),
                      'crops_per_s': round(n_samples * k / dt, 1)},
           # 153.8 GF forward per image at K = 4, x3 for forward + dgrad + wgrad
           'algorithmic_tflops': round(3 * 153.8 * n_samples / dt / 1e3, 2),
           'peak_memory_gb': round(torch.cuda.max_memory_allocated() / 1e9, 2)}
    if roofline is not None:
        rec['roofline'] = roofline
    check = {'ok': None, 'first_step_loss': round(first_loss, 6)}
    if args.full and (n_img, k, args.height, args.width) == (16, 4, 900, 1600):
        try:
            want = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'bench_expected.json')))['radarnet_b16x4_900x1888']['first_step_loss']
            tol = 1e-3      # north_star's fp32 bar; the bf16 loss -- a mean over 1.6e7 pixels -- measures <= 2e-5 (tests/test_configs_gpu.py)
            relerr = abs(first_loss - want) / abs(want)
            check.update({'oracle_first_step_loss': round(want, 6), 'rel_err': float('%.3e' % relerr), 'tol': tol, 'ok': bool(relerr < tol)})
        except Exception:
            check['why'] = 'no recorded oracle value'
    if args.full:
        rec['config']['check'] = check
    if emit:
        print(json.dumps(rec), flush=True)
        return 0 if check.get('ok') is not False else 3
    return rec


def main():
    args = parse()
    if args.gpus < 1:
        raise SystemExit('--gpus must be >= 1')
    if args.steps < 1:
        raise SystemExit('--steps must be >= 1')
    if args.gpus > 1 and 'WORLD_SIZE' not in os.environ:
        return spawn_ranks(args)
    return run_rank(args)


if __name__ == '__main__':
    sys.exit(main())
