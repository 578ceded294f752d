'''
Validation loop with the metrics on the host (the reference's block: .cpu().numpy() + eval_utils per sample, src/fusionnet_main.py:
528-548) against the metrics on the device (rcf_amd.evaluation.MetricsAccumulator), and the loop with no evaluation at all as the
floor.  One process, synthetic data, 900 x 1600; the legs alternate over the same inputs, each timed window ends in a synchronise.

    python tools/validate_bench.py [--height 900 --width 1600 --rounds 3 --samples 32 --replays 8]
    rocprofv3 --kernel-trace --stats -d DIR -o eval -- python tools/validate_bench.py --kernels-only

Two configurations: batch 1, eager, compute_dtype 'fp32' (the reference's validation loop) and batch 32, bf16, captured inference
(BASELINE configuration [4]; a window holds --replays replays there, so that it is not one 19 ms event).  Prints samples/s per leg;
the spread of the floor over the windows is the resolution.  --kernels-only enqueues nothing but MetricsAccumulator.update() at
batch 1, 8 and 32 (20 calls each, on make_eval_case inputs) for a kernel trace: eval_partial_kernel / eval_final_kernel against
n * 11.52 MB / 6.3 TB/s.
'''
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rcf_amd  # noqa: E402,F401
from rcf_amd import eval_utils, synth, train  # noqa: E402
from rcf_amd.evaluation import MetricsAccumulator  # noqa: E402


def host_block(output_depth, ground_truth, lo, hi, sink):
    '''the reference's per-sample block, restated'''
    out_all, gt_all = output_depth.cpu().numpy(), ground_truth.cpu().numpy()
    for s in range(out_all.shape[0]):
        o, g = np.squeeze(out_all[s]), np.squeeze(gt_all[s])
        validity_mask = np.where(np.where(g > 0, 1, 0) > 0, 1, 0)
        mask = np.where(np.logical_and(validity_mask, np.logical_and(g > lo, g < hi)) > 0)
        o, g = o[mask], g[mask]
        sink.append((eval_utils.mean_abs_err(1000.0 * o, 1000.0 * g), eval_utils.root_mean_sq_err(1000.0 * o, 1000.0 * g),
                     eval_utils.inv_mean_abs_err(0.001 * o, 0.001 * g), eval_utils.inv_root_mean_sq_err(0.001 * o, 0.001 * g)))


def run_leg(leg, forward, batches, n_batch, lo, hi):
    n_sample = n_batch * len(batches)
    acc = MetricsAccumulator(n_sample, lo, hi, 'cuda', max_batch=n_batch) if leg == 'device' else None
    sink = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.no_grad():
        for b in batches:
            out = forward(b['image'], b['input_depth'])
            if leg == 'host':
                host_block(out, b['ground_truth'], lo, hi, sink)
            elif leg == 'device':
                acc.update(out, b['ground_truth'])
    if leg == 'device':
        sink = acc.means()
    torch.cuda.synchronize()
    return n_sample / (time.perf_counter() - t0), sink


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--height', type=int, default=900)
    ap.add_argument('--width', type=int, default=1600)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--samples', type=int, default=32, help='samples per timed window (at least --replays batches)')
    ap.add_argument('--replays', type=int, default=8, help='batches per timed window of the captured configuration')
    ap.add_argument('--kernels-only', action='store_true')
    a = ap.parse_args()
    lo, hi = 0.0, 100.0
    if a.kernels_only:
        for n in (1, 8, 32):
            out, gt = synth.make_eval_case(5, n, a.height, a.width, 0.30, 2.0)
            o, g = torch.from_numpy(out).cuda(), torch.from_numpy(gt).cuda()
            acc = MetricsAccumulator(20 * n, lo, hi, 'cuda', max_batch=n)
            for _ in range(20):
                acc.update(o, g)
            print('batch %2d: means %s' % (n, ['%.3f' % v for v in acc.means()]), flush=True)
        return
    for name, tier, n_batch, captured in (('batch 1, eager, fp32', 'fp32', 1, False), ('batch 32, captured, bf16', 'bf16', 32, True)):
        model = train.build_model(synth.PUBLISHED, device='cuda')
        synth.fill_state_dict_([model.encoder, model.decoder], 7)
        model.compute_dtype = tier
        model.eval()
        n_item = max(1, a.samples // n_batch, a.replays if captured else 1)
        one = {k: v.cuda() for k, v in synth.make_batch(n_batch, a.height, a.width, 64, seed=11).items()}
        batches = [one] * n_item
        forward = lambda image, input_depth: model.forward(image=image, input_depth=input_depth)   # noqa: E731
        if captured:
            run = model.capture_inference(one['image'], one['input_depth'])
            forward = lambda image, input_depth: run(image, input_depth)   # noqa: E731
        for leg in ('floor', 'device', 'host'):      # warm-up of every leg
            run_leg(leg, forward, batches[:1], n_batch, lo, hi)
        rates = {'floor': [], 'device': [], 'host': []}
        for _ in range(a.rounds):
            for leg in ('floor', 'device', 'host', 'floor'):
                rates[leg].append(run_leg(leg, forward, batches, n_batch, lo, hi)[0])
        for leg in ('floor', 'device', 'host'):
            r = rates[leg]
            print('%-26s %-7s samples/s: median %8.1f  min %8.1f  max %8.1f  (%d windows of %d samples)'
                  % (name, leg, float(np.median(r)), min(r), max(r), len(r), n_batch * n_item), flush=True)
        del model


if __name__ == '__main__':
    main()
