'''Training step time of the published FusionNet under each fusion type, in one process, alternating the types so that they share the
machine's state: fp32, batch 8, 900 x 1600 by default (the benchmark's shape; bench.py itself keeps measuring 'weight_and_project').

  python tools/fusion_types_bench.py [--types weight_and_project add concat] [--reps 3] [--steps 10] [--warmup 3] [--out FILE.md]

Each repetition times `steps` eager training steps (forward, loss, backward, Adam) per type with a host clock around work that ends in a
device synchronise.  Prints one line per (type, repetition) and a table with the median and the spread (max - min) per type.
'''
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--types', nargs='+', default=['weight_and_project', 'add', 'concat'])
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--height', type=int, default=900)
    ap.add_argument('--width', type=int, default=1600)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--dtype', default='fp32')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    import torch
    import rcf_amd  # noqa: F401
    from rcf_amd import synth, train
    if not torch.cuda.is_available():
        sys.exit('fusion_types_bench needs a GPU: a CPU run cannot give a time')
    b = {k: v.cuda() for k, v in synth.make_batch(args.batch, args.height, args.width, 64, seed=1234).items()}
    models = {}
    for t in args.types:
        m = train.build_model(synth.PUBLISHED, device='cuda', **({} if t == 'weight_and_project' else {'fusion_type': t}))
        synth.fill_state_dict_([m.encoder, m.decoder], 7)
        m.compute_dtype = args.dtype
        m.train()
        models[t] = (m, train.make_optimizer(m, lr=1e-3))

    def steps(t, n):
        m, opt = models[t]
        for _ in range(n):
            train.train_step(m, opt, b['image'], b['input_depth'], b['ground_truth'], b['lidar_map'])
        torch.cuda.synchronize()

    for t in args.types:
        steps(t, args.warmup)
    times = {t: [] for t in args.types}
    for rep in range(args.reps):
        for t in args.types:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            steps(t, args.steps)
            ms = (time.perf_counter() - t0) * 1e3 / args.steps
            times[t].append(ms)
            print('rep %d  %-20s %.2f ms/step' % (rep, t, ms), flush=True)
    lines = ['| fusion_type | ms / step (median of %d x %d steps) | min | max | spread |' % (args.reps, args.steps), '|---|---|---|---|---|']
    for t in args.types:
        v = sorted(times[t])
        lines.append('| `%s` | %.2f | %.2f | %.2f | %.2f |' % (t, v[len(v) // 2], v[0], v[-1], v[-1] - v[0]))
    text = ('%s training, batch %d, %d x %d, eager steps, types alternating within each repetition\n\n' % (args.dtype, args.batch, args.height, args.width)
            + '\n'.join(lines) + '\n')
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
