'''The elementwise kernels of the 'add', 'weight' and 'concat' fusions next to those of 'weight_and_project', at the shapes of the
published net's six levels for a batch of 8 at 900 x 1600: kernel time from a trace against the bytes each kernel must move (every
tensor it reads or writes, once), as a share of the HBM peak.

  rocprofv3 --kernel-trace --stats -d DIR -o fk -- python tools/fusion_kernels_profile.py run        (a run of its own)
  python tools/fusion_kernels_profile.py report DIR [out.md]                                          (reads the rocpd .db)

The 'weight' fusion needs equal branch widths, so its rows use the image branch's widths for both; 'concat' uses (image, depth).
'''
import collections
import glob
import os
import re
import sqlite3
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12        # bytes/s, the MI355X's HBM3E specification
BATCH, H, W = 8, 900, 1600
WIDTHS = [(32, 16), (64, 32), (128, 64), (256, 128), (256, 128), (256, 128)]      # (image, depth) per level: synth.PUBLISHED
REPS = 5


def levels():
    '''(pixels, image width, depth width) of each level's fused tensor: the stem halves the size, then max-pool, then three stride-2
    levels (src/networks.py:853-1003 at padding k // 2).'''
    h, w = (H + 1) // 2, (W + 1) // 2
    out = [(BATCH * h * w, ) + WIDTHS[0]]
    h, w = (h + 1) // 2, (w + 1) // 2
    out.append((BATCH * h * w, ) + WIDTHS[1])
    for ci, cd in WIDTHS[2:]:
        h, w = (h + 1) // 2, (w + 1) // 2
        out.append((BATCH * h * w, ci, cd))
    return out


def plan(elem=4):
    '''{kernel name fragment: (tensors moved per element of width c, as a function of the level)} -> bytes per pass over all levels.
    Each entry: tensors read + written once, in elements.'''
    rows = collections.OrderedDict()
    for n_pix, ci, cd in levels():
        t = n_pix * ci
        for name, elems in (
                ('fuse_fwd_kernel', 4 * t),                    # zw, zp, img -> out
                ('fuse_bwd_reduce_kernel', 3 * t),             # dout, zw, zp
                ('fuse_bwd_apply_kernel', 7 * t),              # dout, zw, zp, dimg (read) -> dzw, dzp, dimg
                ('fuse_add_fwd_kernel', 3 * t),                # z, img -> out
                ('fuse_weight_fwd_kernel', 4 * t),             # zw, d, img -> out
                ('fuse_weight_bwd_reduce_kernel', 3 * t),      # dout, zw, d
                ('fuse_weight_bwd_apply_kernel', 8 * t),       # dout, zw, d, dd, dimg (read) -> dzw, dd, dimg
                ('concat_kernel forward', 2 * n_pix * (ci + cd)),  # a, b -> out
                ('concat_kernel backward', 3 * n_pix * (ci + cd))):  # dout, da, db (read) -> da, db
            rows[name] = rows.get(name, 0) + elems * elem
    return rows


def run():
    import torch
    import rcf_amd  # noqa: F401
    from rcf_amd import ops
    dev = 'cuda'
    for n_pix, ci, cd in levels():
        def t(c):
            return torch.randn((n_pix, c), device=dev)
        coef = torch.rand((4, ci), device=dev) + 0.5
        bcoef = torch.zeros((2, ci), device=dev)
        zw, zp, img, d, dout, out, dzw, dzp, dimg, dd = [t(ci) for _ in range(10)]
        a, b, cat, dcat, da, db = t(ci), t(cd), t(ci + cd), t(ci + cd), t(ci), t(cd)
        nb = ops.ew_blocks(n_pix, ci)
        part4 = torch.empty((nb, 4, ci), dtype=torch.float64, device=dev)
        part2 = torch.empty((nb, 2, ci), dtype=torch.float64, device=dev)
        for _ in range(REPS + 1):      # (the first pass of a shape is in the trace too: REPS + 1 calls per kernel and level)
            ops.fuse_fwd(zw, coef, zp, coef, img, out, n_pix, ci)
            ops.fuse_bwd_reduce(dout, zw, coef, zp, coef, part4, n_pix, ci)
            ops.fuse_bwd_apply(dout, zw, coef, zp, coef, bcoef, bcoef, dzw, dzp, dimg, True, n_pix, ci)
            ops.fuse_add_fwd(zp, coef, img, out, n_pix, ci)
            ops.fuse_weight_fwd(zw, coef, d, img, out, n_pix, ci)
            ops.fuse_weight_bwd_reduce(dout, zw, coef, d, part2, n_pix, ci)
            ops.fuse_weight_bwd_apply(dout, zw, coef, d, bcoef, dzw, dd, True, dimg, True, n_pix, ci)
            ops.concat_fwd(a, b, cat)
            ops.concat_bwd(dcat, da, True, db, True, ci, cd)
        torch.cuda.synchronize()
    print('fusion_kernels_profile: %d passes over %d levels' % (REPS + 1, len(levels())))


def report(trace_dir, out_path=None):
    db = trace_dir if trace_dir.endswith('.db') else sorted(glob.glob(os.path.join(trace_dir, '**', '*.db'), recursive=True))[0]
    cur = sqlite3.connect(db).cursor()
    agg = collections.defaultdict(lambda: [0, 0.0])
    for name, s, e in cur.execute('select name, start, end from kernels order by start'):
        m = re.search(r'(fuse_\w+_kernel|concat_kernel)<([^>]*)>', name)
        if m:
            key = m.group(1) if m.group(1) != 'concat_kernel' else 'concat_kernel ' + ('forward' if 'true' in m.group(2) else 'backward')
            agg[key][0] += 1
            agg[key][1] += (e - s) * 1e-9
    lines = ['| kernel | launches | bytes per pass over the six levels (MB) | time per pass (us) | TB/s | share of the 8 TB/s HBM peak |',
             '|---|---|---|---|---|---|']
    n_lvl = len(levels())
    for name, nbytes in plan().items():
        calls, sec = agg.get(name, (0, 0.0))
        if not calls:
            lines.append('| `%s` | 0 | %.0f | not measured | - | - |' % (name, nbytes / 1e6))
            continue
        per_pass = sec / (calls / float(n_lvl))
        lines.append('| `%s` | %d | %.0f | %.1f | %.2f | %.0f %% |' % (name, calls, nbytes / 1e6, per_pass * 1e6, nbytes / per_pass / 1e12,
                                                                    100.0 * nbytes / per_pass / HBM_PEAK))
    text = '\n'.join(lines) + '\n'
    if out_path:
        with open(out_path, 'w') as f:
            f.write(text)
    print(text)


if __name__ == '__main__':
    if len(sys.argv) >= 3 and sys.argv[1] == 'report':
        report(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else None)
    elif len(sys.argv) == 2 and sys.argv[1] == 'run':
        run()
    else:
        sys.exit(__doc__)
