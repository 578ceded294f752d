'''
Fixtures T14: fusion_type 'add', 'weight' and 'concat' (src/networks.py:350-389, :857-870) from the REAL reference, one file per case:
tests/golden/T14_fusion_<type>_<tiny|wide>.npz.  There is no oracle restatement of these types, so the generator asserts what it can:
the state_dict key lists and gradient-less sets it records, and that a second run of the reference (fresh model, same seeds) reproduces
every recorded value exactly.

  tiny: synth.TINY at 2 x 3 x 70 x 102, 8 points (odd sizes at every level), gradients as L2 norms and sums
  wide: synth.PUBLISHED at 1 x 3 x 224 x 384, 32 points (config #1), gradients as L2 norms and sums
  'weight' runs in the reference with five levels and equal branch widths only: synth.WEIGHT_TINY / synth.WEIGHT_WIDE instead

Per file: meta (n, h, w, points, data seed, weight seed), enc_keys / enc_shapes / dec_keys / dec_shapes (state_dict order), n_params,
output (train mode), loss (total, supervised, lidar), grad_keys / grad_l2 / grad_sum, no_grad_keys, buf_keys / buf_l2 (BatchNorm
running statistics after the step) and eval_output (eval mode, fresh weights).
'''
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
from make_golden import import_reference, named_params, one_step   # noqa: E402

CASES = [   # (fusion type, size tag, synth config name, (n, h, w, points), data seed, weight seed)
    ('add', 'tiny', 'TINY', (2, 70, 102, 8), 151, 16),
    ('concat', 'tiny', 'TINY', (2, 70, 102, 8), 152, 17),
    ('weight', 'tiny', 'WEIGHT_TINY', (2, 70, 102, 8), 155, 20),
    ('add', 'wide', 'PUBLISHED', (1, 224, 384, 32), 153, 18),
    ('weight', 'wide', 'WEIGHT_WIDE', (1, 224, 384, 32), 156, 21),
    ('concat', 'wide', 'PUBLISHED', (1, 224, 384, 32), 154, 19),
]


def build(ref_mod, cfg, fusion_type):
    return ref_mod.FusionNetModel(
        input_channels_image=cfg['input_channels_image'], input_channels_depth=cfg['input_channels_depth'],
        encoder_type=['fusionnet18', 'batch_norm'], n_filters_encoder_image=cfg['n_filters_encoder_image'],
        n_filters_encoder_depth=cfg['n_filters_encoder_depth'], fusion_type=fusion_type, decoder_type=['multiscale', 'batch_norm'],
        n_resolution_decoder=1, n_filters_decoder=cfg['n_filters_decoder'], deconv_type='up', activation_func='leaky_relu',
        weight_initializer='kaiming_uniform', min_predict_depth=1.0, max_predict_depth=100.0, device=torch.device('cpu'))


def run_case(ref_mod, synth, fusion_type, cfg, shape, data_seed, weight_seed):
    n, h, w, points = shape
    batch = synth.make_batch(n, h, w, points, seed=data_seed)
    ref = build(ref_mod, cfg, fusion_type)
    synth.fill_state_dict_([ref.encoder, ref.decoder], weight_seed)
    ref.eval()
    with torch.no_grad():
        eval_out = ref.forward(batch['image'], batch['input_depth']).detach().clone()
    out, loss, grads, bufs = one_step(ref, batch, True)
    enc, dec = ref.encoder.state_dict(), ref.decoder.state_dict()
    keys = [k for k, g in grads.items() if g is not None]
    return dict(
        meta=np.array([n, h, w, points, data_seed, weight_seed]),
        enc_keys=np.array(list(enc.keys())), enc_shapes=np.array([str(tuple(v.shape)) for v in enc.values()]),
        dec_keys=np.array(list(dec.keys())), dec_shapes=np.array([str(tuple(v.shape)) for v in dec.values()]),
        n_params=np.array(sum(p.numel() for _, p in named_params(ref))),
        output=out.numpy(), loss=np.array(loss, np.float64), grad_keys=np.array(keys),
        grad_l2=np.array([float(grads[k].double().norm()) for k in keys]),
        grad_sum=np.array([float(grads[k].double().sum()) for k in keys]),
        no_grad_keys=np.array(sorted(k for k, g in grads.items() if g is None)),
        buf_keys=np.array(list(bufs.keys())), buf_l2=np.array([float(b.double().norm()) for b in bufs.values()]),
        eval_output=eval_out.numpy())


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    from rcf_amd import synth
    ref_mod = import_reference()
    for fusion_type, tag, cfg_name, shape, data_seed, weight_seed in CASES:
        cfg = getattr(synth, cfg_name)
        first = run_case(ref_mod, synth, fusion_type, cfg, shape, data_seed, weight_seed)
        again = run_case(ref_mod, synth, fusion_type, cfg, shape, data_seed, weight_seed)
        for k in first:     # the reference reproduces itself exactly: the fixture is a function of the seeds alone
            assert np.array_equal(first[k], again[k]), (fusion_type, tag, k)
        # what the reference constructs per type (src/networks.py:350-389): no fusion parameters for 'concat', projections only for
        # 'add', gates only for 'weight'
        fusion_keys = [k for k in first['enc_keys'] if '_weight.' in k or '_project.' in k]
        if fusion_type == 'concat':
            assert fusion_keys == []
        else:
            own = '_project.' if fusion_type == 'add' else '_weight.'
            assert fusion_keys and all(own in k for k in fusion_keys)
        # the gradient-less parameters are the unused ResNetBlock.projection layers, nothing else
        assert all('.projection.' in k for k in first['no_grad_keys']), first['no_grad_keys']
        name = 'T14_fusion_%s_%s.npz' % (fusion_type, tag)
        np.savez_compressed(os.path.join(HERE, name), **first)
        size = os.path.getsize(os.path.join(HERE, name))
        assert size < 1000000, (name, size)
        print('wrote %s: %d bytes, %d parameters, %d gradient tensors, %d without gradient'
              % (name, size, int(first['n_params']), len(first['grad_keys']), len(first['no_grad_keys'])))


if __name__ == '__main__':
    main()
