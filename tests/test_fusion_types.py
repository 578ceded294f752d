'''
CPU tests (no GPU) of the host mirror for fusion_type 'add', 'weight' and 'concat' (src/networks.py:350-389, :857-870) against the
T14 fixtures written from the real reference (tests/golden/make_golden_fusion_types.py): state_dict keys and shapes, parameter count,
arena coverage, which parameters the forward never uses -- and the reference's envelopes (what it cannot run raises ValueError here).
'''

import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

CASES = [('add', 'tiny', 'TINY'), ('concat', 'tiny', 'TINY'), ('weight', 'tiny', 'WEIGHT_TINY'),
         ('add', 'wide', 'PUBLISHED'), ('concat', 'wide', 'PUBLISHED'), ('weight', 'wide', 'WEIGHT_WIDE')]


@pytest.fixture(scope='module')
def pkg():
    import __graft_entry__ as entry
    entry.build()
    import rcf_amd
    return rcf_amd


def _named(model):
    return [(prefix + k, p) for prefix, mod in (('encoder.', model.encoder), ('decoder.', model.decoder))
            for k, p in mod.named_parameters()]


@pytest.mark.parametrize('fusion_type,tag,cfg_name', CASES)
def test_host_mirror_matches_the_reference_fixture(pkg, fusion_type, tag, cfg_name):
    from rcf_amd import synth, train
    g = np.load(os.path.join(GOLDEN, 'T14_fusion_%s_%s.npz' % (fusion_type, tag)))
    m = train.build_model(getattr(synth, cfg_name), device='cpu', fusion_type=fusion_type)
    assert m.encoder.fusion_type == fusion_type
    for mod, keys, shapes in ((m.encoder, g['enc_keys'], g['enc_shapes']), (m.decoder, g['dec_keys'], g['dec_shapes'])):
        sd = mod.state_dict()
        assert list(sd.keys()) == keys.tolist()
        assert [str(tuple(v.shape)) for v in sd.values()] == shapes.tolist()
    assert sum(p.numel() for p in m.parameters()) == int(g['n_params'])
    # the arenas cover every parameter exactly once; the used ones come first, in the order their gradients become final
    params = m.parameters()
    spans = sorted((m._param_offset[id(p)], p.numel()) for p in params)
    end = 0
    for off, n in spans:
        assert off == end
        end += n
    assert end == m._param_arena.numel() == m._grad_arena.numel() == int(g['n_params'])
    assert len(set(id(p) for p in m._used_params)) == len(m._used_params)
    assert sum(p.numel() for p in m._used_params) == m._n_used
    assert m._used_params[0] is m.decoder.output0.conv.weight
    assert m._used_params[-1] is m.encoder.conv1_image.conv.weight
    # the parameters the forward never touches are the ones the reference leaves without a gradient
    used = set(id(p) for p in m._used_params)
    assert sorted(k for k, p in _named(m) if id(p) not in used) == g['no_grad_keys'].tolist()
    assert sorted(k for k, p in _named(m) if id(p) in used) == sorted(g['grad_keys'].tolist())


def test_fusion_modules_exist_as_in_the_reference(pkg):
    '''Which convL_weight / convL_project attributes exist, are modules or are None (src/networks.py:350-389, :681-714, :742-765).'''
    from rcf_amd import synth, train
    add = train.build_model(synth.TINY, device='cpu', fusion_type='add').encoder
    for lvl in range(1, 7):
        assert getattr(add, 'conv%d_project' % lvl).conv.weight.shape[2:] == (1, 1)
        assert not hasattr(add, 'conv%d_weight' % lvl)
    assert add.conv7_project is None and add.conv7_weight is None and add.blocks7_image is None
    assert add.conv2_project.activation_func is None and add.conv2_project.use_batch_norm
    cat = train.build_model(synth.TINY, device='cpu', fusion_type='concat').encoder
    assert not any('_weight.' in k or '_project.' in k for k in cat.state_dict())
    assert cat.conv7_project is None and not hasattr(cat, 'conv1_project')
    wgt = train.build_model(synth.WEIGHT_TINY, device='cpu', fusion_type='weight').encoder
    for lvl, c in zip(range(1, 6), synth.WEIGHT_TINY['n_filters_encoder_depth']):
        assert tuple(getattr(wgt, 'conv%d_weight' % lvl).conv.weight.shape) == (c, c, 3, 3)
        assert not hasattr(wgt, 'conv%d_project' % lvl)
    assert wgt.conv6_weight is None and wgt.conv7_weight is None
    # 'concat' widens the decoder: skips and latent carry both branches' channels (src/fusionnet_model.py:75-77, :117-119)
    dec = train.build_model(synth.PUBLISHED, device='cpu', fusion_type='concat').decoder
    assert tuple(dec.deconv5.deconv.conv.conv.weight.shape) == (256, 384, 3, 3)
    assert tuple(dec.deconv5.conv.conv.weight.shape) == (256, 256 + 384, 3, 3)
    assert tuple(dec.deconv1.conv.conv.weight.shape) == (64, 64 + 48, 3, 3)


def test_what_the_reference_cannot_run_raises(pkg):
    from rcf_amd import synth, train
    six = dict(synth.WEIGHT_TINY, n_filters_encoder_image=[8, 16, 32, 32, 32, 32], n_filters_encoder_depth=[8, 16, 32, 32, 32, 32],
               n_filters_decoder=[32, 32, 16, 8, 8, 4])
    with pytest.raises(ValueError, match=r'conv6_weight.*networks\.py:681'):         # AttributeError in the reference's forward (:970)
        train.build_model(six, device='cpu', fusion_type='weight')
    with pytest.raises(ValueError, match=r'equal.*networks\.py:862'):                # the broadcast fails in the reference
        train.build_model(dict(synth.WEIGHT_TINY, n_filters_encoder_depth=[4, 8, 16, 16, 16]), device='cpu', fusion_type='weight')
    seven = dict(synth.TINY, n_filters_encoder_image=[8, 16, 32, 32, 32, 32, 32], n_filters_encoder_depth=[4, 8, 16, 16, 16, 16, 16],
                 n_filters_decoder=[32, 32, 32, 16, 8, 8, 4])
    with pytest.raises(ValueError, match=r'conv7_project.*networks\.py:742'):        # AttributeError in the reference's forward (:989)
        train.build_model(seven, device='cpu', fusion_type='add')
    train.build_model(seven, device='cpu', fusion_type='concat')                     # 'concat' runs with five to seven levels
    train.build_model(seven, device='cpu', fusion_type='weight_and_project')
    five = dict(synth.TINY, n_filters_encoder_image=[8, 16, 32, 32, 32], n_filters_encoder_depth=[4, 8, 16, 16, 16],
                n_filters_decoder=[32, 16, 8, 8, 4])
    train.build_model(five, device='cpu', fusion_type='add')
    with pytest.raises(ValueError):
        train.build_model(synth.TINY, device='cpu', fusion_type='bogus')


def test_weight_and_project_builds_what_it_built_before(pkg):
    from rcf_amd import synth, train
    from oracle.fusionnet_oracle import FusionNetOracle
    m = train.build_model(synth.PUBLISHED, device='cpu')
    assert m.encoder.fusion_type == 'weight_and_project'
    o = FusionNetOracle(**synth.PUBLISHED)
    assert list(m.encoder.state_dict().keys()) == list(o.encoder.state_dict().keys())
    assert list(m.decoder.state_dict().keys()) == list(o.decoder.state_dict().keys())
    assert sum(p.numel() for p in m.parameters()) == 14413568 and m._n_used == 14142208
    assert [tuple(p.shape) for p in m._used_params] == [tuple(p.shape) for p in
                                                        train.build_model(synth.PUBLISHED, device='cpu',
                                                                          fusion_type='weight_and_project')._used_params]


def test_new_entries_refuse_bad_arguments_before_any_launch(pkg):
    '''Null pointers / zero extents answer RCF_EINVAL, widths the kernels do not index answer RCF_EUNSUPPORTED: no HIP call is made.'''
    import ctypes
    from rcf_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p).value
    for sfx in ('', '_b16'):
        assert getattr(lib, 'rcf_fuse_add_fwd' + sfx)(None, p, p, p, 4, 8, None) == -1
        assert getattr(lib, 'rcf_fuse_add_fwd' + sfx)(p, p, p, p, 0, 8, None) == -1
        assert getattr(lib, 'rcf_fuse_add_fwd' + sfx)(p, p, p, p, 4, 12, None) == -2
        assert getattr(lib, 'rcf_fuse_weight_fwd' + sfx)(p, p, None, p, p, 4, 8, None) == -1
        assert getattr(lib, 'rcf_fuse_weight_fwd' + sfx)(p, p, p, p, p, 4, 6, None) == -2
        assert getattr(lib, 'rcf_fuse_weight_bwd_reduce' + sfx)(p, p, p, p, None, 4, 8, None) == -1
        assert getattr(lib, 'rcf_fuse_weight_bwd_reduce' + sfx)(p, p, p, p, p, 4, 24, None) == -2
        assert getattr(lib, 'rcf_fuse_weight_bwd_apply' + sfx)(p, p, p, p, p, None, p, 0, p, 0, 4, 8, None) == -1
        assert getattr(lib, 'rcf_fuse_weight_bwd_apply' + sfx)(p, p, p, p, p, p, p, 0, p, 0, 4, 2, None) == -2
        assert getattr(lib, 'rcf_concat_fwd' + sfx)(p, None, p, 4, 4, 8, None, None, None, None) == -1
        assert getattr(lib, 'rcf_concat_fwd' + sfx)(p, p, p, 4, 4, 8, None, None, p, None) == -1      # amax_out without the sources'
        assert getattr(lib, 'rcf_concat_fwd' + sfx)(p, p, p, 4, 16, 6, None, None, None, None) == -2       # not a multiple of 4
        assert getattr(lib, 'rcf_concat_bwd' + sfx)(p, None, 0, None, 0, 4, 4, 8, None) == -1          # nothing to write
        assert getattr(lib, 'rcf_concat_bwd' + sfx)(p, p, 0, p, 0, 4, 48, 18, None) == -2
    assert lib.rcf_fuse_add_fwd_amax(p, p, p, p, 4, 8, None, None) == -1
    assert lib.rcf_fuse_add_infer_b16(p, p, None, p, p, 4, 16, 32, None) == -1
    assert lib.rcf_fuse_add_infer_b16(p, p, p, p, p, 4, 48, 96, None) == -2      # the widths of rcf_fuse_wp_infer_supported only
    assert lib.rcf_fuse_add_infer_b16(p, p, p, p, p, 4, 16, 31, None) == -2
    assert lib.rcf_fuse_weight_fwd_amax(p, p, p, p, p, 4, 8, None, None) == -1
