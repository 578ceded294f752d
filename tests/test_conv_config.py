'''
CPU tests of the convolution configuration tables (no GPU: rcf_conv2d_query / rcf_conv2d_config only select).

The census: every row of conv_config_cases.CASES reaches exactly the table entry it names, and the rows cover every entry of every
list in both translation units (test_conv_config_gpu.py runs them all against fp64).  The sweep: for every descriptor the query
accepts, the launch's table lookup finds an entry, and the query's fwd_act / bn_bwd_sums are that entry's variants.
'''

import itertools

import numpy as np
import pytest
import torch

import conv_config_cases as ccc
import conv_reference as cref


@pytest.fixture(scope='module')
def ops():
    import __graft_entry__ as entry
    entry.build()
    from rcf_amd import ops as _ops
    yield _ops
    _ops.set_precision('fp32')


@pytest.fixture
def clean_env(monkeypatch):
    for k in ccc.ENV_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def _reach(ops, c, monkeypatch):
    for k in ccc.ENV_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in c.env:
        monkeypatch.setenv(k, v)
    ops.set_precision(c.prec)
    d = ccc.make_desc(ops, c)
    cfg = ops.conv_config(d, ccc.role_of(c.form))
    return d, cfg


def test_census_every_row_reaches_its_entry_and_every_entry_has_one_row(ops, clean_env):
    from rcf_amd import _lib
    seen = {}
    counts = {}
    for c in ccc.CASES:
        assert set(k for k, _ in c.env) <= set(ccc.ENV_SWITCHES), c
        d, cfg = _reach(ops, c, clean_env)
        ops.conv_query(d)   # (the GPU test sizes its buffers from the query)
        assert (cfg.family, cfg.index) == (c.family, c.index), (c, cfg.family, cfg.index)
        assert ccc.unit_of(c.prec) == c.unit, c
        assert (c.unit, c.family, c.index) not in seen, ('two rows for one entry', c, seen.get((c.unit, c.family, c.index)))
        seen[(c.unit, c.family, c.index)] = c
        counts.setdefault((c.unit, c.family), cfg.count)
        assert counts[(c.unit, c.family)] == cfg.count
    fams = {'f32': {_lib.RCF_FAM_FWD, _lib.RCF_FAM_SPLIT, _lib.RCF_FAM_PW, _lib.RCF_FAM_WG, _lib.RCF_FAM_WS, _lib.RCF_FAM_WT},
            'b16': {_lib.RCF_FAM_FWD, _lib.RCF_FAM_SPLIT, _lib.RCF_FAM_DMA, _lib.RCF_FAM_PW, _lib.RCF_FAM_WG, _lib.RCF_FAM_WS,
                    _lib.RCF_FAM_WT}}
    assert set(counts) == set((u, f) for u in fams for f in fams[u]), set(counts) ^ set((u, f) for u in fams for f in fams[u])
    missing = [(u, f, i) for (u, f), n in sorted(counts.items()) for i in range(n)
               if (u, f, i) not in seen and (u, f, i) not in ccc.EXCEPTIONS]
    assert not missing, 'table entries without a row in tests/conv_config_cases.py: %s' % missing
    assert not set(ccc.EXCEPTIONS) & set(seen), 'an exception has a row: drop it from EXCEPTIONS'
    assert sum(counts.values()) == len(seen) + len(ccc.EXCEPTIONS)


def test_census_rows_are_small_enough_for_the_gpu_test():
    for c in ccc.CASES:
        assert c.n * c.h * c.w * (c.c1 + c.c2) * c.co * c.k * c.k < 6e8, c


def _sweep_descs(ops, prec):
    '''(form, descriptor) over kernel sizes, strides, channel counts and small shapes of every form'''
    chans = (4, 12, 16, 40, 48, 64, 128, 200, 256)
    outs = (4, 16, 32, 40, 48, 64, 96, 128, 200, 256)
    shapes = ((1, 9, 13), (2, 7, 23), (3, 5, 41))
    forms = ('fwd', 'dgrad', 'dgrad0', 'pw_s2_dgrad', 'up2x', 'up2x_m', 'up2x_dgrad', 'up2x_dgrad_m', 's2_dgrad', 's2_dgrad_m',
             'stem4', 's2_wgrad', 's2_wgrad_m')
    for form in forms:
        base = 'dgrad' if form == 'dgrad0' else form
        for (k, s), c1, co, (n, h, w) in itertools.product(ccc.FORM_KS[base], chans, outs, shapes):
            if k == 7 and c1 > 4:
                continue
            for c2 in ((0, 16) if form == 'fwd' and k == 3 and s == 1 else (0,)):
                c = ccc.Case(ccc.unit_of(prec), -1, -1, base, prec, k, s, 4 if k == 7 else c1, c2, co, n, h, w, ())
                yield form, ccc.make_desc(ops, c, accumulate=False if form == 'dgrad0' else None)


def _fwd_act_ok(d):
    return d.w_mode == 0 and not d.accumulate


def _bn_sums_ok(d):
    return (d.c2 == 0 and d.out_stride == 1 and d.out_off_y == 0 and d.out_off_x == 0 and d.out_h_phys == d.h_out and
            d.out_w_phys == d.w_out and not d.accumulate)


@pytest.mark.parametrize('prec', ['fp32', 'bf16_operands', 'f16x2', 'bf16'])
def test_query_and_launch_agree_on_every_accepted_descriptor(ops, clean_env, prec):
    '''rcf_conv2d_query never accepts a descriptor whose launch finds no table entry (forward form and weight gradient), and its
    fwd_act / bn_bwd_sums are exactly the variants of the entry the launch runs.'''
    from rcf_amd import _lib
    ops.set_precision(prec)
    n_ok = 0
    for env in ({}, {'RCF_CONV_SPLIT': '0'}, {'RCF_B16_DMA': '0', 'RCF_F32_PW': '0', 'RCF_B16_PW': '0'}):
        for k in ccc.ENV_SWITCHES:
            clean_env.delenv(k, raising=False)
        for k, v in env.items():
            clean_env.setenv(k, v)
        for form, d in _sweep_descs(ops, prec):
            try:
                info = ops.conv_query(d)
            except _lib.RcfError:
                with pytest.raises(_lib.RcfError):
                    ops.conv_config(d)
                continue
            cfg = ops.conv_config(d)   # raises RcfUnsupported when the launch would find no entry
            assert 0 <= cfg.index < cfg.count, (form, cfg.index, cfg.count)
            assert info.fwd_act == int(bool(cfg.has_epi) and _fwd_act_ok(d)), (form, prec, env)
            assert info.bn_bwd_sums == int(bool(cfg.has_bst) and _bn_sums_ok(d)), (form, prec, env)
            if d.w_mode == 0 and d.phase_sum != 3:
                has_wgrad = info.wgrad_kernel_id != 0
                try:
                    w = ops.conv_config(d, _lib.RCF_ROLE_WGRAD)
                    assert has_wgrad and w.family >= _lib.RCF_FAM_WG and 0 <= w.index < w.count, (form, prec, env)
                except _lib.RcfError:
                    assert not has_wgrad, (form, prec, env, info.wgrad_kernel_id)
            n_ok += 1
    assert n_ok > 1000


def test_bf16_pointwise_48_to_65_through_128_channels_selects_an_existing_entry(ops, clean_env):
    '''c1 = 48 (three k-steps of 16) with 65-128 output channels: the pointwise kernel takes two 32-channel tiles per workgroup
    (PwCfg<3, 2>, grid y = 2) as for 64 -> 128; the query used to report nt 3 / 4, which no PwCfg has, and the launch refused.'''
    from rcf_amd import _lib
    ops.set_precision('bf16')
    for co in (68, 80, 96, 128):
        for form in ('fwd', 'dgrad0'):
            if form == 'fwd':
                d = ops.make_fwd_desc(2, 13, 17, 48, 0, co, 1, 1)
            else:
                d = ops.make_dgrad_desc(ops.make_fwd_desc(2, 13, 17, co, 0, 48, 1, 1), 0, co, False)
                if d.c1 != 48:
                    continue
            info = ops.conv_query(d)
            cfg = ops.conv_config(d)
            assert cfg.family == _lib.RCF_FAM_PW and info.kernel_id == 27162, (co, info.kernel_id)


def test_comparison_helpers_reject_subtle_kernel_errors(ops):
    '''The checks test_conv_config_gpu.py applies catch a missing last channel chunk, one element off by 4 ulps, one element left
    NaN and one guard element overwritten.'''
    g = torch.Generator().manual_seed(3)
    d = ccc.make_desc(ops, ccc.Case('f32', 0, 0, 'fwd', 'fp32', 3, 1, 48, 0, 8, 2, 9, 13, ()))
    x = torch.rand(2, 48, 9, 13, generator=g, dtype=torch.float64)   # non-negative operands: |ref| == bound
    w = torch.rand(8, 48, 3, 3, generator=g, dtype=torch.float64) / 20
    ref, mask = cref.forward(d, x, None, [w])
    bound, _ = cref.forward(d, x.abs(), None, [w.abs()])
    tol = cref.TOL['bf16']                          # (the tightest tier: 4 fp32 ulps exceed it where the mantissa is <= 1.5)
    got = ref.float()                               # fp32 rounding of the exact result: passes
    assert cref.error_ratio(got, ref, bound, mask) < tol
    chunk = w.clone()
    chunk[:, 32:] = 0                               # the last 16-channel chunk never added
    miss, _ = cref.forward(d, x, None, [chunk])
    assert cref.error_ratio(miss.float(), ref, bound, mask) > 100 * tol
    off = got.clone()
    m = (ref.abs() / 2.0 ** torch.floor(torch.log2(ref.abs()))) <= 1.5
    idx = tuple(int(i) for i in m.nonzero()[0])
    v = float(off[idx])
    off[idx] = float(np.nextafter(np.nextafter(np.nextafter(np.nextafter(np.float32(v), np.float32(2 * v)), np.float32(2 * v)),
                                                np.float32(2 * v)), np.float32(2 * v)))   # 4 fp32 ulps at one element
    assert cref.error_ratio(off, ref, bound, mask) > tol
    hole = got.clone()
    hole[0, 7, 8, 12] = float('nan')                # one element never written
    assert cref.error_ratio(hole, ref, bound, mask) == float('inf')
    t, buf = cref.guarded((2, 9, 13, 8), torch.float32, 'cpu', float('nan'))
    assert cref.guard_intact(buf, t.numel())
    buf[t.numel() + 17] = 0.0                       # one store past the end
    assert not cref.guard_intact(buf, t.numel())
    # the bf16 output ulp does not hide a relative error of 2^-6
    b = ref.to(torch.bfloat16).double()
    assert cref.error_ratio(b, ref, bound, mask, bf16_out=True) < tol
    b[0, 0, 0, 0] = ref[0, 0, 0, 0] * (1 + 2.0 ** -6)
    assert cref.error_ratio(b, ref, bound, mask, bf16_out=True) > 100 * tol



def test_bf16_stride2_projection_weight_gradient_refuses_a_second_source(ops, clean_env):
    '''The split 1x1 weight gradient re-addresses source 1 at the even positions of a stride-2 projection, not source 2: with a
    concat source it computed a wrong dw (test_conv_config_gpu.py, WsList 1x1 row), so it is refused instead.'''
    from rcf_amd import _lib
    ops.set_precision('bf16')
    d = ops.make_fwd_desc(1, 9, 13, 64, 64, 40, 1, 2)
    assert ops.conv_query(d).wgrad_kernel_id == 0
    with pytest.raises(_lib.RcfUnsupported):
        ops.conv_config(d, _lib.RCF_ROLE_WGRAD)
    d = ops.make_fwd_desc(1, 9, 13, 64, 0, 40, 1, 2)
    assert ops.conv_config(d, _lib.RCF_ROLE_WGRAD).family == _lib.RCF_FAM_WS
