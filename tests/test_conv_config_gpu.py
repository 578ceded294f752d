'''
GPU test of every convolution configuration-table entry (tests/conv_config_cases.py, one row per entry) against an fp64 reference
(tests/conv_reference.py): each row runs in every role and variant its entry has --

  - the plain launch, and for a forward layer its BatchNorm-statistics partials (sum and sum of squares of the written values);
  - the same launch accumulating onto a non-zero base (where the descriptor allows it);
  - with a second (concat) source, where that keeps the entry;
  - the inference epilogue (bias, LeakyReLU, residual) where the entry has it;
  - the BatchNorm-backward sums where the entry has them;
  - the weight-gradient rows: rcf_conv2d_wgrad, its phase and phase-pair forms included.

Outputs start as NaN (or the base) and are followed by a band of sentinels that must survive: the split and DMA kernels store
through buffer descriptors, where an out-of-range store lands.  Every element is held to |got - ref| <= tol * bound of its tier
(conv_reference.TOL), where bound is the same operation on |operands|.
'''

import zlib

import numpy as np
import pytest
import torch

import conv_config_cases as ccc
import conv_reference as cref

pytestmark = pytest.mark.gpu

FAM_FWD, FAM_SPLIT, FAM_DMA, FAM_PW, FAM_WG, FAM_WS, FAM_WT = range(7)
GROUPS = sorted(set((c.unit, c.family) for c in ccc.CASES))


@pytest.fixture(scope='module')
def ops():
    import rcf_amd  # noqa: F401
    from rcf_amd import _lib, ops as _ops
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    assert _lib.load().rcf_device_ok() == 1, 'librcf_hip.so: no gfx950 device'
    yield _ops
    _ops.set_precision('fp32')


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    t = torch.rand(*shape, generator=g, dtype=torch.float64)
    return ((t * 2 - 1) * scale).float().double()   # (fp32 values: what the kernels read)


def tier(c, role_fam):
    '''(arithmetic tier, operands rounded to bf16) of the entry a row reaches'''
    if role_fam in (FAM_FWD, FAM_WG):
        return 'f32', False
    if c.prec == 'f16x2' or (role_fam == FAM_PW and c.unit == 'f32'):
        return 'f16x2', False
    if c.prec in ('bf16', 'bf16_operands'):
        return 'bf16', True
    return 'f32', False


def to_dev(t, b16):
    '''NCHW fp64 -> NHWC device tensor of the row's storage'''
    x = t.permute(0, 2, 3, 1).contiguous().float().cuda()
    return x.bfloat16() if b16 else x


def to_host(t):
    return t.detach().float().cpu().permute(0, 3, 1, 2).double()


class Row(object):
    '''one table row: its descriptor, operands and the checks of its launches; worst[check] = largest error ratio seen'''

    def __init__(self, ops, c, worst):
        self.ops, self.c, self.worst = ops, c, worst
        self.b16 = c.unit == 'b16'
        self.seed = zlib.crc32(repr(tuple(c)).encode()) % 100000

    def note(self, name, r):
        self.worst[name] = max(self.worst.get(name, 0.0), r)
        return r

    def desc(self, accumulate=None, c2=None):
        c = self.c if c2 is None else self.c._replace(c2=c2)
        self.ops.set_precision(c.prec)
        return ccc.make_desc(self.ops, c, accumulate)

    def operands(self, d, nslot):
        '''sources (NCHW fp64, storage-rounded) and weights (fp64 OIHW, one per phase slot)'''
        x1 = rnd(d.n, d.c1, d.h_src1, d.w_src1, seed=self.seed)
        x2 = rnd(d.n, d.c2, d.h_in, d.w_in, seed=self.seed + 1) if d.c2 else None
        if self.b16 and d.ksize != 7:   # (the 7x7 stems read the fp32 network input)
            x1, x2 = cref.b16(x1), cref.b16(x2)
        k = d.ksize
        ws = [rnd(d.w_o, d.w_i, k, k, seed=self.seed + 2 + i, scale=1.0 / np.sqrt(d.w_i * k * k)) for i in range(nslot)]
        if d.phase_sum == 3:   # the stride-2 input gradient's phase (a, b) has the taps ty <= a, tx <= b only
            for ph in range(4):
                ws[ph][:, :, (ph >> 1) + 1:, :] = 0
                ws[ph][:, :, :, (ph & 1) + 1:] = 0
        if d.ksize == 4:       # the stem's 4x4 weights come from a 7x7 one (the structural zeros of the space-to-depth form)
            w7 = rnd(d.c_out, 3, 7, 7, seed=self.seed + 2, scale=1.0 / np.sqrt(3 * 49))
            ws = [self.ops.stem_weights_s2d(w7.float().cuda()).cpu().double()]
        return x1, x2, ws

    def expected(self, d, x1, x2, ws, base, fam, scaled):
        '''the reference results of the tier: [(check name, ref, bound)]'''
        t, rounded = tier(self.c, fam)
        bound, _ = cref.forward(d, x1.abs(), None if x2 is None else x2.abs(), [w.abs() for w in ws],
                                None if base is None else base.abs())
        if rounded:
            ref, _ = cref.forward(d, cref.b16(x1), cref.b16(x2), [cref.b16(w) for w in ws], base)
            return [(t, ref, bound)]
        ref, _ = cref.forward(d, x1, x2, ws, base)
        out = [(t, ref, bound)]
        if t == 'f16x2':
            lin = lambda a, b: cref.forward(d, a[0], a[1], b, None if base is None else base * 0)[0]
            sa = cref.scale_of(max(float(x1.abs().max()), 0.0 if x2 is None else float(x2.abs().max()))) if scaled else 1.0
            sb = cref.scale_of(max(float(w.abs().max()) for w in ws)) if scaled else 1.0
            emu = cref.x3(lin, [x1, x2], ws, sa, sb)
            if base is not None:
                emu = emu + base
            out.append(('f16x2_order', emu, bound))
        return out

    def scaled(self, fam):
        return self.c.prec == 'f16x2' and fam in (FAM_SPLIT, FAM_PW, FAM_WS, FAM_WT)

    def check(self, name, got, refs, mask, what):
        for t, ref, bound in refs:
            r = self.note('%s/%s' % (t, name), cref.error_ratio(got, ref, bound, mask, bf16_out=self.b16))
            assert r <= cref.TOL[t], (self.c, what, t, r, cref.TOL[t])

    # ---- the forward form
    def run_fwd(self, d, fam, variant, stats=False, base=None):
        ops = self.ops
        cfg = ops.conv_config(d)
        assert (cfg.family, cfg.index) == (self.c.family, self.c.index), (self.c, variant)
        info = ops.conv_query(d)
        nslot = 4 if d.phase_sum else 1
        x1, x2, ws = self.operands(d, nslot)
        dt = torch.bfloat16 if self.b16 else torch.float32
        oshape = (d.n, d.out_h_phys, d.out_w_phys, d.c_out)
        init = None if base is None else to_dev(base, self.b16)
        out, obuf = cref.guarded(oshape, dt, 'cuda', float('nan') if init is None else init)
        base_h = None if init is None else to_host(init)
        pk = info.packed_weight_floats
        packed = torch.empty(nslot * pk, device='cuda')
        scaled = self.scaled(fam) and variant != 'act'   # (rcf_conv2d_fwd_act takes no scales: unscaled planes)
        amax_w = ops.amax(torch.cat([w.float().flatten() for w in ws]).cuda()) if scaled else None
        for i, w in enumerate(ws):
            ops.conv_pack(d, w.float().cuda(), packed[i * pk:(i + 1) * pk], amax_w)
        g1 = to_dev(x1, self.b16 and d.ksize != 7)
        g2 = None if x2 is None else to_dev(x2, self.b16)
        amax_x = None
        if scaled:
            amax_x = ops.amax(g1)
            if g2 is not None:
                ops.amax(g2, amax_x, accumulate=True)
        sc = ops.make_scales(amax_x, amax_x if g2 is not None else None, amax_w) if scaled else None
        part = pbuf = None
        if stats:
            part, pbuf = cref.guarded((info.n_partials, 2, d.c_out), torch.float64, 'cuda', float('nan'))
        if variant == 'act':
            bias = rnd(d.c_out, seed=self.seed + 9) * 0.5
            res = rnd(d.n, d.c_out, d.out_h_phys, d.out_w_phys, seed=self.seed + 10)
            if self.b16:
                res = cref.b16(res)
            ops.conv_fwd_act(d, g1, g2, packed, bias.float().cuda(), to_dev(res, self.b16), out)
        elif variant == 'bst':
            z = rnd(d.n, d.c_out, d.out_h_phys, d.out_w_phys, seed=self.seed + 11)
            if self.b16:
                z = cref.b16(z)
            g = torch.Generator().manual_seed(self.seed + 12)
            gamma, beta = torch.rand(d.c_out, generator=g) * 2 - 1, torch.rand(d.c_out, generator=g) - 0.5
            mean, invstd = torch.rand(d.c_out, generator=g) - 0.5, 0.5 + 2 * torch.rand(d.c_out, generator=g)
            coef = torch.stack([gamma * invstd, beta - mean * gamma * invstd, mean, invstd]).contiguous()
            part, pbuf = cref.guarded((info.n_partials, 2, d.c_out), torch.float64, 'cuda', float('nan'))
            ops.conv_dgrad_bn_sums(d, g1, packed, out, to_dev(z, self.b16), coef.cuda(), part,
                                   ops.make_scales(amax_x, None, amax_w) if scaled else None)
        else:
            ops.conv_fwd(d, g1, g2, packed, out, part, scales=sc)
        torch.cuda.synchronize()
        assert cref.guard_intact(obuf, out.numel()), (self.c, variant, 'a store past the end of the output')
        got = to_host(out)
        refs = self.expected(d, x1, x2, ws, base_h, fam, scaled)
        mask = cref.written(d)
        init_h = got.new_full(got.shape, float('nan')) if base_h is None else base_h
        assert cref.untouched(got, init_h, mask), (self.c, variant, 'a pixel outside the output phase was written')
        if variant == 'act':
            lrelu = lambda v: torch.where(v > 0, v, 0.2 * v)
            bb = bias.view(1, -1, 1, 1)
            refs = [(t, lrelu(lrelu(ref + bb) + res), bound + bb.abs() + res.abs()) for t, ref, bound in refs]
        self.check(variant, got, refs, mask, variant)
        if stats:
            assert cref.guard_intact(pbuf, part.numel()), (self.c, 'a store past the statistics partials')
            s = part.sum(0).cpu()
            gm = torch.where(mask.expand_as(got), got, torch.zeros_like(got))
            for j, v in enumerate((gm, gm * gm)):
                want, mag = v.sum((0, 2, 3)), v.abs().sum((0, 2, 3))
                r = self.note('stats', float(((s[j] - want).abs() / (mag + 1e-300)).max()))
                assert r < 1e-5, (self.c, 'statistics', j, r)
        if variant == 'bst':
            assert cref.guard_intact(pbuf, part.numel()), (self.c, 'a store past the BatchNorm-backward partials')
            s = part.sum(0).cpu()
            gd = got * torch.where(z * coef[0].double().view(1, -1, 1, 1) + coef[1].double().view(1, -1, 1, 1) > 0, 1.0, 0.2)
            xh = (z - coef[2].double().view(1, -1, 1, 1)) * coef[3].double().view(1, -1, 1, 1)
            for j, v in enumerate((gd, gd * xh)):
                want, mag = v.sum((0, 2, 3)), v.abs().sum((0, 2, 3))
                r = self.note('bn_bwd_sums', float(((s[j] - want).abs() / (mag + 1e-300)).max()))
                assert r < 1e-5, (self.c, 'BatchNorm-backward sums', j, r)

    def forward_roles(self):
        c, ops = self.c, self.ops
        d0 = self.desc(accumulate=False)
        fam = c.family
        self.run_fwd(d0, fam, 'plain', stats=c.form in ccc.FORWARD_FORMS)
        if d0.phase_sum == 3 and fam == FAM_DMA:   # an input gradient takes no statistics: refused, never left zero
            info = ops.conv_query(d0)
            part = torch.empty((info.n_partials, 2, d0.c_out), dtype=torch.float64, device='cuda')
            with pytest.raises(ops._lib.RcfUnsupported):
                ops.conv_fwd(d0, torch.zeros(d0.n, d0.h_src1, d0.w_src1, d0.c1, device='cuda').bfloat16(), None,
                             torch.zeros(4 * info.packed_weight_floats, device='cuda'),
                             torch.empty(d0.n, d0.out_h_phys, d0.out_w_phys, d0.c_out, device='cuda').bfloat16(), part)
        if d0.phase_sum != 2 and d0.ksize != 4:   # (the merged up-2x forward and the stem write, never add)
            d1 = self.desc(accumulate=True)
            self.run_fwd(d1, fam, 'accumulate', base=rnd(d1.n, d1.c_out, d1.out_h_phys, d1.out_w_phys, seed=self.seed + 5))
        if c.form == 'fwd' and c.c2 == 0 and c.k != 7:   # the concat source where the entry takes one
            dc = self.desc(accumulate=False, c2=c.c1)
            try:
                cfg = ops.conv_config(dc)
                same = (cfg.family, cfg.index) == (c.family, c.index)
            except ops._lib.RcfError:
                same = False
            if same:
                self.run_fwd(dc, fam, 'concat')
        info = ops.conv_query(d0)
        cfg = ops.conv_config(d0)
        if cfg.has_epi:
            assert info.fwd_act == 1
            self.run_fwd(d0, fam, 'act')
        if cfg.has_bst and info.bn_bwd_sums:
            self.run_fwd(d0, fam, 'bst')

    # ---- the weight gradient
    def wgrad_roles(self):
        c, ops = self.c, self.ops
        variants = [(self.desc(), 'wgrad')]
        if c.form == 'wgrad' and c.c2 == 0 and c.k != 7:
            dc = self.desc(c2=c.c1)
            try:
                cfg = ops.conv_config(dc, 1)
                if (cfg.family, cfg.index) == (c.family, c.index):
                    variants.append((dc, 'wgrad_concat'))
            except ops._lib.RcfError:
                pass
        for d, name in variants:
            self.run_wgrad(d, name)

    def run_wgrad(self, d, name):
        ops, c = self.ops, self.c
        cfg = ops.conv_config(d, 1)
        assert (cfg.family, cfg.index) == (c.family, c.index), (c, name)
        info = ops.conv_query(d)
        x1, x2, _ = self.operands(d, 1)
        dz = rnd(d.n, d.c_out, d.out_h_phys, d.out_w_phys, seed=self.seed + 3)
        if self.b16:
            dz = cref.b16(dz)
        nslot = 4 if d.phase_sum in (1, 2) else 1
        wshape = (d.c_out, d.c1 + d.c2, d.ksize, d.ksize)
        dshape = (4,) + wshape if nslot == 4 else wshape
        dw, dbuf = cref.guarded(dshape, torch.float32, 'cuda', float('nan'))
        nws = max(1, info.wgrad_workspace_floats)
        wsb, wbuf = cref.guarded((nws,), torch.float32, 'cuda', 0.0, guard=65536)
        g1 = to_dev(x1, self.b16 and d.ksize != 7)
        g2 = None if x2 is None else to_dev(x2, self.b16)
        gz = to_dev(dz, self.b16)
        scaled = self.scaled(c.family)
        sc = None
        if scaled:
            amax_x = ops.amax(g1)
            if g2 is not None:
                ops.amax(g2, amax_x, accumulate=True)
            amax_z = ops.amax(gz)
            sc = ops.make_scales(amax_x, amax_x if g2 is not None else None, None, amax_z)
        ops.conv_wgrad(d, g1, g2, gz, dw, wsb, scales=sc)
        torch.cuda.synchronize()
        assert cref.guard_intact(dbuf, dw.numel()), (c, name, 'a store past the weight gradient')
        assert cref.guard_intact(wbuf, wsb.numel()), (c, name, 'a store past the workspace the query asked for')
        got = dw.cpu().double()
        t, rounded = tier(c, c.family)
        wg = lambda a, b: cref.weight_grad(d, a[0], a[1], b[0], wshape, nslot)
        bound = wg([x1.abs(), None if x2 is None else x2.abs()], [dz.abs()])
        if rounded:
            refs = [(t, wg([cref.b16(x1), cref.b16(x2)], [cref.b16(dz)]), bound)]
        else:
            refs = [(t, wg([x1, x2], [dz]), bound)]
            if t == 'f16x2':
                sa = cref.scale_of(max(float(x1.abs().max()), 0.0 if x2 is None else float(x2.abs().max()))) if scaled else 1.0
                sb = cref.scale_of(float(dz.abs().max())) if scaled else 1.0
                refs.append(('f16x2_order', cref.x3(wg, [x1, x2], [dz], sa, sb), bound))
        for tt, ref, bd in refs:
            r = self.note('%s/%s' % (tt, name), cref.error_ratio(got, ref, bd))
            assert r <= cref.TOL[tt], (c, name, tt, r, cref.TOL[tt])


@pytest.mark.parametrize('unit,family', GROUPS, ids=['%s-%s' % (u, ccc.FAMILY_NAMES[f]) for u, f in GROUPS])
def test_every_config_entry_against_fp64(ops, monkeypatch, unit, family):
    worst = {}
    failures = []
    for c in ccc.CASES:
        if (c.unit, c.family) != (unit, family):
            continue
        for k in ccc.ENV_SWITCHES:
            monkeypatch.delenv(k, raising=False)
        for k, v in c.env:
            monkeypatch.setenv(k, v)
        row = Row(ops, c, worst)
        try:
            if ccc.role_of(c.form):
                row.wgrad_roles()
            else:
                row.forward_roles()
        except AssertionError as e:
            failures.append('%s: %s' % (tuple(c), e))
    print('\nworst error ratios %s-%s: %s' % (unit, ccc.FAMILY_NAMES[family],
                                               ', '.join('%s %.3g' % kv for kv in sorted(worst.items()))))
    assert not failures, '\n'.join(failures[:20])


@pytest.mark.parametrize('form,c1,co', [('fwd', 48, 96), ('fwd', 48, 80), ('dgrad', 96, 48)])
def test_bf16_pointwise_48_input_channels_to_more_than_64(ops, monkeypatch, form, c1, co):
    '''bf16 1x1 from 48 channels to 65-128: the query accepts it, and PwCfg<3, 2> (two workgroups along the output channels, the
    second one partial for 80 / 96) matches the reference.'''
    for k in ccc.ENV_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    c = ccc.Case('b16', FAM_PW, 9, form, 'bf16', 1, 1, c1, 0, co, 2, 13, 17, ())
    worst = {}
    Row(ops, c, worst).forward_roles()
    assert worst
