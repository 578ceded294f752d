'''
GPU tests of fusion_type 'add', 'weight' and 'concat' (src/networks.py:350-389, :857-870).
  * the new C-ABI entries against fp64 torch math on the CPU (fp32 and bf16 tensors, accumulate flags, maxima, refusals);
  * FusionNetModel against the T14 fixtures written from the real reference (tests/golden/make_golden_fusion_types.py), under the bars
    that pin 'weight_and_project' (tests/test_hip_model.py: BAR, the gradient-norm bar of the fusionnet34 test, the bf16 bars of
    test_bf16_compute_mode_published_net);
  * the schedules: three streams against one (bitwise), captured inference / training step against eager (bitwise), checkpoint
    round trip, a 2-rank data-parallel step against the single-process emulation of nn.DataParallel.
'''

import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BAR = 1e-3
BF16_EPS = 2.0 ** -8
BN_EPS = 1e-5

CASES = [('add', 'tiny', 'TINY'), ('concat', 'tiny', 'TINY'), ('weight', 'tiny', 'WEIGHT_TINY'),
         ('add', 'wide', 'PUBLISHED'), ('concat', 'wide', 'PUBLISHED'), ('weight', 'wide', 'WEIGHT_WIDE')]
TINY_OF = {'add': 'TINY', 'concat': 'TINY', 'weight': 'WEIGHT_TINY'}
WIDE_OF = {'add': 'PUBLISHED', 'concat': 'PUBLISHED', 'weight': 'WEIGHT_WIDE'}


def _rel(a, b):
    a = torch.as_tensor(a).detach().cpu().double()
    b = torch.as_tensor(b).detach().cpu().double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def _named(model, what):
    out = []
    for prefix, mod in (('encoder.', model.encoder), ('decoder.', model.decoder)):
        it = mod.named_parameters() if what == 'p' else mod.named_buffers()
        out += [(prefix + k, v) for k, v in it if not k.endswith('num_batches_tracked')]
    return out


@pytest.fixture(scope='module')
def env():
    import rcf_amd  # noqa: F401
    from rcf_amd import _lib, synth, train
    assert torch.cuda.is_available()
    _lib.load()
    return synth, train


def _build(env, cfg_name, fusion_type, seed):
    synth, train = env
    m = train.build_model(getattr(synth, cfg_name), device='cuda', fusion_type=fusion_type)
    synth.fill_state_dict_([m.encoder, m.decoder], seed)
    return m


def _gpu_batch(b):
    return {k: v.cuda() for k, v in b.items()}


def _loss(m, b, out):
    return m.compute_loss(image=b['image'], output_depth=out, ground_truth=b['ground_truth'], lidar_map=b['lidar_map'],
                          loss_func='l1', w_smoothness=0.0, loss_smoothness_kernel_size=-1,
                          validity_map_loss_smoothness=None, w_lidar_loss=2.0)


# ---------------------------------------------------------------------------------------------------------------- kernels
def _coef(c, seed):
    '''A BatchNorm coefficient table [4][c] (scale, shift, mean, invstd) as rcf_bn_finalize writes it, fp64 and fp32.'''
    rs = np.random.RandomState(seed)
    mean, var = rs.uniform(-0.5, 0.5, c), rs.uniform(0.5, 1.5, c)
    gamma, beta = rs.uniform(0.5, 1.5, c), rs.uniform(-0.2, 0.2, c)
    invstd = 1.0 / np.sqrt(var + BN_EPS)
    k = torch.from_numpy(np.stack([gamma * invstd, beta - mean * gamma * invstd, mean, invstd]))
    k32 = k.float()
    return k32.double(), k32.cuda()


def _acts(shape, seed, dtype, n):
    '''n random activation tensors in `dtype` on the GPU, and the same values (after rounding to dtype) in fp64 on the CPU.'''
    gen = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        t = torch.randn(shape, generator=gen).to(dtype)
        out.append((t.double(), t.cuda()))
    return out


def _close(got, want, dtype, what):
    '''fp32 tensors: 2e-6 relative to the tensor's scale (a handful of fp32 roundings).  bf16 tensors: one bf16 ulp of the result plus
    the same fp32 term (the arithmetic is fp32 on the loaded values; the store rounds once).'''
    got = got.detach().cpu().double()
    scale = float(want.abs().max()) + 1e-30
    tol = 2e-6 * scale + (BF16_EPS * want.abs() if dtype == torch.bfloat16 else 0.0)
    err = (got - want).abs()
    assert bool((err <= tol).all()), (what, float(err.max()), scale)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('c', [4, 32, 256])
def test_fuse_add_fwd_against_fp64(env, dtype, c):
    from rcf_amd import ops
    n_pix = 3 * 37 * 53      # odd pixel count: the unrolled loop's tail runs
    k64, k = _coef(c, 1)
    (z64, z), (i64, img) = _acts((n_pix, c), 2, dtype, 2)
    want = z64 * k64[0] + k64[1] + i64
    out = torch.empty_like(z)
    ops.fuse_add_fwd(z, k, img, out, n_pix, c)
    _close(out, want, dtype, 'out')
    if dtype == torch.float32:
        am = torch.zeros(1, device='cuda')
        out2 = torch.empty_like(z)
        ops.fuse_add_fwd(z, k, img, out2, n_pix, c, amax=am)
        assert torch.equal(out2, out)
        assert float(am) == float(out.abs().max())


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('c', [8, 64, 256])
def test_fuse_weight_forward_and_backward_against_fp64(env, dtype, c):
    from rcf_amd import ops
    n_pix = 2 * 29 * 51
    k64, k = _coef(c, 3)
    (zw64, zw), (d64, d), (i64, img), (g64, dout), (od64, old_d), (oi64, old_i) = _acts((n_pix, c), 4, dtype, 6)
    sg = torch.sigmoid(zw64 * k64[0] + k64[1])
    out = torch.empty_like(zw)
    ops.fuse_weight_fwd(zw, k, d, img, out, n_pix, c)
    _close(out, sg * d64 + i64, dtype, 'out')
    if dtype == torch.float32:
        am = torch.zeros(1, device='cuda')
        out2 = torch.empty_like(zw)
        ops.fuse_weight_fwd(zw, k, d, img, out2, n_pix, c, amax=am)
        assert torch.equal(out2, out) and float(am) == float(out.abs().max())
    # backward, pass 1: the two BatchNorm sums of gw = dout * d * sig * (1 - sig)
    gw = g64 * d64 * sg * (1 - sg)
    xh = (zw64 - k64[2]) * k64[3]
    nb = ops.ew_blocks(n_pix, c)
    part = torch.empty((nb, 2, c), dtype=torch.float64, device='cuda')
    ops.fuse_weight_bwd_reduce(dout, zw, k, d, part, n_pix, c)
    sums = part.sum(0).cpu()
    scale1 = float(gw.abs().sum(0).max())
    assert float((sums[0] - gw.sum(0)).abs().max()) <= 2e-6 * scale1
    assert float((sums[1] - (gw * xh).sum(0)).abs().max()) <= 2e-6 * float((gw * xh).abs().sum(0).max())
    # pass 2 with the finalized coefficients; written (flags 0), accumulated (flags 1) and skipped (null) outputs
    bcoef = torch.empty((2, c), device='cuda')
    dgamma, dbeta = torch.empty(c, device='cuda'), torch.empty(c, device='cuda')
    ops.bn_bwd_finalize(part, nb, 2 * c, c, n_pix, bcoef, dgamma, dbeta)
    b64 = bcoef.cpu().double()
    want_dz = k64[0] * (gw - b64[0] - xh * b64[1])
    for acc in (False, True):
        dzw, dd, dimg = torch.empty_like(zw), old_d.clone(), old_i.clone()
        ops.fuse_weight_bwd_apply(dout, zw, k, d, bcoef, dzw, dd, acc, dimg, acc, n_pix, c)
        _close(dzw, want_dz, dtype, 'dzw')
        _close(dd, g64 * sg + (od64 if acc else 0.0), dtype, 'dd acc=%d' % acc)
        _close(dimg, g64 + (oi64 if acc else 0.0), dtype, 'dimg acc=%d' % acc)
    dzw2, dd = torch.empty_like(zw), old_d.clone()
    ops.fuse_weight_bwd_apply(dout, zw, k, d, bcoef, dzw2, dd, True, None, False, n_pix, c)     # no image gradient wanted
    assert torch.equal(dzw2, dzw)
    _close(dd, g64 * sg + od64, dtype, 'dd alone')


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('ca,cb', [(16, 32), (32, 64), (64, 128), (128, 256), (256, 128), (4, 8), (256, 256), (12, 20)])
def test_concat_forward_and_backward_are_exact_copies(env, dtype, ca, cb):
    '''The interleave moves values: equality with torch.cat, at the published width pairs (and the reverse order of level 1), at an
    odd pixel count.'''
    from rcf_amd import ops
    shape = (2, 23, 37)
    (_, a), = _acts(shape + (ca,), 5, dtype, 1)
    (_, b), = _acts(shape + (cb,), 6, dtype, 1)
    out = torch.empty(shape + (ca + cb,), dtype=dtype, device='cuda')
    ops.concat_fwd(a, b, out)
    assert torch.equal(out, torch.cat([a, b], -1))
    (_, dout), (_, _unused) = _acts(shape + (ca + cb,), 7, dtype, 2)
    da, db = torch.empty_like(a), torch.empty_like(b)
    ops.concat_bwd(dout, da, False, db, False, ca, cb)
    assert torch.equal(da, dout[..., :ca]) and torch.equal(db, dout[..., ca:])
    # accumulate into one branch while the other is written; then each branch from a launch of its own
    da2, db2 = a.clone(), torch.empty_like(b)
    ops.concat_bwd(dout, da2, True, db2, False, ca, cb)
    assert torch.equal(da2, (a.float() + dout[..., :ca].float()).to(dtype)) and torch.equal(db2, db)
    da3, db3 = torch.empty_like(a), b.clone()
    ops.concat_bwd(dout, da3, False, None, False, ca, cb)
    ops.concat_bwd(dout, None, False, db3, True, ca, cb)
    assert torch.equal(da3, da) and torch.equal(db3, (b.float() + dout[..., ca:].float()).to(dtype))
    if dtype == torch.float32:
        ama, amb, amo = ops.amax(a), ops.amax(b), torch.zeros(1, device='cuda')
        out2 = torch.empty_like(out)
        ops.concat_fwd(a, b, out2, amax=(ama, amb, amo))
        assert torch.equal(out2, out) and float(amo) == float(out.abs().max())


def test_new_entries_refuse_what_they_do_not_cover(env):
    from rcf_amd import _lib, ops
    z = torch.zeros((5, 12), device='cuda')
    k = torch.zeros((4, 12), device='cuda')
    with pytest.raises(_lib.RcfUnsupported):
        ops.fuse_add_fwd(z, k, z, torch.empty_like(z), 5, 12)              # 12 / 4 is not a power of two
    with pytest.raises(_lib.RcfUnsupported):
        ops.fuse_weight_fwd(z, k, z, z, torch.empty_like(z), 5, 12)
    with pytest.raises(_lib.RcfUnsupported):
        ops.concat_fwd(z, torch.zeros((5, 6), device='cuda'), torch.empty((5, 18), device='cuda'))   # 6: not a multiple of 4
    with pytest.raises(_lib.RcfError):
        ops.concat_bwd(torch.zeros((5, 12), device='cuda'), None, False, None, False, 4, 8)      # RCF_EINVAL: nothing to write
    with pytest.raises(ValueError):
        ops.concat_fwd(torch.zeros((5, 4), device='cuda'), torch.zeros((6, 8), device='cuda'), torch.empty((5, 12), device='cuda'))
    with pytest.raises(_lib.RcfError):
        ops.fuse_add_fwd(z.bfloat16(), k, z, torch.empty_like(z), 5, 12)   # activation tensors disagree in dtype


def _b16(t):
    return t.bfloat16().float()


def _rnd(*shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


@pytest.mark.parametrize('c_d,c_i,n,h,w', [(16, 32, 2, 37, 53), (32, 64, 2, 19, 23), (64, 128, 1, 31, 17), (128, 256, 2, 8, 13), (16, 24, 1, 9, 11),
                                           (64, 70, 1, 5, 7)])
def test_add_inference_fusion_in_one_pass(env, c_d, c_i, n, h, w):
    '''rcf_fuse_add_infer_b16 = BN(W d) + img with eval-mode BatchNorm (src/networks.py:857-859), under the two bounds
    tests/test_hip_bf16.py::test_inference_fusion_in_one_pass uses for the 'weight_and_project' form: (a) fp64 on the same bf16-rounded
    operands (the scaled weights rounded to bf16 as the kernel's B operand is): one bf16 ulp of the result plus 2e-5 (1 + |y|);
    (b) the two-step arrangement it replaces (a 1x1 convolution that rounds z to bf16, then rcf_fuse_add_fwd_b16): 3 BF16_EPS in
    relative L2.  Ragged pixel counts and channel counts off the 32-channel tile.'''
    from rcf_amd import ops
    d = _b16(_rnd(n, h, w, c_d, seed=1, scale=2.0))
    img = _b16(_rnd(n, h, w, c_i, seed=2))
    wt = _rnd(c_i, c_d, 1, 1, seed=4, scale=(1.0 / c_d) ** 0.5)
    cp = torch.stack([_rnd(c_i, seed=9) * 0.5 + 1.0, _rnd(c_i, seed=10) * 0.3, _rnd(c_i, seed=11) * 0.1, _rnd(c_i, seed=12) * 0.2 + 1.0])
    assert ops.fuse_wp_infer_supported(c_d, c_i)
    out = torch.full((n, h, w, c_i), float('nan'), device='cuda').bfloat16()
    ops.fuse_add_infer(d.cuda().bfloat16(), wt.cuda(), cp.cuda(), img.cuda().bfloat16(), out)
    torch.cuda.synchronize()
    got = out.float().cpu()
    assert torch.isfinite(got).all()
    ws = _b16(wt.view(c_i, c_d) * cp[0][:, None]).double()
    yp = d.double().view(-1, c_d) @ ws.t() + cp[1].double()
    want = (yp + img.double().view(-1, c_i)).view(n, h, w, c_i)
    err = (got.double() - want).abs()
    bound = BF16_EPS * want.abs() + 2e-5 * (1.0 + yp.abs().view(n, h, w, c_i))
    print('add one pass %d -> %d: worst error / bound %.3f' % (c_d, c_i, float((err / bound).max())))
    assert (err <= bound).all(), float((err - bound).max())
    if c_i % 32 == 0:   # (b) the arrangement it replaces (its kernels take whole channel tiles)
        ops.set_precision('bf16')
        try:
            desc = ops.make_fwd_desc(n, h, w, c_d, 0, c_i, 1, 1, h, w, 0)
            info = ops.conv_query(desc)
            packed = torch.empty(info.packed_weight_floats, device='cuda')
            ops.conv_pack(desc, wt.cuda(), packed)
            z = torch.empty((n, h, w, c_i), device='cuda').bfloat16()
            ops.conv_fwd(desc, d.cuda().bfloat16(), None, packed, z, None)
            old = torch.empty_like(out)
            ops.fuse_add_fwd(z, cp.cuda(), img.cuda().bfloat16(), old, n * h * w, c_i)
            torch.cuda.synchronize()
        finally:
            ops.set_precision('fp32')
        rel = float((old.float() - out.float()).norm() / out.float().norm())
        print('add one pass %d -> %d: relative L2 against the two-step path %.2e' % (c_d, c_i, rel))
        assert rel < 3 * BF16_EPS, rel


def test_add_inference_fusion_refuses_what_it_does_not_cover(env):
    from rcf_amd import _lib, ops
    d = torch.zeros((1, 4, 4, 48), device='cuda').bfloat16()
    img = torch.zeros((1, 4, 4, 96), device='cuda').bfloat16()
    coef = torch.zeros((4, 96), device='cuda')
    wt = torch.zeros((96, 48, 1, 1), device='cuda')
    with pytest.raises(_lib.RcfUnsupported):
        ops.fuse_add_infer(d, wt, coef, img, torch.empty_like(img))          # c_d = 48: no tiling
    with pytest.raises(ValueError):
        ops.fuse_add_infer(d.float(), wt, coef, img, torch.empty_like(img))
    with pytest.raises(ValueError):
        ops.fuse_add_infer(d, wt[:, :16], coef, img, torch.empty_like(img))


def test_add_inference_takes_the_one_pass_form_on_bf16_tensors(env):
    '''bf16 eval forward of the published net: the one-pass fusion is really taken (bits differ from the general path with the switch
    off) and agrees with it within the bf16 bar the inference tests use between two arrangements of the same arithmetic.'''
    synth, _ = env
    m = _build(env, 'PUBLISHED', 'add', 5)
    m.compute_dtype = 'bf16'
    m.eval()
    b = _gpu_batch(synth.make_batch(1, 224, 384, 32, seed=71))
    outs = {}
    with torch.no_grad():
        for one_pass in (True, False):
            m._engine.fuse_wp_one_pass = one_pass
            outs[one_pass] = m.forward(image=b['image'], input_depth=b['input_depth']).clone()
    torch.cuda.synchronize()
    assert not torch.equal(outs[True], outs[False])
    assert _rel(outs[True], outs[False]) < 6e-2


# ---------------------------------------------------------------------------------------------------------------- the model
@pytest.mark.parametrize('tier', ['fp32', 'fp32_3plane'])
@pytest.mark.parametrize('fusion_type,tag,cfg_name', CASES)
def test_training_step_and_eval_against_the_reference_fixture(env, golden_dir, fusion_type, tag, cfg_name, tier):
    synth, _ = env
    g = np.load(os.path.join(golden_dir, 'T14_fusion_%s_%s.npz' % (fusion_type, tag)))
    n, h, w, k, dseed, wseed = [int(v) for v in g['meta']]
    b = _gpu_batch(synth.make_batch(n, h, w, k, seed=dseed))
    m = _build(env, cfg_name, fusion_type, wseed)
    m.compute_dtype = tier
    assert sum(p.numel() for p in m.parameters()) == int(g['n_params'])
    m.eval()
    with torch.no_grad():
        e_eval = _rel(m.forward(image=b['image'], input_depth=b['input_depth']), g['eval_output'])
    m.train()
    out = m.forward(image=b['image'], input_depth=b['input_depth'])
    loss, info = _loss(m, b, out)
    loss.backward()
    torch.cuda.synchronize()
    e_out = _rel(out, g['output'])
    got_loss = [float(loss), float(info['loss_supervised']), float(info['loss_lidar'])]
    grads = {kk: p.grad for kk, p in _named(m, 'p') if p.grad is not None}
    e_grad = max(abs(float(grads[key].double().norm()) - l2) / (l2 + 1e-30) for key, l2 in zip(g['grad_keys'].tolist(), g['grad_l2'].tolist())
                 if key in grads)
    print('%s %s %s: eval %.2e  output %.2e  loss %s / %s  worst gradient norm %.2e' % (fusion_type, tag, tier, e_eval, e_out, got_loss,
                                                                                     g['loss'].tolist(), e_grad))
    assert e_eval < BAR
    assert e_out < BAR
    np.testing.assert_allclose(got_loss, g['loss'], rtol=BAR)
    assert sorted(grads) == sorted(g['grad_keys'].tolist())
    for key, l2 in zip(g['grad_keys'].tolist(), g['grad_l2'].tolist()):
        assert abs(float(grads[key].double().norm()) - l2) <= 1e-2 * l2 + 1e-9, key
    # BatchNorm running statistics after the step: linear in the batch statistics the output already depends on
    bufs = dict(_named(m, 'b'))
    for key, l2 in zip(g['buf_keys'].tolist(), g['buf_l2'].tolist()):
        assert abs(float(bufs[key].double().norm()) - l2) <= BAR * l2 + 1e-9, key


@pytest.mark.parametrize('fusion_type', ['add', 'concat', 'weight'])
def test_bf16_compute_mode_at_published_widths(env, golden_dir, fusion_type):
    '''The bars of test_bf16_compute_mode_published_net (tests/test_hip_model.py), on the published-width fixtures.'''
    synth, _ = env
    g = np.load(os.path.join(golden_dir, 'T14_fusion_%s_wide.npz' % fusion_type))
    n, h, w, k, dseed, wseed = [int(v) for v in g['meta']]
    b = _gpu_batch(synth.make_batch(n, h, w, k, seed=dseed))
    outs = {}
    for mode in ('fp32', 'bf16'):
        m = _build(env, WIDE_OF[fusion_type], fusion_type, wseed)
        m.compute_dtype = mode
        m.train()
        out = m.forward(image=b['image'], input_depth=b['input_depth'])
        loss, info = _loss(m, b, out)
        loss.backward()
        torch.cuda.synchronize()
        outs[mode] = (out.detach(), float(loss.detach()), m)
    e16 = _rel(outs['bf16'][0], g['output'])
    grads = dict(_named(outs['bf16'][2], 'p'))
    bad = [key for key, l2 in zip(g['grad_keys'].tolist(), g['grad_l2'].tolist())
           if abs(float(grads[key].grad.double().norm()) - l2) > 0.25 * l2 + 1e-9]
    print('%s bf16: output %.2e vs reference, %.2e vs the fp32 tier; loss %.5f / ref %.5f; %d of %d gradient norms beyond 25 %% (allowed %d): %s'
          % (fusion_type, e16, _rel(outs['bf16'][0], outs['fp32'][0]), outs['bf16'][1], float(g['loss'][0]), len(bad), len(g['grad_keys']),
             len(g['grad_keys']) // 20, bad))
    assert e16 < 6e-2
    assert _rel(outs['bf16'][0], outs['fp32'][0]) > 1e-4       # the mode is really in use
    assert abs(outs['bf16'][1] - float(g['loss'][0])) < 2e-2 * abs(float(g['loss'][0]))
    assert len(bad) <= len(g['grad_keys']) // 20, bad


@pytest.mark.parametrize('fusion_type', ['add', 'concat', 'weight'])
def test_three_stream_step_is_bitwise_the_single_stream_step(env, fusion_type):
    '''The default schedule (weight gradients on a side stream, the depth branch and the fusions on another) against one stream, at
    published widths, batch 2, 900 x 1600 (races only show where kernels run long): output, loss and every parameter over 3 steps.'''
    synth, train = env
    b = _gpu_batch(synth.make_batch(2, 900, 1600, 64, seed=2025))
    runs = []
    for single in (True, False):
        m = _build(env, WIDE_OF[fusion_type], fusion_type, 11)
        eng = m._engine
        if single:
            eng.wgrad_side = eng.branch_stream = False
        else:
            assert eng.wgrad_side and eng.branch_stream and eng.fuse_on_branch, 'the three-stream schedule is the default'
        opt = train.make_optimizer(m, lr=1e-3)
        m.train()
        trace = []
        for _ in range(3):
            loss, _, out = train.train_step(m, opt, b['image'], b['input_depth'], b['ground_truth'], b['lidar_map'])
            torch.cuda.synchronize()
            trace.append((out.detach().clone(), float(loss), m._param_arena.detach().clone()))
        runs.append(trace)
        del m, opt
    for step, ((o1, l1, p1), (o3, l3, p3)) in enumerate(zip(*runs)):
        assert l1 == l3, (step, l1, l3)
        assert torch.equal(o1, o3), step
        assert torch.equal(p1, p3), step


@pytest.mark.parametrize('tier', ['fp32', 'bf16'])
@pytest.mark.parametrize('fusion_type', ['add', 'concat', 'weight'])
def test_captured_inference_is_bitwise_the_eager_eval_forward(env, fusion_type, tier):
    synth, _ = env
    m = _build(env, WIDE_OF[fusion_type], fusion_type, 5)
    m.compute_dtype = tier
    m.eval()
    b = _gpu_batch(synth.make_batch(1, 224, 384, 32, seed=71))
    b2 = _gpu_batch(synth.make_batch(1, 224, 384, 32, seed=72))
    run = m.capture_inference(b['image'], b['input_depth'])
    with torch.no_grad():
        for bb in (b, b2, b):
            got = run(bb['image'], bb['input_depth']).clone()
            ref = m.forward(image=bb['image'], input_depth=bb['input_depth'])
            torch.cuda.synchronize()
            assert torch.equal(got, ref)


@pytest.mark.parametrize('fusion_type', ['add', 'concat', 'weight'])
def test_captured_training_step_is_bitwise_the_eager_step(env, fusion_type):
    synth, train = env
    batches = [_gpu_batch(synth.make_batch(2, 70, 102, 8, seed=300 + i)) for i in range(2)]
    runs = {}
    for mode in ('eager', 'graph'):
        m = _build(env, TINY_OF[fusion_type], fusion_type, 9)
        opt = train.make_optimizer(m, lr=1e-3)
        m.train()
        before = m._param_arena.clone()
        if mode == 'graph':
            b0 = batches[0]
            step = m.capture_training_step(opt, b0['image'], b0['input_depth'], b0['ground_truth'], b0['lidar_map'])
            assert torch.equal(m._param_arena, before), 'capturing changed the parameters'
        losses = []
        for b in batches:
            if mode == 'graph':
                loss = step(b['image'], b['input_depth'], b['ground_truth'], b['lidar_map'])
            else:
                loss = train.train_step(m, opt, b['image'], b['input_depth'], b['ground_truth'], b['lidar_map'])[0]
            losses.append(float(loss.detach()))
        torch.cuda.synchronize()
        runs[mode] = (losses, m._param_arena.clone(),
                      torch.cat([t.reshape(-1).float() for mod in (m.encoder, m.decoder) for t in mod.buffers()]))
    assert runs['eager'][0] == runs['graph'][0], (runs['eager'][0], runs['graph'][0])
    assert torch.equal(runs['eager'][1], runs['graph'][1]) and torch.equal(runs['eager'][2], runs['graph'][2])


@pytest.mark.parametrize('fusion_type', ['add', 'concat', 'weight'])
def test_checkpoint_round_trip(env, tmp_path, fusion_type):
    synth, train = env
    m = _build(env, TINY_OF[fusion_type], fusion_type, 3)
    opt = train.make_optimizer(m, lr=1e-3)
    b = _gpu_batch(synth.make_batch(1, 64, 96, 4, seed=1))
    m.train()
    train.train_step(m, opt, b['image'], b['input_depth'], b['ground_truth'], b['lidar_map'])
    m.data_parallel()      # the reference always calls it before saving (src/fusionnet_main.py:198)
    path = str(tmp_path / 'model-1.pth')
    m.save_model(path, 1, opt)
    ck = torch.load(path, map_location='cpu')
    assert all(k.startswith('module.') for k in ck['encoder_state_dict'])
    assert [k[len('module.'):] for k in ck['encoder_state_dict']] == list(m.encoder.state_dict().keys())
    m2 = train.build_model(getattr(synth, TINY_OF[fusion_type]), device='cuda', fusion_type=fusion_type)
    step, _ = m2.restore_model(path, train.make_optimizer(m2, lr=1e-3))
    assert step == 1
    m.eval(); m2.eval()
    with torch.no_grad():
        assert torch.equal(m.forward(b['image'], b['input_depth']), m2.forward(b['image'], b['input_depth']))
    if fusion_type != 'weight':      # a checkpoint of another type does not load: the state_dict keys differ
        other = train.build_model(getattr(synth, TINY_OF[fusion_type]), device='cuda', fusion_type='weight_and_project')
        with pytest.raises(RuntimeError):
            other.restore_model(path)


# ---------------------------------------------------------------------------------------------------------------- data parallel
def _dp_worker(rank, world, port, tmpdir, fusion_type, cfg_name):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)   # gloo moves CUDA tensors; both ranks share cuda:0
    import rcf_amd  # noqa: F401
    from rcf_amd import synth, train
    torch.manual_seed(7)
    m = train.build_model(getattr(synth, cfg_name), device='cuda', fusion_type=fusion_type)
    synth.fill_state_dict_([m.encoder, m.decoder], 31)
    m.data_parallel()
    assert m._dp is not None
    opt = train.make_optimizer(m, lr=1e-3)
    b = {k: v.cuda() for k, v in synth.make_batch(2, 64, 96, 6, seed=500 + rank).items()}
    m.train()
    out = m.forward(b['image'], b['input_depth'])
    loss, info = m.compute_loss(b['image'], out, b['ground_truth'], b['lidar_map'], 'l1', 0.0, -1, None, 2.0)
    opt.zero_grad(); loss.backward()
    g = m._grad_arena[:m._n_used].clone()
    opt.step()
    torch.cuda.synchronize()
    torch.save({'loss': float(loss), 'grad': g.cpu(), 'param': m._param_arena.detach().cpu().clone()}, os.path.join(tmpdir, 'dp%d.pt' % rank))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)   # a rank that never joins must not hold the suite
@pytest.mark.parametrize('fusion_type', ['add', 'weight'])
def test_data_parallel_step_two_ranks_on_one_gpu(env, tmp_path, fusion_type):
    '''As tests/test_hip_model.py::test_data_parallel_step_two_ranks_on_one_gpu asserts it: loss and gradient arena bitwise equal on
    both ranks; against a single-process emulation of nn.DataParallel (per-replica BatchNorm statistics, ONE masked mean over the
    gathered batch, summed gradients) the loss within 1e-5 and the gradient arena within 1e-4.  A gradient reported final
    (_wgrad_done) before its last kernel is enqueued shows up here.'''
    import torch.multiprocessing as mp
    synth, train = env
    cfg_name = TINY_OF[fusion_type]
    port = 29700 + (os.getpid() % 1000)
    mp.spawn(_dp_worker, args=(2, port, str(tmp_path), fusion_type, cfg_name), nprocs=2, join=True)
    r = [torch.load(os.path.join(str(tmp_path), 'dp%d.pt' % k)) for k in range(2)]
    assert r[0]['loss'] == r[1]['loss']
    assert torch.equal(r[0]['grad'], r[1]['grad']) and torch.equal(r[0]['param'], r[1]['param'])

    from rcf_amd import ops
    batches = [_gpu_batch(synth.make_batch(2, 64, 96, 6, seed=500 + k)) for k in range(2)]
    m = _build(env, cfg_name, fusion_type, 31)
    m.train()
    sums = []
    for b in batches:
        with torch.no_grad():
            out = m.forward(b['image'], b['input_depth'])
        s = torch.empty(4, dtype=torch.float64, device='cuda')
        ops.l1_loss_fwd(out.contiguous(), b['ground_truth'], b['lidar_map'], s)
        sums.append(s)
    m = _build(env, cfg_name, fusion_type, 31)      # (undoes the running-statistics updates of the two probing forwards)
    m.train()
    tot = sums[0] + sums[1]
    want_loss = float(tot[0] / tot[1] + 2.0 * tot[2] / tot[3])
    grad = torch.zeros(m._n_used, device='cuda')
    for b in batches:
        out = m.forward(b['image'], b['input_depth'])
        dd = torch.empty_like(out)
        ops.l1_loss_bwd(out.detach().contiguous(), b['ground_truth'], b['lidar_map'], tot, None, 2.0, dd)
        for p in m.parameters():
            p.grad = None
        out.backward(dd)
        grad += m._grad_arena[:m._n_used]
    print('%s: loss %.8f / emulation %.8f, gradient arena %.2e' % (fusion_type, r[0]['loss'], want_loss, _rel(r[0]['grad'], grad)))
    assert abs(r[0]['loss'] - want_loss) < 1e-5 * abs(want_loss)
    assert _rel(r[0]['grad'], grad) < 1e-4
