'''
Every BASELINE.json configuration at ITS OWN workload, through the C ABI, against the CPU oracle:

  configs[1]  FusionNet fp32 training, batch 8, 900x1600      test_config1_*
  configs[2]  RadarNet stage-1 bf16 training, 900x288 patches  test_config2_*
  configs[3]  FusionNet bf16 training at 900x1600              test_config3_*   (one GPU's share of the 8-GPU job; the exchange is
                                                                                 covered by the 2-rank tests)
  configs[4]  FusionNet bf16 inference, batch 32, hipGraph     test_config4_*

plus the launcher of bench.py on real ranks.  The oracle is run at the full resolution, forward only where a backward at that
size would take minutes on the host; the backward at full batch is checked through an exact property of the domain instead:
with eval-mode BatchNorm every sample is independent, so the batch-8 gradient is the sum of the eight batch-1 gradients and the
batch-8 output rows are the batch-1 outputs (the batch-1 path is pinned to the oracle in tests/test_hip_model.py).

Bars: 1e-3 relative for fp32 (north_star).  bf16 (bf16 tensors in HBM, bf16 MFMA operands, fp32 accumulate) has no bar in
north_star; the bars below are 1.3 x what round 3 measured (the kernels are deterministic and the seeds fixed) and are printed
next to the measured error.
'''

import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-3
# bf16 bars = 1.3 x the value measured in round 3 (deterministic kernels, fixed seeds), printed next to the measurement:
BF16_OUT_BAR = 3.6e-2      # FusionNet training output depth, max |d - d_ref| / max |d_ref|   (measured 2.3e-2 / 2.74e-2)
BF16_INFER_BAR = 1.1e-2    # eval-mode (running statistics) output                            (measured 8.2e-3)
BF16_LOGIT_BAR = 5.3e-2    # RadarNet logits                                                  (measured 4.08e-2)
BF16_LOSS_BAR = 3e-5       # losses are means over ~1e5..1e7 pixels                           (measured 7.5e-7 .. 1.8e-5)
BF16_COS_BAR = 0.9988      # gradient cosine against the fp32 HIP gradient                    (measured 0.9991)
BF16_DEEP_COS_BAR = 0.805  # headline step, sampled elements of one of the ten deepest weight gradients vs fp64 (measured 0.850 [r6])
BF16_POOLED_COS_BAR = 0.843  # the same pooled over the ten tensors                            (measured 0.8792 [r6])
BF16_NORM_BAR = 0.058      # headline step, L2 norm of a convolution weight gradient vs fp64            (measured 4.4e-2 [r6])
BF16_BN_NORM_BAR = 0.24    # ... of a BatchNorm weight / bias gradient (sums of nearly cancelling terms; measured 1.8e-1 [r6])
_ORACLE_CACHE = {}


def _rel(a, b):
    a = torch.as_tensor(a).detach().cpu().double()
    b = torch.as_tensor(b).detach().cpu().double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


@pytest.fixture(scope='module')
def env():
    import rcf_amd  # noqa: F401
    from rcf_amd import _lib, synth, train
    assert torch.cuda.is_available()
    _lib.load()
    return synth, train


def _build(env, seed, dtype='fp32'):
    synth, train = env
    m = train.build_model(synth.PUBLISHED, device='cuda')
    synth.fill_state_dict_([m.encoder, m.decoder], seed)
    m.compute_dtype = dtype
    return m


def _oracle(env, seed):
    from oracle.fusionnet_oracle import FusionNetOracle
    synth, _ = env
    o = FusionNetOracle(**synth.PUBLISHED)
    synth.fill_state_dict_([o.encoder, o.decoder], seed)
    return o


def _loss(m, b, out):
    return m.compute_loss(image=b['image'], output_depth=out, ground_truth=b['ground_truth'], lidar_map=b['lidar_map'],
                          loss_func='l1', w_smoothness=0.0, loss_smoothness_kernel_size=-1,
                          validity_map_loss_smoothness=None, w_lidar_loss=2.0)


# ------------------------------------------------------------------------------------------------------------ configs[1]
def test_config1_fp32_batch8_900x1600_train_forward_and_loss_against_oracle(env):
    '''The workload bench.py times (batch 8, 900x1600, train-mode BatchNorm over the batch): output of samples 0 and 7 and the loss
    against the CPU oracle run on the same batch of 8, then backward + Adam for finite, non-trivial updates.'''
    synth, train = env
    cb = synth.make_batch(8, 900, 1600, 64, seed=1234)
    m = _build(env, 1234)
    opt = train.make_optimizer(m, lr=1e-3)
    b = {k: v.cuda() for k, v in cb.items()}
    m.train()
    out = m.forward(image=b['image'], input_depth=b['input_depth'])
    loss, _ = _loss(m, b, out)
    p_before = m._param_arena.clone()
    opt.zero_grad()
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    g = m._grad_arena[:m._n_used]
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    assert float((m._param_arena - p_before).abs().max()) > 0
    o = _oracle(env, 1234)
    o.train()
    t0 = time.time()
    with torch.no_grad():
        ref = o.forward(cb['image'], cb['input_depth'])
        ref_loss = float(o.compute_loss(ref, cb['ground_truth'], cb['lidar_map'], 2.0)[0])
    e0, e7 = _rel(out[0], ref[0]), _rel(out[7], ref[7])
    mae_mm = float((out.detach().cpu() - ref).abs().mean()) * 1000.0
    print('batch-8 900x1600 fp32: out rel %.2e / %.2e (samples 0 / 7), MAE %.4f mm, loss %.6f vs oracle %.6f (oracle forward %.0f s)'
          % (e0, e7, mae_mm, float(loss), ref_loss, time.time() - t0))
    assert e0 < BAR and e7 < BAR
    assert abs(float(loss) - ref_loss) < BAR * abs(ref_loss)
    # bench.py's recorded first-step loss (tests/golden/bench_expected.json) is this step with the ground-truth outlier removal in front
    rec = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'bench_expected.json')))['train_b8_900x1600_p64']
    from rcf_amd.net_utils import OutlierRemoval
    m2 = _build(env, 1234)
    m2.train()
    with torch.no_grad():
        out2 = m2.forward(image=b['image'], input_depth=b['input_depth'])
    b2 = dict(b)
    b2['ground_truth'] = OutlierRemoval(7, 1.5).remove_outliers(b['ground_truth'])
    l2, _ = _loss(m2, b2, out2)
    assert abs(float(l2) - rec['first_step_loss']) < BAR * rec['first_step_loss']


@pytest.mark.parametrize('tier', ['fp32', 'fp32_3plane'])
def test_config1_fp32_batch8_gradients_are_the_sum_of_batch1_gradients(env, tier):
    '''Full batch, full resolution, forward AND backward, without a minutes-long CPU backward: with eval-mode BatchNorm the samples
    are independent, so (i) row i of the batch-8 output is the batch-1 output of sample i (tiles that straddle images in
    the virtual-tall tiling, 64-bit offsets into 30 GB of activations) and (ii) the batch-8 parameter gradient is the sum of
    the eight batch-1 gradients for the same upstream gradient.  On the three-plane bf16 split (i) holds BITWISE; on the two-plane fp16
    arithmetic the operand scale is a property of the whole tensor (max|x| over the batch), so a batch-1 call may round its planes one
    binade finer than the batch-8 call: equal to fp32 round-off (1e-5 of max-abs) instead of bitwise.'''
    synth, _ = env
    cb = synth.make_batch(8, 900, 1600, 64, seed=77)
    b = {k: v.cuda() for k, v in cb.items()}
    m = _build(env, 21, tier)
    m.eval()
    torch.manual_seed(5)
    dd = (torch.rand(8, 1, 900, 1600, device='cuda') - 0.5) * 1e-3
    out8 = m.forward(b['image'], b['input_depth'])
    for p in m.parameters():
        p.grad = None
    out8.backward(dd)
    g8 = m._grad_arena[:m._n_used].clone()
    gsum = torch.zeros_like(g8, dtype=torch.float64)
    for i in range(8):
        o1 = m.forward(b['image'][i:i + 1].contiguous(), b['input_depth'][i:i + 1].contiguous())
        if i in (0, 3, 7):
            if tier == 'fp32_3plane':
                assert torch.equal(o1[0], out8.detach()[i]), 'sample %d: batch-8 row differs from the batch-1 output' % i
            else:
                e = _rel(o1[0], out8.detach()[i])
                print('sample %d: batch-8 row vs batch-1 output rel %.2e' % (i, e))
                assert e < 1e-5, 'sample %d: batch-8 row differs from the batch-1 output by %.2e' % (i, e)
        for p in m.parameters():
            p.grad = None
        o1.backward(dd[i:i + 1].contiguous())
        gsum += m._grad_arena[:m._n_used].double()
    worst = 0.0
    off = 0
    for p in m._used_params:
        n = p.numel()
        e = _rel(g8[off:off + n], gsum[off:off + n])
        worst = max(worst, e)
        off += n
    print('batch-8 gradient vs sum of batch-1 gradients: worst tensor rel %.2e' % worst)
    assert worst < 2e-4


def _named_params(m):
    out = []
    for prefix, mod in (('encoder.', m.encoder), ('decoder.', m.decoder)):
        for k, p in mod.named_parameters():
            out.append((prefix + k, p))
    return out


@pytest.mark.parametrize('tier', ['fp32', 'fp32_3plane', 'bf16'])
def test_config1_headline_backward_and_three_adam_steps_against_the_oracle(env, tier):
    '''The BACKWARD the metric times, at the metric's own workload: bench.py's step (published net, weights seed 1234, data seed 1234,
    batch 8, 900x1600, train-mode BatchNorm over the eight images, outlier removal (7, 1.5), masked L1 + 2.0 x lidar, Adam lr 1e-3)
    against tests/golden/bench_backward_b8.npz -- the CPU oracle's gradients of that step (make_bench_backward.py; the oracle is pinned
    to the real reference at 0.00e+00 by make_golden.py), with the fp64 run of the same step as yardstick.
      * every parameter gradient's L2 norm: 1e-3 of the oracle's where the fp32 oracle itself is that close to fp64, else within 3 x the
        oracle's own distance from fp64 (fp32 gradients of this net carry LeakyReLU / max-pool decision flips: DESIGN.md 2);
      * 2048 sampled elements of each of the ten largest gradient tensors against fp64, T1b's rule: per tensor within 5 x the fp32
        oracle's own max-norm distance, the median over the ten within 3 x;
      * the losses of the first three optimizer steps (the trajectory through two Adam updates) at 1e-3.
    bf16 tensors: cosine of every sampled tensor against fp64 and the loss trajectory at the bf16 bars.'''
    from rcf_amd.net_utils import OutlierRemoval
    synth, train = env
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'bench_backward_b8.npz'))
    n, h, w, k, dseed, wseed = [int(v) for v in g['meta']]
    b = {kk: v.cuda() for kk, v in synth.make_batch(n, h, w, k, seed=dseed).items()}
    m = _build(env, wseed, tier)
    opt = train.make_optimizer(m, lr=1e-3)
    m.train()
    outl = OutlierRemoval(7, 1.5)
    losses = []
    for step in range(3):
        loss, _, out = train.train_step(m, opt, b['image'], b['input_depth'], b['ground_truth'], b['lidar_map'], outlier_removal=outl)
        torch.cuda.synchronize()
        losses.append(float(loss.detach()))
        if step == 0:
            # (the gradient arena still holds step 1's gradients: optimizer.step() does not touch them)
            grads = {kk: p.grad.detach().double().cpu() for kk, p in _named_params(m) if p.grad is not None}
            out_mean = float(out.detach().double().mean())
    lbar = BF16_LOSS_BAR * 40 if tier == 'bf16' else BAR   # (bf16: after two Adam updates the trajectories of two arithmetics part)
    print('%s losses %s vs oracle %s' % (tier, ['%.5f' % v for v in losses], ['%.5f' % v for v in g['losses']]))
    for got, want in zip(losses, g['losses']):
        assert abs(got - want) < lbar * want, (tier, losses, g['losses'].tolist())
    assert abs(out_mean - float(g['output_mean'])) < (3e-3 if tier == 'bf16' else 1e-4) * float(g['output_mean'])
    assert set(grads.keys()) == set(g['grad_keys'].tolist())
    # ---- sampled elements against fp64
    e_hip, e_ref, cosines = [], [], []
    for key, idx, ref32, v64, amax in zip(g['keys'].tolist(), g['idx'], g['ref32'], g['fp64'], g['fp64_absmax']):
        got = grads[key].reshape(-1).numpy()[idx]
        e_hip.append(float(np.abs(got - v64).max() / amax))
        e_ref.append(float(np.abs(ref32.astype(np.float64) - v64).max() / amax))
        cosines.append(float(np.dot(got, v64) / (np.linalg.norm(got) * np.linalg.norm(v64))))
    print('%s sampled gradient elements vs fp64 (max-norm): HIP %s | the fp32 oracle %s | cosines min %.5f'
          % (tier, ' '.join('%.1e' % e for e in e_hip), ' '.join('%.1e' % e for e in e_ref), min(cosines)))
    if tier == 'bf16':
        # bf16 tensors and operands through 40 layers: the sampled tensors are the DEEPEST ones (blocks4-6, 29x50 .. 57x100), where the
        # gradient has passed through every rounding of the decoder and most of the encoder.  No bar in north_star; bars = the measured
        # values (deterministic kernels, fixed seeds) with the usual 1.3 x slack on 1 - cosine, printed next to them
        pooled_got = np.concatenate([grads[key].reshape(-1).numpy()[idx] / amax for key, idx, amax in zip(g['keys'].tolist(), g['idx'], g['fp64_absmax'])])
        pooled_ref = np.concatenate([v64 / amax for v64, amax in zip(g['fp64'], g['fp64_absmax'])])
        pooled = float(np.dot(pooled_got, pooled_ref) / (np.linalg.norm(pooled_got) * np.linalg.norm(pooled_ref)))
        print('bf16 per-tensor cosines %s; pooled over the ten tensors %.4f (bars %.3f / %.3f)'
              % (' '.join('%.3f' % c for c in cosines), pooled, BF16_DEEP_COS_BAR, BF16_POOLED_COS_BAR))
        assert min(cosines) > BF16_DEEP_COS_BAR and pooled > BF16_POOLED_COS_BAR
    else:
        for key, eh, er in zip(g['keys'].tolist(), e_hip, e_ref):
            assert eh <= 5.0 * er + 2e-4, (key, eh, er)
        assert np.median(e_hip) <= 3.0 * np.median(e_ref) + 2e-5
    # ---- every parameter gradient's norm against fp64.  Convolution weights (4-d: 99.9 % of the parameters) at 1e-3, or 3 x the fp32
    # oracle's own distance from fp64 where that is larger; BatchNorm weights / biases are sums of nearly cancelling terms over up to
    # 11.5 M pixels whose value moves with every LeakyReLU / max-pool decision that differs between two fp32 evaluations:
    # they get fixture T1's bar, 1e-2, and their median must still hold 1e-3.
    shapes = {kk: tuple(p.shape) for kk, p in _named_params(m)}
    worst, worst_key, errs_small, errs_conv = 0.0, None, [], []
    for key, l2, l64 in zip(g['grad_keys'].tolist(), g['grad_l2'], g['grad_l2_fp64']):
        got = float(grads[key].norm())
        ref_dist = abs(l2 - l64) / max(l64, 1e-30)          # the fp32 oracle's own distance from fp64 on this norm
        e = abs(got - l64) / max(l64, 1e-30)
        conv_w = len(shapes[key]) == 4
        if tier == 'bf16':
            bar = BF16_NORM_BAR if conv_w else BF16_BN_NORM_BAR
        else:
            bar = max(BAR if conv_w else 1e-2, 3.0 * ref_dist)
        (errs_conv if conv_w else errs_small).append(e)
        if e / bar > worst:
            worst, worst_key = e / bar, key
        assert e < bar, (tier, key, got, l64, l2)
    print('%s: %d parameter-gradient norms vs fp64, worst at %.2f of its bar (%s); BatchNorm parameters: median %.1e, max %.1e; convolution weights: max %.1e'
          % (tier, len(g['grad_keys']), worst, worst_key, float(np.median(errs_small)), max(errs_small), max(errs_conv)))
    if tier != 'bf16':
        assert np.median(errs_small) < BAR


# ------------------------------------------------------------------------------------------------------------ configs[3]
def test_config3_bf16_train_step_900x1600_against_fp32_oracle(env):
    '''bf16 training arithmetic at the benchmark resolution (batch 2 so the batch statistics are over more than one image)
    against the fp32 CPU oracle, and its gradient against the fp32 HIP gradient.'''
    synth, train = env
    cb = synth.make_batch(2, 900, 1600, 64, seed=4321)
    b = {k: v.cuda() for k, v in cb.items()}
    res = {}
    for dtype in ('bf16', 'fp32'):
        m = _build(env, 9, dtype)
        m.train()
        out = m.forward(image=b['image'], input_depth=b['input_depth'])
        loss, _ = _loss(m, b, out)
        loss.backward()
        torch.cuda.synchronize()
        res[dtype] = (out.detach().cpu(), float(loss), m._grad_arena[:m._n_used].double().cpu())
    o = _oracle(env, 9)
    o.train()
    with torch.no_grad():
        ref = o.forward(cb['image'], cb['input_depth'])
        ref_loss = float(o.compute_loss(ref, cb['ground_truth'], cb['lidar_map'], 2.0)[0])
    e16, e32 = _rel(res['bf16'][0], ref), _rel(res['fp32'][0], ref)
    mae16 = float((res['bf16'][0] - ref).abs().mean()) * 1000.0
    cos = float(torch.dot(res['bf16'][2], res['fp32'][2]) / (res['bf16'][2].norm() * res['fp32'][2].norm()))
    print('900x1600 batch 2: bf16 out rel %.2e (bar %.0e), MAE %.2f mm, loss %.5f vs oracle %.5f; fp32 out rel %.2e; '
          'gradient cosine bf16 vs fp32 %.4f' % (e16, BF16_OUT_BAR, mae16, res['bf16'][1], ref_loss, e32, cos))
    assert e32 < BAR and abs(res['fp32'][1] - ref_loss) < BAR * abs(ref_loss)
    assert e16 < BF16_OUT_BAR and abs(res['bf16'][1] - ref_loss) < BF16_LOSS_BAR * abs(ref_loss)
    assert cos > BF16_COS_BAR


def test_config3_bf16_batch8_900x1600_step_is_the_benchmarked_step(env):
    '''One GPU's share of BASELINE.json configs[3] exactly as bench.py --dtype bf16 runs it: batch 8, 900x1600, bf16 tensors, train-mode
    BatchNorm over the 8 images, outlier removal, masked L1.  The first-step loss against the CPU oracle's recorded value
    (tests/golden/bench_expected.json), the output against the fp32 HIP output of the same step (itself pinned to the oracle by
    test_config1_*), backward + Adam finite.'''
    from rcf_amd.net_utils import OutlierRemoval
    synth, train = env
    rec = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'bench_expected.json')))['train_b8_900x1600_p64']
    b = {k: v.cuda() for k, v in synth.make_batch(8, 900, 1600, 64, seed=1234).items()}
    outl = OutlierRemoval(7, 1.5)
    outs = {}
    for dtype in ('fp32', 'bf16'):
        m = _build(env, 1234, dtype)
        opt = train.make_optimizer(m, lr=1e-3)
        m.train()
        loss, _, out = train.train_step(m, opt, b['image'], b['input_depth'], b['ground_truth'], b['lidar_map'], outlier_removal=outl)
        torch.cuda.synchronize()
        outs[dtype] = (out.detach().float().cpu(), float(loss.detach()))
        assert bool(torch.isfinite(m._grad_arena[:m._n_used]).all()) and bool(torch.isfinite(m._param_arena).all())
        del m, opt
        torch.cuda.empty_cache()
    e = _rel(outs['bf16'][0], outs['fp32'][0])
    le = abs(outs['bf16'][1] - rec['first_step_loss']) / rec['first_step_loss']
    print('bf16 batch-8 900x1600 step: first loss %.5f vs oracle %.5f (rel %.2e, bar %.0e); output vs fp32 HIP rel %.2e (bar %.0e)'
          % (outs['bf16'][1], rec['first_step_loss'], le, BF16_LOSS_BAR, e, BF16_OUT_BAR))
    assert abs(outs['fp32'][1] - rec['first_step_loss']) < BAR * rec['first_step_loss']
    assert le < BF16_LOSS_BAR and e < BF16_OUT_BAR


# ------------------------------------------------------------------------------------------------------------ configs[4]
@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_three_stream_step_is_bitwise_the_single_stream_step_at_900x1600(env, dtype):
    '''The default schedule (weight gradients on a side stream, the encoder's depth branch and the fusions on another: DESIGN.md
    section 5 "Three streams") against the same steps with everything on one stream, at the benchmarked shape (batch 4 to keep the
    test short): output depth, loss and every parameter after each of 3 training steps -- equality, not a tolerance: the same kernels on
    the same operands in the same summation orders; any cross-stream race (a tensor reused by the allocator while another stream still
    reads it, a missing join) shows up as a difference at this size, where kernels run for hundreds of microseconds.'''
    synth, train = env
    cb = synth.make_batch(4, 900, 1600, 64, seed=2024)
    b = {k: v.cuda() for k, v in cb.items()}
    runs = []
    for single in (True, False):
        m = _build(env, 11, dtype)
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


def test_config4_bf16_batch32_hipgraph_inference_900x1600(env):
    '''Batch 32 at 900x1600, eval-mode BatchNorm folded, bf16: the hipGraph replay is bitwise the eager forward, a second replay on
    new inputs too, and a sample of the batch matches the fp32 CPU oracle's eval-mode output within the bf16 bar.'''
    synth, _ = env
    cb = synth.make_batch(32, 900, 1600, 64, seed=99)
    m = _build(env, 3, 'bf16')
    m.eval()
    img, dep = cb['image'].cuda(), cb['input_depth'].cuda()
    with torch.no_grad():
        eager = m.forward(img, dep).clone()
        run = m.capture_inference(img, dep)
        rep = run(img, dep).clone()
        assert torch.equal(rep, eager)
        perm = torch.arange(31, -1, -1, device='cuda')
        rep2 = run(img[perm].contiguous(), dep[perm].contiguous()).clone()
        assert torch.equal(rep2, eager[perm])          # samples are independent in eval mode: replay on permuted inputs
        # the deployment form bench.py times: weights folded / packed once before the recording (fold_once) -- same bits, fewer nodes
        run1 = m.capture_inference(img, dep, fold_once=True)
        assert torch.equal(run1(img, dep), eager) and torch.equal(run1(img[perm].contiguous(), dep[perm].contiguous()), eager[perm])
        assert len(run1.frozen_weights) > 100
        wconv = m.decoder.deconv1.conv.conv.weight      # a convolution weight (folded with its BatchNorm and packed)
        keep = wconv.detach().clone()
        with torch.no_grad():                          # frozen at capture time: a later parameter change reaches `run`, not `run1`
            wconv.mul_(1.5)
        assert not torch.equal(run(img, dep), eager) and torch.equal(run1(img, dep), eager)
        with torch.no_grad():
            wconv.copy_(keep)
    o = _oracle(env, 3)
    o.eval()
    with torch.no_grad():
        ref = o.forward(cb['image'][5:6], cb['input_depth'][5:6])
    e = _rel(eager[5:6], ref)
    print('batch-32 bf16 hipGraph inference: sample 5 vs fp32 oracle rel %.2e (bar %.1e), MAE %.2f mm'
          % (e, BF16_INFER_BAR, float((eager[5:6].cpu() - ref).abs().mean()) * 1000.0))
    assert e < BF16_INFER_BAR


# ------------------------------------------------------------------------------------------------------------ configs[2]
@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_config2_radarnet_900x288_patches_against_oracle(env, dtype):
    '''RadarNet stage 1 at the workload `bench.py --workload radarnet` times (BASELINE.json configs[2]: 16 images x 4 radar points =
    64 crops of 900x288 from 900x1888 edge-padded images, the bench's own seeds), training step; logits and loss against the CPU
    restatement's recorded values (the restatement is pinned to the reference by fixtures T5/T6), gradients finite; bf16 against the
    same fp32 values at the bf16 bar.'''
    from rcf_amd import radarnet_model
    synth, _ = env
    cb = synth.make_radarnet_batch(7, n=16, k=4, h=900, w=1888, patch_w=288)
    m = radarnet_model.RadarNetModel(device=torch.device('cuda'), **synth.RADARNET_PUBLISHED)
    m.compute_dtype = dtype
    synth.fill_state_dict_([m.encoder, m.decoder], 41)
    b = {key: (v.cuda() if isinstance(v, torch.Tensor) else [t.cuda() for t in v]) for key, v in cb.items()}
    m.train()
    logits = m.forward(b['image'], b['point'], b['bounding_boxes'])
    loss, _ = m.compute_loss(logits, b['ground_truth'], b['validity_map'], w_positive_class=2.0)
    loss.backward()
    torch.cuda.synchronize()
    g = m._grad_arena[:m._n_used]
    assert tuple(logits.shape) == (64, 1, 900, 288)
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    # the oracle's values for exactly this step are recorded (tests/golden/make_bench_expected.py --legs: the first-step loss, the
    # largest |logit| and 4096 seeded logits of the 64 x 900 x 288 map; a CPU forward of the 16 images takes ~50 s on the GPU box)
    exp = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'bench_expected.json')))['radarnet_b16x4_900x1888']
    idx = torch.tensor(exp['logit_index'], device=logits.device)
    got = logits.detach().reshape(-1)[idx].float().cpu()
    want = torch.tensor(exp['logits'])
    e = float((got - want).abs().max()) / exp['max_abs_logit']
    oloss = exp['first_step_loss']
    print('RadarNet %s 16 images x 4 crops of 900x288: 4096 sampled logits rel %.2e, loss %.6f vs oracle %.6f, mean logit %.6f vs %.6f'
          % (dtype, e, float(loss), oloss, float(logits.double().mean()), exp['mean_logit']))
    if dtype == 'fp32':
        assert e < BAR and abs(float(loss) - oloss) < BAR * abs(oloss)
        assert abs(float(logits.double().mean()) - exp['mean_logit']) < BAR * exp['max_abs_logit']
    else:
        assert e < BF16_LOGIT_BAR and abs(float(loss) - oloss) < BF16_LOSS_BAR * abs(oloss)


def test_radarnet_frame_with_more_than_64_points(env):
    '''pipeline.radarnet_forward runs EVERY radar point of a frame through one forward (src/radarnet_main.py:534-561); a frame has
    up to ~100 of them.  The fully connected encoder works in row blocks of 64: 70 points against the oracle, forward and the
    gradients of the MLP (whose dW / db sum over all rows).'''
    from oracle.radarnet_oracle import RadarNetOracle
    from rcf_amd import radarnet_model
    synth, _ = env
    cfg = dict(synth.RADARNET_TINY)
    cb = synth.make_radarnet_batch(31, n=1, k=70, h=64, w=160, patch_w=32)
    ora = RadarNetOracle(**cfg)
    synth.fill_state_dict_([ora.encoder, ora.decoder], 13)
    ora.train()
    ol = ora.forward(cb['image'], cb['point'], cb['bounding_boxes'])
    oloss = ora.compute_loss(ol, cb['ground_truth'], cb['validity_map'], 2.0)
    oloss.backward()
    m = radarnet_model.RadarNetModel(device=torch.device('cuda'), **cfg)
    synth.fill_state_dict_([m.encoder, m.decoder], 13)
    b = {key: (v.cuda() if isinstance(v, torch.Tensor) else [t.cuda() for t in v]) for key, v in cb.items()}
    m.train()
    logits = m.forward(b['image'], b['point'], b['bounding_boxes'])
    loss, _ = m.compute_loss(logits, b['ground_truth'], b['validity_map'], w_positive_class=2.0)
    loss.backward()
    torch.cuda.synchronize()
    assert _rel(logits, ol) < BAR
    assert abs(float(loss) - float(oloss)) < BAR * abs(float(oloss))
    for (k, p), (k2, p2) in zip(m.encoder.named_parameters(), ora.encoder.named_parameters()):
        assert k == k2
        if 'encoder_depth' in k:
            assert _rel(p.grad, p2.grad) < 5 * BAR, k


# ------------------------------------------------------------------------------------------------------------ bench.py on real ranks
def _run_bench(extra, env_extra=None, timeout=900):
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_PORT', 'MASTER_ADDR')}
    env.update(env_extra or {})
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + extra, env=env, capture_output=True, text=True, timeout=timeout)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    return r, (json.loads(lines[-1]) if lines else None)


def test_bench_refuses_more_gpus_than_visible():
    n = torch.cuda.device_count()
    r, rec = _run_bench(['--gpus', str(n + 1), '--steps', '1', '--warmup', '0', '--no-cpu-baseline'])
    assert r.returncode == 2 and rec is None, (r.returncode, r.stdout[-300:], r.stderr[-300:])


def test_bench_two_ranks_spawned_by_bench_itself():
    '''`python bench.py --gpus 2` with no launcher: two child ranks, RCCL when two devices are visible, otherwise (1-GPU box) the
    two ranks share cuda:0 over gloo -- the same code path: buckets launched from the tape, global-count loss, max-over-ranks time.'''
    two = torch.cuda.device_count() >= 2
    extra_env = {} if two else {'RCF_BENCH_SINGLE_DEVICE': '1', 'RCF_DIST_BACKEND': 'gloo'}
    args = ['--gpus', '2', '--steps', '3', '--warmup', '1', '--batch', '2', '--height', '224', '--width', '384', '--points', '32',
            '--preheat-s', '0', '--no-cpu-baseline', '--full']
    try:
        r, rec = _run_bench(args, extra_env, timeout=240)     # normally 10-20 s
    except subprocess.TimeoutExpired:
        try:                                                   # one retry on a fresh port: a rendezvous that never completed
            r, rec = _run_bench(args, extra_env, timeout=240)
        except subprocess.TimeoutExpired:
            pytest.skip('the two-rank rendezvous did not complete on this box (twice); the same data-parallel path is covered '
                        'in-process by test_hip_model.py::test_data_parallel_step_two_ranks_on_one_gpu')
    assert r.returncode == 0 and rec is not None, (r.returncode, r.stdout[-500:], r.stderr[-1500:])
    assert rec['n_gpus'] == 2 and rec['rccl_ranks'] == 2 and rec['config']['parallelism'] == 'dp2'
    assert rec['backend'] == ('nccl' if two else 'gloo')
    assert len(rec['per_rank_ms_per_step']) == 2 and rec['config']['global_batch'] == 4
    assert rec['dp']['buckets'] >= 2 and rec['dp']['gradient_bytes'] == 14142208 * 4
    assert rec['value'] > 0
    assert rec['config']['loss_check']['ok'] is True       # the global masked mean of the two ranks' batches, against the oracle's


def test_bench_eight_ranks_spawned_by_bench_itself():
    '''The 8-rank path of `python bench.py --gpus 8` -- what the driver's scaling run launches -- on device tensors: the launch
    probe's all-gather over 8 ranks, six gradient buckets launched from the tape on every rank, the loss normalised by the counts of
    EIGHT data seeds (the oracle's global masked mean from tests/golden/bench_expected.json).  With fewer than eight devices the ranks
    share cuda:0 over gloo at the small shape (the host-blocking backend: no graph segments); with eight, RCCL.'''
    eight = torch.cuda.device_count() >= 8
    extra_env = {} if eight else {'RCF_BENCH_SINGLE_DEVICE': '1', 'RCF_DIST_BACKEND': 'gloo'}
    args = ['--gpus', '8', '--steps', '2', '--warmup', '1', '--batch', '2', '--height', '224', '--width', '384', '--points', '32',
            '--preheat-s', '0', '--no-cpu-baseline', '--full']
    try:
        r, rec = _run_bench(args, extra_env, timeout=600)
    except subprocess.TimeoutExpired:
        pytest.skip('the eight-rank rendezvous did not complete on this box; the 8-rank bucket / loss-sum logic is covered on the CPU by '
                    'tests/test_host_logic.py (gloo, world 8)')
    assert r.returncode == 0 and rec is not None, (r.returncode, r.stdout[-500:], r.stderr[-1500:])
    assert rec['n_gpus'] == 8 and rec['rccl_ranks'] == 8 and rec['config']['parallelism'] == 'dp8'
    assert rec['backend'] == ('nccl' if eight else 'gloo')
    assert len(rec['per_rank_ms_per_step']) == 8 and rec['config']['global_batch'] == 16
    assert rec['dp']['buckets'] >= 2 and rec['dp']['gradient_bytes'] == 14142208 * 4
    assert rec['config']['loss_check']['ok'] is True       # the global masked mean over the eight ranks' batches, against the oracle's
    probe = rec['dp']['launch_probe']
    assert len(probe['host_ms_by_rank']) == 8 and isinstance(probe['decision'], str)
    assert isinstance(rec['dp']['cpu_affinity_rank0'], dict) and 'pinned' in rec['dp']['cpu_affinity_rank0']


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_bench_two_ranks_at_the_headline_shape_pass_their_own_loss_check(dtype):
    '''`python bench.py --gpus 2` at the DEFAULT shape (published net, per-GPU batch 8, 900x1600) -- what the driver's scaling run
    launches.  Rank r trains on data seed 1234 + r and the loss is the reference's single masked mean over the gathered batch, so the
    first-step loss must equal the oracle's GLOBAL value formed from the per-seed sums of tests/golden/bench_expected.json (round 2
    compared it with rank 0's own mean and exited 3).  On a 1-GPU box the two ranks share cuda:0 over gloo (2 x 30 GB).
    dtype bf16 = BASELINE configs[3] ("bf16 x DP"): bf16 tensors under the data-parallel exchange -- the loss sums are all-reduced
    before backward and the fp32 gradient buckets behind it exactly as in fp32; the first-step loss is held to the fp32 oracle's global
    value within bf16's forward error (measured 3e-6 .. 1e-4 on one rank; bar 5e-3).'''
    two = torch.cuda.device_count() >= 2
    extra_env = {} if two else {'RCF_BENCH_SINGLE_DEVICE': '1', 'RCF_DIST_BACKEND': 'gloo'}
    args = ['--gpus', '2', '--steps', '2', '--warmup', '1', '--preheat-s', '0', '--no-cpu-baseline', '--dtype', dtype, '--full']
    r, rec = _run_bench(args, extra_env, timeout=900)
    assert r.returncode == 0 and rec is not None, (r.returncode, r.stdout[-500:], r.stderr[-1500:])
    assert rec['n_gpus'] == 2 and rec['rccl_ranks'] == 2 and rec['config']['global_batch'] == 16 and rec['dtype'] == dtype
    chk = rec['config']['loss_check']
    print('bench.py --gpus 2 --dtype %s: first-step loss rel err vs the oracle\'s global masked mean %.3e' % (dtype, chk['rel_err']))
    assert chk['ok'] is True and chk['rel_err'] < (1e-4 if dtype == 'f32' else 5e-3), chk
    single = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'bench_expected.json')))['train_b8_900x1600_p64']['first_step_loss']
    assert abs(chk['oracle_first_step_loss'] - single) > 1e-3 * single     # and the global value is NOT rank 0's own mean
    assert 'overlap_frac' in rec['dp']
    # the launch mode is decided by all ranks together (round 5): every rank's probe is in the line, and so is the common decision
    probe = rec['dp']['launch_probe']
    assert len(probe['host_ms_by_rank']) == 2 and len(probe['host_bound_by_rank']) == 2 and isinstance(probe['decision'], str)
    assert len(rec['dp']['host_ms_per_step_by_rank']) == 2


def test_bench_single_gpu_line_carries_the_contract_fields():
    '''The driver's command (`python bench.py`, defaults) with few steps: the contract fields, the headline's own loss check, and the
    legs that ride in the same line -- `exact_tier` (the step on three bf16 planes) and `other_configs` (BASELINE.json configs[2..4]),
    each checked against the CPU oracle's recorded values by bench.py itself.  No clock enters an assertion.'''
    r, rec = _run_bench(['--steps', '2', '--warmup', '1', '--preheat-s', '0', '--no-cpu-baseline', '--leg-steps', '2', '--full'], timeout=900)
    assert r.returncode == 0 and rec is not None, (r.returncode, r.stderr[-1500:])
    for key in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline',
                'dtype', 'data', 'config', 'roofline', 'algorithmic_tflops'):
        assert key in rec, key
    assert rec['n_gpus'] == 1 and rec['steps'] == 2 and rec['dtype'] == 'f32'
    assert rec['config']['loss_check']['ok'] is True          # first step == the CPU oracle's loss for these seeds
    for key in ('bound', 'achieved', 'peak', 'unit', 'frac', 'traffic', 'useful_frac', 'pipe', 'events_from', 'products_per_multiply'):
        assert key in rec['roofline'], key
    assert rec['roofline']['products_per_multiply'] == 3 and 'fp16' in rec['roofline']['pipe']
    enc = rec['roofline']['encoder_3x3']
    assert enc['tflops_algorithmic'] > 0 and 0 < enc['frac_of_pipe_peak'] < 1 and enc['gflop_per_step'] > 0
    side = rec['exact_tier']
    assert 'error' not in side, side
    assert side['dtype'] == 'f32_3plane' and side['value'] > 0 and side['steps'] == 4
    assert side['check']['ok'] is True and side['check']['rel_err'] < 1e-5, side['check']
    assert side['roofline']['products_per_multiply'] == 6
    others = rec['other_configs']
    assert len(others) == 3
    for name, leg in others.items():
        assert 'error' not in leg, (name, leg)
        assert leg['value'] > 0 and leg['steps'] == 2 and leg['dtype'] == 'bf16', (name, leg)
        assert leg['check']['ok'] is True, (name, leg['check'])
        assert 0 < leg['roofline']['frac'] < 1, (name, leg['roofline'])
    print({k: (v['value'], v['unit'], v['check']) for k, v in others.items()})


def test_bench_plain_run_is_lean_and_dumps_the_same_outputs_on_every_run(tmp_path):
    '''A run without --full prints the headline alone (no legs, no roofline, no oracle checks) and times exactly --steps steps;
    --dump-outputs writes the last timed step's loss, output and a parameter sample, and two runs with the same arguments write the
    same arrays, however many steps their time-bounded pre-heats ran (those steps are rolled back).'''
    args = ['--steps', '3', '--warmup', '1', '--batch', '2', '--height', '224', '--width', '384', '--points', '32', '--preheat-s', '1']
    recs = []
    for run in ('a', 'b'):
        r, rec = _run_bench(args + ['--dump-outputs', str(tmp_path / run)], timeout=600)
        assert r.returncode == 0 and rec is not None, (r.returncode, r.stderr[-1500:])
        recs.append(rec)
    rec = recs[0]
    for key in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'):
        assert key in rec, key
    assert rec['steps'] == 3 and rec['dtype'] == 'f32' and rec['value'] > 0 and rec['ms_per_step'] > 0
    for key in ('roofline', 'cpu_baseline', 'exact_tier', 'other_configs', 'dp'):
        assert key not in rec, key
    assert 'loss_check' not in rec['config'] and 'arithmetic' not in rec['config']
    names = sorted(os.listdir(tmp_path / 'a'))
    assert names == sorted(os.listdir(tmp_path / 'b'))
    eager = rec['config']['launch_probe']['decision'] == 'eager'
    assert names == sorted(['loss.npy', 'parameters_sample.npy'] + (['output_depth.npy'] if eager else [])), names
    loss = np.load(tmp_path / 'a' / 'loss.npy')
    assert loss.dtype == np.float64 and abs(float(loss) - rec['config']['final_loss']) < 1e-4 * abs(float(loss))
    assert np.load(tmp_path / 'a' / 'parameters_sample.npy').dtype == np.float32
    if eager:
        out = np.load(tmp_path / 'a' / 'output_depth.npy')
        assert out.dtype == np.float32 and out.shape == (2, 1, 224, 384) and np.isfinite(out).all()
    for name in names:
        np.testing.assert_allclose(np.load(tmp_path / 'b' / name), np.load(tmp_path / 'a' / name), rtol=1e-5, atol=1e-7, err_msg=name)


def test_bench_falls_back_to_the_replayed_graph_on_a_host_bound_box():
    '''A host that cannot enqueue a step as fast as the GPU runs it (forced here: threshold 0) gets the replayed graph in the headline
    AND in the training legs, the line says so, and every oracle check still passes.'''
    r, rec = _run_bench(['--steps', '2', '--warmup', '1', '--preheat-s', '0', '--no-cpu-baseline', '--leg-steps', '2', '--full'],
                        env_extra={'RCF_BENCH_HOST_BOUND_FRAC': '0'}, timeout=900)
    assert r.returncode == 0 and rec is not None, (r.returncode, r.stderr[-1500:])
    probe = rec['config']['launch_probe']
    assert probe['host_bound'] is True and probe['decision'] == 'graph', probe
    assert rec['config']['loss_check']['ok'] is True
    assert rec['exact_tier']['launch'].startswith('one hipGraph replay'), rec['exact_tier']
    assert rec['exact_tier']['check']['ok'] is True
    leg = rec['other_configs']['configs[3] FusionNet bf16 training, per-GPU batch 8']
    assert leg['launch'].startswith('one hipGraph replay') and leg['check']['ok'] is True, leg
    assert 0 < leg['roofline']['frac'] < 1
