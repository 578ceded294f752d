'''
GPU tests of rcf_eval_metrics / rcf_amd.evaluation: the kernel against float64 numpy (<= 1e-12 relative, counts exact) and against
the reference's float32 results of fixture T15 (|device - ref32| <= |ref32 - ref64| + 1e-12 |ref64|), its bitwise invariances, the
device-side row cursor, a captured forward + update, validate() against the recorded calls of the reference's validate() and on
the real network, and a two-rank sharded validation.
'''

import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 1e-12
KEYS = ('mae', 'rmse', 'imae', 'irmse')


@pytest.fixture(scope='module')
def env():
    import rcf_amd  # noqa: F401
    from rcf_amd import _lib, synth, train
    assert torch.cuda.is_available()
    _lib.load()
    return synth, train


@pytest.fixture(scope='module')
def t15(golden_dir):
    return np.load(os.path.join(golden_dir, 'T15_eval_metrics.npz'))


def numpy64(out, gt, lo, hi):
    '''float64 numpy on the float32 inputs: n x 4 metrics and the counts; the thresholds compare in float32 as the reference's do'''
    rows, cnt = [], []
    for s in range(out.shape[0]):
        g32 = gt[s].ravel()
        mask = (g32 > 0) & (g32 > np.float32(lo)) & (g32 < np.float32(hi))
        g, o = g32[mask].astype(np.float64), out[s].ravel()[mask].astype(np.float64)
        e, ie = 1000.0 * g - 1000.0 * o, 1.0 / (0.001 * g) - 1.0 / (0.001 * o)
        with np.errstate(all='ignore'):
            rows.append([np.mean(np.abs(e)), np.sqrt(np.mean(e ** 2)), np.mean(np.abs(ie)), np.sqrt(np.mean(ie ** 2))] if g.size else [np.nan] * 4)
        cnt.append(g.size)
    return np.array(rows), np.array(cnt)


def device_rows(out, gt, lo, hi, batch=None):
    '''n x 5 rows from MetricsAccumulator, the samples added `batch` at a time (default: all at once)'''
    from rcf_amd.evaluation import MetricsAccumulator
    n = out.shape[0]
    o, g = torch.as_tensor(out).cuda(), torch.as_tensor(gt).cuda()
    acc = MetricsAccumulator(n, lo, hi, 'cuda')
    step = batch or n
    for s in range(0, n, step):
        acc.update(o[s:s + step], g[s:s + step])
    return acc.rows().numpy()


def check_against_numpy(rows, out, gt, lo, hi, tag):
    want, cnt = numpy64(out, gt, lo, hi)
    assert rows[:, 4].tolist() == cnt.tolist(), tag
    for s in range(out.shape[0]):
        if cnt[s] == 0:
            assert np.isnan(rows[s, :4]).all(), tag
            continue
        rel = np.abs(rows[s, :4] - want[s]) / np.abs(want[s])
        print('%s sample %d: count %d, rel err vs float64 numpy %s' % (tag, s, cnt[s], ['%.1e' % r for r in rel]))
        assert np.all(rel <= REL), (tag, s, rel)


def test_kernel_matches_float64_numpy_and_the_reference_fixture(env, t15):
    synth, _ = env
    for i, (seed, n, h, w, density, sigma, lo, hi) in enumerate(t15['cases']):
        out, gt = synth.make_eval_case(int(seed), int(n), int(h), int(w), density, sigma)
        rows = device_rows(out, gt, lo, hi)
        check_against_numpy(rows, out, gt, lo, hi, 'case %d' % i)
        r32, r64, cnt = t15['c%02d_ref32' % i], t15['c%02d_ref64' % i], t15['c%02d_count' % i]
        assert rows[:, 4].tolist() == cnt.tolist()
        if cnt.all():
            assert np.all(np.abs(rows[:, :4] - r32) <= np.abs(r32 - r64) + REL * np.abs(r64)), i
        else:
            assert np.isnan(rows[:, :4]).all() and np.isnan(r32).all()


def test_kernel_at_8x900x1600_and_batch_invariance(env):
    '''The flagship size (vector path): float64 numpy to 1e-12; sample s of the batch-8 call == the same sample alone; two runs equal.'''
    synth, _ = env
    out, gt = synth.make_eval_case(77, 8, 900, 1600, 0.30, 2.0)
    rows = device_rows(out, gt, 0.0, 100.0)
    check_against_numpy(rows, out, gt, 0.0, 100.0, '8x900x1600')
    assert np.array_equal(rows, device_rows(out, gt, 0.0, 100.0))
    assert np.array_equal(rows, device_rows(out, gt, 0.0, 100.0, batch=1))


def test_unaligned_scalar_path_equals_aligned_copies_bitwise(env):
    '''71 x 103 = 7313 pixels, odd: every second sample of a batch starts off a 16-byte boundary and takes the scalar loads.  The same
    samples, each in a fresh (aligned) allocation and evaluated alone, give the same bits.'''
    synth, _ = env
    from rcf_amd.evaluation import MetricsAccumulator
    out, gt = synth.make_eval_case(78, 4, 71, 103, 0.30, 2.0)
    o, g = torch.as_tensor(out).cuda(), torch.as_tensor(gt).cuda()
    assert o[1].data_ptr() % 16 != 0
    rows = device_rows(out, gt, 0.0, 100.0)
    check_against_numpy(rows, out, gt, 0.0, 100.0, '71x103')
    acc = MetricsAccumulator(4, 0.0, 100.0, 'cuda')
    for s in range(4):
        oc, gc = o[s:s + 1].clone(), g[s:s + 1].clone()
        assert oc.data_ptr() % 16 == 0 and gc.data_ptr() % 16 == 0
        acc.update(oc, gc)
    assert np.array_equal(rows, acc.rows().numpy())


def test_cursor_fills_rows_in_order_and_drops_what_does_not_fit(env):
    synth, _ = env
    from rcf_amd import _lib, ops
    from rcf_amd.evaluation import MetricsAccumulator
    out, gt = synth.make_eval_case(79, 7, 70, 102, 0.30, 2.0)
    o, g = torch.as_tensor(out).cuda(), torch.as_tensor(gt).cuda()
    want, cnt = numpy64(out, gt, 0.0, 100.0)
    acc = MetricsAccumulator(6, 0.0, 100.0, 'cuda')
    guarded = torch.full((7, 5), -7.0, dtype=torch.float64, device='cuda')      # row 6 is the guard behind a capacity of 6
    acc.results = guarded[:6]
    for lo_, hi_ in ((0, 2), (2, 3), (3, 6)):
        acc.update(o[lo_:hi_], g[lo_:hi_])
    rows = acc.rows().numpy()
    assert rows[:, 4].tolist() == cnt[:6].tolist()
    assert np.all(np.abs(rows[:, :4] - want[:6]) <= REL * np.abs(want[:6]))
    acc.update(o[6:7], g[6:7])                                                  # a valid call that finds no room
    torch.cuda.synchronize()
    assert acc.cursor.cpu().tolist() == [6, 1]
    assert guarded[6].cpu().tolist() == [-7.0] * 5 and np.array_equal(guarded[:6].cpu().numpy(), rows)
    with pytest.raises(_lib.RcfError):
        acc.per_sample()
    acc.reset()
    with pytest.raises(_lib.RcfError):                                         # fewer rows than n_sample
        acc.update(o[0:2], g[0:2]) or acc.per_sample()
    with pytest.raises(ValueError):
        ops.eval_metrics(o.double(), g.double(), 0.0, 100.0, acc.workspace, acc.results, acc.cursor)
    with pytest.raises(ValueError):
        ops.eval_metrics(o[:, :, :, ::2], g[:, :, :, ::2], 0.0, 100.0, acc.workspace, acc.results, acc.cursor)


def _tiny_model(env, seed=41):
    synth, train = env
    m = train.build_model(synth.TINY, device='cuda')
    synth.fill_state_dict_([m.encoder, m.decoder], seed)
    m.eval()
    return m


def test_captured_forward_and_update_fill_a_row_per_replay(env):
    '''torch.cuda.graph around model.forward + update, replayed three times with new inputs: three rows, the eager sequence's bits.'''
    synth, _ = env
    from rcf_amd.evaluation import MetricsAccumulator
    m = _tiny_model(env)
    batches = [{k: v.cuda() for k, v in synth.make_batch(1, 70, 102, 8, seed=900 + s).items()} for s in range(3)]
    eager = MetricsAccumulator(3, 0.0, 100.0, 'cuda')
    with torch.no_grad():
        for b in batches:
            eager.update(m.forward(image=b['image'], input_depth=b['input_depth']), b['ground_truth'])
    want = eager.rows().numpy()
    acc = MetricsAccumulator(3, 0.0, 100.0, 'cuda')
    image, depth, gt = (batches[0][k].clone() for k in ('image', 'input_depth', 'ground_truth'))
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        acc.update(m.forward(image=image, input_depth=depth), gt)
    for b in batches:
        image.copy_(b['image']); depth.copy_(b['input_depth']); gt.copy_(b['ground_truth'])
        graph.replay()
    got = acc.rows().numpy()
    assert np.isfinite(got).all() and np.array_equal(got, want)


class _Stub(object):
    def __init__(self, outputs):
        self.outputs, self.k = outputs, 0

    def forward(self, image, input_depth):
        self.k += 1
        return self.outputs[self.k - 1]


class _PassThrough(object):
    def transform(self, images_arr, random_transform_probability=0.0):
        return images_arr


def test_validate_reproduces_the_recorded_calls_of_the_reference(env, t15, tmp_path):
    '''The generator's stub model with its outputs uploaded: `step` exactly, values within the fixture's own bound, the log text equal.'''
    synth, _ = env
    from rcf_amd.evaluation import validate
    n, h, w = (int(v) for v in t15['validate_shape'])
    lo, hi = t15['validate_range']
    best = {'step': -1, 'mae': np.inf, 'rmse': np.inf, 'imae': np.inf, 'irmse': np.inf}
    log_path = str(tmp_path / 'results.txt')
    r32, r64 = t15['validate_ref32'], t15['validate_ref64']
    bound = (np.abs(r32 - r64) + REL * np.abs(r64)).mean(1)          # of a mean over the samples: the mean of the per-sample bounds
    z = torch.zeros(1, 1, h, w)
    for c, sig in enumerate(t15['validate_sigmas']):
        out, gt = synth.make_eval_case(int(t15['validate_seed']), n, h, w, float(t15['validate_density']), synth.banded_sigma(*sig))
        loader = [[torch.zeros(1, 3, h, w), z, z, torch.from_numpy(gt[s:s + 1])] for s in range(n)]
        model = _Stub([torch.from_numpy(out[s:s + 1]).cuda() for s in range(n)])
        best = validate(model, loader, _PassThrough(), 100 * (c + 1), best, lo, hi, torch.device('cuda'), None, log_path=log_path)
        rec = t15['validate_best'][c]
        assert best['step'] == int(rec[0])
        src = [100, 100, 300, 400][c] // 100 - 1                     # the call whose means best_results holds now
        for k, key in enumerate(KEYS):
            print('call %d %s: %.9f, recorded %.9f, bound %.2e' % (c, key, best[key], rec[1 + k], bound[src][k]))
            assert abs(best[key] - rec[1 + k]) <= bound[src][k]
    assert open(log_path).read() == str(t15['validate_log'])


@pytest.mark.parametrize('tier', ['fp32', 'fp32_3plane', 'bf16'])
def test_validate_on_the_real_network_equals_host_float64_metrics(env, tier, tmp_path):
    synth, _ = env
    from rcf_amd.evaluation import evaluate, validate
    from rcf_amd.fusionnet_transforms import Transforms
    m = _tiny_model(env)
    m.compute_dtype = tier
    seen = []
    real_forward = m.forward

    class Spy(object):
        def forward(self, image, input_depth):
            o = real_forward(image=image, input_depth=input_depth)
            seen.append(o.clone())
            return o
    loader = []
    for s, nb in enumerate((1, 2, 1)):                                # any batch size per loader item
        b = synth.make_batch(nb, 70, 102, 8, seed=950 + s)
        loader.append([b['image'], b['input_depth'][:, 0:1], b['input_depth'][:, 1:2], b['ground_truth']])
    tr = Transforms(normalized_image_range=[0, 1])
    best = {'step': -1, 'mae': np.inf, 'rmse': np.inf, 'imae': np.inf, 'irmse': np.inf}
    best = validate(Spy(), loader, tr, 7, best, 0.0, 100.0, torch.device('cuda'), None, log_path=str(tmp_path / 'r.txt'))
    out = torch.cat(seen).cpu().numpy()
    gt = torch.cat([item[3] for item in loader]).numpy()
    want, cnt = numpy64(out, gt, 0.0, 100.0)
    assert best['step'] == 7 and cnt.min() > 0
    for k, key in enumerate(KEYS):
        assert abs(best[key] - want[:, k].mean()) <= REL * want[:, k].mean(), (tier, key)
    means, per_sample = evaluate(m, loader, tr, 0.0, 100.0, torch.device('cuda'))
    assert [float(v) for v in means] == [best[k] for k in KEYS] and per_sample[4].tolist() == cnt.tolist()


def _dp_validate_worker(rank, world, port, tmpdir, total):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)      # both ranks share cuda:0
    import rcf_amd  # noqa: F401
    from rcf_amd import synth
    from rcf_amd.evaluation import evaluate, validate
    out, gt = synth.make_eval_case(81, total, 70, 102, 0.30, 2.0)
    n_local = (total + world - 1) // world
    idx = [(rank + k * world) % total for k in range(n_local)]         # DistributedSampler(shuffle=False, drop_last=False)
    z = torch.zeros(1, 1, 70, 102)
    loader = [[torch.zeros(1, 3, 70, 102), z, z, torch.from_numpy(gt[i:i + 1])] for i in idx]
    outputs = [torch.from_numpy(out[i:i + 1]).cuda() for i in idx]
    means, per_sample = evaluate(_Stub(outputs), loader, _PassThrough(), 0.0, 100.0, torch.device('cuda'), n_sample_total=total,
                                 log_path=os.path.join(tmpdir, 'eval%d.txt' % rank))
    np.save(os.path.join(tmpdir, 'v%d.npy' % rank), np.stack(per_sample))
    best = {'step': -1, 'mae': np.inf, 'rmse': np.inf, 'imae': np.inf, 'irmse': np.inf}
    best = validate(_Stub(outputs), loader, _PassThrough(), 50, best, 0.0, 100.0, torch.device('cuda'), None,
                    log_path=os.path.join(tmpdir, 'val%d.txt' % rank), n_sample_total=total)
    torch.save({'best': best, 'means': means}, os.path.join(tmpdir, 'best%d.pt' % rank))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_data_parallel_validate_two_ranks_on_one_gpu(env, tmp_path):
    '''5 samples over two ranks: both ranks hold the one-process per-sample arrays, bitwise; validate() leaves the same best_results
    on both, the whole set's means, and rank 0 alone writes the logs.'''
    import torch.multiprocessing as mp
    synth, _ = env
    total = 5
    port = 29100 + (os.getpid() % 1000)
    mp.spawn(_dp_validate_worker, args=(2, port, str(tmp_path), total), nprocs=2, join=True)
    out, gt = synth.make_eval_case(81, total, 70, 102, 0.30, 2.0)
    want = device_rows(out, gt, 0.0, 100.0, batch=1).T
    for r in range(2):
        assert np.array_equal(np.load(os.path.join(str(tmp_path), 'v%d.npy' % r)), want)
    b0, b1 = (torch.load(os.path.join(str(tmp_path), 'best%d.pt' % r), weights_only=False) for r in range(2))
    assert b0['best'] == b1['best'] and b0['best']['step'] == 50
    assert [b0['best'][k] for k in KEYS] == [float(np.mean(want[k])) for k in range(4)] == [float(v) for v in b1['means']]
    for name in ('eval', 'val'):
        assert os.path.exists(os.path.join(str(tmp_path), name + '0.txt')) and not os.path.exists(os.path.join(str(tmp_path), name + '1.txt'))
    text = open(os.path.join(str(tmp_path), 'val0.txt')).read()
    assert text.count('Validation results:') == 1 and text.count('Best results:') == 1 and '      50  ' in text


class _BatchIterable(object):
    '''a loader that is neither a DataLoader nor a list: two samples per item, so its length is not its sample count'''

    def __init__(self, items):
        self.items = items

    def __len__(self):
        return len(self.items)

    def __iter__(self):
        return iter(self.items)


def _rccl_gather_worker(rank, world, port, tmpdir):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('nccl', rank=0, world_size=1)              # RCCL: a backend that serves device tensors only
    import rcf_amd  # noqa: F401
    from rcf_amd import _lib, synth
    from rcf_amd.evaluation import MetricsAccumulator, evaluate, gather_sharded, validate
    out, gt = synth.make_eval_case(82, 4, 70, 102, 0.30, 2.0)
    z = torch.zeros(2, 1, 70, 102)
    loader = _BatchIterable([[torch.zeros(2, 3, 70, 102), z, z, torch.from_numpy(gt[i:i + 2])] for i in (0, 2)])
    outputs = [torch.from_numpy(out[i:i + 2]).cuda() for i in (0, 2)]
    means, per_sample = evaluate(_Stub(outputs), loader, _PassThrough(), 0.0, 100.0, torch.device('cuda'), n_sample_total=4, n_sample=4)
    best = {'step': -1, 'mae': np.inf, 'rmse': np.inf, 'imae': np.inf, 'irmse': np.inf}
    best = validate(_Stub(outputs), loader, _PassThrough(), 9, best, 0.0, 100.0, torch.device('cuda'), None, n_sample_total=4, n_sample=4)
    acc = MetricsAccumulator(4, 0.0, 100.0, 'cuda', max_batch=2)
    for o, item in zip(outputs, loader):
        acc.update(o, item[3].cuda())
    direct = gather_sharded(acc.rows(on_device=True), 4)
    uncounted = None
    try:                                                               # without n_sample the length stands for the sample count: 2 of 4 fit
        evaluate(_Stub(outputs), loader, _PassThrough(), 0.0, 100.0, torch.device('cuda'))
    except _lib.RcfError as e:
        uncounted = str(e)
    torch.save({'per_sample': np.stack(per_sample), 'means': means, 'best': best, 'direct': direct.cpu(), 'direct_is_cuda': direct.is_cuda,
                'uncounted': uncounted}, os.path.join(tmpdir, 'rccl.pt'))
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_data_parallel_evaluate_gathers_on_the_device_over_rccl(env, tmp_path):
    '''One rank under 'nccl' (RCCL), the backend parallel.init_from_env selects on a GPU box and which refuses CPU tensors: evaluate()
    and validate() with n_sample_total go through gather_sharded on device tensors and return the one-process rows, bitwise.  The
    loader is a plain iterable of two-sample batches, counted through n_sample.'''
    import torch.multiprocessing as mp
    synth, _ = env
    port = 29400 + (os.getpid() % 1000)
    mp.spawn(_rccl_gather_worker, args=(1, port, str(tmp_path)), nprocs=1, join=True)
    r = torch.load(os.path.join(str(tmp_path), 'rccl.pt'), weights_only=False)
    out, gt = synth.make_eval_case(82, 4, 70, 102, 0.30, 2.0)
    want = device_rows(out, gt, 0.0, 100.0, batch=1)
    assert np.array_equal(r['per_sample'], want.T) and r['direct_is_cuda'] and np.array_equal(r['direct'].numpy(), want)
    assert [float(v) for v in r['means']] == [float(np.mean(want[:, k])) for k in range(4)] == [r['best'][k] for k in KEYS]
    assert r['best']['step'] == 9 and r['uncounted'] is not None and 'dropped' in r['uncounted']


def test_update_does_not_allocate_while_a_graph_is_captured(env):
    '''A batch larger than the reserved workspace raises during capture (and asks for max_batch) instead of allocating from the
    capture's pool; outside a capture the workspace grows; with max_batch the recorded update() replays.'''
    synth, _ = env
    from rcf_amd import _lib
    from rcf_amd.evaluation import MetricsAccumulator
    out, gt = synth.make_eval_case(83, 2, 70, 102, 0.30, 2.0)
    o, g = torch.as_tensor(out).cuda(), torch.as_tensor(gt).cuda()
    want = device_rows(out, gt, 0.0, 100.0)
    acc = MetricsAccumulator(4, 0.0, 100.0, 'cuda')                     # max_batch 1
    raised, scratch = False, torch.zeros(4, device='cuda')
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        scratch.zero_()                                                 # (so that the recording is not empty)
        try:
            acc.update(o, g)
        except _lib.RcfError as e:
            raised = 'max_batch' in str(e)
    assert raised
    acc.update(o, g)                                                    # eager: grows
    ready = MetricsAccumulator(4, 0.0, 100.0, 'cuda', max_batch=2)
    graph2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph2):
        ready.update(o, g)
    graph2.replay(); graph2.replay()
    acc.update(o, g)
    assert np.array_equal(acc.rows().numpy(), np.concatenate([want, want])) and np.array_equal(ready.rows().numpy(), np.concatenate([want, want]))
