'''
CPU tests of the validation / evaluation layer (no GPU): the host functions of rcf_amd.eval_utils against the reference's float32
results (fixture T15, tests/golden/make_golden_eval.py), the checkpoint-selection rule and the log lines against four recorded calls
of the reference's validate(), the data-parallel gather over gloo, and the C ABI of rcf_eval_metrics.
'''

import ctypes
import math
import os
import re
import sys
import warnings

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def pkg():
    import __graft_entry__ as entry
    entry.build()
    import rcf_amd
    return rcf_amd


@pytest.fixture(scope='module')
def t15(golden_dir):
    return np.load(os.path.join(golden_dir, 'T15_eval_metrics.npz'))


def host_metrics(eval_utils, out, gt, lo, hi, dtype):
    '''the per-sample block of src/fusionnet_main.py:529-548 on rcf_amd.eval_utils, in `dtype`'''
    rows = []
    for s in range(out.shape[0]):
        o, g = np.squeeze(out[s]), np.squeeze(gt[s])
        mask = np.where(np.logical_and(g > 0, np.logical_and(g > lo, g < hi)))
        o, g = o[mask].astype(dtype), g[mask].astype(dtype)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            rows.append([eval_utils.mean_abs_err(1000.0 * o, 1000.0 * g), eval_utils.root_mean_sq_err(1000.0 * o, 1000.0 * g),
                         eval_utils.inv_mean_abs_err(0.001 * o, 0.001 * g), eval_utils.inv_root_mean_sq_err(0.001 * o, 0.001 * g)])
    return np.array(rows, dtype=np.float64)


def test_eval_utils_match_the_reference_float32_results(pkg, t15):
    '''Same numpy expressions as the reference, so normally the same bits; numpy builds may block a pairwise sum differently, hence the
    pairwise-summation bound (ceil(log2 count) + 3) * 2^-24, relative.'''
    from rcf_amd import eval_utils, synth
    for name in ('root_mean_sq_err', 'mean_abs_err', 'inv_root_mean_sq_err', 'inv_mean_abs_err', 'mean_abs_rel_err'):
        assert callable(getattr(eval_utils, name))
    assert len(t15['cases']) == 13
    for i, (seed, n, h, w, density, sigma, lo, hi) in enumerate(t15['cases']):
        out, gt = synth.make_eval_case(int(seed), int(n), int(h), int(w), density, sigma)
        got = host_metrics(eval_utils, out, gt, lo, hi, np.float32)
        ref, cnt = t15['c%02d_ref32' % i], t15['c%02d_count' % i]
        for s in range(int(n)):
            if cnt[s] == 0:
                assert np.isnan(got[s]).all() and np.isnan(ref[s]).all()
                continue
            bound = (math.ceil(math.log2(cnt[s])) + 3) * 2.0 ** -24
            assert np.all(np.abs(got[s] - ref[s]) <= bound * np.abs(ref[s])), (i, s, got[s], ref[s])
    a, b = np.array([1.0, 2.0, 4.0]), np.array([2.0, 2.0, 5.0])
    assert eval_utils.mean_abs_rel_err(a, b) == pytest.approx((0.5 + 0.0 + 0.2) / 3)


def test_best_results_rule_and_log_lines_replay_the_recorded_validate_calls(pkg, t15, tmp_path, capsys):
    '''update_best_results + log_evaluation_results from the means the reference logged: the dictionaries it returned (updated at
    steps 100, 300 and -- with exactly three of four metrics improved -- 400; kept at 200) and the text it appended to log_path.'''
    from rcf_amd.evaluation import log_evaluation_results, update_best_results
    best = {'step': -1, 'mae': np.inf, 'rmse': np.inf, 'imae': np.inf, 'irmse': np.inf}
    log_path = str(tmp_path / 'new_dir' / 'results.txt')      # the directory does not exist yet
    n_improved = []
    for c, means in enumerate(t15['validate_means']):
        step = 100 * (c + 1)
        n_improved.append(sum(1 for k, key in enumerate(('mae', 'rmse', 'imae', 'irmse')) if np.round(means[k], 2) <= np.round(best[key], 2)))
        log_evaluation_results('Validation results', *means, step=step, log_path=log_path)
        assert update_best_results(best, step, *means) is best
        log_evaluation_results('Best results', best['mae'], best['rmse'], best['imae'], best['irmse'], step=best['step'], log_path=log_path)
        assert [best['step'], best['mae'], best['rmse'], best['imae'], best['irmse']] == t15['validate_best'][c].tolist()
    assert n_improved == [4, 0, 4, 3]
    assert [int(b[0]) for b in t15['validate_best']] == [100, 100, 300, 400]
    text = open(log_path).read()
    assert text == str(t15['validate_log'])
    assert capsys.readouterr().out == text                    # the same lines go to the console
    # two of four is not enough
    best2 = dict(best)
    update_best_results(best2, 500, best['mae'] - 1, best['rmse'] - 1, best['imae'] + 1, best['irmse'] + 1)
    assert best2 == best


def _gather_worker(rank, world, port, tmpdir, total):
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    import rcf_amd  # noqa: F401
    from rcf_amd.evaluation import gather_sharded
    n_local = (total + world - 1) // world
    idx = [(rank + k * world) % total for k in range(n_local)]     # DistributedSampler(shuffle=False, drop_last=False): the tail wraps round
    rows = torch.tensor([[float(i), 10.0 * i, 0.5 * i, -float(i), 100.0 + i] for i in idx], dtype=torch.float64)
    full = gather_sharded(rows, total)
    torch.save(full, os.path.join(tmpdir, 'g%d.pt' % rank))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
@pytest.mark.parametrize('world', [2, 3])
def test_data_parallel_gather_sharded_restores_the_data_set_order(pkg, tmp_path, world):
    '''7 samples over 2 and 3 gloo ranks: rows back in data-set order, the sampler's padding dropped, every rank the same tensor.'''
    import torch.multiprocessing as mp
    total = 7
    port = 29300 + (os.getpid() % 2000) + world
    mp.spawn(_gather_worker, args=(world, port, str(tmp_path), total), nprocs=world, join=True)
    want = torch.tensor([[float(i), 10.0 * i, 0.5 * i, -float(i), 100.0 + i] for i in range(total)], dtype=torch.float64)
    for r in range(world):
        got = torch.load(os.path.join(str(tmp_path), 'g%d.pt' % r))
        assert got.shape == (total, 5) and torch.equal(got, want)


def test_eval_metrics_export_is_declared_bound_and_rejects_bad_arguments(pkg):
    from rcf_amd import _lib, ops
    header = open(os.path.join(ROOT, 'include', 'rcf_hip.h')).read()
    assert re.search(r'\bint rcf_eval_metrics\s*\(', header)
    m = re.search(r'#define RCF_EVAL_BLOCKS (\d+)', header)
    assert m and int(m.group(1)) == _lib.RCF_EVAL_BLOCKS
    assert 'RCF_EVAL_WORKSPACE_DOUBLES(n) ((size_t)(n) * 5 * RCF_EVAL_BLOCKS)' in header
    assert ops.eval_workspace_doubles(3) == 3 * 5 * _lib.RCF_EVAL_BLOCKS
    assert 'rcf_eval_metrics' in _lib._SIGNATURES
    fn = _lib.load().rcf_eval_metrics
    fake = 0x10000      # a non-null "device pointer": a rejected call must not dereference it (and there is no device here)
    good = dict(depth=fake, gt=fake, n=2, pix=100, lo=0.0, hi=100.0, ws=fake, res=fake, cap=4, cur=fake, st=None)
    assert fn(None, None, 0, 0, 0.0, 0.0, None, None, 0, None, None) == -1
    for key, bad in (('depth', None), ('gt', None), ('ws', None), ('res', None), ('cur', None), ('n', 0), ('n', -1), ('pix', 0),
                     ('pix', -5), ('cap', 0), ('cap', -2)):
        args = dict(good)
        args[key] = bad
        assert fn(*args.values()) == -1, key      # RCF_EINVAL, before any HIP call


def test_evaluation_has_no_cpu_path(pkg):
    from rcf_amd import _lib, ops
    from rcf_amd.evaluation import MetricsAccumulator
    with pytest.raises(_lib.RcfError):
        MetricsAccumulator(4, 0.0, 100.0, torch.device('cpu'))
    z = torch.zeros(2, 1, 8, 8)
    with pytest.raises(_lib.RcfError):
        ops.eval_metrics(z, z, 0.0, 100.0, torch.zeros(ops.eval_workspace_doubles(2), dtype=torch.float64),
                         torch.zeros(4, 5, dtype=torch.float64), torch.zeros(2, dtype=torch.int32))
