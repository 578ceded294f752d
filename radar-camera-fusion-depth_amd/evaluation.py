'''
Validation and test-time evaluation with the metrics computed on the device.

The reference's validate() (src/fusionnet_main.py:476-606) and the evaluation block of run() (:787-843, :881-896) copy every
output and ground truth to the host and reduce them there, with a device synchronise per sample.  Here each sample's four
numbers are left in a device buffer by rcf_eval_metrics (include/rcf_hip.h) and the host waits once, after the last sample:

    from rcf_amd.evaluation import validate          # replaces fusionnet_main.validate, same arguments and return value

MetricsAccumulator is the piece for custom loops and for captured inference: update() only enqueues, so it can follow
model.forward inside torch.cuda.graph and every replay fills the next rows.
'''

import os

import numpy as np
import torch
import torch.distributed as dist

from . import _lib, ops

METRICS = ('mae', 'rmse', 'imae', 'irmse')


def log(s, filepath=None, to_console=True):
    '''print and append to filepath (src/log_utils.py:20-42); the file's directory is created when missing'''
    if to_console:
        print(s)
    if filepath is not None:
        dirpath = os.path.dirname(filepath)
        if dirpath:
            os.makedirs(dirpath, exist_ok=True)
        with open(filepath, 'a+') as o:
            o.write(s + '\n')


def log_evaluation_results(title, mae, rmse, imae, irmse, step=-1, log_path=None):
    '''The three lines of src/fusionnet_main.py:1101-1120.'''
    log(title + ':', log_path)
    log('{:>8}  {:>8}  {:>8}  {:>8}  {:>8}'.format('Step', 'MAE', 'RMSE', 'iMAE', 'iRMSE'), log_path)
    log('{:8}  {:8.3f}  {:8.3f}  {:8.3f}  {:8.3f}'.format(step, mae, rmse, imae, irmse), log_path)


def update_best_results(best_results, step, mae, rmse, imae, irmse):
    '''The checkpoint-selection rule of src/fusionnet_main.py:580-595: a metric counts as improved when, rounded to two decimals, it
    is <= the best one; more than two of the four replace all of best_results (in place).  Returns best_results.'''
    new = dict(zip(METRICS, (mae, rmse, imae, irmse)))
    n_improve = sum(1 for k in METRICS if np.round(new[k], 2) <= np.round(best_results[k], 2))
    if n_improve > 2:
        best_results['step'] = step
        best_results.update(new)
    return best_results


class MetricsAccumulator(object):
    '''
    Per-sample MAE / RMSE / iMAE / iRMSE (+ valid-pixel count) of up to n_sample samples, held on the device.

    update() enqueues rcf_eval_metrics on the current stream and returns nothing: no synchronise, and no allocation once the
    workspace covers the batch.  max_batch reserves the workspace up front; a larger batch grows it, except while a graph is being
    captured -- memory allocated there would belong to the capture's pool -- where update() raises and asks for max_batch.  The next
    free row is a device integer, so a recorded update() fills new rows on every replay.  rows() / per_sample() are the one place
    that waits for the device.
    '''

    def __init__(self, n_sample, min_evaluate_depth, max_evaluate_depth, device, max_batch=1):
        device = torch.device(device)
        if device.type != 'cuda':
            raise _lib.RcfError('MetricsAccumulator computes on the GPU; got device %s -- there is no CPU path '
                                '(rcf_amd.eval_utils holds the host functions of the reference)' % device)
        if n_sample <= 0:
            raise ValueError('n_sample must be positive')
        self.n_sample = int(n_sample)
        self.min_evaluate_depth = float(min_evaluate_depth)
        self.max_evaluate_depth = float(max_evaluate_depth)
        self.device = device
        self.results = torch.zeros((self.n_sample, 5), dtype=torch.float64, device=device)
        self.cursor = torch.zeros(2, dtype=torch.int32, device=device)
        self.workspace = torch.empty(ops.eval_workspace_doubles(max(1, max_batch)), dtype=torch.float64, device=device)

    def reset(self):
        self.cursor.zero_()

    def update(self, output_depth, ground_truth):
        n = output_depth.shape[0] if output_depth.dim() > 0 else 0
        if self.workspace.numel() < ops.eval_workspace_doubles(n):
            if torch.cuda.is_current_stream_capturing():
                raise _lib.RcfError('MetricsAccumulator.update: a batch of %d needs a larger workspace, which is not allocated while a '
                                    'graph is being captured -- construct the accumulator with max_batch=%d' % (n, n))
            self.workspace = torch.empty(ops.eval_workspace_doubles(n), dtype=torch.float64, device=self.device)
        ops.eval_metrics(output_depth, ground_truth, self.min_evaluate_depth, self.max_evaluate_depth, self.workspace, self.results,
                         self.cursor)

    def rows(self, on_device=False):
        '''n_sample x 5 float64 tensor (mae, rmse, imae, irmse, count per sample), on the CPU or (on_device: for a collective of a
        device-only backend) a copy on the device.  Synchronises; raises RcfError when samples were dropped for lack of room or
        fewer than n_sample were added.'''
        filled, dropped = self.cursor.cpu().tolist()
        if dropped:
            raise _lib.RcfError('MetricsAccumulator(n_sample=%d): %d samples did not fit and were dropped' % (self.n_sample, dropped))
        if filled != self.n_sample:
            raise _lib.RcfError('MetricsAccumulator(n_sample=%d): only %d samples were added' % (self.n_sample, filled))
        return self.results.clone() if on_device else self.results.cpu()

    def per_sample(self):
        '''(mae, rmse, imae, irmse, count): float64 numpy arrays of n_sample elements, in the order the samples were added.'''
        return split_rows(self.rows())

    def means(self):
        '''np.mean over the samples of each metric (src/fusionnet_main.py:551-554).'''
        return tuple(np.mean(a) for a in self.per_sample()[:4])


def split_rows(rows):
    r = rows.cpu().numpy() if torch.is_tensor(rows) else np.asarray(rows)
    return tuple(np.ascontiguousarray(r[:, k]) for k in range(5))


def gather_sharded(rows, n_sample_total, group=None):
    '''
    Per-sample rows of a data set evaluated by the ranks of a process group, back in data-set order.  Rank r holds the rows of the
    samples r, r + world, ... (DistributedSampler(shuffle=False, drop_last=False): every rank ceil(n_sample_total / world) of them,
    the tail padded with repeated samples).  All-gathers them, interleaves and drops the padding: every rank returns the same
    n_sample_total x K tensor, where `rows` lives.  That is for the caller to choose by the group's backend: gloo moves CPU and
    device tensors, nccl (RCCL) device tensors only -- validate() and evaluate() gather on the device.
    '''
    world = dist.get_world_size(group)
    n_local = (n_sample_total + world - 1) // world
    if rows.dim() != 2 or rows.shape[0] != n_local:
        raise ValueError('gather_sharded: expected %d rows on every rank (%d samples over %d ranks); got %s'
                         % (n_local, n_sample_total, world, tuple(rows.shape)))
    rows = rows.contiguous()
    parts = [torch.empty_like(rows) for _ in range(world)]
    dist.all_gather(parts, rows, group=group)
    return torch.stack(parts, dim=1).reshape(n_local * world, rows.shape[1])[:n_sample_total].contiguous()


def _count_samples(dataloader):
    '''Samples this process will see, which sizes the result buffer before the loop: a torch DataLoader's sampler knows (drop_last
    honoured); a list or tuple of batches is counted; any other iterable is taken to yield one sample per item, as the reference's
    loaders do -- with larger batches there, pass n_sample to validate() / evaluate().'''
    sampler = getattr(dataloader, 'sampler', None)
    if sampler is not None and hasattr(sampler, '__len__'):
        n = len(sampler)
        batch_size = getattr(dataloader, 'batch_size', None)
        if getattr(dataloader, 'drop_last', False) and batch_size:
            n = (n // batch_size) * batch_size
        return n
    if isinstance(dataloader, (list, tuple)):
        return sum(int(item[0].shape[0]) for item in dataloader)
    return len(dataloader)


def _sharded(n_sample_total):
    return n_sample_total is not None and dist.is_available() and dist.is_initialized()


def _run_loop(model, dataloader, transforms, min_evaluate_depth, max_evaluate_depth, device, on_sample=None, n_sample=None):
    '''forward + MetricsAccumulator.update over the loader (src/fusionnet_main.py:501-548, :796-843); nothing here waits for the device.'''
    device = torch.device(device)
    acc = MetricsAccumulator(_count_samples(dataloader) if n_sample is None else n_sample, min_evaluate_depth, max_evaluate_depth, device)
    with torch.no_grad():
        for idx, inputs in enumerate(dataloader):
            image, depth, response, ground_truth = [in_.to(device) for in_ in inputs]
            [image] = transforms.transform(images_arr=[image], random_transform_probability=0.0)
            input_depth = torch.cat([depth, response], dim=1)
            output_depth = model.forward(image=image, input_depth=input_depth)
            acc.update(output_depth.contiguous(), ground_truth.contiguous())
            if on_sample is not None:
                on_sample(idx, image, depth, response, ground_truth, output_depth)
    return acc


def _collect(acc, n_sample_total):
    '''the rows of the whole data set on the host; under a process group gathered ON THE DEVICE (RCCL serves device tensors only) and
    copied afterwards'''
    if _sharded(n_sample_total):
        return split_rows(gather_sharded(acc.rows(on_device=True), n_sample_total).cpu())
    return split_rows(acc.rows())


def validate(model, dataloader, transforms, step, best_results, min_evaluate_depth, max_evaluate_depth, device, summary_writer,
             n_summary_display=4, n_summary_display_interval=250, log_path=None, n_sample_total=None, n_sample=None):
    '''
    fusionnet_main.validate (src/fusionnet_main.py:476-606): the same arguments, log lines, log_summary call and return value
    (best_results, updated in place).  The loader may yield batches of any size -- a torch DataLoader or a list of batches is
    counted beforehand, for any other iterable whose items hold more than one sample give n_sample, the number of samples this
    process will see; `model` is anything with
    .forward(image=, input_depth=) -- a FusionNetModel in eval(), or a small object around a captured `run`.  The host waits for
    the device once, after the last sample.

    n_sample_total: under an initialised process group, the size of the whole validation set, of which this rank has evaluated the
    samples rank, rank + world, ... (DistributedSampler(shuffle=False)).  Every rank then gets the metrics of the whole set --
    the same bits as a one-process run -- and only rank 0 writes the log.
    '''
    summary = []

    def keep(idx, image, depth, response, ground_truth, output_depth):
        if (idx % n_summary_display_interval) == 0 and summary_writer is not None:
            summary.append((image, depth, response, ground_truth, output_depth.clone()))   # a captured forward reuses its output tensor

    acc = _run_loop(model, dataloader, transforms, min_evaluate_depth, max_evaluate_depth, device, keep, n_sample)
    mae, rmse, imae, irmse = (np.mean(a) for a in _collect(acc, n_sample_total)[:4])

    if summary_writer is not None:
        image, depth, response, ground_truth, output_depth = (torch.cat(t, dim=0) for t in zip(*summary))
        model.log_summary(
            summary_writer=summary_writer, tag='eval', step=step, image=image, input_depth=depth, input_response=response,
            output_depth=output_depth, ground_truth=ground_truth, scalars={'mae': mae, 'rmse': rmse, 'imae': imae, 'irmse': irmse},
            n_display=n_summary_display)

    writes = not _sharded(n_sample_total) or dist.get_rank() == 0
    if writes:
        log_evaluation_results(title='Validation results', mae=mae, rmse=rmse, imae=imae, irmse=irmse, step=step, log_path=log_path)
    update_best_results(best_results, step, mae, rmse, imae, irmse)
    if writes:
        log_evaluation_results(title='Best results', mae=best_results['mae'], rmse=best_results['rmse'], imae=best_results['imae'],
                               irmse=best_results['irmse'], step=best_results['step'], log_path=log_path)
    return best_results


def evaluate(model, dataloader, transforms, min_evaluate_depth, max_evaluate_depth, device, step=-1, log_path=None,
             n_sample_total=None, n_sample=None):
    '''
    The evaluation part of run() with ground truth available (src/fusionnet_main.py:787-843, :881-896): forwards every sample, logs
    'Evaluation results' and returns ((mae, rmse, imae, irmse), per_sample) with per_sample = (mae, rmse, imae, irmse, count) arrays
    in data-set order.  Writing the output images (save_outputs) is not part of this.  n_sample_total and n_sample as in validate().
    '''
    acc = _run_loop(model, dataloader, transforms, min_evaluate_depth, max_evaluate_depth, device, None, n_sample)
    per_sample = _collect(acc, n_sample_total)
    means = tuple(np.mean(a) for a in per_sample[:4])
    if not _sharded(n_sample_total) or dist.get_rank() == 0:
        log_evaluation_results(title='Evaluation results', mae=means[0], rmse=means[1], imae=means[2], irmse=means[3], step=step,
                               log_path=log_path)
    return means, per_sample
