'''
The host-side error measures of the reference's evaluation (src/eval_utils.py), under its names and argument order
(src = prediction, tgt = ground truth), on numpy arrays: what a script that imports `eval_utils` keeps calling.  The
arithmetic runs in the arrays' own dtype, like the reference's.  The device-side counterpart, which validation and
evaluation use here, is rcf_amd.evaluation.MetricsAccumulator.
'''

import numpy as np


def root_mean_sq_err(src, tgt):
    '''sqrt(mean((tgt - src)^2))  (src/eval_utils.py:17-29)'''
    return np.sqrt(np.mean((tgt - src) ** 2))


def mean_abs_err(src, tgt):
    '''mean(|tgt - src|)  (src/eval_utils.py:31-43)'''
    return np.mean(np.abs(tgt - src))


def inv_root_mean_sq_err(src, tgt):
    '''sqrt(mean((1/tgt - 1/src)^2))  (src/eval_utils.py:45-57)'''
    return np.sqrt(np.mean(((1.0 / tgt) - (1.0 / src)) ** 2))


def inv_mean_abs_err(src, tgt):
    '''mean(|1/tgt - 1/src|)  (src/eval_utils.py:59-71)'''
    return np.mean(np.abs((1.0 / tgt) - (1.0 / src)))


def mean_abs_rel_err(src, tgt):
    '''mean(|src - tgt| / tgt)  (src/eval_utils.py:73-85)'''
    return np.mean(np.abs(src - tgt) / tgt)
