'''
One descriptor recipe per entry of every convolution configuration table (csrc/rcf_conv_impl.h: FwdList, SplitList, DmaList,
PwList, WgList, WsList, WtList of the fp32-tensor and the bf16-tensor translation units).  Each row names the entry it must reach,
as rcf_conv2d_config reports it: (unit, family, index).  test_conv_config.py checks on the CPU that every row reaches exactly its
entry and that the rows cover every entry; test_conv_config_gpu.py runs every row against an fp64 reference.  A new table entry
therefore needs a row here (or a reasoned place in EXCEPTIONS).

A row: unit ('f32' / 'b16'), family (RCF_FAM_*), index, form (FORMS), precision (an ops.set_precision name), ksize, stride,
c1, c2, c_out, n, h, w (the forward problem the form is derived from: input n x h x w with c1 (+ c2) channels, c_out outputs; the
up-2x forms: the source extent), env (per-call switches, ENV_SWITCHES).
'''

import collections

Case = collections.namedtuple('Case', 'unit family index form prec k s c1 c2 co n h w env')

# switches the selection reads on every call (RCF_UP2X_MERGED and RCF_XCD_BANDS are read once per process: not usable here)
ENV_SWITCHES = ('RCF_CONV_SPLIT', 'RCF_S2_SPLIT', 'RCF_B16_DMA', 'RCF_F32_PW', 'RCF_B16_PW', 'RCF_WGRAD_TR', 'RCF_NO_VT')

FAMILY_NAMES = ('fwd', 'split', 'dma', 'pw', 'wg', 'ws', 'wt')

# form -> (ksize, stride) of the forward problem it is built from
FORM_KS = {
    'fwd': [(1, 1), (1, 2), (3, 1), (3, 2), (7, 2)],
    'stem4': [(4, 1)],                # the 7x7 stem as a 4x4 convolution of the space-to-depth image (c1 = 16)
    'dgrad': [(1, 1), (1, 2), (3, 1), (3, 2)],   # input gradient of source 1 (all c1 channels), accumulating
    'pw_s2_dgrad': [(1, 2)],          # 1x1 stride-2 input gradient at dZ's resolution, accumulating
    'up2x': [(2, 1)],                 # one output phase (0, 1) of conv3x3(up2x(x))
    'up2x_m': [(2, 1)],               # the four output phases in one launch (phase_sum 2)
    'up2x_dgrad': [(2, 1)],           # one input phase (1, 0) of the up-2x input gradient, accumulating
    'up2x_dgrad_m': [(2, 1)],         # the four phases summed in one launch (phase_sum 1), accumulating
    's2_dgrad': [(3, 2)],             # one output phase (1, 1) of a 3x3 stride-2 input gradient, accumulating
    's2_dgrad_m': [(3, 2)],           # the four output phases in one launch (phase_sum 3), accumulating
    'wgrad': [(1, 1), (1, 2), (3, 1), (3, 2), (7, 2)],   # rcf_conv2d_wgrad of the 'fwd' descriptor
    'up2x_wgrad': [(2, 1)],           # weight gradient of one up-2x phase
    'up2x_wgrad_m': [(2, 1)],         # of the four up-2x phases in one launch (phase pairs)
    's2_wgrad': [(3, 2)],             # of one stride-2 phase (0, 1)
    's2_wgrad_m': [(3, 2)],           # of the four stride-2 phases in one launch (phase_sum 1)
}
FORMS = tuple(FORM_KS)
FORWARD_FORMS = ('fwd', 'stem4', 'up2x', 'up2x_m')   # a layer's forward pass: the launches that take BatchNorm statistics
WGRAD_FORMS = ('wgrad', 'up2x_wgrad', 'up2x_wgrad_m', 's2_wgrad', 's2_wgrad_m')


def unit_of(prec):
    return 'b16' if prec == 'bf16' else 'f32'


def role_of(form):
    '''RCF_ROLE_WGRAD for the weight-gradient forms, else RCF_ROLE_FWD'''
    return 1 if form in WGRAD_FORMS else 0


def make_desc(ops, c, accumulate=None):
    '''The descriptor of row c under the current ops.set_precision (c.prec); accumulate overrides the form's default (the input
    gradients accumulate, the others write).'''
    k, s, c1, c2, co, n, h, w = c.k, c.s, c.c1, c.c2, c.co, c.n, c.h, c.w
    acc = ('dgrad' in c.form) if accumulate is None else bool(accumulate)
    f = c.form
    if f in ('fwd', 'wgrad'):
        d = ops.make_fwd_desc(n, h, w, c1, c2, co, k, s)
    elif f == 'stem4':
        d = ops.make_stem_s2d_desc(n, h, w, co, f32=c.prec != 'bf16')
    elif f == 'dgrad':
        d = ops.make_dgrad_desc(ops.make_fwd_desc(n, h, w, c1, 0, co, k, s), 0, c1, acc)
    elif f == 'pw_s2_dgrad':
        d = ops.make_pw_s2_dgrad_desc(ops.make_fwd_desc(n, h, w, c1, 0, co, 1, 2), acc)
    elif f in ('up2x', 'up2x_wgrad'):
        d = ops.make_up2x_fwd_desc(n, h, w, c1, co, 0, 1)
    elif f in ('up2x_m', 'up2x_wgrad_m'):
        d = ops.make_up2x_fwd_desc(n, h, w, c1, co, 0, 0, phase_out=True)
    elif f == 'up2x_dgrad':
        d = ops.make_up2x_dgrad_desc(n, h, w, c1, co, 1, 0, acc)
    elif f == 'up2x_dgrad_m':
        d = ops.make_up2x_dgrad_desc(n, h, w, c1, co, 0, 0, acc, phase_sum=True)
    elif f == 's2_dgrad':
        d = ops.make_s2_dgrad_desc(ops.make_fwd_desc(n, h, w, c1, 0, co, 3, 2), 1, 1, acc)
    elif f == 's2_dgrad_m':
        d = ops.make_s2_dgrad_desc(ops.make_fwd_desc(n, h, w, c1, 0, co, 3, 2), 0, 0, acc, phase_out=True)
    elif f == 's2_wgrad':
        d = ops.make_s2_wgrad_desc(ops.make_fwd_desc(n, h, w, c1, 0, co, 3, 2), 0, 1)
    elif f == 's2_wgrad_m':
        d = ops.make_s2_wgrad_desc(ops.make_fwd_desc(n, h, w, c1, 0, co, 3, 2), 0, 0, all_phases=True)
    else:
        raise ValueError(f)
    d.accumulate = 1 if acc else 0
    return d


# entries no descriptor reaches: (unit, family, index) -> reason
EXCEPTIONS = {
}

CASES = [Case(*r) for r in [
    ('b16', 0, 0, 'fwd', 'bf16', 3, 1, 12, 0, 4, 2, 7, 23, (('RCF_CONV_SPLIT', '0'),)),
    ('b16', 0, 1, 'fwd', 'bf16', 3, 1, 12, 0, 40, 2, 7, 23, (('RCF_CONV_SPLIT', '0'),)),
    ('b16', 0, 2, 'fwd', 'bf16', 3, 1, 12, 0, 4, 1, 9, 13, (('RCF_CONV_SPLIT', '0'),)),
    ('b16', 0, 3, 'fwd', 'bf16', 3, 1, 12, 0, 40, 1, 9, 13, (('RCF_CONV_SPLIT', '0'),)),
    ('b16', 0, 4, 'fwd', 'bf16', 3, 1, 12, 0, 4, 1, 21, 37, (('RCF_CONV_SPLIT', '0'),)),
    ('b16', 0, 5, 'fwd', 'bf16', 3, 1, 12, 0, 40, 1, 21, 37, (('RCF_CONV_SPLIT', '0'),)),
    ('b16', 0, 6, 'fwd', 'bf16', 3, 1, 4, 0, 4, 2, 7, 23, ()),
    ('b16', 0, 7, 'fwd', 'bf16', 3, 1, 4, 0, 40, 2, 7, 23, ()),
    ('b16', 0, 8, 'fwd', 'bf16', 3, 1, 4, 0, 4, 1, 9, 13, ()),
    ('b16', 0, 9, 'fwd', 'bf16', 3, 1, 4, 0, 40, 1, 9, 13, ()),
    ('b16', 0, 10, 'fwd', 'bf16', 3, 2, 4, 0, 4, 1, 9, 13, ()),
    ('b16', 0, 11, 'fwd', 'bf16', 3, 2, 4, 0, 40, 1, 9, 13, ()),
    ('b16', 0, 12, 'fwd', 'bf16', 3, 2, 4, 0, 4, 1, 41, 9, ()),
    ('b16', 0, 13, 'fwd', 'bf16', 3, 2, 4, 0, 40, 1, 41, 9, ()),
    ('b16', 0, 14, 'fwd', 'bf16', 1, 2, 32, 0, 4, 1, 9, 13, (('RCF_B16_PW', '0'),)),
    ('b16', 0, 15, 'fwd', 'bf16', 1, 2, 32, 0, 40, 1, 9, 13, (('RCF_B16_PW', '0'),)),
    ('b16', 0, 16, 'fwd', 'bf16', 1, 1, 32, 0, 4, 1, 9, 13, (('RCF_B16_PW', '0'),)),
    ('b16', 0, 17, 'fwd', 'bf16', 1, 1, 32, 0, 40, 1, 9, 13, (('RCF_B16_PW', '0'),)),
    ('b16', 0, 18, 'fwd', 'bf16', 1, 2, 4, 0, 4, 1, 9, 13, ()),
    ('b16', 0, 19, 'fwd', 'bf16', 1, 2, 4, 0, 40, 1, 9, 13, ()),
    ('b16', 0, 20, 'fwd', 'bf16', 1, 1, 4, 0, 4, 1, 9, 13, ()),
    ('b16', 0, 21, 'fwd', 'bf16', 1, 1, 4, 0, 40, 1, 9, 13, ()),
    ('b16', 0, 22, 's2_dgrad', 'bf16', 3, 2, 4, 0, 4, 1, 9, 13, ()),
    ('b16', 0, 23, 's2_dgrad', 'bf16', 3, 2, 48, 0, 4, 1, 9, 13, ()),
    ('b16', 0, 24, 'up2x', 'bf16', 2, 1, 4, 0, 4, 1, 9, 13, ()),
    ('b16', 0, 25, 'up2x', 'bf16', 2, 1, 4, 0, 40, 1, 9, 13, ()),
    ('b16', 0, 26, 'fwd', 'bf16', 7, 2, 4, 0, 4, 1, 9, 13, ()),
    ('b16', 0, 27, 'fwd', 'bf16', 7, 2, 4, 0, 4, 1, 41, 9, ()),
    ('b16', 1, 0, 'fwd', 'bf16', 3, 1, 12, 0, 4, 1, 9, 13, ()),
    ('b16', 1, 1, 'fwd', 'bf16', 3, 1, 12, 0, 96, 1, 261, 127, ()),
    ('b16', 1, 2, 'fwd', 'bf16', 3, 1, 12, 0, 4, 2, 9, 13, ()),
    ('b16', 1, 3, 'fwd', 'bf16', 3, 1, 12, 0, 96, 2, 129, 131, ()),
    ('b16', 1, 4, 'fwd', 'bf16', 3, 1, 12, 0, 40, 2, 7, 23, ()),
    ('b16', 1, 5, 'fwd', 'bf16', 3, 1, 12, 0, 40, 1, 9, 13, ()),
    ('b16', 1, 6, 's2_dgrad', 'bf16', 3, 2, 4, 0, 16, 1, 9, 13, (('RCF_B16_DMA', '0'),)),
    ('b16', 1, 7, 's2_dgrad', 'bf16', 3, 2, 48, 0, 16, 1, 9, 13, (('RCF_B16_DMA', '0'),)),
    ('b16', 1, 8, 'up2x', 'bf16', 2, 1, 16, 0, 4, 1, 9, 13, (('RCF_B16_DMA', '0'),)),
    ('b16', 1, 9, 'up2x', 'bf16', 2, 1, 16, 0, 40, 1, 9, 13, (('RCF_B16_DMA', '0'),)),
    ('b16', 1, 10, 'fwd', 'bf16', 3, 2, 16, 0, 4, 1, 9, 13, (('RCF_B16_DMA', '0'),)),
    ('b16', 1, 11, 'fwd', 'bf16', 3, 2, 16, 0, 40, 1, 9, 13, (('RCF_B16_DMA', '0'),)),
    ('b16', 1, 12, 'fwd', 'bf16', 3, 2, 16, 0, 4, 1, 41, 9, (('RCF_B16_DMA', '0'),)),
    ('b16', 1, 13, 'fwd', 'bf16', 3, 2, 16, 0, 40, 1, 41, 9, (('RCF_B16_DMA', '0'),)),
    ('b16', 2, 0, 'fwd', 'bf16', 3, 1, 16, 0, 96, 1, 261, 127, ()),
    ('b16', 2, 1, 'fwd', 'bf16', 3, 1, 16, 0, 96, 2, 129, 131, ()),
    ('b16', 2, 2, 'fwd', 'bf16', 3, 1, 16, 0, 4, 1, 9, 13, ()),
    ('b16', 2, 3, 'fwd', 'bf16', 3, 1, 16, 0, 4, 2, 9, 13, ()),
    ('b16', 2, 4, 'fwd', 'bf16', 3, 1, 16, 0, 40, 2, 7, 23, ()),
    ('b16', 2, 5, 'fwd', 'bf16', 3, 1, 16, 0, 40, 1, 9, 13, ()),
    ('b16', 2, 6, 's2_dgrad', 'bf16', 3, 2, 48, 0, 16, 1, 9, 13, ()),
    ('b16', 2, 7, 'up2x', 'bf16', 2, 1, 16, 0, 40, 1, 9, 13, ()),
    ('b16', 2, 8, 's2_dgrad', 'bf16', 3, 2, 4, 0, 16, 1, 9, 13, ()),
    ('b16', 2, 9, 'up2x', 'bf16', 2, 1, 16, 0, 4, 1, 9, 13, ()),
    ('b16', 2, 10, 'up2x_m', 'bf16', 2, 1, 16, 0, 4, 1, 9, 13, ()),
    ('b16', 2, 11, 'up2x_m', 'bf16', 2, 1, 16, 0, 40, 1, 9, 13, ()),
    ('b16', 2, 12, 's2_dgrad_m', 'bf16', 3, 2, 4, 0, 16, 1, 9, 13, ()),
    ('b16', 2, 13, 's2_dgrad_m', 'bf16', 3, 2, 48, 0, 16, 1, 9, 13, ()),
    ('b16', 2, 14, 'fwd', 'bf16', 3, 2, 16, 0, 40, 2, 7, 23, ()),
    ('b16', 2, 15, 'fwd', 'bf16', 3, 2, 16, 0, 40, 1, 9, 13, ()),
    ('b16', 2, 16, 'fwd', 'bf16', 3, 2, 16, 0, 4, 2, 7, 23, ()),
    ('b16', 2, 17, 'fwd', 'bf16', 3, 2, 16, 0, 4, 1, 9, 13, ()),
    ('b16', 2, 18, 'stem4', 'bf16', 4, 1, 4, 0, 4, 1, 9, 13, ()),
    ('b16', 2, 19, 'stem4', 'bf16', 4, 1, 4, 0, 4, 1, 41, 9, ()),
    ('b16', 3, 0, 'fwd', 'bf16', 1, 1, 16, 0, 4, 1, 9, 13, ()),
    ('b16', 3, 1, 'fwd', 'bf16', 1, 1, 16, 0, 40, 1, 9, 13, ()),
    ('b16', 3, 2, 'fwd', 'bf16', 1, 1, 16, 0, 96, 1, 9, 13, ()),
    ('b16', 3, 3, 'fwd', 'bf16', 1, 1, 16, 0, 128, 1, 9, 13, ()),
    ('b16', 3, 4, 'fwd', 'bf16', 1, 1, 32, 0, 4, 1, 9, 13, ()),
    ('b16', 3, 5, 'fwd', 'bf16', 1, 1, 32, 0, 40, 1, 9, 13, ()),
    ('b16', 3, 6, 'fwd', 'bf16', 1, 1, 32, 0, 96, 1, 9, 13, ()),
    ('b16', 3, 7, 'fwd', 'bf16', 1, 1, 32, 0, 128, 1, 9, 13, ()),
    ('b16', 3, 8, 'fwd', 'bf16', 1, 1, 48, 0, 4, 1, 9, 13, ()),
    ('b16', 3, 9, 'fwd', 'bf16', 1, 1, 48, 0, 40, 1, 9, 13, ()),
    ('b16', 3, 10, 'fwd', 'bf16', 1, 1, 64, 0, 4, 1, 9, 13, ()),
    ('b16', 3, 11, 'fwd', 'bf16', 1, 1, 64, 0, 40, 1, 9, 13, ()),
    ('b16', 3, 12, 'fwd', 'bf16', 1, 1, 64, 0, 96, 1, 9, 13, ()),
    ('b16', 3, 13, 'fwd', 'bf16', 1, 1, 128, 0, 4, 1, 9, 13, ()),
    ('b16', 3, 14, 'fwd', 'bf16', 1, 1, 128, 0, 40, 1, 9, 13, ()),
    ('b16', 3, 15, 'fwd', 'bf16', 1, 1, 256, 0, 4, 1, 9, 13, ()),
    ('b16', 4, 0, 'wgrad', 'bf16', 3, 1, 4, 0, 4, 2, 7, 23, (('RCF_CONV_SPLIT', '0'),)),
    ('b16', 4, 1, 'wgrad', 'bf16', 3, 1, 4, 0, 4, 1, 9, 13, (('RCF_CONV_SPLIT', '0'),)),
    ('b16', 4, 2, 'wgrad', 'bf16', 3, 2, 4, 0, 4, 2, 7, 23, ()),
    ('b16', 4, 3, 'wgrad', 'bf16', 3, 2, 4, 0, 4, 1, 9, 13, ()),
    ('b16', 4, 4, 'wgrad', 'bf16', 1, 2, 4, 0, 4, 1, 9, 13, (('RCF_CONV_SPLIT', '0'),)),
    ('b16', 4, 5, 'wgrad', 'bf16', 1, 1, 4, 0, 4, 1, 9, 13, (('RCF_CONV_SPLIT', '0'),)),
    ('b16', 4, 6, 's2_wgrad', 'bf16', 3, 2, 4, 0, 4, 1, 9, 13, (('RCF_CONV_SPLIT', '0'),)),
    ('b16', 4, 7, 'up2x_wgrad', 'bf16', 2, 1, 4, 0, 4, 1, 9, 13, (('RCF_CONV_SPLIT', '0'),)),
    ('b16', 4, 8, 'wgrad', 'bf16', 7, 2, 4, 0, 4, 1, 9, 13, ()),
    ('b16', 4, 9, 'wgrad', 'bf16', 7, 2, 4, 0, 4, 1, 41, 9, ()),
    ('b16', 5, 0, 'wgrad', 'bf16', 3, 1, 64, 0, 40, 1, 9, 13, (('RCF_WGRAD_TR', '0'),)),
    ('b16', 5, 1, 'wgrad', 'bf16', 3, 1, 4, 0, 40, 1, 9, 13, ()),
    ('b16', 5, 2, 'wgrad', 'bf16', 3, 1, 64, 0, 4, 1, 9, 13, ()),
    ('b16', 5, 3, 'wgrad', 'bf16', 3, 1, 4, 0, 4, 1, 9, 13, ()),
    ('b16', 5, 4, 'up2x_wgrad', 'bf16', 2, 1, 64, 0, 40, 1, 9, 13, (('RCF_WGRAD_TR', '0'),)),
    ('b16', 5, 5, 'up2x_wgrad', 'bf16', 2, 1, 4, 0, 40, 1, 9, 13, ()),
    ('b16', 5, 6, 'up2x_wgrad', 'bf16', 2, 1, 64, 0, 4, 1, 9, 13, ()),
    ('b16', 5, 7, 'up2x_wgrad', 'bf16', 2, 1, 4, 0, 4, 1, 9, 13, ()),
    ('b16', 5, 8, 'up2x_wgrad_m', 'bf16', 2, 1, 64, 0, 40, 1, 9, 13, ()),
    ('b16', 5, 9, 'up2x_wgrad_m', 'bf16', 2, 1, 16, 0, 40, 1, 9, 13, ()),
    ('b16', 5, 10, 'up2x_wgrad_m', 'bf16', 2, 1, 64, 0, 4, 1, 9, 13, ()),
    ('b16', 5, 11, 'up2x_wgrad_m', 'bf16', 2, 1, 16, 0, 4, 1, 9, 13, ()),
    ('b16', 5, 12, 'wgrad', 'bf16', 1, 2, 64, 0, 40, 1, 9, 13, ()),
    ('b16', 5, 13, 'wgrad', 'bf16', 1, 1, 4, 0, 40, 1, 9, 13, ()),
    ('b16', 5, 14, 'wgrad', 'bf16', 1, 1, 64, 0, 4, 1, 9, 13, ()),
    ('b16', 5, 15, 'wgrad', 'bf16', 1, 1, 4, 0, 4, 1, 9, 13, ()),
    ('b16', 6, 0, 'wgrad', 'bf16', 3, 1, 64, 0, 40, 1, 9, 13, ()),
    ('b16', 6, 1, 'wgrad', 'bf16', 3, 1, 8, 0, 40, 1, 9, 13, ()),
    ('b16', 6, 2, 'wgrad', 'bf16', 3, 1, 64, 0, 16, 1, 9, 13, ()),
    ('b16', 6, 3, 'wgrad', 'bf16', 3, 1, 8, 0, 16, 1, 9, 13, ()),
    ('b16', 6, 4, 'up2x_wgrad', 'bf16', 2, 1, 64, 0, 40, 1, 9, 13, ()),
    ('b16', 6, 5, 'up2x_wgrad', 'bf16', 2, 1, 8, 0, 40, 1, 9, 13, ()),
    ('b16', 6, 6, 'up2x_wgrad', 'bf16', 2, 1, 64, 0, 16, 1, 9, 13, ()),
    ('b16', 6, 7, 'up2x_wgrad', 'bf16', 2, 1, 8, 0, 16, 1, 9, 13, ()),
    ('b16', 6, 8, 'wgrad', 'bf16', 1, 1, 64, 0, 40, 1, 9, 13, ()),
    ('b16', 6, 9, 'wgrad', 'bf16', 1, 1, 8, 0, 40, 1, 9, 13, ()),
    ('b16', 6, 10, 'wgrad', 'bf16', 1, 1, 64, 0, 16, 1, 9, 13, ()),
    ('b16', 6, 11, 'wgrad', 'bf16', 1, 1, 8, 0, 16, 1, 9, 13, ()),
    ('f32', 0, 0, 'fwd', 'fp32', 3, 1, 12, 0, 4, 2, 7, 23, (('RCF_CONV_SPLIT', '0'),)),
    ('f32', 0, 1, 'fwd', 'fp32', 3, 1, 12, 0, 40, 2, 7, 23, (('RCF_CONV_SPLIT', '0'),)),
    ('f32', 0, 2, 'fwd', 'fp32', 3, 1, 12, 0, 4, 1, 9, 13, (('RCF_CONV_SPLIT', '0'),)),
    ('f32', 0, 3, 'fwd', 'fp32', 3, 1, 12, 0, 40, 1, 9, 13, (('RCF_CONV_SPLIT', '0'),)),
    ('f32', 0, 4, 'fwd', 'fp32', 3, 1, 12, 0, 4, 1, 21, 37, (('RCF_CONV_SPLIT', '0'),)),
    ('f32', 0, 5, 'fwd', 'fp32', 3, 1, 12, 0, 40, 1, 21, 37, (('RCF_CONV_SPLIT', '0'),)),
    ('f32', 0, 6, 'fwd', 'fp32', 3, 1, 4, 0, 4, 2, 7, 23, ()),
    ('f32', 0, 7, 'fwd', 'fp32', 3, 1, 4, 0, 40, 2, 7, 23, ()),
    ('f32', 0, 8, 'fwd', 'fp32', 3, 1, 4, 0, 4, 1, 9, 13, ()),
    ('f32', 0, 9, 'fwd', 'fp32', 3, 1, 4, 0, 40, 1, 9, 13, ()),
    ('f32', 0, 10, 'fwd', 'fp32', 3, 2, 4, 0, 4, 1, 9, 13, ()),
    ('f32', 0, 11, 'fwd', 'fp32', 3, 2, 4, 0, 40, 1, 9, 13, ()),
    ('f32', 0, 12, 'fwd', 'fp32', 3, 2, 4, 0, 4, 1, 41, 9, ()),
    ('f32', 0, 13, 'fwd', 'fp32', 3, 2, 4, 0, 40, 1, 41, 9, ()),
    ('f32', 0, 14, 'fwd', 'fp32', 1, 2, 32, 0, 4, 1, 9, 13, ()),
    ('f32', 0, 15, 'fwd', 'fp32', 1, 2, 32, 0, 40, 1, 9, 13, ()),
    ('f32', 0, 16, 'fwd', 'fp32', 1, 1, 32, 0, 4, 1, 9, 13, ()),
    ('f32', 0, 17, 'fwd', 'fp32', 1, 1, 32, 0, 40, 1, 9, 13, ()),
    ('f32', 0, 18, 'fwd', 'fp32', 1, 2, 4, 0, 4, 1, 9, 13, ()),
    ('f32', 0, 19, 'fwd', 'fp32', 1, 2, 4, 0, 40, 1, 9, 13, ()),
    ('f32', 0, 20, 'fwd', 'fp32', 1, 1, 4, 0, 4, 1, 9, 13, ()),
    ('f32', 0, 21, 'fwd', 'fp32', 1, 1, 4, 0, 40, 1, 9, 13, ()),
    ('f32', 0, 22, 's2_dgrad', 'fp32', 3, 2, 4, 0, 4, 1, 9, 13, ()),
    ('f32', 0, 23, 's2_dgrad', 'fp32', 3, 2, 48, 0, 4, 1, 9, 13, ()),
    ('f32', 0, 24, 'up2x', 'fp32', 2, 1, 4, 0, 4, 1, 9, 13, ()),
    ('f32', 0, 25, 'up2x', 'fp32', 2, 1, 4, 0, 40, 1, 9, 13, ()),
    ('f32', 0, 26, 'fwd', 'fp32', 7, 2, 4, 0, 4, 1, 9, 13, ()),
    ('f32', 0, 27, 'fwd', 'fp32', 7, 2, 4, 0, 4, 1, 41, 9, ()),
    ('f32', 1, 0, 'fwd', 'bf16_operands', 3, 1, 12, 0, 4, 1, 9, 13, ()),
    ('f32', 1, 1, 'fwd', 'bf16_operands', 3, 1, 12, 0, 96, 1, 261, 127, ()),
    ('f32', 1, 2, 'fwd', 'bf16_operands', 3, 1, 12, 0, 4, 2, 9, 13, ()),
    ('f32', 1, 3, 'fwd', 'bf16_operands', 3, 1, 12, 0, 96, 2, 129, 131, ()),
    ('f32', 1, 4, 'fwd', 'bf16_operands', 3, 1, 12, 0, 40, 2, 7, 23, ()),
    ('f32', 1, 5, 'fwd', 'bf16_operands', 3, 1, 12, 0, 40, 1, 9, 13, ()),
    ('f32', 1, 6, 's2_dgrad', 'bf16_operands', 3, 2, 4, 0, 16, 1, 9, 13, ()),
    ('f32', 1, 7, 's2_dgrad', 'bf16_operands', 3, 2, 48, 0, 16, 1, 9, 13, ()),
    ('f32', 1, 8, 'up2x', 'bf16_operands', 2, 1, 16, 0, 4, 1, 9, 13, ()),
    ('f32', 1, 9, 'up2x', 'bf16_operands', 2, 1, 16, 0, 40, 1, 9, 13, ()),
    ('f32', 1, 10, 'fwd', 'bf16_operands', 3, 2, 16, 0, 4, 1, 9, 13, ()),
    ('f32', 1, 11, 'fwd', 'bf16_operands', 3, 2, 16, 0, 40, 1, 9, 13, ()),
    ('f32', 1, 12, 'fwd', 'bf16_operands', 3, 2, 16, 0, 4, 1, 41, 9, ()),
    ('f32', 1, 13, 'fwd', 'bf16_operands', 3, 2, 16, 0, 40, 1, 41, 9, ()),
    ('f32', 1, 14, 'fwd', 'fp32', 3, 1, 12, 0, 4, 1, 9, 13, ()),
    ('f32', 1, 15, 'fwd', 'fp32', 3, 1, 12, 0, 96, 1, 261, 127, ()),
    ('f32', 1, 16, 'fwd', 'fp32', 3, 1, 12, 0, 4, 2, 9, 13, ()),
    ('f32', 1, 17, 'fwd', 'fp32', 3, 1, 12, 0, 96, 2, 129, 131, ()),
    ('f32', 1, 18, 'fwd', 'fp32', 3, 1, 12, 0, 40, 2, 7, 23, ()),
    ('f32', 1, 19, 'fwd', 'fp32', 3, 1, 12, 0, 40, 1, 9, 13, ()),
    ('f32', 1, 20, 's2_dgrad', 'fp32', 3, 2, 4, 0, 16, 1, 9, 13, ()),
    ('f32', 1, 21, 's2_dgrad', 'fp32', 3, 2, 48, 0, 16, 1, 9, 13, ()),
    ('f32', 1, 22, 'up2x', 'fp32', 2, 1, 16, 0, 4, 1, 9, 13, ()),
    ('f32', 1, 23, 'up2x', 'fp32', 2, 1, 16, 0, 40, 1, 9, 13, ()),
    ('f32', 1, 24, 'fwd', 'fp32', 3, 2, 16, 0, 4, 2, 7, 23, (('RCF_S2_SPLIT', '1'),)),
    ('f32', 1, 25, 'fwd', 'fp32', 3, 2, 16, 0, 40, 2, 7, 23, (('RCF_S2_SPLIT', '1'),)),
    ('f32', 1, 26, 'fwd', 'fp32', 3, 2, 16, 0, 4, 1, 9, 13, (('RCF_S2_SPLIT', '1'),)),
    ('f32', 1, 27, 'fwd', 'fp32', 3, 2, 16, 0, 40, 1, 9, 13, (('RCF_S2_SPLIT', '1'),)),
    ('f32', 1, 28, 'fwd', 'f16x2', 3, 1, 12, 0, 4, 1, 9, 13, ()),
    ('f32', 1, 29, 'fwd', 'f16x2', 3, 1, 12, 0, 96, 1, 261, 127, ()),
    ('f32', 1, 30, 'fwd', 'f16x2', 3, 1, 12, 0, 4, 2, 9, 13, ()),
    ('f32', 1, 31, 'fwd', 'f16x2', 3, 1, 12, 0, 96, 2, 129, 131, ()),
    ('f32', 1, 32, 'fwd', 'f16x2', 3, 1, 12, 0, 40, 2, 7, 23, ()),
    ('f32', 1, 33, 'fwd', 'f16x2', 3, 1, 12, 0, 40, 1, 9, 13, ()),
    ('f32', 1, 34, 's2_dgrad', 'f16x2', 3, 2, 4, 0, 16, 1, 9, 13, ()),
    ('f32', 1, 35, 's2_dgrad', 'f16x2', 3, 2, 48, 0, 16, 1, 9, 13, ()),
    ('f32', 1, 36, 'up2x', 'f16x2', 2, 1, 16, 0, 4, 1, 9, 13, ()),
    ('f32', 1, 37, 'up2x', 'f16x2', 2, 1, 16, 0, 40, 1, 9, 13, ()),
    ('f32', 1, 38, 'fwd', 'f16x2', 3, 2, 16, 0, 4, 2, 7, 23, ()),
    ('f32', 1, 39, 'fwd', 'f16x2', 3, 2, 16, 0, 40, 2, 7, 23, ()),
    ('f32', 1, 40, 'fwd', 'f16x2', 3, 2, 16, 0, 4, 1, 9, 13, ()),
    ('f32', 1, 41, 'fwd', 'f16x2', 3, 2, 16, 0, 40, 1, 9, 13, ()),
    ('f32', 1, 42, 'stem4', 'fp32', 4, 1, 4, 0, 4, 1, 9, 13, ()),
    ('f32', 1, 43, 'stem4', 'fp32', 4, 1, 4, 0, 4, 1, 41, 9, ()),
    ('f32', 1, 44, 'up2x_m', 'f16x2', 2, 1, 16, 0, 4, 1, 9, 13, ()),
    ('f32', 1, 45, 'up2x_m', 'f16x2', 2, 1, 16, 0, 40, 1, 9, 13, ()),
    ('f32', 1, 46, 's2_dgrad_m', 'f16x2', 3, 2, 4, 0, 16, 1, 9, 13, ()),
    ('f32', 1, 47, 's2_dgrad_m', 'f16x2', 3, 2, 48, 0, 16, 1, 9, 13, ()),
    ('f32', 3, 0, 'fwd', 'f16x2', 1, 1, 16, 0, 4, 1, 9, 13, ()),
    ('f32', 3, 1, 'fwd', 'f16x2', 1, 1, 16, 0, 40, 1, 9, 13, ()),
    ('f32', 3, 2, 'fwd', 'f16x2', 1, 1, 16, 0, 96, 1, 9, 13, ()),
    ('f32', 3, 3, 'fwd', 'f16x2', 1, 1, 16, 0, 128, 1, 9, 13, ()),
    ('f32', 3, 4, 'fwd', 'f16x2', 1, 1, 32, 0, 4, 1, 9, 13, ()),
    ('f32', 3, 5, 'fwd', 'f16x2', 1, 1, 32, 0, 40, 1, 9, 13, ()),
    ('f32', 3, 6, 'fwd', 'f16x2', 1, 1, 32, 0, 96, 1, 9, 13, ()),
    ('f32', 3, 7, 'fwd', 'f16x2', 1, 1, 32, 0, 128, 1, 9, 13, ()),
    ('f32', 3, 8, 'fwd', 'f16x2', 1, 1, 48, 0, 4, 1, 9, 13, ()),
    ('f32', 3, 9, 'fwd', 'f16x2', 1, 1, 48, 0, 40, 1, 9, 13, ()),
    ('f32', 3, 10, 'fwd', 'f16x2', 1, 1, 64, 0, 4, 1, 9, 13, ()),
    ('f32', 3, 11, 'fwd', 'f16x2', 1, 1, 64, 0, 40, 1, 9, 13, ()),
    ('f32', 4, 0, 'wgrad', 'fp32', 3, 1, 4, 0, 4, 1, 21, 37, (('RCF_CONV_SPLIT', '0'),)),
    ('f32', 4, 1, 'wgrad', 'fp32', 3, 1, 4, 0, 4, 2, 7, 23, (('RCF_CONV_SPLIT', '0'),)),
    ('f32', 4, 2, 'wgrad', 'fp32', 3, 1, 4, 0, 4, 1, 9, 13, (('RCF_CONV_SPLIT', '0'),)),
    ('f32', 4, 3, 'wgrad', 'fp32', 3, 2, 4, 0, 4, 2, 7, 23, ()),
    ('f32', 4, 4, 'wgrad', 'fp32', 3, 2, 4, 0, 4, 1, 9, 13, ()),
    ('f32', 4, 5, 'wgrad', 'fp32', 1, 2, 4, 0, 4, 1, 9, 13, ()),
    ('f32', 4, 6, 'wgrad', 'fp32', 1, 1, 4, 0, 4, 1, 9, 13, ()),
    ('f32', 4, 7, 's2_wgrad', 'fp32', 3, 2, 4, 0, 4, 1, 9, 13, (('RCF_CONV_SPLIT', '0'),)),
    ('f32', 4, 8, 'up2x_wgrad', 'fp32', 2, 1, 4, 0, 4, 1, 9, 13, (('RCF_CONV_SPLIT', '0'),)),
    ('f32', 4, 9, 'wgrad', 'fp32', 7, 2, 4, 0, 4, 1, 9, 13, ()),
    ('f32', 4, 10, 'wgrad', 'fp32', 7, 2, 4, 0, 4, 1, 41, 9, ()),
    ('f32', 5, 0, 'wgrad', 'bf16_operands', 3, 1, 64, 0, 40, 1, 9, 13, ()),
    ('f32', 5, 1, 'wgrad', 'bf16_operands', 3, 1, 4, 0, 40, 1, 9, 13, ()),
    ('f32', 5, 2, 'wgrad', 'bf16_operands', 3, 1, 64, 0, 4, 1, 9, 13, ()),
    ('f32', 5, 3, 'wgrad', 'bf16_operands', 3, 1, 4, 0, 4, 1, 9, 13, ()),
    ('f32', 5, 4, 'up2x_wgrad', 'bf16_operands', 2, 1, 64, 0, 40, 1, 9, 13, ()),
    ('f32', 5, 5, 'up2x_wgrad', 'bf16_operands', 2, 1, 4, 0, 40, 1, 9, 13, ()),
    ('f32', 5, 6, 'up2x_wgrad', 'bf16_operands', 2, 1, 64, 0, 4, 1, 9, 13, ()),
    ('f32', 5, 7, 'up2x_wgrad', 'bf16_operands', 2, 1, 4, 0, 4, 1, 9, 13, ()),
    ('f32', 5, 8, 'up2x_wgrad_m', 'bf16_operands', 2, 1, 64, 0, 40, 1, 9, 13, ()),
    ('f32', 5, 9, 'up2x_wgrad_m', 'bf16_operands', 2, 1, 16, 0, 40, 1, 9, 13, ()),
    ('f32', 5, 10, 'up2x_wgrad_m', 'bf16_operands', 2, 1, 64, 0, 4, 1, 9, 13, ()),
    ('f32', 5, 11, 'up2x_wgrad_m', 'bf16_operands', 2, 1, 16, 0, 4, 1, 9, 13, ()),
    ('f32', 5, 12, 'wgrad', 'f16x2', 3, 1, 64, 0, 40, 1, 9, 13, (('RCF_WGRAD_TR', '0'),)),
    ('f32', 5, 13, 'wgrad', 'f16x2', 3, 1, 4, 0, 40, 1, 9, 13, (('RCF_WGRAD_TR', '0'),)),
    ('f32', 5, 14, 'wgrad', 'f16x2', 3, 1, 64, 0, 4, 1, 9, 13, (('RCF_WGRAD_TR', '0'),)),
    ('f32', 5, 15, 'wgrad', 'f16x2', 3, 1, 4, 0, 4, 1, 9, 13, (('RCF_WGRAD_TR', '0'),)),
    ('f32', 5, 16, 'up2x_wgrad', 'f16x2', 2, 1, 64, 0, 40, 1, 9, 13, (('RCF_WGRAD_TR', '0'),)),
    ('f32', 5, 17, 'up2x_wgrad', 'f16x2', 2, 1, 4, 0, 40, 1, 9, 13, (('RCF_WGRAD_TR', '0'),)),
    ('f32', 5, 18, 'up2x_wgrad', 'f16x2', 2, 1, 64, 0, 4, 1, 9, 13, (('RCF_WGRAD_TR', '0'),)),
    ('f32', 5, 19, 'up2x_wgrad', 'f16x2', 2, 1, 4, 0, 4, 1, 9, 13, (('RCF_WGRAD_TR', '0'),)),
    ('f32', 5, 20, 'up2x_wgrad_m', 'f16x2', 2, 1, 64, 0, 40, 1, 9, 13, ()),
    ('f32', 5, 21, 'up2x_wgrad_m', 'f16x2', 2, 1, 16, 0, 40, 1, 9, 13, ()),
    ('f32', 5, 22, 'up2x_wgrad_m', 'f16x2', 2, 1, 64, 0, 4, 1, 9, 13, ()),
    ('f32', 5, 23, 'up2x_wgrad_m', 'f16x2', 2, 1, 16, 0, 4, 1, 9, 13, ()),
    ('f32', 5, 24, 'wgrad', 'fp32', 3, 1, 64, 0, 40, 1, 9, 13, ()),
    ('f32', 5, 25, 'wgrad', 'fp32', 3, 1, 4, 0, 40, 1, 9, 13, ()),
    ('f32', 5, 26, 'wgrad', 'fp32', 3, 1, 64, 0, 4, 1, 9, 13, ()),
    ('f32', 5, 27, 'wgrad', 'fp32', 3, 1, 4, 0, 4, 1, 9, 13, ()),
    ('f32', 5, 28, 'up2x_wgrad', 'fp32', 2, 1, 64, 0, 40, 1, 9, 13, ()),
    ('f32', 5, 29, 'up2x_wgrad', 'fp32', 2, 1, 4, 0, 40, 1, 9, 13, ()),
    ('f32', 5, 30, 'up2x_wgrad', 'fp32', 2, 1, 64, 0, 4, 1, 9, 13, ()),
    ('f32', 5, 31, 'up2x_wgrad', 'fp32', 2, 1, 4, 0, 4, 1, 9, 13, ()),
    ('f32', 6, 0, 'wgrad', 'f16x2', 3, 1, 64, 0, 40, 1, 9, 13, ()),
    ('f32', 6, 1, 'wgrad', 'f16x2', 3, 1, 4, 0, 40, 1, 9, 13, ()),
    ('f32', 6, 2, 'wgrad', 'f16x2', 3, 1, 64, 0, 4, 1, 9, 13, ()),
    ('f32', 6, 3, 'wgrad', 'f16x2', 3, 1, 4, 0, 4, 1, 9, 13, ()),
    ('f32', 6, 4, 'up2x_wgrad', 'f16x2', 2, 1, 64, 0, 40, 1, 9, 13, ()),
    ('f32', 6, 5, 'up2x_wgrad', 'f16x2', 2, 1, 4, 0, 40, 1, 9, 13, ()),
    ('f32', 6, 6, 'up2x_wgrad', 'f16x2', 2, 1, 64, 0, 4, 1, 9, 13, ()),
    ('f32', 6, 7, 'up2x_wgrad', 'f16x2', 2, 1, 4, 0, 4, 1, 9, 13, ()),
]]
