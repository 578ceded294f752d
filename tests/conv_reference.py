'''
fp64 reference of what one rcf_conv_desc launch computes (include/rcf_hip.h), built from F.conv2d on the CPU, and the per-element
checks test_conv_config_gpu.py holds the kernels to.

An element passes when |got - ref| <= tol * bound (+ one bf16 ulp of the output for bf16 tensors), where bound is the same
operation on |operands| (|x| conv |w|, plus |base| when accumulating): an error at a small-valued edge pixel is measured against
that pixel's own magnitude, not against the tensor's largest value.
'''

import torch
import torch.nn.functional as F

DIRECT, NEAREST, ZERO_INSERT, STRIDED2 = 0, 1, 2, 3
BF16_EPS = 2.0 ** -8   # one bf16 ulp relative to the value

# tol of each arithmetic tier: the largest |got - ref| / bound over every row, role and variant of test_conv_config_gpu.py on an
# MI355X (first run), and the bound chosen from it.  One missing tap or 16-channel chunk costs 1e-2 .. 0.5 of the bound.
#   f32          fp32 accumulation of exact operands (f32 MFMA, three-plane split, fp32 weight-gradient kernels), against fp64:
#                measured 3.6e-7 (three-plane split, 3x3 forward), bound 6e-7
#   f16x2_order  two fp16 planes against the emulated three-product formula: measured 2.4e-7, bound 4e-7
#   f16x2        two fp16 planes against fp64 of the fp32 operands: measured 2.6e-7, bound 4e-7
#   bf16         bf16 operands (fp32 tensors with bf16 operands, bf16 tensors) against fp64 of the bf16-rounded operands; bf16
#                tensors also one bf16 ulp of the output: measured 1.2e-7, bound 2.5e-7
TOL = {'f32': 6e-7, 'f16x2_order': 4e-7, 'f16x2': 4e-7, 'bf16': 2.5e-7}


def _gather(d, src1, ioy, iox):
    '''source 1 (N, C, h_src1, w_src1) as the logical h_in x w_in input of the convolution'''
    n, c = src1.shape[:2]
    if d.gather1 == DIRECT:
        return src1
    if d.gather1 == NEAREST:
        return F.interpolate(src1, size=(d.h_in, d.w_in), mode='nearest')
    x = src1.new_zeros(n, c, d.h_in, d.w_in)
    if d.gather1 == ZERO_INSERT:
        hy, wx = min(d.h_src1, (d.h_in + 1) // 2), min(d.w_src1, (d.w_in + 1) // 2)
        x[:, :, 0:2 * hy:2, 0:2 * wx:2] = src1[:, :, :hy, :wx]
        return x
    ph = src1[:, :, ioy::2, iox::2][:, :, :d.h_in, :d.w_in]   # RCF_GATHER_STRIDED2
    x[:, :, :ph.shape[2], :ph.shape[3]] = ph
    return x


def _conv(d, x, w, pad_y, pad_x):
    '''x (N, C, h_in, w_in) convolved with w (O, C, k, k), top / left padding pad_y / pad_x, cropped to h_out x w_out'''
    k, s = d.ksize, d.stride
    need_h, need_w = (d.h_out - 1) * s + k, (d.w_out - 1) * s + k
    xp = F.pad(x, (pad_x, max(0, need_w - pad_x - x.shape[3]), pad_y, max(0, need_h - pad_y - x.shape[2])))
    return F.conv2d(xp, w, stride=s)[:, :, :d.h_out, :d.w_out]


def _phases(d, wgrad):
    '''(input phase, weight slot, top / left pad, output offset) of each convolution the descriptor sums or places'''
    if d.phase_sum == 0:
        return [((d.in_off_y, d.in_off_x), 0, (d.pad, d.pad_x), (d.out_off_y, d.out_off_x))]
    ab = [(a, b) for a in (0, 1) for b in (0, 1)]
    if d.phase_sum == 1 and wgrad:   # the four phase weight gradients of a stride-2 convolution: the descriptor's pad, x at (2y+a, 2x+b)
        return [((a, b), 2 * a + b, (d.pad, d.pad_x), (0, 0)) for a, b in ab]
    if d.phase_sum == 1:             # the up-2x input gradient: phase (a, b) of dZ with pad (a, b), summed
        return [((a, b), 2 * a + b, (a, b), (0, 0)) for a, b in ab]
    if d.phase_sum == 2:             # the up-2x forward: phase (a, b) with pad (1 - a, 1 - b) written at (2y + a, 2x + b)
        return [((0, 0), 2 * a + b, (1 - a, 1 - b), (a, b)) for a, b in ab]
    return [((0, 0), 2 * a + b, (0, 0), (a, b)) for a, b in ab]   # 3: the stride-2 input gradient's output phases


def forward(d, src1, src2, ws, base=None, wgrad=False):
    '''The physical output (N, c_out, out_h_phys, out_w_phys) of a launch on d, in the dtype of the operands, and the mask of the
    pixels it writes.  src1 / src2: NCHW sources; ws: the weight tensor(s) (one per phase slot, OIHW of w_o x w_i); base: the
    output's previous content (accumulate) or None (unwritten pixels are NaN).  wgrad: read phase_sum 1 as the weight gradient does.'''
    n = src1.shape[0]
    out = src1.new_full((n, d.c_out, d.out_h_phys, d.out_w_phys), float('nan')) if base is None else base.clone()
    acc = torch.zeros_like(out)
    mask = torch.zeros((d.out_h_phys, d.out_w_phys), dtype=torch.bool)
    os_ = d.out_stride
    for (ioy, iox), slot, (py, px), (oy, ox) in _phases(d, wgrad):
        x = _gather(d, src1, ioy, iox)
        if src2 is not None:
            x = torch.cat([x, src2], 1)
        w = ws[slot]
        if d.w_mode == 1:   # RCF_W_DGRAD: the slice [w_i_off, w_i_off + c_out) of the input channels, transposed, taps flipped
            w = w[:, d.w_i_off:d.w_i_off + d.c_out].transpose(0, 1).flip(2, 3)
        y = _conv(d, x, w, py, px)
        hy = min(d.h_out, (d.out_h_phys - oy + os_ - 1) // os_)
        wx = min(d.w_out, (d.out_w_phys - ox + os_ - 1) // os_)
        acc[:, :, oy:oy + os_ * hy:os_, ox:ox + os_ * wx:os_] += y[:, :, :hy, :wx]
        mask[oy:oy + os_ * hy:os_, ox:ox + os_ * wx:os_] = True
    m = mask.expand_as(out)
    out[m] = (acc if base is None else base + acc)[m]
    return out, mask


def written(d):
    '''the mask (out_h_phys, out_w_phys) of the pixels a launch on d writes'''
    mask = torch.zeros((d.out_h_phys, d.out_w_phys), dtype=torch.bool)
    os_ = d.out_stride
    for _, _, _, (oy, ox) in _phases(d, False):
        hy = min(d.h_out, (d.out_h_phys - oy + os_ - 1) // os_)
        wx = min(d.w_out, (d.out_w_phys - ox + os_ - 1) // os_)
        mask[oy:oy + os_ * hy:os_, ox:ox + os_ * wx:os_] = True
    return mask


def weight_grad(d, x1, x2, dz, w_shape, nslots):
    '''rcf_conv2d_wgrad's dw (nslots == 4: [4][c_out][c_in][2][2]) as the gradient of <forward(d, x, W), dZ> over the written pixels'''
    ws = [torch.zeros(w_shape, dtype=x1.dtype, requires_grad=True) for _ in range(nslots)]
    out, mask = forward(d, x1, x2, ws, base=torch.zeros((x1.shape[0], d.c_out, d.out_h_phys, d.out_w_phys), dtype=x1.dtype), wgrad=True)
    (out * dz * mask).sum().backward()
    g = [w.grad for w in ws]
    return g[0] if nslots == 1 else torch.stack(g)


def scale_of(amax):
    '''rcf_scale_of_amax (csrc/rcf_common.h): the power of two that puts amax into [2^14, 2^15); 1 for an all-zero tensor'''
    import math
    amax = float(amax)
    if amax == 0.0:
        return 1.0
    e = math.floor(math.log2(amax)) if amax >= 2.0 ** -126 else -127
    return 2.0 ** min(max(14 - e, -126), 126)


def planes(t, s):
    '''the two fp16 planes of t * s as the kernels form them, in fp64'''
    ts = (t.float() * s).contiguous()
    p0 = ts.to(torch.float16).to(torch.float32)
    p1 = (ts - p0).to(torch.float16).to(torch.float32)
    return p0.double(), p1.double()


def x3(fn, a, b, sa, sb):
    '''fn bilinear in the tensor lists (a, b): the three products of their two-plane forms (scales sa, sb), in fp64, rescaled'''
    ap = [planes(t, sa) if t is not None else (None, None) for t in a]
    bp = [planes(t, sb) for t in b]
    a0, a1 = [p[0] for p in ap], [p[1] for p in ap]
    b0, b1 = [p[0] for p in bp], [p[1] for p in bp]
    return (fn(a0, b0) + fn(a0, b1) + fn(a1, b0)) / (sa * sb)


def b16(t):
    '''the values of t rounded to bf16 (nearest even)'''
    return None if t is None else t.to(torch.bfloat16).to(t.dtype)


def error_ratio(got, ref, bound, mask=None, bf16_out=False):
    '''max over the (masked) elements of |got - ref| / bound after the bf16 output ulp is taken off; inf where an element is NaN,
    or off while its bound is 0'''
    got, ref, bound = got.double(), ref.double(), bound.double()
    if mask is not None:
        m = mask.expand_as(got)
        got, ref, bound = got[m], ref[m], bound[m]
    err = (got - ref).abs()
    if bf16_out:
        err = (err - BF16_EPS * torch.maximum(got.abs(), ref.abs())).clamp(min=0.0)
    err = torch.where(torch.isnan(err), torch.full_like(err, float('inf')), err)
    r = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, float('inf')), err))
    return float(r.max()) if r.numel() else 0.0


def untouched(got, init, mask):
    '''True when every element outside the written pixels still holds init (NaN included)'''
    m = ~mask.expand_as(got)
    g, i = got.double()[m], init.double()[m]
    return bool(((g == i) | (torch.isnan(g) & torch.isnan(i))).all())


def guarded(shape, dtype, device, fill, guard=4096, sentinel=7.0):
    '''(tensor of `shape` filled with `fill`, the whole buffer): `guard` sentinel elements follow the tensor'''
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + guard,), sentinel, dtype=dtype, device=device)
    t = buf[:n].view(shape)
    if torch.is_tensor(fill):
        t.copy_(fill)
    else:
        t.fill_(fill)
    return t, buf


def guard_intact(buf, n, sentinel=7.0):
    return bool((buf[n:] == sentinel).all())
