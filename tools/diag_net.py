'''Diagnostic (GPU box): per-layer forward activations and incoming activation gradients of the tiny net,
HIP engine vs fp64 CPU oracle.'''
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import rcf_amd
from rcf_amd import synth, train, engine as eng_mod
from oracle.fusionnet_oracle import FusionNetOracle, Conv2d as OConv

import sys as _s
if len(_s.argv) > 1 and _s.argv[1] == 'pub':
    cfg, wseed, shape, dseed = synth.PUBLISHED, 5, (2, 113, 200, 16), 9
else:
    cfg, wseed, shape, dseed = synth.TINY, 11, (2, 70, 102, 8), 101
# RCF_DIAG_CASE=tiny_inputs: the hostile case of tests/test_hip_f16x2.py (weights seed 17, data seed 321, every input x 1e-6)
if os.environ.get('RCF_DIAG_CASE') == 'tiny_inputs':
    wseed, dseed = 17, 321
b = synth.make_batch(*shape, seed=dseed)
if os.environ.get('RCF_DIAG_CASE') == 'tiny_inputs':
    b['image'] *= 1e-6
    b['input_depth'] *= 1e-6
rel = lambda a, b_: float((a.double() - b_.double()).abs().max() / (b_.double().abs().max() + 1e-30))
nchw = lambda t: t.detach().cpu().permute(0, 3, 1, 2).contiguous()

# ---- oracle fp64 with hooks
o = FusionNetOracle(**cfg); synth.fill_state_dict_([o.encoder, o.decoder], wseed)
for mod in (o.encoder, o.decoder): mod.double()
o.train()
ref = {}
def mk(name):
    def hook(mod, inp, out):
        out.retain_grad(); ref[name] = out
    return hook
zref = {}
def mkz(name):
    def hook(mod, inp, out):
        out.retain_grad(); zref[name] = out
    return hook
def getattr_path(model, dotted):
    cur = model
    for part in dotted.split('.'):
        cur = getattr(cur, part)
    return cur
for pre, mod in (('encoder.', o.encoder), ('decoder.', o.decoder)):
    for k, sub in mod.named_modules():
        if isinstance(sub, OConv):
            sub.register_forward_hook(mk(pre + k))
            sub.conv.register_forward_hook(mkz(pre + k))
out = o.forward(b['image'].double(), b['input_depth'].double())
loss = o.compute_loss(out, b['ground_truth'].double(), b['lidar_map'].double(), 2.0)[0]
loss.backward()

# ---- oracle fp32 with hooks
o32 = FusionNetOracle(**cfg); synth.fill_state_dict_([o32.encoder, o32.decoder], wseed)
o32.train()
ref32 = {}
def mk32(name):
    def hook(mod, inp, out):
        out.retain_grad(); ref32[name] = out
    return hook
for pre, mod in (('encoder.', o32.encoder), ('decoder.', o32.decoder)):
    for k, sub in mod.named_modules():
        if isinstance(sub, OConv): sub.register_forward_hook(mk32(pre + k))
out32 = o32.forward(b['image'], b['input_depth'])
loss32 = o32.compute_loss(out32, b['ground_truth'], b['lidar_map'], 2.0)[0]
loss32.backward()

# ---- HIP with recording
m = train.build_model(cfg, device='cuda'); synth.fill_state_dict_([m.encoder, m.decoder], wseed)
names = {}
for pre, mod in (('encoder.', m.encoder), ('decoder.', m.decoder)):
    for k, sub in mod.named_modules(): names[id(sub)] = pre + k
rec = {}
E = m._engine
orig_cba = E.conv_bn_act
def cba(layer, x, x2=None, up_hw=None, res=None, feeds_head=False):
    out_ = orig_cba(layer, x, x2=x2, up_hw=up_hw, res=res, feeds_head=feeds_head)
    nm = names[id(layer)]
    rec[nm] = {'out': None if out_.t is None else out_.t.clone(), 'res': res is not None}
    if E.tape is not None:
        inner = E.tape[-1]
        def wrapped():
            if out_.g is not None:
                rec[nm]['g'] = out_.g.clone()
            inner()
        E.tape[-1] = wrapped
    return out_
E.conv_bn_act = cba
zrec = {}
orig_cb = E._conv_backward
def cb(layer, rec_, x, x2, dz, dz_amax=None):
    nm = names.get(id(layer))
    if nm is not None:
        zrec.setdefault(nm, {})['dz'] = dz.clone()
    return orig_cb(layer, rec_, x, x2, dz, dz_amax)
E._conv_backward = cb
orig_conv = E._conv
def cv(layer, x, x2=None, up_hw=None, want_stats=False, fold=None):
    r_ = orig_conv(layer, x, x2, up_hw, want_stats, fold)
    nm = names.get(id(layer))
    if nm is not None:
        zrec.setdefault(nm, {})['z'] = r_[0].clone()
    return r_
E._conv = cv
m.train()
g = {k: v.cuda() for k, v in b.items()}
oh = m.forward(g['image'], g['input_depth'])
lh, _ = m.compute_loss(g['image'], oh, g['ground_truth'], g['lidar_map'], 'l1', 0.0, -1, None, 2.0)
lh.backward(); torch.cuda.synchronize()
print('out %.2e loss %.9f vs %.9f' % (rel(oh.cpu(), out.detach()), float(lh), float(loss)))
order = list(rec.keys())
print('%-40s %10s %10s %10s %10s  %s' % ('layer (forward order)', 'fwd hip', 'fwd cpu32', 'grad hip', 'grad cpu32', 'shape'))
for nm in order:
    r = rec[nm]
    if r['res']:
        print('%-40s %10s %10s   (residual tail: oracle module output differs by design)' % (nm, '-', '-')); continue
    fe = rel(nchw(r['out']), ref[nm].detach()) if r['out'] is not None else float('nan')
    ge = rel(nchw(r['g']), ref[nm].grad) if 'g' in r else float('nan')
    print('%-40s %10.2e %10.2e %10.2e %10.2e  %s' % (nm, fe, rel(ref32[nm].detach(), ref[nm].detach()), ge, rel(ref32[nm].grad, ref[nm].grad), tuple(ref[nm].shape)))

# ---- parameter gradients, worst first
def named(mm):
    out_ = []
    for pre, mod in (('encoder.', mm.encoder), ('decoder.', mm.decoder)):
        out_ += [(pre + k, p) for k, p in mod.named_parameters()]
    return out_
g64 = {k: p.grad for k, p in named(o) if p.grad is not None}
g32 = {k: p.grad for k, p in named(o32) if p.grad is not None}
gh = {k: p.grad.detach().cpu() for k, p in named(m) if p.grad is not None}
rows = sorted(((rel(gh[k], g64[k]), rel(g32[k], g64[k]), k) for k in g64), reverse=True)
print('parameter gradients vs fp64, worst first (hip, cpu32)')
for eh, e32, k in rows[:12]:
    print('  hip %.2e  cpu32 %.2e  %s' % (eh, e32, k))

# ---- one block in detail: the raw conv output z of decoder.deconv0.deconv.conv and its gradient dz (BatchNorm backward's result), HIP vs fp64
if os.environ.get('RCF_DIAG_BLOCK'):
    blk = os.environ['RCF_DIAG_BLOCK']
    zr, dzr = zref[blk].detach(), zref[blk].grad
    zh, dzh = nchw(zrec[blk]['z']), nchw(zrec[blk]['dz'])
    for nm_, a_, r_ in (('z', zh, zr), ('dz', dzh, dzr)):
        e = (a_.double() - r_).abs()
        print('%s %s: max|ref| %.3e rms ref %.3e; err max %.3e rms %.3e; per channel rms err / rms ref: %s' % (
            blk, nm_, float(r_.abs().max()), float(r_.pow(2).mean().sqrt()), float(e.max()), float(e.pow(2).mean().sqrt()),
            ['%.1e' % float(e[:, c_].pow(2).mean().sqrt() / r_[:, c_].pow(2).mean().sqrt()) for c_ in range(r_.shape[1])]))
        inner = (slice(None), slice(None), slice(4, -4), slice(4, -4))
        print('   interior only: rms ref %.3e rms err %.3e' % (float(r_[inner].pow(2).mean().sqrt()), float(e[inner].pow(2).mean().sqrt())))
    # the same BatchNorm backward in fp64 on mixed inputs: which perturbation carries the error?
    gr = ref[blk].grad
    gh = nchw(rec[blk]['g']).double()
    def bnbwd(g_, z_):
        y = ref[blk].detach()   # sign of the BatchNorm output = sign of the block's output (LeakyReLU keeps it)
        gp = g_ * torch.where(y > 0, 1.0, 0.2)
        mean = z_.mean((0, 2, 3), keepdim=True)
        var = (z_ * z_).mean((0, 2, 3), keepdim=True) - mean * mean
        invstd = 1.0 / torch.sqrt(var + 1e-5)
        xh = (z_ - mean) * invstd
        gam = getattr_path(o, blk).batch_norm.weight.detach().view(1, -1, 1, 1)
        return gam * invstd * (gp - gp.mean((0, 2, 3), keepdim=True) - xh * (gp * xh).mean((0, 2, 3), keepdim=True))
    for nm_, g_, z_ in (('g ref, z ref', gr, zr), ('g hip, z ref', gh, zr), ('g ref, z hip', gr, zh.double()), ('g hip, z hip', gh, zh.double())):
        d_ = bnbwd(g_, z_)
        print('   fp64 BN backward on (%s): rel err vs oracle dz %.2e, vs hip dz %.2e' % (nm_, rel(d_, dzr), rel(d_, dzh)))
