#!/usr/bin/env python3
"""Every call the Python layer makes into segland_amd.ops and segland_amd.ops_swin (names prefixed `swin.`) during one seeded forward + backward, one text line per call: the
order and the arguments of the launches.

    python tools/ops_calls_dump.py TREE OUT CONFIG [CONFIG ...]         (TREE: a checkout with its library built, `.` or _ab/<sha> of tools/ab_commits.sh prepare)
    python tools/ops_calls_dump.py _ab/<sha> a.txt all && python tools/ops_calls_dump.py . b.txt all && diff a.txt b.txt

A line: config | wrapper name | per parameter of its signature name=shape:dtype, None, the scalar or the ConvSpec fields | -> the shapes of what it returned.
Two trees drive the library the same way when their dumps are equal (profiles/ab_backward_chain.txt, profiles/ab_pyramid_stages.txt).  Only names both trees have are
used; a hook is looked up in segland_amd.functional, then in segland_amd.functional_swin, set by name and put back to the value it had.  SEGLAND_BN_FUSE=0 in the
environment gives the master-switch-off dump of any config.
Swin-POP configs: swin (swin-t bf16, B 8 as bench config 5, 512x512, one train step; DropPath / Dropout2d draws fixed by the seed), swin_f32 (B 2), off_PSP_GROUPED (swin with
the pyramid hook off), swin_eval (model.eval() forward under no_grad).  r50_eval: the same for the ResNet model -- PPMFn's _frozen branch without the fine-tune head around it.
Not covered: `ft` freezes backbone and decoder, so its BottleneckFn / PPMFn run the _frozen forward and have no backward -- a backward with train-mode BatchNorm and
need_w false (parameters frozen, statistics not) occurs in no config."""
import inspect
import os
import sys

import torch

TREE = os.path.abspath(sys.argv[1])
sys.path.insert(0, TREE)
import segland_amd  # noqa: E402,F401
from segland_amd import functional as sf, functional_swin as sfs, ops, ops_swin  # noqa: E402
from segland_amd.loss.criterion import OrthLoss  # noqa: E402
from segland_amd.networks import swin_pop  # noqa: E402
from segland_amd.networks.pspnet_pop import GFSS_Model  # noqa: E402

assert os.path.abspath(ops.__file__).startswith(TREE + os.sep), 'segland_amd was imported from %s' % ops.__file__
DEV = 'cuda'
HOOKS_OFF = ('_BN_DUAL', '_BN_DUAL_FWD', '_BN_CROSS', '_DS_HALF', '_STAGE_BN_GROUPED', '_PPM_WGRAD_GROUPED', '_PSP_GROUPED')
LINES, TAG = [], ['']


def show(v):
    if v is None or isinstance(v, (bool, int, float, str, torch.dtype)):
        return str(v)
    if isinstance(v, torch.Tensor):
        return '%s:%s' % ('x'.join(map(str, v.shape)), str(v.dtype).replace('torch.', ''))
    if isinstance(v, ops.ConvSpec):
        return 'ConvSpec(%s)' % ','.join(str(getattr(v, f)) for f in ops.ConvSpec.__slots__)
    if isinstance(v, (list, tuple, torch.Size)):
        return '[%s]' % ','.join(show(e) for e in v)
    return type(v).__name__


def wrap(name, fn):
    sig = inspect.signature(fn)

    def wrapped(*a, **k):
        b = sig.bind(*a, **k)
        b.apply_defaults()
        i = len(LINES)
        LINES.append(None)                     # a call is listed before the calls it makes itself
        out = fn(*a, **k)
        LINES[i] = '%s | %s | %s | -> %s' % (TAG[0], name, ' '.join('%s=%s' % (n, show(v)) for n, v in b.arguments.items()), show(out))
        return out
    return wrapped


def model(backbone='resnet50', dtype=torch.bfloat16, **kw):
    torch.manual_seed(3)
    return GFSS_Model(n_base=7, criterion=OrthLoss(255), backbone=backbone, pretrained_model=None, dilated=True, os=8, compute_dtype=dtype, **kw).to(DEV)


def swin_model(dtype=torch.bfloat16):
    torch.manual_seed(3)
    return swin_pop.GFSS_Model(n_base=7, criterion=OrthLoss(255), backbone='swin-t', pretrained_model=None, compute_dtype=dtype).to(DEV)


def batch(B, seed=5, lo=0, n=8):
    g = torch.Generator(device='cpu').manual_seed(seed)
    mask = torch.randint(lo, lo + n, (B, 512, 512), generator=g)
    mask[:, :40] = 255
    return torch.randn(B, 3, 512, 512, generator=g).to(DEV), mask.to(DEV)


def train_step(m, B=16, passes=1):
    m.train()
    torch.manual_seed(9)                        # the DropPath / Dropout2d draws of the Swin-POP configs
    losses = [m(*batch(B, seed=5 + k))['total_loss'] for k in range(passes)]        # passes = 2: two forward passes before the first backward
    for loss in losses:
        loss.backward()


def fine_tune_step():
    from segland_amd.utils.pyt_utils import get_parameters
    m = model(is_ft=True, n_novel=4)
    m.init_cls_n()
    get_parameters(m, lr=1e-3, freeze_backbone=True)          # frozen backbone and decoder: need_w false, the _frozen branches
    m.train_mode()
    (img, mask), (img_b, mask_b) = batch(2, lo=8, n=4), batch(2, seed=6)
    m(img, mask, img_b, mask_b.contiguous())['total_loss'].backward()


def eval_forward(m):
    m.eval()
    with torch.no_grad():
        m(batch(2)[0])


def bottleneck_stack():
    """layer1 + layer2's first block on an input that needs no gradient (need_x false in the first block)."""
    net = model().backbone.train()
    g = torch.Generator(device='cpu').manual_seed(7)
    x = torch.randn(16, 128, 128, net.layer1[0].conv1.in_channels, generator=g).to(DEV).to(torch.bfloat16)
    prev = None
    for blk in list(net.layer1) + [net.layer2[0]]:
        blk.__dict__['_sl_prev'] = prev
        x, prev = blk(x), blk
    x.backward(torch.randn(x.shape, generator=g).to(DEV).to(x.dtype))


def hook_off(name):
    def run():
        mod = sf if hasattr(sf, name) else sfs
        was = getattr(mod, name, None)         # None: a tree from before this hook -- it runs what the hook switches back to
        if was is not None:
            setattr(mod, name, False)
        try:
            train_step(model()) if mod is sf else train_step(swin_model(), B=8)
        finally:
            if was is not None:
                setattr(mod, name, was)
    return run


def ppm_direct():
    sf.set_ppm_factorised(False)
    try:
        train_step(model())
    finally:
        sf.set_ppm_factorised(True)


CONFIGS = {'r50': lambda: train_step(model()), 'r50v2': lambda: train_step(model('resnet50v2')), 'f32': lambda: train_step(model(dtype=torch.float32), B=2),
           'ft': fine_tune_step, 'stack': bottleneck_stack, 'two_passes': lambda: train_step(model(), B=4, passes=2), 'ppm_direct': ppm_direct}
CONFIGS.update({'swin': lambda: train_step(swin_model(), B=8), 'swin_f32': lambda: train_step(swin_model(torch.float32), B=2),
                'swin_eval': lambda: eval_forward(swin_model()), 'r50_eval': lambda: eval_forward(model())})
CONFIGS.update({'off' + h: hook_off(h) for h in HOOKS_OFF})


def main():
    for mod, prefix in ((ops, ''), (ops_swin, 'swin.')):
        for name, fn in list(vars(mod).items()):
            if inspect.isfunction(fn) and fn.__module__ == mod.__name__ and not name.startswith('_'):
                setattr(mod, name, wrap(prefix + name, fn))
    names = list(CONFIGS) if sys.argv[3:] == ['all'] else sys.argv[3:]
    for TAG[0] in names:
        CONFIGS[TAG[0]]()
        torch.cuda.synchronize()
        print('%s: %d calls so far' % (TAG[0], len(LINES)), flush=True)
    with open(sys.argv[2], 'w') as f:
        f.write('\n'.join(LINES) + '\n')


if __name__ == '__main__':
    main()
