"""Seeded cases of the depthwise feature pyramid (Tiny-DSOD D-FPN, bf/modules/features.py:123-212) that run through ANY implementation of the
reference's ``DepthwiseFeaturePyramid``: ``tools/gen_golden_dfpn.py`` runs them through the reference's own class on the CPU and writes
``tests/golden/dfpn_small.npz``; ``tests/test_dfpn_gpu.py`` runs them through this repository's class on the GPU and compares.  The harness
is blocks_cases.run_case's (eval() forward + backward, then ONE train() step; outputs, input and parameter gradients, BatchNorm buffers
afterwards).  This file holds no reference code: constructor arguments, shapes and seeds only."""
import zlib

import numpy as np
import torch

from blocks_cases import _StubBase, _flatten, fill_module_, pack

# name -> (constructor keyword arguments besides the stub backbone, input shape).  Level sizes (the stub's taps are at strides 2, 4, 8):
#   stub6:   H 38 -> 19 -> 10 -> 5 -> 3 -> 2, W 30 -> 15 -> 8 -> 4 -> 2 -> 1: a pad that is used (odd edge), one that is not (even edge),
#            none at 2, H != W, non-integer nearest ratios; the smallest BatchNorm still sees 2 x 2 x 1 = 4 values per channel
#   one_tap: one tap 12 x 10 -> 6 x 5 -> 3 x 3 -> 2 x 2, no activation anywhere
#   no_down: pyramid_layers == len(out_layers): no downsample level, the up path alone
CASES = {
    'stub6': (dict(out_layers=(1, 3, 4), pyramid_layers=6, pyramid_channels=32), (2, 3, 75, 60)),
    'one_tap': (dict(out_layers=(4,), pyramid_layers=4, pyramid_channels=16, activation=None), (2, 3, 96, 80)),
    'no_down': (dict(out_layers=(1, 3, 4), pyramid_layers=3, pyramid_channels=16), (2, 3, 40, 36)),
}


def case_seed(name):
    return zlib.crc32(('dfpn_' + name).encode()) % 100000


def build(cls, name):
    """The case's module: ``cls`` is the reference's DepthwiseFeaturePyramid (generator) or this repository's (test)."""
    torch.manual_seed(0)
    return fill_module_(cls(_StubBase(), **CASES[name][0]), case_seed(name))


def run_case(name, cls, device):
    """Build, fill, run: eval() forward + backward, then ONE train() forward + backward; returns {key: array} (blocks_cases.pack)."""
    module = build(cls, name).to(device)
    x_np = np.random.default_rng(case_seed(name) + 1).standard_normal(CASES[name][1], dtype=np.float32)
    res = {}
    for mode in ('eval', 'train'):
        module.train(mode == 'train')
        module.zero_grad(set_to_none=True)
        x = torch.from_numpy(x_np).to(device).requires_grad_(True)
        ys = _flatten(module(x)[0])
        grng = np.random.default_rng(case_seed(name) + 7)
        gs = [torch.from_numpy(grng.standard_normal(tuple(y.shape), dtype=np.float32)).to(device) for y in ys]
        torch.autograd.backward(ys, gs)
        for i, y in enumerate(ys):
            pack(f'{name}/{mode}/y{i}', y.detach().cpu().numpy(), res)
        pack(f'{name}/{mode}/dx0', x.grad.detach().cpu().numpy(), res)
        for pname, p in sorted(module.named_parameters()):
            if pname.startswith('base.'):
                continue   # (the stub backbone is stock torch on both sides)
            assert p.grad is not None, (name, mode, pname)
            pack(f'{name}/{mode}/dp/{pname}', p.grad.detach().cpu().numpy(), res)
    for bname, b in sorted(module.named_buffers()):   # after the one train() step: momentum, unbiased variance, the step counter
        res[f'{name}/buffers/{bname}'] = b.detach().cpu().numpy()
    shapes = {n: tuple(t.shape) for n, t in module.state_dict().items() if not n.startswith('base.')}
    res[f'{name}/state_names'] = np.array(sorted(shapes))
    res[f'{name}/state_shapes'] = np.array([str(shapes[n]) for n in sorted(shapes)])
    return res
