"""Seeded cases of the necks in ``interpolation_mode='bilinear'`` (bf/modules/features.py:52-120 FPN, :215-270 TUM, :303-393 MLFPN) that run
through ANY implementation of the reference's module interface: ``tools/gen_golden_bilinear.py`` runs them through the reference's own
classes on the CPU and writes ``tests/golden/necks_bilinear.npz``; ``tests/test_bilinear_gpu.py`` runs them through this repository's
classes on the GPU and compares.  The harness is blocks_cases.run_case's (eval() forward + backward, then ONE train() step; outputs, input
and parameter gradients, BatchNorm buffers afterwards).  This file holds no reference code: constructor arguments, shapes and seeds only."""
import zlib

import numpy as np
import torch

from blocks_cases import _StubBase, _flatten, fill_module_, pack

MODE = 'bilinear'

# name -> (build(mods) -> module, input shape, forward(module, x) -> nested lists of tensors).  `mods` offers FeaturePyramid,
# ThinnedUshapeModule and MultilevelFeaturePyramid.  The stub's taps are at strides 2, 4, 8 (3 x 3, stride 2, pad 1: n -> (n - 1) // 2 + 1):
#   fpn_bilinear:      taps 32 / 16 / 8: exact 2 x ratios (weights 1/4 and 3/4)
#   fpn_bilinear_odd:  76 x 52 -> taps 38 x 26 / 19 x 13 / 10 x 7: H 10 -> 19 -> 38, W 7 -> 13 -> 26 (one odd step, one exact 2 x)
#   tum_bilinear:      13 -> 7 -> 4 -> 2 and back
#   mlfp_bilinear:     taps 19 and 10: the base features are upscaled 10 -> 19 in the neck's mode, the TUMs go 19 -> 10 -> 5 and back
# (the dictionaries are built per call: the reference's MultilevelFeaturePyramid updates its `tum` / `sfam` arguments in place)
CASES = {
    'fpn_bilinear': (lambda m: m.FeaturePyramid(_StubBase(), (1, 3, 4), pyramid_layers=5, pyramid_channels=32, interpolation_mode=MODE),
                     (2, 3, 64, 64), lambda mod, x: mod(x)[0]),
    'fpn_bilinear_odd': (lambda m: m.FeaturePyramid(_StubBase(), (1, 3, 4), pyramid_layers=5, pyramid_channels=32, interpolation_mode=MODE),
                         (2, 3, 76, 52), lambda mod, x: mod(x)[0]),
    'tum_bilinear': (lambda m: m.ThinnedUshapeModule(in_channels=48, inner_channels=32, out_channels=16, num_scales=4,
                                                     interpolation_mode=MODE),
                     (2, 48, 13, 13), lambda mod, x: mod(x)),
    'mlfp_bilinear': (lambda m: m.MultilevelFeaturePyramid(_StubBase(), (3, 4), num_scales=3, num_tums=2, base_reduced_channels=[16, 32],
                                                           reduced_channels=16, interpolation_mode=MODE,
                                                           tum={'inner_channels': 32, 'out_channels': 16}, sfam={'reduction_ratio': 4}),
                      (2, 3, 76, 76), lambda mod, x: mod(x)[0]),
}


N_OUTPUTS = {'fpn_bilinear': 5, 'fpn_bilinear_odd': 5, 'tum_bilinear': 4, 'mlfp_bilinear': 3}   # pyramid levels / scales


def case_seed(name):
    return zlib.crc32(name.encode()) % 100000


SAMPLE_ABOVE = 2048   # blocks_cases.pack stores up to 10 000 elements whole; with these necks' 3 x 3 weights (9 216 elements each, in
N_SAMPLES = 1024      # four cases and two modes) that is a 1.5 MB fixture.  Same keys, same checksums, a lower threshold and fewer samples.


def pack_sampled(key, arr, res):
    """blocks_cases.pack for a small array; a larger one in pack's sampled form (``__samples`` at seeded positions, ``__sum_l2`` = the fp64
    sum and L2 norm of the WHOLE array, ``__shape``) with this file's threshold."""
    a = np.ascontiguousarray(arr)
    if a.size <= SAMPLE_ABOVE:
        return pack(key, a, res)
    idx = np.random.default_rng(zlib.crc32(key.encode())).choice(a.size, N_SAMPLES, replace=False)
    res[key + '__samples'] = a.reshape(-1)[idx]
    res[key + '__sum_l2'] = np.array([a.astype(np.float64).sum(), np.sqrt((a.astype(np.float64) ** 2).sum())])
    res[key + '__shape'] = np.array(a.shape, np.int64)


def build(name, mods):
    """The case's module: ``mods`` holds the reference's classes (generator) or this repository's (test)."""
    torch.manual_seed(0)
    return fill_module_(CASES[name][0](mods), case_seed(name))


def run_case(name, mods, device):
    """Build, fill, run: eval() forward + backward, then ONE train() forward + backward; returns {key: array} (pack_sampled)."""
    module = build(name, mods).to(device)
    _, shape, forward = CASES[name]
    x_np = np.random.default_rng(case_seed(name) + 1).standard_normal(shape, dtype=np.float32)
    res = {}
    for mode in ('eval', 'train'):
        module.train(mode == 'train')
        module.zero_grad(set_to_none=True)
        x = torch.from_numpy(x_np).to(device).requires_grad_(True)
        ys = _flatten(forward(module, x))
        grng = np.random.default_rng(case_seed(name) + 7)
        gs = [torch.from_numpy(grng.standard_normal(tuple(y.shape), dtype=np.float32)).to(device) for y in ys]
        torch.autograd.backward(ys, gs)
        for i, y in enumerate(ys):
            pack_sampled(f'{name}/{mode}/y{i}', y.detach().cpu().numpy(), res)
        pack_sampled(f'{name}/{mode}/dx0', x.grad.detach().cpu().numpy(), res)
        for pname, p in sorted(module.named_parameters()):
            if pname.startswith('base.'):
                continue   # (the stub backbone is stock torch on both sides)
            assert p.grad is not None, (name, mode, pname)
            pack_sampled(f'{name}/{mode}/dp/{pname}', p.grad.detach().cpu().numpy(), res)
    for bname, b in sorted(module.named_buffers()):   # after the one train() step: momentum, unbiased variance, the step counter
        res[f'{name}/buffers/{bname}'] = b.detach().cpu().numpy()
    return res


SUFFIXES = ('__samples', '__sum_l2', '__shape')   # blocks_cases.pack's keys of a sampled array


def expected_keys(name, mods):
    """The keys run_case writes for a case, sampling suffixes stripped, from the module's structure alone (no forward pass)."""
    module = build(name, mods)
    keys = set()
    for mode in ('eval', 'train'):
        keys |= {f'{name}/{mode}/y{i}' for i in range(N_OUTPUTS[name])} | {f'{name}/{mode}/dx0'}
        keys |= {f'{name}/{mode}/dp/{pname}' for pname, _ in module.named_parameters() if not pname.startswith('base.')}
    keys |= {f'{name}/buffers/{bname}' for bname, _ in module.named_buffers()}
    return keys
