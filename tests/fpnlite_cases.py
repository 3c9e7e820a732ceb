"""Seeded cases of the FPN-lite neck -- ``FeaturePyramid(..., use_depthwise=True)``, bf/modules/features.py:52-120: every ``pyramid_output`` block
is ``Conv2dBn(C, C, 3, groups=C)`` (:79-98), padding 1 throughout, stride 1 on the tapped levels and stride 2 on the extra ones -- that run
through ANY implementation of the reference's module interface: ``tools/gen_golden_fpnlite.py`` runs them through the reference's own class
on the CPU and writes ``tests/golden/fpn_lite.npz``; ``tests/test_fpnlite_gpu.py`` runs them through this repository's class on the GPU and
compares.  The stub backbone, the harness and the packing are bilinear_cases' (eval() forward + backward, then ONE train() step; outputs,
input and parameter gradients, BatchNorm buffers afterwards).  This file holds no reference code: constructor arguments, shapes and seeds
only."""
import bilinear_cases
from bilinear_cases import _StubBase, case_seed, pack_sampled, SUFFIXES   # noqa: F401  (re-exported for the tests)


def _fpn(levels, **extra):
    return lambda m: m.FeaturePyramid(_StubBase(), (1, 3, 4), pyramid_layers=levels, pyramid_channels=32, use_depthwise=True, **extra)


# name -> (build(mods) -> module, input shape, forward(module, x) -> list of tensors).  Batch 2 everywhere: the last levels are a few pixels
# and a training-mode BatchNorm needs more than one row.  The stub's taps (1, 3, 4) are at strides 2, 4, 8, and an extra level is the same
# geometry (3 x 3, stride 2, padding 1 -- features.py:92-98): n -> (n - 1) // 2 + 1.
CASES = {
    'fpnlite': (_fpn(5), (2, 3, 64, 64), lambda mod, x: mod(x)[0]),
    'fpnlite_odd': (_fpn(5), (2, 3, 76, 52), lambda mod, x: mod(x)[0]),
    'fpnlite_bilinear': (_fpn(5, interpolation_mode='bilinear'), (2, 3, 64, 64), lambda mod, x: mod(x)[0]),
    'fpnlite_deep': (_fpn(4), (2, 3, 96, 96), lambda mod, x: mod(x)[0]),   # an input 1.5 x that of `fpnlite` through the same stub
}

# the (H, W) of every pyramid level, finest first: run_case asserts them
LEVEL_SIZES = {
    'fpnlite': ((32, 32), (16, 16), (8, 8), (4, 4), (2, 2)),
    'fpnlite_odd': ((38, 26), (19, 13), (10, 7), (5, 4), (3, 2)),
    'fpnlite_bilinear': ((32, 32), (16, 16), (8, 8), (4, 4), (2, 2)),
    'fpnlite_deep': ((48, 48), (24, 24), (12, 12), (6, 6)),
}
N_OUTPUTS = {name: len(sizes) for name, sizes in LEVEL_SIZES.items()}


def _registered(fn):
    """Run ``fn`` with this file's cases visible to bilinear_cases' harness (build / run_case / expected_keys look their case up by name in
    bilinear_cases.CASES and N_OUTPUTS); the harness's tables are left as they were."""
    def wrapped(name, *args, **kwargs):
        assert name in CASES and name not in bilinear_cases.CASES, name
        bilinear_cases.CASES[name], bilinear_cases.N_OUTPUTS[name] = CASES[name], N_OUTPUTS[name]
        try:
            return fn(name, *args, **kwargs)
        finally:
            del bilinear_cases.CASES[name], bilinear_cases.N_OUTPUTS[name]
    return wrapped


build = _registered(bilinear_cases.build)
expected_keys = _registered(bilinear_cases.expected_keys)
_run = _registered(bilinear_cases.run_case)


def run_case(name, mods, device):
    """bilinear_cases.run_case on a case of this file; every level's size is asserted as LEVEL_SIZES states it."""
    res = _run(name, mods, device)
    for mode in ('eval', 'train'):
        for i, (h, w) in enumerate(LEVEL_SIZES[name]):
            key = f'{name}/{mode}/y{i}'
            shape = tuple(res[key + '__shape']) if key + '__shape' in res else res[key].shape
            assert shape == (CASES[name][1][0], 32, h, w), (key, shape, (h, w))
    return res
