"""Seeded cases of the depthwise RetinaNet-lite tower -- ``SharedConvPredictor(..., use_depthwise=True)``, detection/modules/predictors.py:8-76
-- that run through ANY implementation of the reference's class: ``tools/gen_golden_dwtower.py`` runs them through the reference's own
class on the CPU and writes ``tests/golden/tower_depthwise.npz``; ``tests/test_depthwise_tower_gpu.py`` runs them through this
repository's class on the GPU and compares.  The harness is blocks_cases.run_case's (eval() forward + backward, then ONE train() step;
outputs, input and parameter gradients, BatchNorm buffers afterwards, state_dict names and shapes).  This file holds no reference code:
constructor arguments, shapes and seeds only."""
import zlib

import numpy as np
import torch

from blocks_cases import _flatten, fill_module_, pack

# name -> (constructor arguments, batch, level sizes).  Every norm sees at least 16 rows (4 x 2 x 2); with kernel_size=5 and the tower's
# padding of 1 a layer shrinks its maps by 2, so the levels of 'k5' end at 12, 5 and 3.
CASES = {
    'k3': (dict(source_out_channels=[32] * 5, num_boxes=[9] * 5, num_classes=8, use_depthwise=True, num_layers=2, num_channels=32), 4, (16, 8, 4, 3, 2)),
    'k5': (dict(source_out_channels=[32] * 3, num_boxes=[9] * 3, num_classes=8, use_depthwise=True, num_layers=2, num_channels=32, kernel_size=5), 4,
           (16, 9, 7)),
}


def case_seed(name):
    return zlib.crc32(('dwtower_' + name).encode()) % 100000


def build(cls, name):
    torch.manual_seed(0)
    return fill_module_(cls(**CASES[name][0]), case_seed(name))


def case_inputs(name):
    kw, batch, sizes = CASES[name]
    rng = np.random.default_rng(case_seed(name) + 1)
    return [rng.standard_normal((batch, kw['source_out_channels'][0], n, n), dtype=np.float32) for n in sizes]


def run_case(name, cls, device, dtype=torch.float32):
    """Build, fill, run: eval() forward + backward, then ONE train() forward + backward; returns {key: array} (blocks_cases.pack).
    ``dtype=torch.float64`` runs the same graph in double precision (the generator's check of how far fp32 is from it)."""
    module = build(cls, name).to(device=device, dtype=dtype)
    xs_np = case_inputs(name)
    res = {}
    for mode in ('eval', 'train'):
        module.train(mode == 'train')
        module.zero_grad(set_to_none=True)
        xs = [torch.from_numpy(x).to(device=device, dtype=dtype).requires_grad_(True) for x in xs_np]
        ys = _flatten(module(xs))
        grng = np.random.default_rng(case_seed(name) + 7)
        gs = [torch.from_numpy(grng.standard_normal(tuple(y.shape), dtype=np.float32)).to(device=device, dtype=dtype) for y in ys]
        torch.autograd.backward(ys, gs)
        for i, y in enumerate(ys):
            pack(f'{name}/{mode}/y{i}', y.detach().cpu().numpy(), res)
        for i, x in enumerate(xs):
            pack(f'{name}/{mode}/dx{i}', x.grad.detach().cpu().numpy(), res)
        for pname, p in sorted(module.named_parameters()):
            assert p.grad is not None, (name, mode, pname)
            pack(f'{name}/{mode}/dp/{pname}', p.grad.detach().cpu().numpy(), res)
    for bname, b in sorted(module.named_buffers()):   # after the one train() step: momentum, unbiased variance, the step counter
        res[f'{name}/buffers/{bname}'] = b.detach().cpu().numpy()
    shapes = {n: tuple(t.shape) for n, t in module.state_dict().items()}
    res[f'{name}/state_names'] = np.array(sorted(shapes))
    res[f'{name}/state_shapes'] = np.array([str(shapes[n]) for n in sorted(shapes)])
    return res


def worst_ratio(got, want, bar):
    """max over every float entry of |got - want| / (bar * (|want| + max|want|)): <= 1 passes the bar (test_blocks_golden_gpu.py's rule);
    names, shapes and the step counter must be equal.  -> (ratio, key of the worst entry)"""
    assert sorted(got) == sorted(want), sorted(set(got) ^ set(want))[:10]
    worst = (0.0, None)
    for key in sorted(want):
        ref, val = np.asarray(want[key]), np.asarray(got[key])
        if ref.dtype.kind in 'US' or key.endswith('__shape') or key.endswith('num_batches_tracked'):
            assert np.array_equal(ref, val), (key, ref, val)
            continue
        ref, val = ref.astype(np.float64), val.astype(np.float64)
        assert ref.shape == val.shape, (key, ref.shape, val.shape)
        if key.endswith('__sum_l2'):
            ratio = max(abs(val[1] - ref[1]) / (bar * ref[1] + 1e-12), abs(val[0] - ref[0]) / (10 * bar * ref[1] + 1e-12))
        else:
            scale = float(np.abs(ref).max()) if ref.size else 0.0
            ratio = float((np.abs(val - ref) / (bar * (np.abs(ref) + scale) + 1e-12)).max()) if ref.size else 0.0
        if ratio > worst[0]:
            worst = (float(ratio), key)
    return worst
