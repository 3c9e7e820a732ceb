"""GPU parity of the pyramid tail's GEMMs at the sizes the benchmark runs them: the eight SSD-300 tail layers at batch 32 and the ten
SSD-512 ones at batch 16 -- each alone, and with their weight gradients deferred into grouped launches (ops.deferred_weight_gradients:
up to eight problems per launch, sized for the launch as a whole) -- forward, dx, dw (db for a variant with a bias) against torch's fp32
CPU convolution under test_conv_bn_gpu._close's bar, |got - want| <= 1e-4 * (|want| + max|want|) per element; deterministic mode bit
for bit over two runs; gradients written into an attached GradBucket against unattached ones; a HIP-graph replay of the flagship train
step against the eager step; and the shapes the launch-wide sizing has to survive."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from single_shot_detection_amd import ops
from single_shot_detection_amd.distributed import GradBucket

pytestmark = pytest.mark.gpu


def _close(got, want, bar=1e-4, err_msg=''):
    """test_conv_bn_gpu._close: |got - want| <= 1e-4 * (|want| + max|want|) for every element."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (err_msg, got.shape, want.shape)
    scale = float(np.abs(want).max()) if want.size else 0.0
    err = np.abs(got - want)
    tol = bar * (np.abs(want) + scale) + 1e-12
    bad = err > tol
    assert not bad.any(), (err_msg, int(bad.sum()), float((err / tol).max()), scale)


def _tail(cin, hw, couts):
    """(cin, cout, ksize, stride, pad, hin) of the 's' extras (detector_builder.get_extras): 1 x 1 to cout / 2, then 3 x 3 stride 2 pad 1."""
    out = []
    for c in couts:
        out.append((cin, c // 2, 1, 1, 0, hw))
        out.append((c // 2, c, 3, 2, 1, hw))
        cin, hw = c, (hw + 2 - 3) // 2 + 1
    return out


TAILS = {'ssd300_b32': (32, _tail(512, 18, (512, 256, 256, 256))),
         'ssd512_b16': (16, _tail(512, 32, (512, 256, 256, 256, 256)))}
# what the sizing logic must survive, as groups of (cin, cout, ksize, stride, pad, hin) at a batch:
EDGE_GROUPS = {
    'one_problem': (32, [(256, 512, 3, 2, 1, 18)]),
    'single_split_beside_a_large_one': (32, [(512, 256, 1, 1, 0, 18), (128, 256, 3, 2, 1, 3)]),
    'rows_not_a_multiple_of_32': (3, [(64, 128, 1, 1, 0, 5), (128, 64, 3, 1, 1, 5), (64, 64, 3, 2, 1, 7)]),
    # 2 880 rows = 90 slices beside a small problem: 11 chains of 9 slices would leave the last split without rows
    'last_split_without_rows': (5, [(64, 128, 1, 1, 0, 24), (128, 128, 1, 1, 0, 4)]),
    'cout_4': (8, [(128, 4, 3, 1, 1, 6), (4, 128, 1, 1, 0, 6), (64, 4, 1, 1, 0, 9)]),
    'one_by_one_map': (16, [(256, 128, 1, 1, 0, 1), (128, 256, 3, 2, 1, 1), (128, 256, 3, 1, 1, 1)]),
    'odd_size_under_stride_2': (4, [(64, 128, 3, 2, 1, 7), (64, 128, 3, 2, 1, 5), (32, 64, 3, 2, 0, 9), (128, 64, 1, 2, 0, 5)]),
}


def _inputs(batch, layers, bias, seed):
    rng = np.random.default_rng(seed)
    out = []
    for cin, cout, k, stride, pad, hin in layers:
        ho = (hin + 2 * pad - k) // stride + 1
        out.append(dict(x=rng.standard_normal((batch, cin, hin, hin), dtype=np.float32),
                        w=rng.standard_normal((cout, cin, k, k), dtype=np.float32) * np.float32(1.0 / np.sqrt(cin * k * k)),
                        b=rng.standard_normal((cout,), dtype=np.float32) if bias else None,
                        g=rng.standard_normal((batch, cout, ho, ho), dtype=np.float32), stride=stride, pad=pad))
    return out


def _reference(batch, layers, bias, seed):
    """y, dx, dw, db of every layer from torch's fp32 CPU convolution."""
    out = []
    for t in _inputs(batch, layers, bias, seed):
        x = torch.from_numpy(t['x']).requires_grad_(True)
        w = torch.from_numpy(t['w']).requires_grad_(True)
        b = None if t['b'] is None else torch.from_numpy(t['b']).requires_grad_(True)
        y = F.conv2d(x, w, b, stride=t['stride'], padding=t['pad'])
        (y * torch.from_numpy(t['g'])).sum().backward()
        out.append(dict(y=y.detach().numpy(), dx=x.grad.numpy(), dw=w.grad.numpy(), db=None if b is None else b.grad.numpy()))
    return out


@functools.lru_cache(maxsize=None)
def _tail_reference(name, bias):
    batch, layers = TAILS[name]
    return _reference(batch, layers, bias, 5)


def _run(batch, layers, bias, seed, defer, bucket=False, one_backward=True):
    """The layers on the GPU, independent inputs, ONE backward pass over all of them (deferred: their weight gradients leave in grouped
    launches of up to eight at its end) or one pass per layer; returns per layer y, dx, dw, db as numpy arrays."""
    dev = torch.device('cuda:0')
    ts = _inputs(batch, layers, bias, seed)
    xs = [torch.from_numpy(t['x']).to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True) for t in ts]
    ws = [torch.nn.Parameter(torch.from_numpy(t['w']).to(dev).contiguous(memory_format=torch.channels_last)) for t in ts]
    bs = [None if t['b'] is None else torch.nn.Parameter(torch.from_numpy(t['b']).to(dev)) for t in ts]
    gs = [torch.from_numpy(t['g']).to(dev) for t in ts]
    flat = None
    if bucket:
        flat = GradBucket(ws + [b for b in bs if b is not None]).attach_(dev)
    with ops.deferred_weight_gradients(defer):
        ys = [ops.conv2d(x, w, b, stride=t['stride'], padding=t['pad']) for x, w, b, t in zip(xs, ws, bs, ts)]
        if one_backward:
            sum((y * g).sum() for y, g in zip(ys, gs)).backward()
        else:
            for y, g in zip(ys, gs):
                (y * g).sum().backward()
    torch.cuda.synchronize()
    if bucket:   # the gradients ARE the bucket's slots
        for p, v in zip(flat.params, flat.views):
            assert p.grad is not None and p.grad.data_ptr() == v.data_ptr(), 'a gradient was not written into its bucket slot'
    return [dict(y=y.detach().cpu().numpy(), dx=x.grad.cpu().numpy(), dw=w.grad.cpu().numpy(), db=None if b is None else b.grad.cpu().numpy())
            for y, x, w, b in zip(ys, xs, ws, bs)]


def _check(got, want, what=('y', 'dx', 'dw', 'db')):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        for k in what:
            if b[k] is None:
                assert a[k] is None
                continue
            _close(a[k], b[k], err_msg=f'layer {i} {k}')


def _same_bits(a, b, what=('dx', 'dw', 'db')):
    for i, (p, q) in enumerate(zip(a, b)):
        for k in what:
            if p[k] is None:
                assert q[k] is None
                continue
            assert np.array_equal(p[k].view(np.uint32), q[k].view(np.uint32)), f'layer {i} {k} differs between two runs'


@pytest.mark.parametrize('name', sorted(TAILS))
def test_tail_layers_alone_vs_torch(name):
    batch, layers = TAILS[name]
    _check(_run(batch, layers, False, 5, defer=False, one_backward=False), _tail_reference(name, False))


@pytest.mark.parametrize('bias', [False, True])
@pytest.mark.parametrize('name', sorted(TAILS))
def test_tail_layers_grouped_weight_gradients_vs_torch(name, bias):
    batch, layers = TAILS[name]
    _check(_run(batch, layers, bias, 5, defer=True), _tail_reference(name, bias))


@pytest.mark.parametrize('defer', [False, True])
@pytest.mark.parametrize('name', sorted(TAILS))
def test_tail_layers_deterministic_mode_is_bitwise_reproducible(name, defer):
    batch, layers = TAILS[name]
    with ops.deterministic():
        a = _run(batch, layers, True, 5, defer=defer)
        b = _run(batch, layers, True, 5, defer=defer)
    _same_bits(a, b)
    _check(a, _tail_reference(name, True))


@pytest.mark.parametrize('name', sorted(TAILS))
def test_tail_weight_gradients_in_an_attached_bucket_equal_the_unattached_ones(name):
    batch, layers = TAILS[name]
    with ops.deterministic():   # (fixed summation order: equal means bit for bit)
        plain = _run(batch, layers, True, 5, defer=True)
        attached = _run(batch, layers, True, 5, defer=True, bucket=True)
    _same_bits(plain, attached)
    # the default mode adds its K splits with atomics: both hold to the reference
    _check(_run(batch, layers, True, 5, defer=True, bucket=True), _tail_reference(name, True))


@pytest.mark.parametrize('defer', [False, True])
@pytest.mark.parametrize('name', sorted(EDGE_GROUPS))
def test_sizing_edge_shapes_vs_torch(name, defer):
    batch, layers = EDGE_GROUPS[name]
    want = _reference(batch, layers, True, 17)
    _check(_run(batch, layers, True, 17, defer=defer), want)
    with ops.deterministic():
        a = _run(batch, layers, True, 17, defer=defer)
        b = _run(batch, layers, True, 17, defer=defer)
    _same_bits(a, b)
    _check(a, want)


@pytest.mark.parametrize('name', sorted(TAILS))
def test_deterministic_mode_gives_the_same_bits_grouped_and_alone(name):
    """Deterministic mode keeps the per-problem K splits: a layer's weight gradient has the same bits whether its launch is its own or
    a deferred group's (what the graphed hot path against the eager step relies on)."""
    batch, layers = TAILS[name]
    with ops.deterministic():
        alone = _run(batch, layers, True, 5, defer=False)
        grouped = _run(batch, layers, True, 5, defer=True)
    _same_bits(alone, grouped)


def test_deterministic_workspace_is_that_of_the_problems_alone():
    """The K-split copies of deterministic mode are sized by the same function as the launch, per problem: a grouped call's workspace is
    the sum of its problems' own, and larger than the default mode's (which keeps no copies)."""
    from single_shot_detection_amd import _lib
    lib = _lib.lib()
    batch, layers = TAILS['ssd300_b32']
    dev = torch.device('cuda:0')
    keep = []

    def desc_array(sel):
        arr = (_lib.ConvDesc * len(sel))()
        for d, (cin, cout, k, stride, pad, hin) in zip(arr, sel):
            ho = (hin + 2 * pad - k) // stride + 1
            x = torch.zeros((batch, hin, hin, cin), device=dev)
            w = torch.zeros((cout, k, k, cin), device=dev)
            dy = torch.zeros((batch, ho, ho, cout), device=dev)
            dw = torch.zeros((cout, k, k, cin), device=dev)
            keep.extend([x, w, dy, dw])
            d.x, d.hin, d.win, d.cin = x.data_ptr(), hin, hin, cin
            d.w, d.bias, d.cout, d.ksize, d.stride, d.pad, d.relu = w.data_ptr(), None, cout, k, stride, pad, 0
            d.dy, d.dx, d.dw, d.db = dy.data_ptr(), None, dw.data_ptr(), None
        return arr

    with ops.deterministic():
        together = lib.ssdk_conv2d_bwd_workspace_bytes(desc_array(layers), len(layers), batch)
        alone = sum(lib.ssdk_conv2d_bwd_workspace_bytes(desc_array([l]), 1, batch) for l in layers)
    plain = lib.ssdk_conv2d_bwd_workspace_bytes(desc_array(layers), len(layers), batch)
    assert plain < together == alone, (plain, together, alone)


def test_graph_replay_of_the_flagship_train_step_matches_the_eager_step():
    """SSD-300, 81 classes, batch 32 (the benchmark's step) under the existing graph test's comparison."""
    import test_end_to_end_gpu
    test_end_to_end_gpu.test_graphed_training_steps_match_eager_ones('ssd_300_vgg16_voc', 32)
