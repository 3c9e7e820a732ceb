"""GPU: the depthwise RetinaNet-lite tower, SharedConvPredictor(..., use_depthwise=True) (detection/modules/predictors.py:8-76), on libssdk:
per layer and head ONE grouped depthwise stencil over the levels (ops.depthwise_conv2d on a list), ONE grouped 1 x 1 GEMM with the ReLU
and the BatchNorm statistics in its epilogue, and the per-level norm kernels.

* against stock torch modules on the CPU (1e-4, test_conv_bn_gpu.py's rule), train() and eval();
* against fixtures the REFERENCE's own class wrote (tests/golden/tower_depthwise.npz, tools/gen_golden_dwtower.py) at the 2e-5 bar of
  test_blocks_golden_gpu.py;
* no stock convolution / ReLU / BatchNorm kernel and no autograd sum of the shared weights' gradients in forward or backward;
* marked by distributed.convert_sync_batchnorm the per-level norms synchronise: two ranks on half the batch each equal one process on
  the whole batch, and the five norms of a tower layer share one all-reduce;
* another activation (ReLU6) still runs level by level on the stock modules and matches torch."""
import copy
import logging
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import dwtower_cases
from conftest import GOLDEN
from single_shot_detection_amd import ops
from single_shot_detection_amd.bf.modules import conv
from single_shot_detection_amd.detection.modules.predictors import SharedConvPredictor

pytestmark = pytest.mark.gpu


def _close(got, want, bar=1e-4, err_msg='', scale=None):
    """|got - want| <= bar * (|want| + max|want|) for every element: relative to the tensor's own scale, because the GPU's GEMMs and
    reductions sum in another order than torch's CPU kernels (test_conv_bn_gpu.py's rule, restated)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (err_msg, got.shape, want.shape)
    if scale is None:
        scale = float(np.abs(want).max()) if want.size else 0.0
    err = np.abs(got - want)
    tol = bar * (np.abs(want) + scale) + 1e-12
    bad = err > tol
    assert not bad.any(), (err_msg, int(bad.sum()), float((err / tol).max()), scale)


def _randomize(m, rng):
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.from_numpy(rng.standard_normal(tuple(p.shape), dtype=np.float32) * (0.1 if p.dim() > 1 else 0.5) + (1.0 if p.dim() == 1 else 0.0)))


def _ref_forward(ref, srcs, act=torch.relu):
    """predictors.py:60-76 with stock torch ops: the block's submodules in order -> activation -> the level's norm."""
    def block(b, x):
        for name in ('depthwise_conv', 'depthwise_bn', 'depthwise_activation', 'pointwise_conv', 'pointwise_bn', 'pointwise_activation'):
            if name in b._modules:
                x = b._modules[name](x)
        return x
    s = l = list(srcs)
    for sc, lc, sn, ln in zip(ref.convs['score'], ref.convs['loc'], ref.norms['score'], ref.norms['loc']):
        s = [n(act(block(sc, x))) for n, x in zip(sn, s)]
        l = [n(act(block(lc, x))) for n, x in zip(ln, l)]
    return s, l


def _compare_with_torch(tower, ref, xs_np, rng, act=torch.relu):
    xr = [torch.from_numpy(x).requires_grad_(True) for x in xs_np]
    xg = [torch.from_numpy(x).cuda().requires_grad_(True) for x in xs_np]
    sr, lr = _ref_forward(ref, xr, act)
    sg, lg = tower(xg)
    gw = [torch.from_numpy(rng.standard_normal(tuple(a.shape), dtype=np.float32)) for a in sr + lr]   # sum(BN(x)) alone has zero gradient
    tot_r = sum((a * a).sum() for a in sr) + sum((a * g).sum() for a, g in zip(sr + lr, gw))
    tot_g = sum((a * a).sum() for a in sg) + sum((a * g.cuda()).sum() for a, g in zip(list(sg) + list(lg), gw))
    for i, (a, b) in enumerate(zip(list(sg) + list(lg), sr + lr)):
        _close(a.detach().cpu().numpy(), b.detach().numpy(), err_msg=f'y{i}')
    tot_r.backward(); tot_g.backward()
    for i, (a, b) in enumerate(zip(xg, xr)):
        _close(a.grad.cpu().numpy(), b.grad.numpy(), err_msg=f'dx{i}')
    for (n1, p1), (n2, p2) in zip(sorted(tower.named_parameters()), sorted(ref.named_parameters())):
        assert n1 == n2
        _close(p1.grad.cpu().numpy(), p2.grad.numpy(), err_msg=n1)
    for (n1, b1), (n2, b2) in zip(sorted(tower.named_buffers()), sorted(ref.named_buffers())):
        assert n1 == n2
        np.testing.assert_allclose(b1.cpu().numpy(), b2.numpy(), rtol=1e-4, atol=1e-5, err_msg=n1)


def _tower(**kw):
    return SharedConvPredictor([32] * 5, [9] * 5, 8, True, num_layers=2, num_channels=32, **kw)


SIZES = [16, 8, 4, 3, 2]   # batch 4: >= 16 rows per BatchNorm


@pytest.mark.parametrize('train', [True, False])
def test_depthwise_tower_vs_torch(train):
    rng = np.random.default_rng(13)
    tower = _tower()
    _randomize(tower, rng)
    ref = copy.deepcopy(tower)
    tower = tower.cuda()
    tower.train(train); ref.train(train)
    _compare_with_torch(tower, ref, [rng.standard_normal((4, 32, h, h), dtype=np.float32) for h in SIZES], rng)


@pytest.fixture(scope='module')
def golden_tower():
    return np.load(os.path.join(GOLDEN, 'tower_depthwise.npz'))


@pytest.mark.parametrize('case', sorted(dwtower_cases.CASES))
def test_depthwise_tower_vs_reference_golden(case, golden_tower):
    got = dwtower_cases.run_case(case, SharedConvPredictor, torch.device('cuda'))
    want = {k: golden_tower[k] for k in golden_tower.files if k.startswith(case + '/')}
    ratio, key = dwtower_cases.worst_ratio(got, want, 2e-5)
    print(f'{case}: worst entry at {ratio:.3f} of the 2e-5 bar ({key})')
    assert ratio <= 1.0, (key, ratio)


# ---- what runs ---------------------------------------------------------------------------------------------------------------------

FWD_BANNED = ('aten.convolution', 'aten._convolution', 'aten.cudnn_convolution', 'aten.miopen_convolution', 'aten.miopen_depthwise_convolution',
              'aten.relu', 'aten.threshold', 'aten.clamp_min', 'aten.native_batch_norm', 'aten._native_batch_norm', 'aten.miopen_batch_norm',
              'aten.batch_norm', 'aten.cudnn_batch_norm')
BWD_BANNED = ('aten.convolution_backward', 'aten.miopen_convolution_backward', 'aten.miopen_depthwise_convolution_backward', 'aten.threshold_backward',
              'aten.native_batch_norm_backward', 'aten.miopen_batch_norm_backward', 'aten.cudnn_batch_norm_backward')


def _recorder():
    from torch.utils._python_dispatch import TorchDispatchMode

    class _Rec(TorchDispatchMode):
        def __init__(self):
            super().__init__()
            self.names, self.adds = [], []

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            name = str(func)
            self.names.append(name)
            if name.startswith(('aten.add.Tensor', 'aten.add_.Tensor')):
                self.adds.append(tuple(args[0].shape))
            return func(*args, **(kwargs or {}))
    return _Rec()


@pytest.mark.parametrize('train', [True, False])
def test_no_stock_kernel_in_forward_or_backward(train, caplog):
    tower = _tower().cuda().train(train)
    rng = np.random.default_rng(3)
    xs = [torch.from_numpy(rng.standard_normal((4, 32, h, h), dtype=np.float32)).cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
          for h in SIZES]
    conv._warned.clear()
    with caplog.at_level(logging.WARNING):
        rec = _recorder()
        with rec:
            s, l = tower(xs)
        bad = [n for n in rec.names if n.startswith(FWD_BANNED)]
        assert not bad, bad
        assert rec.names, 'the recorder saw nothing'
        outs = list(s) + list(l)
        rec = _recorder()
        with rec:
            torch.autograd.backward(outs, [torch.ones_like(o) for o in outs])
    bad = [n for n in rec.names if n.startswith(BWD_BANNED + FWD_BANNED)]
    assert not bad, bad
    # a weight shared by the levels gets ONE gradient from the grouped kernels: autograd has nothing to add up (the two heads' input
    # gradients of a level are added, and only those)
    weight_shapes = {tuple(p.shape) for p in tower.convs.parameters()}
    assert not [shape for shape in rec.adds if shape in weight_shapes], rec.adds
    assert all(x.grad is not None for x in xs) and all(p.grad is not None for p in tower.parameters())
    assert not [r.getMessage() for r in caplog.records if 'stock PyTorch-ROCm' in r.getMessage()]


# ---- synchronised statistics -------------------------------------------------------------------------------------------------------

def _sync_tower():
    return SharedConvPredictor([16, 16], [3, 3], 5, True, num_layers=2, num_channels=16)


def _sync_bn_rank(rank, world, port, out_dir):
    import torch.distributed as dist
    from single_shot_detection_amd.distributed import convert_sync_batchnorm
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    torch.cuda.set_device(0)
    d = np.load(os.path.join(out_dir, 'in.npz'))
    torch.manual_seed(0)
    tower = _sync_tower()
    tower.load_state_dict({k: torch.from_numpy(v) for k, v in np.load(os.path.join(out_dir, 'state.npz')).items()})
    tower = convert_sync_batchnorm(tower).cuda().train()
    half = slice(rank * 2, rank * 2 + 2)
    xs = [torch.from_numpy(d[f'x{i}'][half]).cuda().requires_grad_(True) for i in range(2)]
    s, l = tower(xs)
    gs = [torch.from_numpy(d[f'g{i}'][half]).cuda() for i in range(4)]
    loss = sum((y * g).sum() for y, g in zip(list(s) + list(l), gs))
    loss.backward()
    out = {f'y{i}': y.detach().cpu().numpy() for i, y in enumerate(list(s) + list(l))}
    out.update({f'dx{i}': x.grad.cpu().numpy() for i, x in enumerate(xs)})
    out.update({'p_' + n: p.grad.cpu().numpy() for n, p in tower.named_parameters()})
    out.update({'b_' + n: b.cpu().numpy() for n, b in tower.named_buffers()})
    np.savez(os.path.join(out_dir, f'out{rank}.npz'), **out)
    dist.destroy_process_group()


def test_sync_batchnorm_two_ranks_equal_one_process_on_the_whole_batch(tmp_path):
    """Two ranks (both on this one GPU, gloo between them), half the batch each, through a DEPTHWISE tower whose per-level norms are
    marked for synchronisation == the same tower in ONE process on the whole batch with torch's own modules on the CPU: outputs, running
    statistics, input gradients; parameter gradients sum over the ranks.  (With the norms called as plain torch modules every rank
    normalised with its own half's statistics.)"""
    import socket
    import torch.multiprocessing as mp
    rng = np.random.default_rng(5)
    torch.manual_seed(0)
    tower = _sync_tower()
    with torch.no_grad():
        for n, p in tower.named_parameters():
            p.copy_(torch.from_numpy(rng.standard_normal(tuple(p.shape), dtype=np.float32) * (0.2 if p.dim() > 1 else 0.5)) + (1.0 if n.endswith('weight') and p.dim() == 1 else 0.0))
    np.savez(tmp_path / 'state.npz', **{k: v.numpy() for k, v in tower.state_dict().items()})
    data = {'x0': rng.standard_normal((4, 16, 6, 6), dtype=np.float32), 'x1': rng.standard_normal((4, 16, 3, 3), dtype=np.float32)}
    for i, hw in enumerate((6, 3, 6, 3)):
        data[f'g{i}'] = rng.standard_normal((4, 16, hw, hw), dtype=np.float32)
    np.savez(tmp_path / 'in.npz', **data)
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_sync_bn_rank, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    ref = _sync_tower()
    ref.load_state_dict(tower.state_dict())
    ref.train()
    xs = [torch.from_numpy(data[f'x{i}']).requires_grad_(True) for i in range(2)]
    ss, ls = _ref_forward(ref, xs)
    sum((y * torch.from_numpy(data[f'g{i}'])).sum() for i, y in enumerate(ss + ls)).backward()
    outs = [np.load(tmp_path / f'out{r}.npz') for r in range(2)]
    for i, y in enumerate(ss + ls):
        _close(np.concatenate([outs[0][f'y{i}'], outs[1][f'y{i}']], 0), y.detach().numpy(), err_msg=f'y{i}')
    for i, x in enumerate(xs):
        _close(np.concatenate([outs[0][f'dx{i}'], outs[1][f'dx{i}']], 0), x.grad.numpy(), err_msg=f'dx{i}')
    for n, p in ref.named_parameters():
        _close(outs[0]['p_' + n] + outs[1]['p_' + n], p.grad.numpy(), err_msg=n)
    for n, b in ref.named_buffers():
        for r in range(2):
            np.testing.assert_allclose(outs[r]['b_' + n], b.numpy(), rtol=1e-4, atol=1e-5, err_msg=n)


def test_marked_tower_with_one_rank_is_the_unmarked_one_and_shares_one_exchange_per_layer(monkeypatch):
    """In process, one rank: the marked tower takes the split path (statistics -> [all-reduce] -> apply) -- ONE ops.allreduce_sums_ per
    tower layer and head in the forward for the levels' norms together -- and the norms' outputs are the unmarked tower's bit for bit.
    (Compared layer by layer on the same input of the norms: the grouped GEMM's epilogue statistics of the unmarked path and the
    separate statistics pass of the marked one are checked against each other on the norm alone in test_conv_bn_gpu.py.)"""
    from single_shot_detection_amd.distributed import convert_sync_batchnorm
    rng = np.random.default_rng(17)
    plain = _tower()
    _randomize(plain, rng)
    marked = convert_sync_batchnorm(copy.deepcopy(plain))
    plain, marked = plain.cuda().train(), marked.cuda().train()
    assert all(type(n) is nn.BatchNorm2d and ops.sync_group_of(n) == (None,) for n in marked.norms.modules() if isinstance(n, nn.BatchNorm2d))
    assert all(ops.sync_group_of(n) is None for n in plain.norms.modules() if isinstance(n, nn.BatchNorm2d))
    calls = []
    real = ops.allreduce_sums_
    monkeypatch.setattr(ops, 'allreduce_sums_', lambda buf, group=None: (calls.append(int(buf.numel())), real(buf, group))[1])
    xs = [torch.from_numpy(rng.standard_normal((4, 32, h, h), dtype=np.float32)).cuda() for h in SIZES]
    with torch.no_grad():
        sm, lm = marked(xs)
    assert len(calls) == 2 * 2 and all(c == 5 * (2 * 32 + 2) for c in calls), calls   # 2 layers x 2 heads, five norms packed in each
    with torch.no_grad():
        sp, lp = plain(xs)
    # the norms alone, on identical inputs: the marked norms of the last layer against the unmarked ones
    for head in ('score', 'loc'):
        block = plain.convs[head][0]
        with torch.no_grad():
            ys = ops.depthwise_conv2d(xs, block.depthwise_conv.weight, block.depthwise_conv.bias, 1, 1)
            ys = ops.conv2d(ys, block.pointwise_conv.weight, block.pointwise_conv.bias, relu=True)
            a = [copy.deepcopy(n) for n in plain.norms[head][0]]
            b = [copy.deepcopy(n) for n in a]   # the same buffers to start from; marked below
            for n in b:
                n._ssdk_sync_group = (None,)
            out_a = [ops.batch_norm(y, n) for y, n in zip(ys, a)]
            out_b = ops.batch_norm_levels(ys, b)
        for ya, yb, na, nb in zip(out_a, out_b, a, b):
            assert torch.equal(ya, yb)
            assert torch.equal(na.running_mean, nb.running_mean) and torch.equal(na.running_var, nb.running_var)
    for a, b in zip(list(sm) + list(lm), list(sp) + list(lp)):   # and the whole towers agree to rounding (epilogue statistics against a separate pass)
        _close(a.cpu().numpy(), b.cpu().numpy(), bar=1e-5)


# ---- other activations keep the stock path -----------------------------------------------------------------------------------------

def test_relu6_tower_runs_level_by_level_and_matches_torch():
    """Another activation keeps the level-by-level line: the block's own forward on one map per call, then the stock nn.ReLU6 and
    nn.BatchNorm2d modules.  Held to torch on the CPU at the 1e-4 bar: the outputs in train() mode, and outputs, input gradients and
    every parameter gradient in eval() mode.  The train()-mode GRADIENTS are not compared: on this path the batch statistics and their
    backward are the GPU runtime's own BatchNorm kernels, which sum in fp32, against the CPU's -- measured on an MI355X, the same
    comparison in train() mode left the last level's input gradient at 1.5 of the bar on the five-level shape and a depthwise bias
    gradient at 2.7 of it on levels 16, 8, 4; the library's kernels on this path (stencil, 1 x 1 GEMM) are the ones the eval() comparison
    holds, where the norm is an affine map."""
    rng = np.random.default_rng(29)
    tower = _tower(activation={'name': 'ReLU6', 'args': {'inplace': True}})
    _randomize(tower, rng)
    with torch.no_grad():
        for n, b in tower.named_buffers():
            if n.endswith('running_var'):
                b.copy_(torch.from_numpy(rng.uniform(0.5, 2.0, tuple(b.shape)).astype(np.float32)))
    ref = copy.deepcopy(tower)
    tower = tower.cuda()
    xs_np = [rng.standard_normal((4, 32, h, h), dtype=np.float32) for h in SIZES]
    calls = []
    real = ops.depthwise_conv2d
    try:
        ops.depthwise_conv2d = lambda x, *a, **k: (calls.append(isinstance(x, torch.Tensor)), real(x, *a, **k))[1]
        tower.eval(); ref.eval()
        _compare_with_torch(tower, ref, xs_np, rng, act=nn.functional.relu6)
        tower.train(); ref.train()
        with torch.no_grad():
            sg, lg = tower([torch.from_numpy(x).cuda() for x in xs_np])
            sr, lr = _ref_forward(ref, [torch.from_numpy(x) for x in xs_np], nn.functional.relu6)
        for i, (a, b) in enumerate(zip(list(sg) + list(lg), sr + lr)):
            _close(a.cpu().numpy(), b.numpy(), err_msg=f'train y{i}')
    finally:
        ops.depthwise_conv2d = real
    assert len(calls) == 2 * 2 * 2 * len(SIZES) and all(calls), calls   # one map per call: the block's own forward, level by level
