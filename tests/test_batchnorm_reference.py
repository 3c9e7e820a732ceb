"""The float64 numpy model the BatchNorm kernels are tested against (tests/batchnorm_reference.py) agrees with torch.nn.BatchNorm2d in
float64 on the CPU to 1e-12 -- outputs, buffers after one step, autograd gradients, training and evaluation mode, with and without
affine parameters, the ReLU bits against torch.relu composed around the module.  And the nearest-neighbour index rule of the up-sampling
kernels agrees with torch's CPU kernel for every size pair up to 48 x 48.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import batchnorm_reference as bnref

B, H, W = 3, 5, 4   # rows = 60


def _rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    return float(np.abs(got - want).max() / max(float(np.abs(want).max()), 1e-300))


def _rows(t):   # [B, C, H, W] -> [rows, C]
    return t.detach().permute(0, 2, 3, 1).reshape(-1, t.shape[1]).numpy()


def _maps(a):   # [rows, C] -> [B, C, H, W]
    return torch.from_numpy(np.ascontiguousarray(a.reshape(B, H, W, -1).transpose(0, 3, 1, 2)))


@pytest.mark.parametrize('relu', [0, 1, 2, 3])
@pytest.mark.parametrize('affine', [True, False])
@pytest.mark.parametrize('training', [True, False])
def test_reference_equals_torch_batchnorm2d_in_float64(training, affine, relu):
    C = 6
    rng = np.random.default_rng(17 + relu)
    x0 = rng.standard_normal((B * H * W, C)) * rng.uniform(0.5, 3.0, C) + rng.uniform(-2.0, 2.0, C)
    dy = rng.standard_normal((B * H * W, C))
    momentum, eps = 0.3, 1e-3
    bn = torch.nn.BatchNorm2d(C, eps=eps, momentum=momentum, affine=affine).double()
    with torch.no_grad():
        bn.running_mean.copy_(torch.from_numpy(rng.standard_normal(C)))
        bn.running_var.copy_(torch.from_numpy(rng.uniform(0.5, 2.0, C)))
        if affine:
            bn.weight.copy_(torch.from_numpy(rng.uniform(0.5, 1.5, C) * rng.choice([-1.0, 1.0], C)))
            bn.bias.copy_(torch.from_numpy(rng.standard_normal(C)))
    rm0, rv0 = bn.running_mean.numpy().copy(), bn.running_var.numpy().copy()
    gamma = bn.weight.detach().numpy().copy() if affine else None
    beta = bn.bias.detach().numpy().copy() if affine else None
    bn.train(training)

    leaf = _maps(x0).requires_grad_(True)
    xin = torch.relu(leaf) if relu & 2 else leaf     # bit 1: the norm's input is a ReLU output, and dx is taken through that ReLU
    yt = bn(xin)
    if relu & 1:
        yt = torch.relu(yt)
    yt.backward(_maps(dy))

    x = _rows(xin)
    ref = bnref.reference(x, gamma, beta, rm0, rv0, momentum, eps, training, relu, dy)
    assert _rel(ref['y'], _rows(yt)) <= 1e-12
    assert _rel(ref['dx'], _rows(leaf.grad)) <= 1e-12
    assert _rel(ref['running_mean'], bn.running_mean.numpy()) <= 1e-12
    assert _rel(ref['running_var'], bn.running_var.numpy()) <= 1e-12
    assert int(bn.num_batches_tracked) == (1 if training else 0)
    if affine:
        assert _rel(ref['dgamma'], bn.weight.grad.numpy()) <= 1e-12
        assert _rel(ref['dbeta'], bn.bias.grad.numpy()) <= 1e-12
    if training:
        assert _rel(ref['save_mean'], x.mean(axis=0)) <= 1e-12
        assert _rel(ref['save_rstd'], 1.0 / np.sqrt(x.var(axis=0) + eps)) <= 1e-12
        assert _rel(ref['sum_x'], x.sum(axis=0)) <= 1e-12 and _rel(ref['sum_x2'], (x * x).sum(axis=0)) <= 1e-12
        assert ref['count'] == B * H * W
    else:
        assert _rel(ref['save_rstd'], 1.0 / np.sqrt(rv0 + eps)) <= 1e-12
    # the backward sums are what their names say
    g = dy * (ref['y'] > 0) if relu & 1 else dy
    assert _rel(ref['sums_dy'], g.sum(axis=0)) <= 1e-12
    assert _rel(ref['sums_dy_xhat'], (g * ref['xhat']).sum(axis=0)) <= 1e-12


def test_reference_with_statistics_of_a_larger_row_set_equals_torch_on_the_union():
    """stats_of / global_sums (synchronised statistics): the local half of a batch normalised with the statistics of the whole batch is the
    local half of torch's output on the whole batch, and so is dx when it is formed from the whole batch's backward sums."""
    C = 4
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2 * B * H * W, C)) * 2.0 + 1.0
    dy = rng.standard_normal(x.shape)
    gamma, beta = rng.uniform(0.5, 1.5, C), rng.standard_normal(C)
    bn = torch.nn.BatchNorm2d(C).double().train()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(gamma)); bn.bias.copy_(torch.from_numpy(beta))
    xt = torch.from_numpy(x.reshape(2 * B, H, W, C).transpose(0, 3, 1, 2).copy()).requires_grad_(True)
    yt = bn(xt)
    yt.backward(torch.from_numpy(dy.reshape(2 * B, H, W, C).transpose(0, 3, 1, 2).copy()))
    n = B * H * W
    whole = bnref.reference(x, gamma, beta, np.zeros(C), np.ones(C), 0.1, 1e-5, True, 0, dy)
    local = bnref.reference(x[:n], gamma, beta, np.zeros(C), np.ones(C), 0.1, 1e-5, True, 0, None, stats_of=x)
    assert _rel(local['y'], _rows(yt)[:n]) <= 1e-12
    assert _rel(local['running_var'], bn.running_var.numpy()) <= 1e-12
    back = bnref.backward(x[:n], None, dy[:n], gamma, local['save_mean'], local['save_rstd'], 0, True,
                          global_sums=(whole['sums_dy'], whole['sums_dy_xhat'], float(2 * n)))
    assert _rel(back['dx'], _rows(xt.grad)[:n]) <= 1e-12
    assert _rel(back['dbeta'], dy[:n].sum(axis=0)) <= 1e-12


def test_reference_defines_one_row_as_the_kernel_does():
    ref = bnref.reference(np.array([[1.5, -2.0, 0.0, 7.0]]), None, None, np.zeros(4), np.ones(4), 0.5, 1e-5, True)
    assert np.array_equal(ref['save_mean'], [1.5, -2.0, 0.0, 7.0])
    assert np.array_equal(ref['batch_var_unbiased'], np.zeros(4))
    assert np.array_equal(ref['running_var'], np.full(4, 0.5))
    assert np.array_equal(ref['y'], np.zeros((1, 4)))


def test_ideal_fp32_is_float32_and_close_to_the_reference():
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((64, 8)) * 2.0 + 30.0).astype(np.float32)
    dy = rng.standard_normal((64, 8)).astype(np.float32)
    ref = bnref.reference(x, None, None, None, None, 0.1, 1e-5, True, 0, dy)
    ideal = bnref.ideal_fp32(x, None, None, None, None, 0.1, 1e-5, True, 0, dy)
    assert ideal['y'].dtype == np.float32 and ideal['dx'].dtype == np.float32
    assert np.abs(ideal['y'] - ref['y']).max() < 1e-4 and np.abs(ideal['dx'] - ref['dx']).max() < 1e-5
    bar = bnref.elementwise_bar(ideal['y'], ref['y'])
    assert bar.shape == (8,) and (bar > 0).all()
    assert np.array_equal(bnref.ulps_fp32(np.float32([1.0, 1.0 + 2.0 ** -22]), [1.0, 1.0]), [0.0, 2.0])


def test_nearest_index_rule_of_the_upsampling_kernels_equals_torch_cpu():
    """floorf(dst * ((float)in / (float)out)), clamped: the index arithmetic shared by the up-sampling kernels, against
    F.interpolate(mode='nearest') on the CPU, every pair of sizes up to 48 x 48 in both directions."""
    for n_in in range(1, 49):
        src = torch.arange(n_in, dtype=torch.float32).reshape(1, 1, n_in, 1)
        for n_out in range(1, 49):
            want = F.interpolate(src, size=(n_out, 1), mode='nearest').reshape(-1).numpy().astype(np.int64)
            assert np.array_equal(bnref.nearest_src_index(n_in, n_out), want), (n_in, n_out)
