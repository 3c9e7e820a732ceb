"""Numpy model of the grouped depthwise convolution (ssdk_depthwise_conv2d_group_*): one k x k depthwise stencil, shared weight
[C, k, k] and bias [C], over a list of NHWC maps [B, H_l, W_l, C].  Everything is computed in the dtype asked for -- int64 (exact on
integer operands) or float64 -- by shifted slices of the zero-padded map, so no summation order of the kernels is imitated.

  forward(xs, w, bias, stride, pad)          -> [y_l]
  data_grad(dys, w, shapes, stride, pad)     -> [dx_l]
  weight_grad(xs, dys, k, stride, pad)       -> dw [C, k, k], db [C]
  weight_grad_terms(xs, dys, k, stride, pad) -> (n_w [k, k], abs_w [C, k, k], n_b, abs_b [C]): per element of dw / db the number of
      products the kernels add (taps that fall on the zero padding add nothing) and the sum of their magnitudes -- the two figures of
      the bound |fp32 sum in any order - exact sum| <= 1.01 * n * 2^-24 * sum |terms|.
"""
import numpy as np


def out_dim(n, k, stride, pad):
    return (n + 2 * pad - k) // stride + 1


def _padded(x, pad):
    return np.pad(x, ((0, 0), (pad, pad), (pad, pad), (0, 0)))


def _window(ky, kx, ho, wo, stride):
    return (slice(None), slice(ky, ky + stride * (ho - 1) + 1, stride), slice(kx, kx + stride * (wo - 1) + 1, stride), slice(None))


def forward(xs, w, bias, stride, pad, dtype=np.float64):
    w = np.asarray(w, dtype)
    k = w.shape[-1]
    ys = []
    for x in xs:
        x = np.asarray(x, dtype)
        B, H, W, C = x.shape
        ho, wo = out_dim(H, k, stride, pad), out_dim(W, k, stride, pad)
        xp = _padded(x, pad)
        y = np.zeros((B, ho, wo, C), dtype)
        if bias is not None:
            y += np.asarray(bias, dtype)
        for ky in range(k):
            for kx in range(k):
                y += w[:, ky, kx] * xp[_window(ky, kx, ho, wo, stride)]
        ys.append(y)
    return ys


def data_grad(dys, w, shapes, stride, pad, dtype=np.float64):
    w = np.asarray(w, dtype)
    k = w.shape[-1]
    dxs = []
    for dy, (H, W) in zip(dys, shapes):
        dy = np.asarray(dy, dtype)
        B, ho, wo, C = dy.shape
        dxp = np.zeros((B, H + 2 * pad, W + 2 * pad, C), dtype)
        for ky in range(k):
            for kx in range(k):
                dxp[_window(ky, kx, ho, wo, stride)] += w[:, ky, kx] * dy
        dxs.append(np.ascontiguousarray(dxp[:, pad:pad + H, pad:pad + W, :]))
    return dxs


def weight_grad(xs, dys, k, stride, pad, dtype=np.float64):
    C = xs[0].shape[-1]
    dw = np.zeros((C, k, k), dtype)
    db = np.zeros((C,), dtype)
    for x, dy in zip(xs, dys):
        xp = _padded(np.asarray(x, dtype), pad)
        dy = np.asarray(dy, dtype)
        _, ho, wo, _ = dy.shape
        db += dy.sum(axis=(0, 1, 2))
        for ky in range(k):
            for kx in range(k):
                dw[:, ky, kx] += (dy * xp[_window(ky, kx, ho, wo, stride)]).sum(axis=(0, 1, 2))
    return dw, db


def weight_grad_terms(xs, dys, k, stride, pad):
    C = xs[0].shape[-1]
    n_w = np.zeros((k, k), np.int64)
    abs_w = np.zeros((C, k, k), np.float64)
    n_b, abs_b = 0, np.zeros((C,), np.float64)
    for x, dy in zip(xs, dys):
        x = np.asarray(x, np.float64)
        dy = np.asarray(dy, np.float64)
        B, ho, wo, _ = dy.shape
        xp = _padded(x, pad)
        inside = _padded(np.ones(x.shape[:3] + (1,), np.int64), pad)
        n_b += B * ho * wo
        abs_b += np.abs(dy).sum(axis=(0, 1, 2))
        for ky in range(k):
            for kx in range(k):
                win = _window(ky, kx, ho, wo, stride)
                n_w[ky, kx] += int(inside[win].sum())
                abs_w[:, ky, kx] += np.abs(dy * xp[win]).sum(axis=(0, 1, 2))
    return n_w, abs_w, n_b, abs_b


# name: (batch, channels, levels [(h, w)], ksize, stride, pad) -- the smallest shapes that reach every branch of the kernels
PYRAMID4 = [(7, 5), (4, 3), (2, 2), (1, 1)]
CASES = {
    'c8_k3': (3, 8, PYRAMID4, 3, 1, 1),
    'c260_k3': (3, 260, PYRAMID4, 3, 1, 1),                    # 65 channel quads: the second channel block holds one quad
    'c8_k5_shrinks': (3, 8, [(7, 5), (4, 3), (3, 3)], 5, 1, 1),
    'c8_k3_stride2': (3, 8, PYRAMID4, 3, 2, 1),
    'c32_8levels': (2, 32, [(n, n) for n in range(9, 1, -1)], 3, 1, 1),
    'c64_chunks': (4, 64, [(16, 16), (9, 7), (3, 3), (1, 1)], 3, 1, 1),    # 1 316 output pixels: chunk boundaries inside levels
    'c128_chunks': (4, 128, [(16, 16), (9, 7), (3, 3), (1, 1)], 3, 1, 1),
    'c16_chunks': (4, 16, [(16, 16), (9, 7), (3, 3), (1, 1)], 3, 1, 1),
}


def integer_operands(name, seed=0):
    """x, dy in {-3..3}, w in {-2..2}, bias in {-4..4} as float32 arrays: every sum is an integer far below 2^24."""
    B, C, levels, k, stride, pad = CASES[name]
    rng = np.random.default_rng(seed)
    xs = [rng.integers(-3, 4, (B, h, w, C)).astype(np.float32) for h, w in levels]
    dys = [rng.integers(-3, 4, (B, out_dim(h, k, stride, pad), out_dim(w, k, stride, pad), C)).astype(np.float32) for h, w in levels]
    weight = rng.integers(-2, 3, (C, k, k)).astype(np.float32)
    bias = rng.integers(-4, 5, (C,)).astype(np.float32)
    return xs, dys, weight, bias


def normal_operands(name, seed=1):
    B, C, levels, k, stride, pad = CASES[name]
    rng = np.random.default_rng(seed)
    xs = [rng.standard_normal((B, h, w, C), dtype=np.float32) for h, w in levels]
    dys = [rng.standard_normal((B, out_dim(h, k, stride, pad), out_dim(w, k, stride, pad), C), dtype=np.float32) for h, w in levels]
    weight = rng.standard_normal((C, k, k), dtype=np.float32)
    bias = rng.standard_normal((C,), dtype=np.float32)
    return xs, dys, weight, bias
