"""A float64 model of F.interpolate(mode='bilinear', align_corners=False) and its backward, and the error bounds the fp32 kernels
(ssdk_upsample_bilinear_add_fwd / _bwd, csrc/norm.hip) are held to.  Shared by tests/test_bilinear_reference.py (the model against torch
on the CPU) and tests/test_bilinear_gpu.py (the kernels against the model).

Per axis, for output index dst of `n_out` from `n_in` inputs:  src = max(n_in / n_out * (dst + 0.5) - 0.5, 0), i0 = min(floor(src),
n_in - 1), i1 = i0 + (i0 < n_in - 1), l1 = clamp(src - i0, 0, 1), l0 = 1 - l1 -- the ratio exact, everything in float64.  As a matrix
W[n_out, n_in] with W[dst, i0] += l0, W[dst, i1] += l1:  forward Wy . X . Wx^T, backward Wy^T . G . Wx.

Bounds (derived, not tuned).  A source position computed in fp32 is off by up to about one ulp of src < n_in (the rounded n_in / n_out, the
fused or unfused multiply-add), i.e. 2^-23 * n_in.  The interpolant is continuous and piecewise linear in src with slope |v1 - v0| <=
2 max|v|, so a tap weight that is off by 2^-23 * n_in per axis moves the output by at most 2^-22 * n_in * max|coarse| per axis, also where
i0 flips at an integer; the blend's own roundings are a few ulp of max|coarse|, covered by the + 4:
    forward:   |got - model| <= 2^-21 * (hc + wc + 4) * max|coarse|   (+ 2^-24 * |out| for the rounding of fine + value)
    backward:  the same per-tap bound, times (ny + 2) * (nx + 2) * max|dout| -- ny, nx the largest numbers of fine rows / columns that feed
               one coarse row / column in the model (+ 2: a tap that the fp32 position moves across an integer lands on the neighbour)."""
import numpy as np


def axis_matrix(n_in, n_out):
    """W [n_out, n_in] float64 of one axis."""
    dst = np.arange(n_out, dtype=np.float64)
    src = np.maximum(n_in / n_out * (dst + 0.5) - 0.5, 0.0)
    i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = np.clip(src - i0, 0.0, 1.0)
    w = np.zeros((n_out, n_in), np.float64)
    np.add.at(w, (np.arange(n_out), i0), 1.0 - l1)
    np.add.at(w, (np.arange(n_out), i1), l1)
    return w


def forward(coarse, hf, wf):
    """coarse [B, C, hc, wc] -> [B, C, hf, wf] in float64."""
    x = np.asarray(coarse, np.float64)
    wy, wx = axis_matrix(x.shape[2], hf), axis_matrix(x.shape[3], wf)
    return np.matmul(np.matmul(wy, x), wx.T)


def backward(dout, hc, wc):
    """dout [B, C, hf, wf] -> dcoarse [B, C, hc, wc] in float64."""
    g = np.asarray(dout, np.float64)
    wy, wx = axis_matrix(hc, g.shape[2]), axis_matrix(wc, g.shape[3])
    return np.matmul(np.matmul(wy.T, g), wx)


def fan_in(n_in, n_out):
    """The largest number of outputs that read one input along an axis in the model."""
    return int((axis_matrix(n_in, n_out) != 0).sum(axis=0).max())


def forward_bound(hc, wc, max_coarse, out=None):
    """Elementwise bound of |kernel - model| for the forward; `out` (the model's fine + value) adds the rounding of the final add."""
    b = 2.0 ** -21 * (hc + wc + 4) * float(max_coarse)
    return b if out is None else b + 2.0 ** -24 * np.abs(out)


def backward_bound(hc, wc, hf, wf, max_dout):
    return 2.0 ** -21 * (hc + wc + 4) * (fan_in(hc, hf) + 2) * (fan_in(wc, wf) + 2) * float(max_dout)
