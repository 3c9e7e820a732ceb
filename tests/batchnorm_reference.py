"""float64 numpy model of the BatchNorm family of csrc/norm.hip (no torch, no GPU): what the kernels are compared with.

`reference` is the operation in float64.  `ideal_fp32` is the same operation as the best fp32 kernel could do it -- the exact
statistics rounded ONCE to float32, then the elementwise chain in float32 -- and is the yardstick of the tolerances: a kernel is held
to a small multiple of |ideal_fp32 - reference|, a figure that comes from the number format and never from the library.
test_batchnorm_reference.py pins `reference` against torch.nn.BatchNorm2d in float64 before anything is compared with it.

Layout: x, y, dy, dx are [rows, C] (NHWC maps flattened over batch and pixels), everything per channel is [C].
relu bit 0: the norm's own fused ReLU (y = max(y, 0); dy' = dy where y > 0, else 0).
relu bit 1 (backward only): x is the output of a ReLU whose gradient is taken here too (dx = 0 where not x > 0).
"""
import numpy as np

F64 = np.float64
F32 = np.float32


def _f64(a):
    return None if a is None else np.asarray(a, F64)


def statistics(x):
    """Per-channel (mean, biased variance) of x[rows, C] in float64, two-pass (no cancellation)."""
    x = _f64(x)
    mean = x.sum(axis=0) / x.shape[0]
    var = ((x - mean) ** 2).sum(axis=0) / x.shape[0]
    return mean, var


def raw_sums(x):
    """What a `sums` buffer holds after the forward statistics: (sum x, sum x^2, rows), float64."""
    x = _f64(x)
    return x.sum(axis=0), (x * x).sum(axis=0), float(x.shape[0])


def reference(x, gamma=None, beta=None, running_mean=None, running_var=None, momentum=0.1, eps=1e-5, training=True, relu=0, dy=None,
              stats_of=None):
    """Forward (and, with `dy`, backward) of BatchNorm (+ ReLU bits) in float64.

    stats_of: the rows the training statistics are taken over when they are not the call's own (synchronised statistics: the sums and
    the row count of all ranks); the backward sums it then returns are still those of the local rows (`sums_dy`, `sums_dy_xhat`) and the
    ones dx is formed from have to be handed in by the caller through `backward`.
    Returns a dict; see the keys below."""
    x = _f64(x)
    rows, C = x.shape
    gamma, beta, running_mean, running_var = _f64(gamma), _f64(beta), _f64(running_mean), _f64(running_var)
    eps, momentum = F64(eps), F64(momentum)
    out = {}
    if training:
        src = x if stats_of is None else _f64(stats_of)
        n = src.shape[0]
        mean, var = statistics(src)
        unbias = n / (n - 1.0) if n > 1 else 1.0   # (rows == 1: the kernel defines the factor as 1, torch refuses the call)
        out['sum_x'], out['sum_x2'], out['count'] = raw_sums(src)
        if running_mean is not None:
            out['running_mean'] = (1.0 - momentum) * running_mean + momentum * mean
        if running_var is not None:
            out['running_var'] = (1.0 - momentum) * running_var + momentum * var * unbias
        out['batch_var'], out['batch_var_unbiased'] = var, var * unbias
    else:
        mean, var = running_mean, running_var
        out['running_mean'], out['running_var'] = running_mean, running_var
    rstd = 1.0 / np.sqrt(var + eps)
    xhat = (x - mean) * rstd
    y = xhat * (1.0 if gamma is None else gamma) + (0.0 if beta is None else beta)
    if relu & 1:
        y = np.maximum(y, 0.0)
    out.update(y=y, save_mean=mean, save_rstd=rstd, xhat=xhat)
    if dy is not None:
        out.update(backward(x, y, dy, gamma, mean, rstd, relu, training))
    return out


def backward(x, y, dy, gamma, save_mean, save_rstd, relu=0, training=True, global_sums=None):
    """dx, dgamma, dbeta and the backward sums, float64.  global_sums = (sum dy', sum dy' xhat, rows) to form dx from sums that are not
    the local ones (synchronised statistics); dgamma / dbeta are always the local sums."""
    x, dy = _f64(x), _f64(dy)
    rows = x.shape[0]
    g = dy.copy()
    if relu & 1:
        g[~(_f64(y) > 0.0)] = 0.0
    xhat = (x - _f64(save_mean)) * _f64(save_rstd)
    s_dy, s_dyx = g.sum(axis=0), (g * xhat).sum(axis=0)
    v = g
    if training:
        t_dy, t_dyx, n = (s_dy, s_dyx, float(rows)) if global_sums is None else global_sums
        v = g - _f64(t_dy) / n - xhat * (_f64(t_dyx) / n)
    dx = (1.0 if gamma is None else _f64(gamma)) * _f64(save_rstd) * v
    if relu & 2:
        dx = np.where(x > 0.0, dx, 0.0)
    return dict(dx=dx, dgamma=s_dyx, dbeta=s_dy, sums_dy=s_dy, sums_dy_xhat=s_dyx)


def ideal_fp32(x, gamma=None, beta=None, running_mean=None, running_var=None, momentum=0.1, eps=1e-5, training=True, relu=0, dy=None,
               stats_of=None):
    """The operation as the best fp32 kernel could do it: every statistic exact (from `reference`) and rounded once to float32, the
    elementwise chains evaluated operation by operation in float32.  Keys: y, and dx when dy is given."""
    ref = reference(x, gamma, beta, running_mean, running_var, momentum, eps, training, relu, dy, stats_of)
    x = np.asarray(x, F32)
    m, rs = ref['save_mean'].astype(F32), ref['save_rstd'].astype(F32)
    ga = np.ones_like(m) if gamma is None else np.asarray(gamma, F32)
    be = np.zeros_like(m) if beta is None else np.asarray(beta, F32)
    y = (x - m) * rs * ga + be
    if relu & 1:
        y = np.maximum(y, F32(0))
    out = dict(y=y)
    if dy is not None:
        # The backward is handed save_mean / save_rstd as float32 (the ABI of the library, as of torch): xhat -- in the backward sums as
        # well as in the elementwise chain -- is formed from the ROUNDED statistics, the best any backward can do with what it is given.
        # (The ReLU mask is the reference's: elements are compared, not decisions at a rounding boundary.)
        out['dx'] = ideal_fp32_backward(x, ref['y'], dy, gamma, m, rs, relu, training)['dx']
    return out


def ideal_fp32_backward(x, y, dy, gamma, save_mean, save_rstd, relu=0, training=True, global_sums=None):
    """`backward` as the best fp32 kernel could do it, given save_mean / save_rstd: they are rounded once to float32 (a no-op when they
    are handed over as float32), the backward sums are those of `backward` over the xhat they define, exact, divided by the row count and
    rounded once to float32; the chain dx = gamma * rstd * (dy' - (m1 + xhat * m2)) in float32."""
    save_mean, save_rstd = np.asarray(save_mean, F64).astype(F32), np.asarray(save_rstd, F64).astype(F32)
    ref = backward(x, y, dy, gamma, save_mean, save_rstd, relu, training, global_sums)
    x = np.asarray(x, F32)
    m, rs = np.asarray(save_mean, F64).astype(F32), np.asarray(save_rstd, F64).astype(F32)
    ga = np.ones_like(m) if gamma is None else np.asarray(gamma, F32)
    g = np.asarray(dy, F32).copy()
    if relu & 1:
        g[~(np.asarray(y) > 0)] = 0
    v = g
    if training:
        t_dy, t_dyx, n = (ref['sums_dy'], ref['sums_dy_xhat'], float(x.shape[0])) if global_sums is None else global_sums
        xhat = (x - m) * rs
        v = g - ((np.asarray(t_dy, F64) / n).astype(F32) + xhat * (np.asarray(t_dyx, F64) / n).astype(F32))
    dx = ga * rs * v
    if relu & 2:
        dx = np.where(x > 0, dx, F32(0))
    return dict(dx=dx.astype(F32))


def elementwise_bar(ideal, ref, margin=4.0):
    """Per-channel tolerance of an elementwise output [rows, C]: margin * max_rows |ideal_fp32 - reference| + margin * 2^-24 * max_rows
    |reference| (the margin of 4: FMA contraction and the device's reciprocal square root)."""
    ideal, ref = np.asarray(ideal, F64), np.asarray(ref, F64)
    return margin * np.abs(ideal - ref).max(axis=0) + margin * 2.0 ** -24 * np.abs(ref).max(axis=0)


def ulps_fp32(got, want64):
    """|got - float32(want)| in units of the float32 spacing at want."""
    want32 = np.asarray(want64, F64).astype(F32)
    return np.abs(np.asarray(got, F64) - want32.astype(F64)) / np.spacing(np.maximum(np.abs(want32), np.finfo(F32).tiny)).astype(F64)


def nearest_src_index(n_in, n_out):
    """Source index of every destination index of a nearest-neighbour resize n_in -> n_out by the rule of the up-sampling kernels:
    min(floorf(dst * ((float)n_in / (float)n_out)), n_in - 1), in float32."""
    scale = F32(n_in) / F32(n_out)
    src = np.floor(np.arange(n_out, dtype=F32) * scale).astype(np.int64)
    return np.minimum(src, n_in - 1)
