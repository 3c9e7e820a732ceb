"""Autograd wrappers over libssdk's generic NHWC convolution and BatchNorm (csrc/conv.hip, csrc/norm.hip).

Tensors are logical [B,C,H,W] with channels_last memory (= the NHWC buffers the kernels read); weights are logical
[Cout,Cin,k,k] with channels_last memory (= [Cout][k][k][Cin]).  GPU only -- CPU tensors raise.

The convolution half does each job once: ``_set_desc`` is the only writer of a ``ssdk_conv_desc``, ``_conv_out`` allocates a forward
output, ``_upstream_grad`` prepares what autograd delivers, ``_grad_targets`` says where a parameter's gradient goes, ``_may_defer`` whether
it may wait for the end of the pass, and ``_conv_backward`` is the backward of both convolution Functions (and ``_flush_jobs`` that of the
deferred weight gradients).  ``_sums_chain_of`` / ``_norm_of_ready_sums`` wire a BatchNorm to the convolution that took its statistics.
"""
import ctypes
import os
import weakref

import torch

from . import _lib
from .distributed import grad_sink


def _nhwc(x):
    return x.float().contiguous(memory_format=torch.channels_last)


def _dp(t):
    return None if t is None or t.numel() == 0 else t.data_ptr()


def _out_dim(n, k, s, p):
    return (n + 2 * p - k) // s + 1


def _conv_out(x, cout, k, stride, pad):
    """The (uninitialised) output map of a k x k convolution of the NHWC map ``x`` to ``cout`` channels."""
    batch, _, hin, win = x.shape
    return torch.empty((batch, cout, _out_dim(hin, k, stride, pad), _out_dim(win, k, stride, pad)), dtype=torch.float32, device=x.device,
                       memory_format=torch.channels_last)


def _set_desc(d, hin, win, cin, cout, ksize, stride, pad, x=None, w=None, bias=None, relu=0, y=None, stats=None,
              dy=None, dx=None, dw=None, db=None, w_t=None, dx_is_zero=False):
    """Writes the ssdk_conv_desc ``d`` -- the ONLY place in this module that assigns a field of one, so a field added to the ABI is threaded
    through here and nowhere else.  The geometry is explicit (SFAM's [n_scales, B, C] rows are 1 x 1 maps; prepare_weight_transposes and
    _DxLink.describe give nothing but geometry); the operands are tensors (None or empty: a null pointer), ``stats`` is the address of an
    fp64 `sums` buffer.  ``d`` is fresh (ctypes made it all zeros) and each call writes the half it is for: without ``dy`` the forward
    operands, with it the backward ones (a backward entry point reads neither bias nor y)."""
    d.hin, d.win, d.cin, d.cout, d.ksize, d.stride, d.pad, d.relu = hin, win, cin, cout, ksize, stride, pad, relu
    d.x, d.w = _dp(x), _dp(w)
    if dy is None:
        d.bias, d.y, d.stats = _dp(bias), _dp(y), stats
    else:
        d.dy, d.dx, d.dw, d.db, d.w_t, d.dx_is_zero = _dp(dy), _dp(dx), _dp(dw), _dp(db), _dp(w_t), int(dx_is_zero)


def _upstream_grad(dy, shape, device, y=None, stream=None):
    """What autograd delivered for an output of ``shape``, as the NHWC fp32 map the library reads: zeros for an output nobody used
    downstream (None), and -- ``y``: the saved output of a forward that fused a ReLU -- with that ReLU undone (ssdk_relu_bwd)."""
    dy = torch.zeros(shape, dtype=torch.float32, device=device).contiguous(memory_format=torch.channels_last) if dy is None else _nhwc(dy)
    if y is None:
        return dy
    g = torch.empty_like(dy, memory_format=torch.channels_last)
    _lib.check(_lib.lib().ssdk_relu_bwd(_dp(y), _dp(dy), dy.numel(), _dp(g), stream), 'ssdk_relu_bwd')
    return g


def _grad_targets(w, weight, bias, need_w, need_b):
    """(dw, db): where the library writes (it zeroes them first) the gradients of the parameters ``weight`` -- saved as ``w`` -- and
    ``bias``; None where not needed.  A parameter's slot in a gradient bucket (distributed.GradBucket) when it has one -- for a weight, one
    laid out like ``w`` -- and a fresh tensor otherwise."""
    dw = db = None
    if need_w:
        dw = grad_sink(weight)
        if dw is None or dw.stride() != w.stride():
            dw = torch.empty_like(w, memory_format=torch.channels_last)
    if need_b:
        db = grad_sink(bias)
        if db is None:
            db = torch.empty((w.shape[0],), dtype=torch.float32, device=w.device)
    return dw, db


def _fast_min_flops():
    """fast mode: smaller launches stay fp32 (the library applies the same bound, from the same variable, to the data gradients)."""
    e = os.environ.get('SSDK_FAST_MIN_FLOPS')
    return float(e) if e else 1.0e9


class _ConvFn(torch.autograd.Function):
    """apply(weight, bias, stride, pad, relu, stats, links, *xs) -> tuple of outputs; the n inputs share `weight` (one grouped launch).
    stats: None, or one fp64 `sums` buffer address (or None) per input: the BatchNorm statistics of that output are accumulated into it.
    links: None, or one _DxLink (or None) per input, shared with the norm that consumes that output (conv2d_batch_norm)."""

    @staticmethod
    def forward(ctx, weight, bias, stride, pad, relu, stats, links, *xs):
        lib = _lib.lib()
        _lib.require_cuda(weight, *xs)
        w = weight.float().contiguous(memory_format=torch.channels_last)
        b = None if bias is None else bias.float().contiguous()
        cout, cin, k, k2 = w.shape
        assert k == k2
        xs = [_nhwc(x) for x in xs]
        B = xs[0].shape[0]
        ys = []
        arr = (_lib.ConvDesc * len(xs))()
        for i, x in enumerate(xs):
            assert x.shape[0] == B and x.shape[1] == cin, (tuple(x.shape), cin)
            y = _conv_out(x, cout, k, stride, pad)
            ys.append(y)
            _set_desc(arr[i], x.shape[2], x.shape[3], cin, cout, k, stride, pad, x, w, b, int(bool(relu)), y, None if stats is None else stats[i])
        # opt-in split-bf16 forward (heads.set_fast_mode) -- for launches of at least ~1 GFLOP: below that the split of the weights and the
        # statistics pass behind the launch cost more than three bf16 MFMAs save over one fp32 one (the SSD tail's small layers)
        flops = 2.0 * B * cout * cin * k * k * sum(y.shape[2] * y.shape[3] for y in ys)
        if _lib.fast_mode == 'bf16x3' and cin % 32 == 0 and flops >= _fast_min_flops():
            fw = _lib.scratch(lib.ssdk_conv2d_fwd_fast_workspace_bytes(arr, len(xs)), xs[0].device, 'conv_fwd_fast')
            _lib.check(lib.ssdk_conv2d_fwd_fast(arr, len(xs), B, 3, _dp(fw), fw.numel(), _lib.current_stream()), 'ssdk_conv2d_fwd_fast')
        else:
            _conv2d_fwd(lib, arr, len(xs), B, xs[0].device)
        ctx.w_t = _transposed_weights_of(weight, stride)   # (prepare_weight_transposes ran for this step: the backward skips its re-layout)
        ctx.save_for_backward(w, *xs, *(ys if relu == 1 else []))
        # relu == 2: ReLU in the forward epilogue as usual, but its gradient is taken by the consumer (a BatchNorm that masks its dx where
        # its input is not positive, conv2d_batch_norm): the backward gets dy already masked and skips its own pass over it
        ctx.meta = (stride, pad, relu == 1, len(xs), bias is not None, tuple(tuple(y.shape) for y in ys))
        ctx.params = (weight, bias)   # leaves: their gradient-bucket slots (distributed.GradBucket) are looked up in the backward
        ctx.links = links
        for i, link in enumerate(links or ()):
            if link is not None:
                link.describe(xs[i], cout, k, stride, pad, ctx.needs_input_grad[7 + i])
        return tuple(ys)

    @staticmethod
    def backward(ctx, *dys):
        stride, pad, relu, n, has_bias, yshapes = ctx.meta
        saved = ctx.saved_tensors
        w, xs = saved[0], saved[1:1 + n]
        ys = saved[1 + n:] if relu else [None] * n   # (relu: undo the ReLU fused into the forward epilogue)
        weight, bias = ctx.params
        need = ctx.needs_input_grad
        need_w, need_b = need[0], need[1] and has_bias
        # weight gradients of single-input convolutions can wait for the end of the backward pass: nothing in the chain depends on
        # them, and eight small launches that each underfill the chip become one grouped launch (_flush_weight_gradients)
        defer = n == 1 and (need_w or need_b) and _may_defer(weight, bias)
        links = ctx.links or [None] * n
        grads, launched = _conv_backward([(w, weight, bias, need_w, need_b, defer, xs[i], ys[i], dys[i], yshapes[i], stride, pad, need[7 + i],
                                           ctx.w_t, links[i]) for i in range(n)], shared=True)
        if launched:   # (a deferred call whose inputs need no gradient has nothing to compute: every gradient below is None)
            _forget_transposed_weights(weight)
        return (grads[1], grads[2], None, None, None, None, None) + tuple(grads[0::3])


def _may_defer(weight, bias):
    """May the gradients of this weight / bias pair wait for the end of the backward pass (defer_weight_gradients)?  Leaf parameters
    without hooks only: the flush writes ``.grad`` itself."""
    return _defer_wgrad and weight.is_leaf and (bias is None or bias.is_leaf) and not _has_hooks(weight) and not _has_hooks(bias)


def _conv_backward(probs, shared):
    """The backward pass of one grouped convolution call: allocates, describes, queues the deferred jobs, launches (unless nothing is to
    be computed).  ``probs``: one tuple per problem,
        (w, weight, bias, need_w, need_b, defer, x, y, dy, yshape, stride, pad, need_x, w_t, link)
    w, x: the saved weight and input;  weight, bias: the parameters (their gradient-bucket slots, the deferred jobs);  need_*: which
    gradients are wanted;  defer: dw / db wait for _flush_weight_gradients;  y: the saved output where the forward fused a ReLU, else
    None;  dy: what autograd delivered, of shape yshape;  w_t: the prepared transposed weight, or None;  link: a _DxLink, or None.
    ``shared``: the problems share ONE weight and bias (_ConvFn) and the library accumulates one dw / db over the list; otherwise
    (_GroupConvFn) every problem has its own.  Returns ([dx, dw, db of problem 0, dx, dw, db of problem 1, ...], launched)."""
    lib = _lib.lib()
    stream = _lib.current_stream()
    n = len(probs)
    if shared:
        w, weight, bias, need_w, need_b, defer = probs[0][:6]
        dw, db = _grad_targets(w, weight, bias, need_w and not defer, need_b and not defer)
    arr = (_lib.ConvDesc * n)()
    grads, keep = [], []   # keep: every prepared dy lives until the launch is enqueued (its block must not be handed to a later dx)
    launch = False
    for i, (w, weight, bias, need_w, need_b, defer, x, y, dy, yshape, stride, pad, need_x, w_t, link) in enumerate(probs):
        dy = _upstream_grad(dy, yshape, w.device, y, stream)
        keep.append(dy)
        if not shared:
            dw, db = _grad_targets(w, weight, bias, need_w and not defer, need_b and not defer)
        # (a dx that the consumer norm's backward apply launch has zero-filled in this graph task, on this stream: _DxLink)
        zeroed = link.take(x) if link is not None and need_x else None
        dx = zeroed if zeroed is not None else (torch.empty_like(x, memory_format=torch.channels_last) if need_x else None)
        cout, cin, k, _ = w.shape
        _set_desc(arr[i], x.shape[2], x.shape[3], cin, cout, k, stride, pad, x, w, dy=dy, dx=dx, dw=dw, db=db, w_t=w_t, dx_is_zero=zeroed is not None)
        if defer:
            # jobs belong to ONE autograd graph task: a backward pass that raised leaves its callbacks unrun and its jobs behind -- they are
            # dropped (never added into a later step's gradients), and the flush is queued once per task, not "when the list was empty"
            _queue_deferred_wgrad(dict(x=x, dy=dy, w=w, weight=weight if need_w else None, bias=bias if need_b else None, stride=stride, pad=pad))
        launch = launch or dx is not None or dw is not None or db is not None
        grads += (dx, dw, db)
    if launch:
        _conv2d_bwd(lib, arr, n, probs[0][6].shape[0], probs[0][0].device, stream)
    return grads, launch


# stream-K for the generic convolutions: the library takes it for launches of two rounds of tiles and more (conv.hip streamk_would_take:
# the RetinaNet tower, the large maps of the M2Det neck; slower on the one-round launches of a pyramid tail), so these calls carry the
# heads' 33 MB stream-K workspace (one cached buffer per device and stream); SSDK_CONV_STREAMK_GENERIC=0: never, no workspace.  Read once
_GENERIC_STREAMK = os.environ.get('SSDK_CONV_STREAMK_GENERIC', '') != '0'


def _conv2d_fwd(lib, arr, n, batch, device):
    if _GENERIC_STREAMK:
        sk = _lib.scratch(lib.ssdk_heads_fwd_workspace_bytes(), device, _lib.STREAMK_TAG, zeroed=True)   # (the stream-K state the heads use too)
        _lib.check(lib.ssdk_conv2d_fwd_ws(arr, n, batch, _dp(sk), sk.numel(), _lib.current_stream()), 'ssdk_conv2d_fwd')
    else:   # (the library's sticky stream-K error word is checked either way)
        _lib.check(lib.ssdk_conv2d_fwd_ws(arr, n, batch, None, 0, _lib.current_stream()), 'ssdk_conv2d_fwd')


def _conv2d_bwd(lib, arr, n, batch, device, stream):
    """ssdk_conv2d_bwd, or -- in the opt-in fast mode -- ssdk_conv2d_bwd_fast (stride-1 data gradients on the split-bf16 GEMM)."""
    if _lib.fast_mode == 'bf16x3':
        need = lib.ssdk_conv2d_bwd_fast_workspace_bytes(arr, n, batch)
        ws = _lib.scratch(need, device, 'conv2d_bwd')
        _lib.check(lib.ssdk_conv2d_bwd_fast(arr, n, batch, 0, 3, _dp(ws), ws.numel(), stream), 'ssdk_conv2d_bwd_fast')
    else:
        need = lib.ssdk_conv2d_bwd_workspace_bytes(arr, n, batch)
        ws = _lib.scratch(need, device, 'conv2d_bwd')
        if _GENERIC_STREAMK:   # (the stride-1 data gradients of a tower take stream-K like its forward launch: same state, same rule)
            sk = _lib.scratch(lib.ssdk_heads_fwd_workspace_bytes(), device, _lib.STREAMK_TAG, zeroed=True)
            _lib.check(lib.ssdk_conv2d_bwd_sk(arr, n, batch, 0, _dp(ws), ws.numel(), _dp(sk), sk.numel(), stream), 'ssdk_conv2d_bwd')
        else:
            _lib.check(lib.ssdk_conv2d_bwd(arr, n, batch, 0, _dp(ws), ws.numel(), stream), 'ssdk_conv2d_bwd')


class _GroupConvFn(torch.autograd.Function):
    """apply(meta, x_0, w_0, b_0, x_1, w_1, b_1, ...) -> outputs: n <= 8 INDEPENDENT convolutions -- own input, weights, kernel size, stride --
    in one grouped launch forward and one grouped call backward (the six scale branches of an M2Det TUM's smoothing layers, SFAM's per-scale
    gates: bf/modules/features.py:267, 290-296).  meta[i] = (stride, pad, relu, stats): relu / stats as in _ConvFn."""

    @staticmethod
    def forward(ctx, meta, *flat):
        lib = _lib.lib()
        n = len(meta)
        xs = [_nhwc(flat[3 * i]) for i in range(n)]
        weights = [flat[3 * i + 1] for i in range(n)]
        biases = [flat[3 * i + 2] for i in range(n)]
        _lib.require_cuda(*xs, *weights)
        ws = [w.float().contiguous(memory_format=torch.channels_last) for w in weights]
        bs = [None if b is None else b.float().contiguous() for b in biases]
        B = xs[0].shape[0]
        arr = (_lib.ConvDesc * n)()
        ys = []
        for i in range(n):
            stride, pad, relu, stats = meta[i]
            x, w = xs[i], ws[i]
            cout, cin, k, k2 = w.shape
            assert k == k2 and x.shape[0] == B and x.shape[1] == cin, (tuple(x.shape), tuple(w.shape))
            y = _conv_out(x, cout, k, stride, pad)
            ys.append(y)
            _set_desc(arr[i], x.shape[2], x.shape[3], cin, cout, k, stride, pad, x, w, bs[i], int(bool(relu)), y, stats)
        _conv2d_fwd(lib, arr, n, B, xs[0].device)
        ctx.w_ts = [_transposed_weights_of(weights[i], meta[i][0]) for i in range(n)]
        ctx.save_for_backward(*ws, *xs, *[ys[i] if meta[i][2] == 1 else xs[i].new_empty(0) for i in range(n)])
        ctx.meta = tuple((m[0], m[1], m[2] == 1) for m in meta)
        ctx.params = [(weights[i], biases[i]) for i in range(n)]
        ctx.yshapes = [tuple(y.shape) for y in ys]
        return tuple(ys)

    @staticmethod
    def backward(ctx, *dys):
        n = len(ctx.meta)
        saved = ctx.saved_tensors   # n weights, n inputs, n outputs (empty where the forward fused no ReLU)
        need = ctx.needs_input_grad
        probs = []
        for i in range(n):
            stride, pad, relu = ctx.meta[i]
            weight, bias = ctx.params[i]
            need_w, need_b = need[2 + 3 * i], need[3 + 3 * i] and bias is not None
            defer = (need_w or need_b) and _may_defer(weight, bias)
            probs.append((saved[i], weight, bias, need_w, need_b, defer, saved[n + i], saved[2 * n + i] if relu else None, dys[i], ctx.yshapes[i],
                          stride, pad, need[1 + 3 * i], ctx.w_ts[i], None))
        grads, _ = _conv_backward(probs, shared=False)
        for weight, _ in ctx.params:
            _forget_transposed_weights(weight)
        return (None, *grads)


def _queue_deferred_wgrad(job):
    """One deferred weight-gradient job of the current autograd graph task (see _ConvFn.backward)."""
    global _flush_queued_for
    task = torch._C._current_graph_task_id()
    if any(j['task'] != task for j in _pending_wgrads):
        _pending_wgrads[:] = [j for j in _pending_wgrads if j['task'] == task]
    job['task'] = task
    job['stream'] = torch.cuda.current_stream()   # (the node's stream: x and dy are complete there, the flush enqueues behind them)
    _pending_wgrads.append(job)
    if _flush_queued_for != task:
        _flush_queued_for = task
        torch.autograd.Variable._execution_engine.queue_callback(_flush_weight_gradients)


def conv2d_bn_group(xs, blocks):
    """[block(x) for block, x in zip(blocks, xs)] for INDEPENDENT Conv2dBn blocks (bf/modules/conv.py:30-36: conv -> BatchNorm -> ReLU) with
    the n <= 8 convolutions in ONE grouped launch (and one grouped backward call); the norms' statistics come from the convolutions'
    epilogues where they can.  Blocks the kernels do not take (see Conv2dBn._why_not_hip) must not be passed."""
    n = len(blocks)
    assert n == len(xs) and 0 < n <= 8
    chains = []
    for x, blk in zip(xs, blocks):
        bn = blk._modules.get('bn')
        ok = bn is not None and type(bn) is torch.nn.BatchNorm2d and x.is_cuda and torch.is_grad_enabled() and blk.conv.out_channels % 4 == 0
        chains.append(_local_training_chain(bn, x.device) if ok else None)
    global fused_stats_calls
    for c in chains:
        if c is not None:
            c.clean[0] = False
    fused_stats_calls += sum(c is not None for c in chains)
    meta, flat = [], []
    for x, blk, c in zip(xs, blocks, chains):
        cv = blk.conv
        has_bn, has_act = 'bn' in blk._modules, 'activation' in blk._modules
        meta.append((cv.stride[0], cv.padding[0], 1 if (has_act and not has_bn) else 0, None if c is None else c.buf[0].data_ptr()))
        flat += [x, cv.weight, cv.bias]
    ys = _GroupConvFn.apply(tuple(meta), *flat)
    out = []
    for y, blk, c in zip(ys, blocks, chains):
        bn = blk._modules.get('bn')
        has_act = 'activation' in blk._modules
        if bn is None:
            out.append(y)
        elif c is None:
            out.append(batch_norm(y, bn, relu=has_act) if type(bn) is torch.nn.BatchNorm2d else (torch.relu(bn(y)) if has_act else bn(y)))
        else:
            out.append(_norm_of_ready_sums(y, bn, c, int(has_act)))
    return out


def conv2d_group(xs, convs, relu=False):
    """[conv(x) (-> ReLU)] for independent nn.Conv2d layers, one grouped launch (SFAM's per-scale fc1 / fc2, features.py:290-296)."""
    meta, flat = [], []
    for x, cv in zip(xs, convs):
        meta.append((cv.stride[0], cv.padding[0], 1 if relu else 0, None))
        flat += [x, cv.weight, cv.bias]
    return list(_GroupConvFn.apply(tuple(meta), *flat))


_defer_wgrad = False
_pending_wgrads = []
_flush_queued_for = None   # the autograd graph task (torch._C._current_graph_task_id) whose end-of-backward callback is queued


def _has_hooks(p):
    """Tensor hooks / post-accumulate-grad hooks on a parameter: they only fire when autograd itself delivers the gradient, so such a
    parameter's gradient is never deferred.  (The one exception: a parameter whose only hook is libssdk's own exchange wrapper --
    distributed.BucketedDataParallel marks it ``_ssdk_exchange_hook`` -- which flushes the deferred gradients itself before it starts
    the bucket they belong to.)"""
    if p is None:
        return False
    if getattr(p, '_backward_hooks', None):
        return True
    post = getattr(p, '_post_accumulate_grad_hooks', None)
    return bool(post) and not (len(post) == 1 and getattr(p, '_ssdk_exchange_hook', False))

# weights re-laid out for the backward-data GEMMs, keyed by id(parameter): (weakref to it, (version, data_ptr), stride == 1, the layout)
_wt_cache = {}


def _transposed_weights_of(weight, stride):
    ent = _wt_cache.get(id(weight))
    if ent is None or ent[0]() is not weight or ent[1] != (weight._version, weight.data_ptr()) or ent[2] != (stride == 1):
        return None   # (another tensor, changed in place, or its storage swapped through .data since the layout was made)
    return ent[3]


def _forget_all_transposed_weights(*_args, **_kwargs):
    """Global optimizer-step post hook: EVERY prepared layout is dropped when any optimizer has stepped.  An entry normally lives from
    ``prepare_weight_transposes`` to the backward pass of the same step, which forgets it; but a forward pass without a backward pass, or a
    backward pass that raised, leaves it behind, and a fused optimizer step changes the weights without bumping ``_version`` -- a later
    forward pass that does not prepare again would then multiply with the old step's weights (advisor, round 4)."""
    _wt_cache.clear()


try:
    from torch.optim.optimizer import register_optimizer_step_post_hook as _reg
    _reg(_forget_all_transposed_weights)
    del _reg
except ImportError:   # (an older torch: the per-backward forgetting and the version / data_ptr key are what is left)
    pass


def _forget_transposed_weights(weight):
    """A prepared layout serves ONE backward pass (the one of the forward pass prepare_weight_transposes preceded): an optimizer step comes
    next, and a fused one leaves no trace in the parameter's version counter."""
    _wt_cache.pop(id(weight), None)


def prepare_weight_transposes(module):
    """Call at the start of a training step's forward pass over a chain of libssdk convolutions (the pyramid tail, the RetinaNet
    tower): the weights of every ``nn.Conv2d`` under ``module`` that the hot-path blocks run on libssdk are re-laid out for their
    backward-data GEMMs in ONE launch (``ssdk_conv2d_transpose_weights``) instead of one small launch in front of every backward call
    (8 per SSD-300 step, 40 per tower step: a shared tower weight was re-laid out once per level).  The layouts are keyed by parameter
    identity and version, so a stale one is never used: after an optimizer step (or for a convolution that was not prepared) the
    backward simply re-lays out its own weights as before.  No-op when gradients are off.  The entries only carry the layout from this
    call to the backward pass of the forward pass it precedes: the next call makes new ones."""
    if not torch.is_grad_enabled():
        return 0
    convs = [m for m in module.modules() if isinstance(m, torch.nn.Conv2d) and m.groups == 1 and m.weight.is_cuda and m.weight.requires_grad
             and m.weight.dtype == torch.float32 and m.weight.is_contiguous(memory_format=torch.channels_last)
             and m.kernel_size[0] == m.kernel_size[1] and m.stride[0] == m.stride[1] and m.in_channels % 4 == 0 and m.out_channels % 4 == 0]
    # EVERY call re-lays out every weight: a layout made by an earlier step is never trusted.  (Round 3 skipped weights whose cache entry
    # still matched the parameter's ``_version`` -- but a fused optimizer step (torch.optim.SGD(fused=True): torch._fused_sgd_) updates
    # the parameter WITHOUT bumping its version counter, so from the second step on the backward-data GEMMs multiplied with the weights
    # of the step in which the entry was made.  Found by the deterministic-mode test, tools/determinism_step_diag.py.)
    seen, todo = set(), []
    for m in convs:
        w = m.weight
        if id(w) in seen:
            continue
        seen.add(id(w))
        todo.append((w, m.kernel_size[0], m.stride[0]))
    if not todo:
        return 0
    lib = _lib.lib()
    dev = todo[0][0].device
    sizes = [(w.numel() + 63) // 64 * 64 for w, _, _ in todo]   # (256-byte aligned slices of one arena)
    arena = torch.empty((sum(sizes),), dtype=torch.float32, device=dev)
    off = 0
    for first in range(0, len(todo), 24):
        group = todo[first:first + 24]
        arr = (_lib.ConvDesc * len(group))()
        outs = (ctypes.c_void_p * len(group))()
        for i, (w, k, stride) in enumerate(group):
            _set_desc(arr[i], 0, 0, w.shape[1], w.shape[0], k, stride, 0, w=w)   # (the re-layout reads the weight and its geometry only)
            view = arena[off:off + w.numel()]
            off += sizes[first + i]
            outs[i] = view.data_ptr()
            _wt_cache[id(w)] = (weakref.ref(w), (w._version, w.data_ptr()), stride == 1, view)
        _lib.check(lib.ssdk_conv2d_transpose_weights(arr, len(group), outs, _lib.current_stream()), 'ssdk_conv2d_transpose_weights')
    for key in [k_ for k_, v in _wt_cache.items() if v[0]() is None]:   # parameters that no longer exist
        del _wt_cache[key]
    return len(todo)


def defer_weight_gradients(enabled=True):
    """OPT-IN (off by default, process-wide).  Weight (and bias) gradients of single-input ``conv2d`` calls are computed at the END of the
    backward pass, all in grouped launches (up to eight convolutions each), and written into ``param.grad`` directly -- autograd's
    AccumulateGrad never sees them.  Restrictions: ``torch.autograd.grad`` with respect to such a weight returns None for it (and the
    flush still adds into ``.grad``); do NOT enable it under a wrapper that waits for AccumulateGrad (torch DistributedDataParallel);
    parameters with tensor hooks / post-accumulate-grad hooks are never deferred.  libssdk's own GradBucket path is fine (the flush runs
    before ``backward()`` returns).  A backward pass that raises leaves nothing behind: its jobs are dropped by the next pass.
    Returns the previous setting."""
    global _defer_wgrad
    prev = _defer_wgrad
    _defer_wgrad = bool(enabled)
    return prev


def set_deterministic(enabled=True):
    """Process-wide deterministic mode of libssdk (``ssdk_set_deterministic``; also ``SSDK_DETERMINISTIC=1`` in the environment) -- the
    counterpart of the reference's ``torch.backends.cudnn.deterministic = True`` (bf/training/env.py:74-76).  On: no fp32 atomics anywhere
    in the training kernels -- convolutions are not split over K, data gradients take the output-stationary form (the heads' sparse
    scatter forms are not used), weight and bias gradients are reduced in a fixed order -- so the same inputs give the same bits, run to
    run and eager vs HIP-graph replay.  Slower (bench.py reports ``deterministic_ms_per_step`` per config).  Returns the previous
    setting; ``with ops.deterministic():`` scopes it."""
    return bool(_lib.lib().ssdk_set_deterministic(1 if enabled else 0))


def is_deterministic():
    return bool(_lib.lib().ssdk_get_deterministic())


class deterministic(object):
    def __init__(self, enabled=True):
        self.enabled = enabled

    def __enter__(self):
        self.prev = set_deterministic(self.enabled)
        return self

    def __exit__(self, *exc):
        set_deterministic(self.prev)
        return False


class deferred_weight_gradients(object):
    """``with ops.deferred_weight_gradients():`` -- the opt-in of ``defer_weight_gradients`` for the backward passes run inside the block
    only (the previous setting comes back on exit, also when the block raises): a training step that owns its parameters' gradients
    (bench.HotPath.train_step) scopes it to itself instead of changing what ``torch.autograd.grad`` returns for the rest of the process."""

    def __init__(self, enabled=True):
        self.enabled = enabled

    def __enter__(self):
        self.prev = defer_weight_gradients(self.enabled)
        return self

    def __exit__(self, *exc):
        defer_weight_gradients(self.prev)
        return False


def _flush_weight_gradients():
    global _flush_queued_for
    task = torch._C._current_graph_task_id()
    jobs = [j for j in _pending_wgrads if j['task'] == task or task < 0]
    del _pending_wgrads[:]   # (jobs of another task are leftovers of a backward pass that raised)
    _flush_queued_for = None
    if not jobs:
        return
    # jobs queued by nodes of another stream (a pyramid tail differentiated beside the heads: detection/modules/heads.py
    # multi_level_heads_split) are flushed on THAT stream, behind the launches that made their operands, and the caller's stream --
    # on which the optimizer runs next -- waits for it
    caller = torch.cuda.current_stream()
    streams = []
    for j in jobs:
        if all(j['stream'] != s_ for s_ in streams):
            streams.append(j['stream'])
    for s_ in streams:
        mine = [j for j in jobs if j['stream'] == s_]
        if s_ == caller:
            _flush_jobs(mine)
        else:
            with torch.cuda.stream(s_):
                _flush_jobs(mine)
            caller.wait_stream(s_)


def _flush_jobs(jobs):
    lib = _lib.lib()
    stream = _lib.current_stream()
    for first in range(0, len(jobs), 8):
        group = jobs[first:first + 8]
        if len({j['x'].shape[0] for j in group}) != 1:
            group_list = [[j] for j in group]   # (a grouped call shares the batch size)
        else:
            group_list = [group]
        for grp in group_list:
            arr = (_lib.ConvDesc * len(grp))()
            outs = []
            for i, j in enumerate(grp):
                w, x = j['w'], j['x']
                cout, cin, k, _ = w.shape
                dw, db = _grad_targets(w, j['weight'], j['bias'], j['weight'] is not None, j['bias'] is not None)
                _set_desc(arr[i], x.shape[2], x.shape[3], cin, cout, k, j['stride'], j['pad'], x, w, dy=j['dy'], dw=dw, db=db)
                outs.append((j['weight'], dw, j['bias'], db))
            B = grp[0]['x'].shape[0]
            need = lib.ssdk_conv2d_bwd_workspace_bytes(arr, len(grp), B)
            ws = _lib.scratch(need, grp[0]['w'].device, 'conv2d_bwd')
            _lib.check(lib.ssdk_conv2d_bwd(arr, len(grp), B, 0, _dp(ws), ws.numel(), stream), 'ssdk_conv2d_bwd')
            for weight, dw, bias, db in outs:
                for p_, g_ in ((weight, dw), (bias, db)):
                    if p_ is None:
                        continue
                    if p_.grad is None:
                        p_.grad = g_
                    else:
                        p_.grad = p_.grad + g_


def conv2d(xs, weight, bias=None, stride=1, padding=0, relu=False):
    """Conv2d on a list of maps that share the weights (one grouped GEMM launch); returns a list."""
    single = isinstance(xs, torch.Tensor)
    out = _ConvFn.apply(weight, bias, int(stride), int(padding), bool(relu), None, None, *([xs] if single else list(xs)))
    return out[0] if single else list(out)


_NO_FUSED_STATS = bool(os.environ.get('SSDK_NO_FUSED_STATS'))   # (measurement knob)
_NO_BN_CHAIN = bool(os.environ.get('SSDK_NO_BN_CHAIN'))         # (measurement knob: every norm call zero-fills a scratch workspace)
_NO_RELU_BY_NORM = bool(os.environ.get('SSDK_NO_RELU_BY_NORM'))   # (measurement knob)
_NO_DX_ZERO_BY_NORM = bool(os.environ.get('SSDK_NO_DX_ZERO_BY_NORM'))   # (measurement knob: the convolution zero-fills its own dx)
fused_stats_calls = 0   # (norm layers whose forward statistics were handed to a convolution's epilogue; tests read it)


def _local_training_chain(bn, device):
    """The layer's `sums` chain when its forward statistics can be taken by the producing convolution's epilogue: a plain BatchNorm2d in
    training mode, per-process statistics, its forward buffer known to hold zeros.  None otherwise."""
    if _NO_FUSED_STATS or type(bn) is not torch.nn.BatchNorm2d or not bn.training or bn.momentum is None or not bn.track_running_stats or sync_group_of(bn) is not None:
        return None
    chain = _sums_chain_of(bn, device)
    return chain if chain.usable(0, device) else None


def _sums_chain_of(bn, device):
    """The layer's _SumsChain on ``device`` (made on first use, and again when the layer moved or changed its width)."""
    chain = getattr(bn, '_ssdk_sums_chain', None)
    if chain is None or chain.buf.device != device or chain.buf.shape[1] != 2 * bn.num_features + 2:
        chain = bn._ssdk_sums_chain = _SumsChain(bn.num_features, device)
    return chain


def _norm_of_ready_sums(y, bn, chain, relu, link=None):
    """Training-mode BatchNorm of ``y`` whose statistics the producing convolution has left in chain.buf[0]: ONE apply launch.  relu: the
    flags of _BatchNormFn;  link: the _DxLink shared with that convolution, or None."""
    return _BatchNormFn.apply(y, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked, bn.momentum, bn.eps,
                              True, relu, chain, True, link)


def conv2d_batch_norm(xs, weight, bias, stride, padding, bns, conv_relu=False, bn_relu=False):
    """conv (-> ReLU) -> BatchNorm (-> ReLU) on a list of maps that share the convolution's weights and have a norm layer each
    (bf/modules/conv.py:30-36; the per-level norms of a RetinaNet tower layer, detection/modules/predictors.py:60-76).  Where a norm is a
    training-mode BatchNorm2d with per-process statistics, the convolution's epilogue accumulates its statistics (ssdk_conv_desc::stats)
    and the norm is ONE launch (apply) instead of two -- and the statistics pass over the activation is gone; anywhere else this is
    conv2d followed by batch_norm."""
    single = isinstance(xs, torch.Tensor)
    xs = [xs] if single else list(xs)
    bns = [bns] if single else list(bns)
    chains = [_local_training_chain(bn, x.device) if x.is_cuda and torch.is_grad_enabled() else None for x, bn in zip(xs, bns)]
    if not any(c is not None for c in chains) or weight.shape[0] % 4:
        ys = conv2d(xs, weight, bias, stride, padding, relu=conv_relu)
        out = [batch_norm(y, bn, relu=bn_relu) for y, bn in zip(ys, bns)]
        return out[0] if single else out
    for c in chains:
        if c is not None:
            c.clean[0] = False   # (handed to the convolution: whatever happens next, it no longer holds zeros)
    global fused_stats_calls
    fused_stats_calls += sum(c is not None for c in chains)
    stats = tuple(None if c is None else c.buf[0].data_ptr() for c in chains)
    # conv -> ReLU -> norm with every norm on this path: the norms' backward also takes the ReLU's gradient (dx = 0 where the norm's input
    # is not positive), and the convolution's backward skips its own pass over dy
    relu_by_norm = bool(conv_relu) and all(c is not None for c in chains) and not _NO_RELU_BY_NORM
    # a strided convolution's data gradient is scatter-added into a zeroed dx: the norm's backward apply launch zero-fills it (_DxLink)
    links = tuple(_DxLink() if c is not None and int(stride) > 1 and not _NO_DX_ZERO_BY_NORM else None for c in chains)
    ys = _ConvFn.apply(weight, bias, int(stride), int(padding), 2 if relu_by_norm else int(bool(conv_relu)), stats, links, *xs)
    out = []
    for y, bn, c, link in zip(ys, bns, chains, links):
        if c is None:
            out.append(batch_norm(y, bn, relu=bn_relu))
        else:
            out.append(_norm_of_ready_sums(y, bn, c, int(bool(bn_relu)) | (2 if relu_by_norm else 0), link))
    return out[0] if single else out


class _DxLink(object):
    """What the two autograd nodes of a conv -> BatchNorm block share (conv2d_batch_norm makes one per block): the norm's backward, which
    runs first, allocates the convolution's dx and has its apply launch zero-fill it (ssdk_batchnorm_bwd_chained_ex); the convolution's
    backward takes that tensor and tells the library that it is zero (ssdk_conv_desc::dx_is_zero) -- the zero-fill launch in front of a
    scatter-form data gradient is gone.  Only when the library says the data gradient WILL take the scatter form (ssdk_conv2d_dx_form: the
    plan's rule, with the deterministic flag of the moment), the input needs a gradient, and both nodes run in the same graph task on the
    same stream; anything else -- and a tensor left over from a backward pass that raised -- is dropped and the call runs as without it."""
    __slots__ = ('desc', 'shape', 'needs_dx', 'dx', 'task', 'stream')

    def __init__(self):
        self.desc = self.shape = self.dx = self.task = self.stream = None
        self.needs_dx = False

    def describe(self, x, cout, ksize, stride, pad, needs_dx):
        self.desc = _lib.ConvDesc()
        _set_desc(self.desc, x.shape[2], x.shape[3], x.shape[1], cout, ksize, stride, pad)
        self.shape, self.needs_dx = tuple(x.shape), bool(needs_dx)

    def _scatter(self):
        return self.desc is not None and _lib.lib().ssdk_conv2d_dx_form(ctypes.byref(self.desc)) == 1

    def offer(self, device):
        """(norm backward) the convolution's dx to zero-fill, or None."""
        self.dx = None
        if not self.needs_dx or not self._scatter():
            return None
        self.dx = torch.empty(self.shape, dtype=torch.float32, device=device, memory_format=torch.channels_last)
        self.task, self.stream = torch._C._current_graph_task_id(), _lib.raw_stream(device)
        return self.dx

    def take(self, x):
        """(convolution backward) the zero-filled dx of this graph task and stream, or None."""
        dx, self.dx = self.dx, None
        if dx is None or self.task != torch._C._current_graph_task_id() or self.stream != _lib.raw_stream(x.device):
            return None
        return dx if dx.shape == x.shape and dx.device == x.device and self._scatter() else None


class _SumsChain(object):
    """Two fp64 `sums` buffers of one BatchNorm layer (forward, backward) and which of them currently hold zeros.  A forward call
    accumulates into the forward buffer and has its apply launch zero the backward one; the backward call does the reverse: in
    steady-state training no zero-fill launch runs for the layer at all (they were 16 of the ~150 launches of an SSD-300 step).
    Whenever the buffer a call needs is not known to be clean -- a second forward before the backward, an evaluation pass in training
    mode, another stream -- the call takes the plain entry point, which zero-fills a scratch workspace itself."""

    def __init__(self, channels, device):
        self.buf = torch.zeros((2, 2 * channels + 2), dtype=torch.float64, device=device)
        self.clean = [True, True]   # forward buffer, backward buffer
        self.stream = _lib.raw_stream(device)

    def usable(self, which, device):
        return not _NO_BN_CHAIN and self.clean[which] and self.buf.device == device and self.stream == _lib.raw_stream(device)


class _BatchNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, num_batches_tracked, momentum, eps, training, relu, chain, sums_ready=False, link=None):
        lib = _lib.lib()
        _lib.require_cuda(x)
        x = _nhwc(x)
        B, C, H, W = x.shape
        rows = B * H * W
        y = torch.empty_like(x, memory_format=torch.channels_last)
        mean = torch.empty((C,), dtype=torch.float32, device=x.device)
        rstd = torch.empty((C,), dtype=torch.float32, device=x.device)
        g = None if gamma is None else gamma.float().contiguous()
        b = None if beta is None else beta.float().contiguous()
        relu = int(relu)      # bit 0: the norm's own fused ReLU; bit 1 (backward only): the input is a ReLU output, its gradient is taken here too
        own = relu & 1
        if sums_ready:   # the producing convolution's epilogue left the statistics in chain.buf[0] (conv2d_batch_norm)
            _lib.check(lib.ssdk_batchnorm_apply_chained(_dp(x), rows, C, _dp(g), _dp(b), _dp(running_mean), _dp(running_var), _dp(num_batches_tracked),
                                                        float(momentum), float(eps), own, _dp(y), _dp(mean), _dp(rstd), chain.buf[0].data_ptr(),
                                                        chain.buf[1].data_ptr(), _lib.current_stream()), 'ssdk_batchnorm_apply_chained')
            chain.clean = [False, True]
        elif training and chain is not None and chain.usable(0, x.device):
            _lib.check(lib.ssdk_batchnorm_fwd_chained(_dp(x), rows, C, _dp(g), _dp(b), _dp(running_mean), _dp(running_var), _dp(num_batches_tracked),
                                                      float(momentum), float(eps), own, _dp(y), _dp(mean), _dp(rstd), chain.buf[0].data_ptr(),
                                                      chain.buf[1].data_ptr(), _lib.current_stream()), 'ssdk_batchnorm_fwd_chained')
            chain.clean = [False, True]
        else:
            ws = _lib.scratch(lib.ssdk_batchnorm_workspace_bytes(C), x.device, 'batchnorm')
            _lib.check(lib.ssdk_batchnorm_fwd(_dp(x), rows, C, _dp(g), _dp(b), _dp(running_mean), _dp(running_var),
                                              _dp(num_batches_tracked) if training else None, float(momentum), float(eps), int(training), own, _dp(y), _dp(mean), _dp(rstd), _dp(ws), ws.numel(),
                                              _lib.current_stream()), 'ssdk_batchnorm_fwd')
        ctx.save_for_backward(x, y if own else x.new_empty(0), g if g is not None else x.new_empty(0), mean, rstd)
        ctx.meta = (relu, bool(training), gamma is not None, beta is not None)
        ctx.chain, ctx.link = chain, link
        ctx.mark_non_differentiable(mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.lib()
        x, y, g, mean, rstd = ctx.saved_tensors
        relu, training, has_g, has_b = ctx.meta
        chain = ctx.chain
        B, C, H, W = x.shape
        dy = _nhwc(dy)
        dx = torch.empty_like(x, memory_format=torch.channels_last)
        dgamma = torch.empty((C,), dtype=torch.float32, device=x.device)
        dbeta = torch.empty((C,), dtype=torch.float32, device=x.device)
        if training and chain is not None and chain.usable(1, x.device):
            also = ctx.link.offer(x.device) if ctx.link is not None else None   # (the producing convolution's dx: zero-filled by the apply launch)
            _lib.check(lib.ssdk_batchnorm_bwd_chained_ex(_dp(x), _dp(y) if relu & 1 else None, _dp(dy), B * H * W, C, _dp(g) if has_g else None, _dp(mean),
                                                         _dp(rstd), relu, _dp(dx), _dp(dgamma), _dp(dbeta), chain.buf[1].data_ptr(),
                                                         chain.buf[0].data_ptr(), _dp(also), 0 if also is None else also.numel(),
                                                         _lib.current_stream()), 'ssdk_batchnorm_bwd_chained')
            chain.clean = [True, False]
        else:
            ws = _lib.scratch(lib.ssdk_batchnorm_workspace_bytes(C), x.device, 'batchnorm')
            _lib.check(lib.ssdk_batchnorm_bwd(_dp(x), _dp(y) if relu & 1 else None, _dp(dy), B * H * W, C, _dp(g) if has_g else None, _dp(mean),
                                              _dp(rstd), relu, int(training), _dp(dx), _dp(dgamma), _dp(dbeta), _dp(ws), ws.numel(),
                                              _lib.current_stream()), 'ssdk_batchnorm_bwd')
        return dx, dgamma if has_g else None, dbeta if has_b else None, None, None, None, None, None, None, None, None, None, None


def batch_norm(x, bn, relu=False):
    """``bn`` is a torch.nn.BatchNorm2d (its parameters / buffers are used and updated exactly like torch does)."""
    if bn.momentum is None or not bn.track_running_stats:
        raise NotImplementedError('BatchNorm2d with momentum=None / track_running_stats=False is not on the GPU path')
    training = bn.training
    mark = sync_group_of(bn)
    if mark is not None and training:   # statistics over all ranks (detection.init(distributed=True))
        return sync_batch_norm([x], [bn], relu, mark[0])[0]
    nbt = bn.num_batches_tracked   # incremented inside the library's launch (torch: a launch of its own per layer)
    if nbt is not None:
        assert nbt.dtype == torch.int64 and nbt.is_cuda
    chain = _sums_chain_of(bn, x.device) if training and x.is_cuda else None
    return _BatchNormFn.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, nbt, bn.momentum, bn.eps, training, relu, chain, False)


def sync_group_of(bn):
    """The process group a BatchNorm2d was marked with by distributed.convert_sync_batchnorm (detection.init(distributed=True)), as a
    1-tuple -- (None,) is the default group -- or None for a plain, per-process BatchNorm."""
    return getattr(bn, '_ssdk_sync_group', None)


def allreduce_sums_(buf, group=None):
    """The one exchange step of synchronised BatchNorm: all-reduce(sum) of a packed fp64 buffer [sum_i (2 C_i + 2)] holding, per
    norm layer, (sum, sum of squares / products, row count, padding).  No-op without an initialised process group or with one rank."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        dist.all_reduce(buf, group=group)
    return buf


class _SyncBatchNormFn(torch.autograd.Function):
    """Training-mode BatchNorm2d (+ fused ReLU) over the GLOBAL batch for n layers at once (e.g. the five per-level norms of one
    RetinaNet tower layer): per-layer partial sums on libssdk -> ONE all-reduce of the packed buffer -> per-layer apply.
    apply(group, relu, n, x_0, gamma_0, beta_0, running_mean_0, running_var_0, nbt_0, momentum_0, eps_0, x_1, ...) -> y_0, y_1, ...
    (apex convert_syncbn_model in the reference, detection/init.py:85)."""

    @staticmethod
    def forward(ctx, group, relu, n, *args):
        lib = _lib.lib()
        stream = _lib.current_stream()
        layers = []
        for i in range(n):
            x, gamma, beta, rm, rv, nbt, momentum, eps = args[8 * i:8 * i + 8]
            _lib.require_cuda(x)
            x = _nhwc(x)
            layers.append(dict(x=x, C=x.shape[1], rows=x.shape[0] * x.shape[2] * x.shape[3],
                               g=None if gamma is None else gamma.float().contiguous(), b=None if beta is None else beta.float().contiguous(),
                               rm=rm, rv=rv, nbt=nbt, momentum=float(momentum), eps=float(eps)))
        dev = layers[0]['x'].device
        offs, tot = [], 0
        for lv in layers:
            offs.append(tot)
            tot += 2 * lv['C'] + 2   # (sum, sum of squares, rows, padding)
        sums = torch.empty((tot,), dtype=torch.float64, device=dev)
        for lv, off in zip(layers, offs):
            _lib.check(lib.ssdk_batchnorm_stats(_dp(lv['x']), lv['rows'], lv['C'], sums[off:].data_ptr(), stream), 'ssdk_batchnorm_stats')
        allreduce_sums_(sums, group)
        ys, saved = [], []
        for lv, off in zip(layers, offs):
            x, C = lv['x'], lv['C']
            y = torch.empty_like(x, memory_format=torch.channels_last)
            mean = torch.empty((C,), dtype=torch.float32, device=dev)
            rstd = torch.empty((C,), dtype=torch.float32, device=dev)
            _lib.check(lib.ssdk_batchnorm_apply(_dp(x), lv['rows'], C, _dp(lv['g']), _dp(lv['b']), _dp(lv['rm']), _dp(lv['rv']), _dp(lv['nbt']),
                                                lv['momentum'], lv['eps'], int(relu), _dp(y), _dp(mean), _dp(rstd), sums[off:].data_ptr(), 1, stream),
                       'ssdk_batchnorm_apply')
            ys.append(y)
            saved += [x, y if relu else x.new_empty(0), lv['g'] if lv['g'] is not None else x.new_empty(0), mean, rstd]
        ctx.save_for_backward(*saved)
        ctx.meta = (group, bool(relu), n, [(lv['C'], lv['rows'], lv['g'] is not None, lv['b'] is not None) for lv in layers], offs, tot)
        return tuple(ys)

    @staticmethod
    def backward(ctx, *dys):
        lib = _lib.lib()
        stream = _lib.current_stream()
        group, relu, n, shapes, offs, tot = ctx.meta
        saved = ctx.saved_tensors
        dev = saved[0].device
        sums = torch.empty((tot,), dtype=torch.float64, device=dev)
        dys = [torch.zeros_like(saved[5 * i], memory_format=torch.channels_last) if dy is None else _nhwc(dy) for i, dy in enumerate(dys)]
        for i in range(n):
            x, y, g, mean, rstd = saved[5 * i:5 * i + 5]
            C, rows, _, _ = shapes[i]
            _lib.check(lib.ssdk_batchnorm_bwd_stats(_dp(x), _dp(y) if relu else None, _dp(dys[i]), rows, C, _dp(mean), _dp(rstd), int(relu),
                                                    sums[offs[i]:].data_ptr(), stream), 'ssdk_batchnorm_bwd_stats')
        local = sums.clone()   # the affine parameters' gradients are this rank's own sums (the gradient exchange averages them later)
        allreduce_sums_(sums, group)
        out = [None, None, None]
        for i in range(n):
            x, y, g, mean, rstd = saved[5 * i:5 * i + 5]
            C, rows, has_g, has_b = shapes[i]
            dx = torch.empty_like(x, memory_format=torch.channels_last)
            dgamma = torch.empty((C,), dtype=torch.float32, device=dev)
            dbeta = torch.empty((C,), dtype=torch.float32, device=dev)
            base = sums[offs[i]:].data_ptr()
            _lib.check(lib.ssdk_batchnorm_bwd_apply(_dp(x), _dp(y) if relu else None, _dp(dys[i]), rows, C, _dp(g) if has_g else None, _dp(mean),
                                                    _dp(rstd), int(relu), 1, base, local[offs[i]:].data_ptr(), base + 16 * C, _dp(dx), _dp(dgamma),
                                                    _dp(dbeta), stream), 'ssdk_batchnorm_bwd_apply')
            out += [dx, dgamma if has_g else None, dbeta if has_b else None, None, None, None, None, None]
        return tuple(out)


def sync_batch_norm(xs, bns, relu=False, group=None):
    """Synchronised training-mode BatchNorm of several maps with their own norm layers, one exchange for all of them."""
    args = []
    for x, bn in zip(xs, bns):
        if bn.momentum is None or not bn.track_running_stats:
            raise NotImplementedError('BatchNorm2d with momentum=None / track_running_stats=False is not on the GPU path')
        args += [x, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked, bn.momentum, bn.eps]
    return list(_SyncBatchNormFn.apply(group, bool(relu), len(bns), *args))


def batch_norm_levels(xs, bns, relu=False):
    """One BatchNorm2d per map (the per-level norms of a RetinaNet tower layer, detection/modules/predictors.py:39-42,69-70).  Layers
    marked for synchronisation share ONE packed all-reduce in training mode; otherwise each runs on its own."""
    marks = [sync_group_of(bn) for bn in bns]
    if all(m is not None for m in marks) and all(bn.training for bn in bns) and len({id(m[0]) for m in marks}) == 1:
        return sync_batch_norm(xs, bns, relu, marks[0][0])
    return [batch_norm(x, bn, relu) for x, bn in zip(xs, bns)]


UPSAMPLE_MODES = ('nearest', 'bilinear')   # the interpolation modes on libssdk: ssdk_upsample_<mode>_add_fwd / _bwd


def _upsample_entry(mode, direction):
    if mode not in UPSAMPLE_MODES:
        raise ValueError(f"upsampling mode {mode!r} is not on libssdk: the modes are 'nearest' and 'bilinear'")
    name = f'ssdk_upsample_{mode}_add_{direction}'
    return getattr(_lib.lib(), name), name


class _UpsampleAddFn(torch.autograd.Function):
    """out = fine + F.interpolate(coarse, size of fine, mode)   (FPN top-down step, bf/modules/features.py:106-108; TUM, :263-265)"""

    @staticmethod
    def forward(ctx, fine, coarse, mode):
        fwd, name = _upsample_entry(mode, 'fwd')
        _lib.require_cuda(fine, coarse)
        fine, coarse = _nhwc(fine), _nhwc(coarse)
        B, C, Hf, Wf = fine.shape
        assert coarse.shape[0] == B and coarse.shape[1] == C
        out = torch.empty_like(fine, memory_format=torch.channels_last)
        _lib.check(fwd(_dp(fine), _dp(coarse), B, Hf, Wf, coarse.shape[2], coarse.shape[3], C, _dp(out), _lib.current_stream()), name)
        ctx.shapes = (B, C, Hf, Wf, coarse.shape[2], coarse.shape[3])
        ctx.mode = mode
        return out

    @staticmethod
    def backward(ctx, dout):
        B, C, Hf, Wf, Hc, Wc = ctx.shapes
        dout = _nhwc(dout)
        dcoarse = None
        if ctx.needs_input_grad[1]:
            bwd, name = _upsample_entry(ctx.mode, 'bwd')
            dcoarse = torch.empty((B, C, Hc, Wc), dtype=torch.float32, device=dout.device, memory_format=torch.channels_last)
            _lib.check(bwd(_dp(dout), B, Hf, Wf, Hc, Wc, C, _dp(dcoarse), _lib.current_stream()), name)
        return (dout if ctx.needs_input_grad[0] else None), dcoarse, None


def upsample_add(fine, coarse, mode='nearest'):
    """fine + F.interpolate(coarse, size=fine.shape[2:], mode=mode) in one launch; ``mode`` is 'nearest' or 'bilinear' (align_corners=False,
    as F.interpolate runs it).  The backward passes dout through to ``fine`` and gathers ``dcoarse`` without atomics in either mode."""
    return _UpsampleAddFn.apply(fine, coarse, mode)


class _UpsampleFn(torch.autograd.Function):
    """F.interpolate(x, size=(h, w), mode=mode) (bf/modules/features.py:371-373)."""

    @staticmethod
    def forward(ctx, coarse, hf, wf, mode):
        fwd, name = _upsample_entry(mode, 'fwd')
        _lib.require_cuda(coarse)
        coarse = _nhwc(coarse)
        B, C, Hc, Wc = coarse.shape
        out = torch.empty((B, C, hf, wf), dtype=torch.float32, device=coarse.device, memory_format=torch.channels_last)
        _lib.check(fwd(None, _dp(coarse), B, hf, wf, Hc, Wc, C, _dp(out), _lib.current_stream()), name)
        ctx.shapes = (B, C, hf, wf, Hc, Wc)
        ctx.mode = mode
        return out

    @staticmethod
    def backward(ctx, dout):
        B, C, Hf, Wf, Hc, Wc = ctx.shapes
        bwd, name = _upsample_entry(ctx.mode, 'bwd')
        dout = _nhwc(dout)
        dcoarse = torch.empty((B, C, Hc, Wc), dtype=torch.float32, device=dout.device, memory_format=torch.channels_last)
        _lib.check(bwd(_dp(dout), B, Hf, Wf, Hc, Wc, C, _dp(dcoarse), _lib.current_stream()), name)
        return dcoarse, None, None, None


def upsample(x, size, mode='nearest'):
    """F.interpolate(x, size=size, mode=mode) for the modes of ``upsample_add``."""
    return _UpsampleFn.apply(x, int(size[0]), int(size[1]), mode)


def upsample_nearest(x, size):
    return upsample(x, size, 'nearest')


class _AvgPoolFn(torch.autograd.Function):
    """F.adaptive_avg_pool2d(x, 1) -> [B, C, 1, 1]"""

    @staticmethod
    def forward(ctx, x):
        _lib.require_cuda(x)
        x = _nhwc(x)
        B, C, H, W = x.shape
        out = torch.empty((B, C, 1, 1), dtype=torch.float32, device=x.device)
        _lib.check(_lib.lib().ssdk_global_avgpool_fwd(_dp(x), B, H * W, C, _dp(out), _lib.current_stream()), 'ssdk_global_avgpool_fwd')
        ctx.shape = (B, C, H, W)
        return out

    @staticmethod
    def backward(ctx, dout):
        B, C, H, W = ctx.shape
        dout = dout.float().contiguous()
        dx = torch.empty((B, C, H, W), dtype=torch.float32, device=dout.device, memory_format=torch.channels_last)
        _lib.check(_lib.lib().ssdk_global_avgpool_bwd(_dp(dout), B, H * W, C, _dp(dx), _lib.current_stream()), 'ssdk_global_avgpool_bwd')
        return dx


def global_avg_pool(x):
    return _AvgPoolFn.apply(x)


class _GateFn(torch.autograd.Function):
    """x * sigmoid(z), z [B, C, 1, 1] (bf/modules/features.py:296-298)"""

    @staticmethod
    def forward(ctx, x, z):
        _lib.require_cuda(x, z)
        x = _nhwc(x)
        z = z.float().contiguous()
        B, C, H, W = x.shape
        out = torch.empty_like(x, memory_format=torch.channels_last)
        _lib.check(_lib.lib().ssdk_sigmoid_gate_fwd(_dp(x), _dp(z), B, H * W, C, _dp(out), _lib.current_stream()), 'ssdk_sigmoid_gate_fwd')
        ctx.save_for_backward(x, z)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, z = ctx.saved_tensors
        B, C, H, W = x.shape
        dout = _nhwc(dout)
        dx = torch.empty_like(x, memory_format=torch.channels_last)
        dz = torch.empty_like(z)
        _lib.check(_lib.lib().ssdk_sigmoid_gate_bwd(_dp(x), _dp(z), _dp(dout), B, H * W, C, _dp(dx), _dp(dz), _lib.current_stream()),
                   'ssdk_sigmoid_gate_bwd')
        return dx, dz


def sigmoid_gate(x, z):
    return _GateFn.apply(x, z)


class _SfamFn(torch.autograd.Function):
    """M2Det SFAM over PIECES: apply(n_scales, n_pieces, *pieces (scale-major), *(fc1.weight, fc1.bias, fc2.weight, fc2.bias per scale))
    -> n_scales gated maps [B, n_pieces * Cp, H_s, W_s].  What bf/modules/features.py:385 + :286-298 compute -- torch.cat of a scale's TUM
    outputs, adaptive_avg_pool2d, fc1 + ReLU, fc2, sigmoid gate -- without ever building the concatenated map: the pool and the gate read
    the pieces where they are (ssdk_sfam_*), the two 1 x 1 "fc" convolutions of all scales run as grouped launches, and the backward pass
    writes each piece's gradient (gate's part + pool's part) as its own contiguous map in one pass."""

    @staticmethod
    def forward(ctx, n_scales, n_pieces, *flat):
        lib = _lib.lib()
        stream = _lib.current_stream()
        pieces = [[_nhwc(flat[s * n_pieces + k]) for k in range(n_pieces)] for s in range(n_scales)]
        params = flat[n_scales * n_pieces:]
        _lib.require_cuda(*[p for ps in pieces for p in ps])
        w1 = [params[4 * s].float().contiguous(memory_format=torch.channels_last) for s in range(n_scales)]
        b1 = [None if params[4 * s + 1] is None else params[4 * s + 1].float().contiguous() for s in range(n_scales)]
        w2 = [params[4 * s + 2].float().contiguous(memory_format=torch.channels_last) for s in range(n_scales)]
        b2 = [None if params[4 * s + 3] is None else params[4 * s + 3].float().contiguous() for s in range(n_scales)]
        B, Cp = pieces[0][0].shape[0], pieces[0][0].shape[1]
        C, Hc = n_pieces * Cp, w1[0].shape[0]
        dev = pieces[0][0].device
        for s in range(n_scales):
            shape = pieces[s][0].shape
            assert all(p.shape == shape for p in pieces[s]) and shape[0] == B and shape[1] == Cp, 'the pieces of a scale must share one shape'
            assert tuple(w1[s].shape) == (Hc, C, 1, 1) and tuple(w2[s].shape) == (C, Hc, 1, 1), (tuple(w1[s].shape), tuple(w2[s].shape))
        pooled = torch.empty((n_scales, B, C), dtype=torch.float32, device=dev)
        hidden = torch.empty((n_scales, B, Hc), dtype=torch.float32, device=dev)
        z = torch.empty((n_scales, B, C), dtype=torch.float32, device=dev)
        ptrs = [(ctypes.c_void_p * n_pieces)(*[p.data_ptr() for p in pieces[s]]) for s in range(n_scales)]
        hw = [pieces[s][0].shape[2] * pieces[s][0].shape[3] for s in range(n_scales)]
        for s in range(n_scales):
            _lib.check(lib.ssdk_sfam_pool_fwd(ptrs[s], n_pieces, B, hw[s], Cp, pooled[s].data_ptr(), stream), 'ssdk_sfam_pool_fwd')
        for x, w, b, y, relu in ((pooled, w1, b1, hidden, 1), (hidden, w2, b2, z, 0)):   # fc1 + F.relu, fc2: one grouped launch each
            arr = (_lib.ConvDesc * n_scales)()
            for s in range(n_scales):   # (a [B, C] row block is a batch of 1 x 1 maps)
                _set_desc(arr[s], 1, 1, x.shape[2], y.shape[2], 1, 1, 0, x=x[s], w=w[s], bias=b[s], relu=relu, y=y[s])
            _conv2d_fwd(lib, arr, n_scales, B, dev)
        outs = []
        for s in range(n_scales):
            out = torch.empty((B, C) + tuple(pieces[s][0].shape[2:]), dtype=torch.float32, device=dev, memory_format=torch.channels_last)
            _lib.check(lib.ssdk_sfam_gate_fwd(ptrs[s], n_pieces, B, hw[s], Cp, z[s].data_ptr(), _dp(out), stream), 'ssdk_sfam_gate_fwd')
            outs.append(out)
        ctx.save_for_backward(pooled, hidden, z, *w1, *w2, *[p for ps in pieces for p in ps])
        ctx.meta = (n_scales, n_pieces, [b is not None for b in b1], [b is not None for b in b2])
        ctx.params = params
        return tuple(outs)

    @staticmethod
    def backward(ctx, *douts):
        lib = _lib.lib()
        stream = _lib.current_stream()
        n_scales, n_pieces, has_b1, has_b2 = ctx.meta
        saved = ctx.saved_tensors
        pooled, hidden, z = saved[:3]
        w1, w2 = saved[3:3 + n_scales], saved[3 + n_scales:3 + 2 * n_scales]
        flat_pieces = saved[3 + 2 * n_scales:]
        pieces = [flat_pieces[s * n_pieces:(s + 1) * n_pieces] for s in range(n_scales)]
        B, Cp = pieces[0][0].shape[0], pieces[0][0].shape[1]
        C, Hc = n_pieces * Cp, hidden.shape[2]
        dev = pooled.device
        hw = [pieces[s][0].shape[2] * pieces[s][0].shape[3] for s in range(n_scales)]
        ptrs = [(ctypes.c_void_p * n_pieces)(*[p.data_ptr() for p in pieces[s]]) for s in range(n_scales)]
        douts = [_upstream_grad(g, (B, C) + tuple(pieces[s][0].shape[2:]), dev) for s, g in enumerate(douts)]
        # 1. dz = sigmoid'(z) * sum_hw dout * piece
        dz = torch.empty_like(z)
        for s in range(n_scales):
            _lib.check(lib.ssdk_sfam_gate_bwd_reduce(ptrs[s], n_pieces, B, hw[s], Cp, z[s].data_ptr(), _dp(douts[s]), dz[s].data_ptr(), stream),
                       'ssdk_sfam_gate_bwd_reduce')
        # 2. fc2 and fc1 backward (data, weight and bias gradients; one grouped call each), the ReLU between them
        d_hidden = torch.empty_like(hidden)
        dpool = torch.empty_like(pooled)
        dw1 = [torch.empty_like(w, memory_format=torch.channels_last) for w in w1]
        dw2 = [torch.empty_like(w, memory_format=torch.channels_last) for w in w2]
        db1 = [torch.empty((Hc,), dtype=torch.float32, device=dev) if h else None for h in has_b1]
        db2 = [torch.empty((C,), dtype=torch.float32, device=dev) if h else None for h in has_b2]

        def conv_bwd(x, w, dy, dx, dw, db):
            arr = (_lib.ConvDesc * n_scales)()
            for s in range(n_scales):
                _set_desc(arr[s], 1, 1, x.shape[2], dy.shape[2], 1, 1, 0, x=x[s], w=w[s], dy=dy[s], dx=dx[s], dw=dw[s], db=db[s])
            _conv2d_bwd(lib, arr, n_scales, B, dev, stream)
        conv_bwd(hidden, w2, dz, d_hidden, dw2, db2)
        g_hidden = torch.empty_like(d_hidden)
        _lib.check(lib.ssdk_relu_bwd(_dp(hidden), _dp(d_hidden), hidden.numel(), _dp(g_hidden), stream), 'ssdk_relu_bwd')
        conv_bwd(pooled, w1, g_hidden, dpool, dw1, db1)
        # 3. every piece's gradient: dout * sigmoid(z) + dpool / HW, one pass
        dpieces = []
        for s in range(n_scales):
            ds = [torch.empty_like(p, memory_format=torch.channels_last) for p in pieces[s]]
            darr = (ctypes.c_void_p * n_pieces)(*[t.data_ptr() for t in ds])
            _lib.check(lib.ssdk_sfam_gate_bwd_apply(darr, n_pieces, B, hw[s], Cp, z[s].data_ptr(), _dp(douts[s]), dpool[s].data_ptr(), stream),
                       'ssdk_sfam_gate_bwd_apply')
            dpieces += ds
        need = ctx.needs_input_grad
        grads = [g if need[2 + i] else None for i, g in enumerate(dpieces)]
        base = 2 + n_scales * n_pieces
        for s in range(n_scales):
            for j, g in enumerate((dw1[s], db1[s], dw2[s], db2[s])):
                grads.append(g if need[base + 4 * s + j] else None)
        return (None, None) + tuple(grads)


def sfam_pieces(pieces, fc1, fc2):
    """[cat(pieces_s, 1) * sigmoid(fc2_s(relu(fc1_s(avgpool(cat(pieces_s, 1)))))) for every scale s] (bf/modules/features.py:385, :286-298)
    with no concatenated map (``_SfamFn``).  ``pieces``: per scale the list of [B, Cp, H_s, W_s] maps; ``fc1`` / ``fc2``: per scale the 1 x 1
    nn.Conv2d layers.  ``sfam_pieces_ok`` says whether the kernels take the arguments."""
    n_scales, n_pieces = len(pieces), len(pieces[0])
    flat = [p for ps in pieces for p in ps]
    for a, b in zip(fc1, fc2):
        flat += [a.weight, a.bias, b.weight, b.bias]
    return list(_SfamFn.apply(n_scales, n_pieces, *flat))


def sfam_pieces_ok(pieces, fc1, fc2):
    if not pieces or len(pieces) != len(fc1) or len(pieces) != len(fc2) or len(pieces) > 8:
        return False
    n = len(pieces[0])
    if not (0 < n <= 8) or any(len(ps) != n for ps in pieces):
        return False
    first = pieces[0][0]
    Cp, B = first.shape[1], first.shape[0]
    for ps, a, b in zip(pieces, fc1, fc2):
        if any((not p.is_cuda) or p.dim() != 4 or p.dtype != torch.float32 or p.shape != ps[0].shape or p.shape[1] != Cp or p.shape[0] != B for p in ps):
            return False
        for m in (a, b):
            if not isinstance(m, torch.nn.Conv2d) or m.kernel_size != (1, 1) or m.stride != (1, 1) or m.padding != (0, 0) or m.groups != 1:
                return False
        if a.in_channels != n * Cp or b.out_channels != n * Cp or a.out_channels != b.in_channels or a.out_channels != fc1[0].out_channels:
            return False
    return Cp % 4 == 0 and fc1[0].out_channels % 4 == 0 and (B * fc1[0].out_channels * len(pieces)) % 4 == 0


class _DepthwiseFn(torch.autograd.Function):
    """Depthwise k x k convolution (groups = channels) on libssdk; weight is torch's [C, 1, k, k] parameter."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride, pad, stats=None):
        """stats: None, or the address of an fp64 `sums` buffer: the same launch adds the BatchNorm statistics of y to it
        (ssdk_depthwise_conv2d_stats_fwd; depthwise_conv2d_batch_norm)."""
        lib = _lib.lib()
        _lib.require_cuda(x, weight)
        x = _nhwc(x)
        B, C, H, W = x.shape
        k = weight.shape[-1]
        w = weight.float().contiguous()
        b = None if bias is None else bias.float().contiguous()
        y = _conv_out(x, C, k, stride, pad)
        if stats is None:
            _lib.check(lib.ssdk_depthwise_conv2d_fwd(_dp(x), _dp(w), _dp(b), B, H, W, C, k, stride, pad, _dp(y), _lib.current_stream()),
                       'ssdk_depthwise_conv2d_fwd')
        else:
            _lib.check(lib.ssdk_depthwise_conv2d_stats_fwd(_dp(x), _dp(w), _dp(b), B, H, W, C, k, stride, pad, _dp(y), stats, _lib.current_stream()),
                       'ssdk_depthwise_conv2d_stats_fwd')
        ctx.save_for_backward(x, w)
        ctx.meta = (stride, pad, bias is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.lib()
        x, w = ctx.saved_tensors
        stride, pad, has_bias = ctx.meta
        B, C, H, W = x.shape
        k = w.shape[-1]
        dy = _nhwc(dy)
        dx = torch.empty_like(x, memory_format=torch.channels_last) if ctx.needs_input_grad[0] else None
        dw = torch.empty_like(w)
        db = torch.empty((C,), dtype=torch.float32, device=x.device) if has_bias else None
        _lib.check(lib.ssdk_depthwise_conv2d_bwd(_dp(x), _dp(w), _dp(dy), B, H, W, C, k, stride, pad, _dp(dx), _dp(dw), _dp(db), 0,
                                                 _lib.current_stream()), 'ssdk_depthwise_conv2d_bwd')
        return dx, dw, db, None, None, None


class _DepthwiseGroupFn(torch.autograd.Function):
    """The depthwise convolution of n <= 8 maps that share weight and bias (the levels of a RetinaNet tower layer,
    detection/modules/predictors.py:33-35,67-68): one launch forward, one for the data gradients, two for dw / db
    (ssdk_depthwise_conv2d_group_*; no atomics, the same bits in both modes of ``set_deterministic``).
    apply(weight, bias, stride, pad, x_0, x_1, ...) -> y_0, y_1, ..."""

    @staticmethod
    def _levels(xs):
        n = len(xs)
        hs = (ctypes.c_int * n)(*[x.shape[2] for x in xs])
        ws = (ctypes.c_int * n)(*[x.shape[3] for x in xs])
        return n, hs, ws

    @staticmethod
    def _ptrs(ts):
        return (ctypes.c_void_p * len(ts))(*[_dp(t) for t in ts])

    @staticmethod
    def forward(ctx, weight, bias, stride, pad, *xs):
        lib = _lib.lib()
        _lib.require_cuda(weight, *xs)
        xs = [_nhwc(x) for x in xs]
        B, C = xs[0].shape[:2]
        if any(x.shape[0] != B or x.shape[1] != C for x in xs):
            raise ValueError('depthwise_conv2d: the maps of a list share batch and channels; got ' + str([tuple(x.shape) for x in xs]))
        k = weight.shape[-1]
        w = weight.float().contiguous()
        b = None if bias is None else bias.float().contiguous()
        ys = [_conv_out(x, C, k, stride, pad) for x in xs]
        n, hs, ws = _DepthwiseGroupFn._levels(xs)
        _lib.check(lib.ssdk_depthwise_conv2d_group_fwd(_DepthwiseGroupFn._ptrs(xs), hs, ws, n, _dp(w), _dp(b), B, C, k, stride, pad,
                                                       _DepthwiseGroupFn._ptrs(ys), _lib.current_stream()), 'ssdk_depthwise_conv2d_group_fwd')
        ctx.save_for_backward(w, *xs)
        ctx.meta = (stride, pad, bias is not None)
        return tuple(ys)

    @staticmethod
    def backward(ctx, *dys):
        lib = _lib.lib()
        w, xs = ctx.saved_tensors[0], list(ctx.saved_tensors[1:])
        stride, pad, has_bias = ctx.meta
        B, C = xs[0].shape[:2]
        k = w.shape[-1]
        n, hs, ws = _DepthwiseGroupFn._levels(xs)
        dys = [_conv_out(x, C, k, stride, pad).zero_() if dy is None else _nhwc(dy) for x, dy in zip(xs, dys)]   # (None: a level nobody used)
        dxs = [torch.empty_like(x, memory_format=torch.channels_last) if need else None for x, need in zip(xs, ctx.needs_input_grad[4:])]
        want_w = ctx.needs_input_grad[0] or (has_bias and ctx.needs_input_grad[1])
        dw = torch.empty_like(w) if want_w else None
        db = torch.empty((C,), dtype=torch.float32, device=w.device) if want_w and has_bias else None
        work, nbytes = None, 0
        if want_w:
            nbytes = lib.ssdk_depthwise_conv2d_group_workspace_bytes(hs, ws, n, B, C, k, stride, pad)
            if nbytes < 0:
                _lib.check(int(nbytes), 'ssdk_depthwise_conv2d_group_workspace_bytes')
            work = torch.empty((nbytes,), dtype=torch.uint8, device=w.device)
        if want_w or any(d is not None for d in dxs):
            _lib.check(lib.ssdk_depthwise_conv2d_group_bwd(_DepthwiseGroupFn._ptrs(xs), hs, ws, n, _dp(w), _DepthwiseGroupFn._ptrs(dys), B, C, k, stride, pad,
                                                           _DepthwiseGroupFn._ptrs(dxs), _dp(dw), _dp(db), _dp(work), nbytes, _lib.current_stream()),
                       'ssdk_depthwise_conv2d_group_bwd')
        return (dw if ctx.needs_input_grad[0] else None, db if has_bias and ctx.needs_input_grad[1] else None, None, None) + tuple(dxs)


def depthwise_conv2d(x, weight, bias=None, stride=1, padding=0):
    """Depthwise convolution of a map, or of a list of at most 8 maps that share the weights (one launch; returns a list)."""
    if isinstance(x, torch.Tensor):
        return _DepthwiseFn.apply(x, weight, bias, int(stride), int(padding))
    return list(_DepthwiseGroupFn.apply(weight, bias, int(stride), int(padding), *x))


def depthwise_conv2d_batch_norm(x, weight, bias, stride, padding, bn, relu=False):
    """depthwise conv -> BatchNorm (-> ReLU) of one map: a Conv2dBn block with groups = channels (bf/modules/conv.py:30-36; the
    `pyramid_output` blocks of FeaturePyramid(use_depthwise=True), bf/modules/features.py:79-98).
      training, a plain BatchNorm2d with per-process statistics and a clean `sums` chain: the stencil's launch accumulates the norm's
        statistics (ssdk_depthwise_conv2d_stats_fwd) and the norm is ONE apply launch -- no statistics pass over the activation
        (SSDK_NO_FUSED_STATS: off, the two-pass form);
      evaluation, a plain BatchNorm2d, nothing needs a gradient: ONE launch (ssdk_depthwise_conv2d_norm_fwd), the same bits as the two
        (which SSDK_NO_FUSED_STATS brings back as well);
      anything else (a norm marked for synchronisation, evaluation with gradients, a chain that is not clean, momentum=None, deterministic
        mode, an output above _DW_STATS_MAX_N4 where the two-pass form measured faster): depthwise_conv2d followed by batch_norm."""
    stride, padding = int(stride), int(padding)
    plain = type(bn) is torch.nn.BatchNorm2d and x.is_cuda and weight.shape[0] % 4 == 0
    chain = _local_training_chain(bn, x.device) if plain and torch.is_grad_enabled() and _dw_stats_fused(x, weight, stride, padding) else None
    if chain is not None:
        global fused_stats_calls
        chain.clean[0] = False   # (handed to the stencil: whatever happens next, it no longer holds zeros)
        fused_stats_calls += 1
        y = _DepthwiseFn.apply(x, weight, bias, stride, padding, chain.buf[0].data_ptr())
        return _norm_of_ready_sums(y, bn, chain, int(bool(relu)))
    if (plain and not _NO_FUSED_STATS and not bn.training and bn.momentum is not None and bn.track_running_stats
            and not (torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, weight, bias, bn.weight, bn.bias)))):
        lib = _lib.lib()
        _lib.require_cuda(x, weight)
        x = _nhwc(x)
        B, C, H, W = x.shape
        k = weight.shape[-1]
        w = weight.detach().float().contiguous()
        b, g, be = [None if t is None else t.detach().float().contiguous() for t in (bias, bn.weight, bn.bias)]
        y = _conv_out(x, C, k, stride, padding)
        _lib.check(lib.ssdk_depthwise_conv2d_norm_fwd(_dp(x), _dp(w), _dp(b), B, H, W, C, k, stride, padding, _dp(g), _dp(be), _dp(bn.running_mean),
                                                      _dp(bn.running_var), float(bn.eps), int(bool(relu)), _dp(y), _lib.current_stream()),
                   'ssdk_depthwise_conv2d_norm_fwd')
        return y
    return batch_norm(depthwise_conv2d_single(x, weight, bias, stride, padding), bn, relu=relu)


# Above this many float4 elements of output the statistics stay a pass of their own: on the 63 x 63 x 256 map at batch 32 (8.1 M float4) the
# stencil + bn_reduce pair takes 304 us and the fused launch 325; at 32 x 32 (2.1 M) they tie at 95 us, below it the fused launch wins
# (16 x 16: 32 against 36 us) -- profiles/fpnlite_kernel_stats.md.  SSDK_DW_STATS_MAX_N4 overrides (measurement knob).
_DW_STATS_MAX_N4 = int(os.environ.get('SSDK_DW_STATS_MAX_N4') or (1 << 21))


def _dw_stats_fused(x, weight, stride, padding):
    k = weight.shape[-1]
    n4 = x.shape[0] * _out_dim(x.shape[2], k, stride, padding) * _out_dim(x.shape[3], k, stride, padding) * (x.shape[1] // 4)
    # deterministic mode: the block's backward is the grouped entry's (depthwise_conv2d_single), and its forward the plain two-pass form
    return n4 <= _DW_STATS_MAX_N4 and not is_deterministic()


def depthwise_conv2d_single(x, weight, bias=None, stride=1, padding=0):
    """depthwise_conv2d of one map for a block whose maps can be large (the FPN-lite neck).  In deterministic mode the weight gradient of
    ssdk_depthwise_conv2d_bwd is ONE workgroup per 64 channel quads walking every pixel -- fine on the few-pixel maps of the SSD extras, 40 x
    the stock modules' time on a 63 x 63 map at batch 32 -- so there the map goes through the grouped entry as a group of one: its two-launch
    weight gradient has no atomics and the same bits in both modes."""
    if is_deterministic():
        return _DepthwiseGroupFn.apply(weight, bias, int(stride), int(padding), x)[0]
    return _DepthwiseFn.apply(x, weight, bias, int(stride), int(padding))


# ---- depthwise feature pyramid (Tiny-DSOD D-FPN, bf/modules/features.py:123-212) ------------------------------------------------

class _MaxPool2x2Fn(torch.autograd.Function):
    """nn.MaxPool2d(2)(F.pad(x, [0, pad_right, 0, pad_bottom])) (features.py:188-195): the pad is a real 0.0 in the max, its gradient is
    dropped; the backward recomputes each window's maximum from x (ssdk_maxpool2x2_*)."""

    @staticmethod
    def forward(ctx, x, pad_bottom, pad_right):
        _lib.require_cuda(x)
        x = _nhwc(x)
        B, C, H, W = x.shape
        y = torch.empty((B, C, (H + pad_bottom) // 2, (W + pad_right) // 2), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
        _lib.check(_lib.lib().ssdk_maxpool2x2_fwd(_dp(x), B, H, W, C, pad_bottom, pad_right, _dp(y), _lib.current_stream()), 'ssdk_maxpool2x2_fwd')
        ctx.save_for_backward(x)
        ctx.pads = (pad_bottom, pad_right)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, = ctx.saved_tensors
        B, C, H, W = x.shape
        dy = _nhwc(dy)
        dx = torch.empty_like(x, memory_format=torch.channels_last)
        _lib.check(_lib.lib().ssdk_maxpool2x2_bwd(_dp(x), _dp(dy), B, H, W, C, ctx.pads[0], ctx.pads[1], _dp(dx), _lib.current_stream()),
                   'ssdk_maxpool2x2_bwd')
        return dx, None, None


def maxpool2x2(x, pad_bottom=0, pad_right=0):
    """2 x 2 / stride 2 max-pool of ``x`` zero-padded by ``pad_bottom`` rows and ``pad_right`` columns (0 or 1 each).  A map without a
    single 2 x 2 window raises (as torch's max_pool2d does)."""
    if x.shape[2] + int(pad_bottom) < 2 or x.shape[3] + int(pad_right) < 2:
        raise ValueError(f'maxpool2x2: a {x.shape[2]} x {x.shape[3]} map padded by ({int(pad_bottom)}, {int(pad_right)}) has no 2 x 2 window '
                         '(zero-sized pooled output)')
    return _MaxPool2x2Fn.apply(x, int(pad_bottom), int(pad_right))


class _ConcatFn(torch.autograd.Function):
    """torch.cat(xs, dim=1) of NHWC maps (features.py:198); the backward writes each piece's gradient as its own contiguous map."""

    @staticmethod
    def forward(ctx, *xs):
        _lib.require_cuda(*xs)
        xs = [_nhwc(x) for x in xs]
        B, _, H, W = xs[0].shape
        assert all(x.shape[0] == B and x.shape[2:] == xs[0].shape[2:] for x in xs), [tuple(x.shape) for x in xs]
        chans = [x.shape[1] for x in xs]
        out = torch.empty((B, sum(chans), H, W), dtype=torch.float32, device=xs[0].device, memory_format=torch.channels_last)
        ptrs = (ctypes.c_void_p * len(xs))(*[x.data_ptr() for x in xs])
        cs = (ctypes.c_int * len(xs))(*chans)
        _lib.check(_lib.lib().ssdk_concat_channels_fwd(ptrs, cs, len(xs), B * H * W, _dp(out), _lib.current_stream()), 'ssdk_concat_channels_fwd')
        ctx.shapes = [tuple(x.shape) for x in xs]
        return out

    @staticmethod
    def backward(ctx, dout):
        dout = _nhwc(dout)
        B, _, H, W = dout.shape
        ds = [torch.empty(s, dtype=torch.float32, device=dout.device, memory_format=torch.channels_last) for s in ctx.shapes]
        ptrs = (ctypes.c_void_p * len(ds))(*[d.data_ptr() for d in ds])
        cs = (ctypes.c_int * len(ds))(*[s[1] for s in ctx.shapes])
        _lib.check(_lib.lib().ssdk_concat_channels_bwd(_dp(dout), cs, len(ds), B * H * W, ptrs, _lib.current_stream()), 'ssdk_concat_channels_bwd')
        return tuple(ds)


def concat_channels(xs):
    """torch.cat(xs, dim=1) for up to 8 maps of one batch and size (channels of each % 4 == 0)."""
    return _ConcatFn.apply(*xs)


class _DepthwiseUpsampleFn(torch.autograd.Function):
    """F.conv2d(F.interpolate(coarse, size=(hf, wf), mode='nearest'), weight, bias, padding=1, groups=C) (features.py:203-205, the
    convolution of up_conv[i]) without the upsampled map: ssdk_depthwise_upsample_conv2d_*; weight is torch's [C, 1, 3, 3] parameter."""

    @staticmethod
    def forward(ctx, coarse, weight, bias, hf, wf):
        lib = _lib.lib()
        _lib.require_cuda(coarse, weight)
        coarse = _nhwc(coarse)
        B, C, Hc, Wc = coarse.shape
        assert tuple(weight.shape) == (C, 1, 3, 3), tuple(weight.shape)
        w = weight.float().contiguous()
        b = None if bias is None else bias.float().contiguous()
        y = torch.empty((B, C, hf, wf), dtype=torch.float32, device=coarse.device, memory_format=torch.channels_last)
        _lib.check(lib.ssdk_depthwise_upsample_conv2d_fwd(_dp(coarse), _dp(w), _dp(b), B, Hc, Wc, hf, wf, C, _dp(y), _lib.current_stream()),
                   'ssdk_depthwise_upsample_conv2d_fwd')
        ctx.save_for_backward(coarse, w)
        ctx.meta = (hf, wf, bias is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        coarse, w = ctx.saved_tensors
        hf, wf, has_bias = ctx.meta
        B, C, Hc, Wc = coarse.shape
        dy = _nhwc(dy)
        dc = torch.empty_like(coarse, memory_format=torch.channels_last) if ctx.needs_input_grad[0] else None
        dw = torch.empty_like(w)
        db = torch.empty((C,), dtype=torch.float32, device=coarse.device) if has_bias else None
        _lib.check(_lib.lib().ssdk_depthwise_upsample_conv2d_bwd(_dp(coarse), _dp(w), _dp(dy), B, Hc, Wc, hf, wf, C, _dp(dc), _dp(dw), _dp(db),
                                                                 _lib.current_stream()), 'ssdk_depthwise_upsample_conv2d_bwd')
        return dc, dw, db, None, None


def depthwise_upsample_conv2d(coarse, weight, bias, size):
    """3 x 3 depthwise convolution (pad 1, stride 1) of ``F.interpolate(coarse, size, mode='nearest')``."""
    return _DepthwiseUpsampleFn.apply(coarse, weight, bias, int(size[0]), int(size[1]))
