"""Child process of tests/test_dwgroup_gpu.py: ops.depthwise_conv2d on a list of levels and its backward (ssdk_depthwise_conv2d_group_*)
captured in ONE torch.cuda.graph on one stream and replayed twice -- the outputs, the input gradients and dw / db of every replay are the
eager bits.  The entry points take host pointer arrays and pack them into the kernel argument: nothing of a call lives on the device but
the maps and the torch-allocated workspace, so a replay needs no table that a later call could have overwritten.  A process of its own, so
that the captured graph and its memory pool are not the starting state of the tests that follow.  One JSON line is printed at the end.
Usage: python tests/dwgroup_graph_worker.py"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dwgroup_reference as ref                    # noqa: E402
from single_shot_detection_amd import ops          # noqa: E402


def bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float32).view(np.uint32)


def tensors(name, seed):
    xs, dys, weight, bias = ref.normal_operands(name, seed=seed)
    nchw = lambda a: torch.from_numpy(a).cuda().permute(0, 3, 1, 2)   # noqa: E731  (channels_last memory = the NHWC array)
    return [nchw(x) for x in xs], [nchw(d) for d in dys], torch.from_numpy(weight).cuda()[:, None].contiguous(), torch.from_numpy(bias).cuda()


def step(xs, dys, weight, bias, stride, pad):
    ys = ops.depthwise_conv2d(xs, weight, bias, stride, pad)
    return list(ys) + list(torch.autograd.grad(ys, xs + [weight, bias], dys))


def main():
    name = 'c32_8levels'
    _, _, _, k, stride, pad = ref.CASES[name]
    first, second = tensors(name, 3), tensors(name, 4)
    eager = []
    for xs, dys, weight, bias in (first, second):
        eager.append([bits(t) for t in step([x.clone().requires_grad_(True) for x in xs], dys, weight.clone().requires_grad_(True),
                                            bias.clone().requires_grad_(True), stride, pad)])
    xs = [x.clone().requires_grad_(True) for x in first[0]]
    dys = [d.clone() for d in first[1]]
    weight, bias = first[2].clone().requires_grad_(True), first[3].clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(xs, dys, weight, bias, stride, pad)      # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        outs = step(xs, dys, weight, bias, stride, pad)
    compared = 0
    for (nx, ndy, nw, nb), want in zip((first, second), eager):
        with torch.no_grad():
            for dst, src in zip(xs + dys + [weight, bias], nx + ndy + [nw, nb]):
                dst.copy_(src)
            for o in outs:
                o.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        for got, ref_bits in zip(outs, want):
            assert np.array_equal(bits(got), ref_bits)
            compared += 1
    print(json.dumps({'replays': 2, 'tensors_compared': compared}))


if __name__ == '__main__':
    main()
