"""Case tables and input builders of the fused optimizer steps (no pytest): the six entry points r3m_{adam,sgd}_step{,_ranges,_groups} of
csrc/adam.hip. tests/test_gpu_optim_steps.py, tests/test_gpu_optim_ranges.py and tests/test_gpu_optim_groups.py run them on the GPU;
tools/optim_bits.py hashes what the entry points write for them.

SIZES are the buffer sizes at which the launch changes shape: one f32x4 group; one block plus one group; opt_grid's cap of 4096 blocks
plus a ragged second trip of three groups. CASES are range lists (offset, count, step) -- multiples of 4, sorted, disjoint -- over a
buffer of N elements: a single group, one group past a block, neighbours, a range that ends at the buffer end, step counts that
differ, one range more than a launch holds, and an empty range between two others."""
import ctypes as C

import torch

from util import DEV

GRID_CAP = 4096 * 256                                   # f32x4 groups one trip of the capped grid covers (csrc/adam.hip opt_grid)
SIZES = [4, 1028, 4 * GRID_CAP + 12]

N = 4 * 257 * 9 + 64          # a few blocks of 256 float4 groups, not a multiple of the block
CASES = {
    "count4": [(8, 4, 1)],
    "count4x257": [(16, 4 * 257, 3)],
    "adjacent": [(0, 64, 2), (64, 1024, 2), (1088, 4, 5)],
    "ends_at_buffer_end": [(4, 12, 1), (N - 4 * 300, 4 * 300, 7)],
    "distinct_steps": [(0, 256, 1), (512, 2048, 2), (4096, 4 * 257, 1000), (N - 8, 8, 4)],
    "65_ranges": [(32 * i, 4 * (1 + i % 7), 1 + i % 3) for i in range(65)],
    "empty_range_between": [(0, 8, 1), (8, 0, 1), (16, 8, 2)],
}
HYPER = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, gs=0.5)

# SGD in four configurations: as keyword arguments of torch.optim.SGD (the four of tests/test_gpu_ops.py::test_sgd_matches_torch) ...
SGD_CFGS = [dict(momentum=0.0), dict(momentum=0.9), dict(momentum=0.9, dampening=0.1, weight_decay=1e-2),
            dict(momentum=0.9, nesterov=True, weight_decay=1e-3)]
SGD_IDS = ["plain", "momentum", "damp_wd", "nesterov"]
# ... and as the scalars of the C entry points, for the ranged and grouped steps
SGD = [dict(momentum=0.0, damp=0.0, wd=0.0, nesterov=0), dict(momentum=0.9, damp=0.0, wd=0.0, nesterov=0),
       dict(momentum=0.9, damp=0.1, wd=1e-2, nesterov=0), dict(momentum=0.9, damp=0.0, wd=1e-2, nesterov=1)]


def _ll(v):
    return (C.c_longlong * len(v))(*v)


def _dd(v):
    return (C.c_double * len(v))(*v)


def _state(seed, n=N):
    """p, gradient, m, v (or a momentum buffer in m's place) on the GPU"""
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g)
    grad = torch.randn(n, generator=g) * 0.01
    m = torch.randn(n, generator=g) * 0.01
    v = torch.rand(n, generator=g) * 1e-4
    return [t.to(DEV) for t in (p, grad, m, v)]
