"""The kernel-instance table the instance tests are driven by (tests/test_instance_table.py on the CPU,
tests/test_gpu_instances.py on the GPU).

Every entry of the kernel registry (``ff_kernel_count`` / ``ff_kernel_name``: the f32 instances of build.py ``INSTANCES``
and ``WIDE_INSTANCES``, the split-precision ones of ``SPLIT_INSTANCES``) has at least two rows here, each a network shape
the planner (``ff_mlp_plan_prec``) must land on that instance:

* ``top``: the largest state dimension, conditional dimension and width the instance holds -- D = dregs * 64 / tile,
  C = cregs * 64 / tile, widest layer = H (split: D = 16 per state tile, C = 16, the compiled depth) -- with ragged widths
  (H, H - 1, just above the next narrower width) five hidden layers deep on f32;
* ``bottom``: the smallest shape that still lands on it rather than on a neighbour (smallest C, then D, then width).

The table is static on purpose: an instance added to the build without rows here fails test_instance_table.py, and a row
that no longer plans to its instance names the instance.  ``_a9`` instances (activation chosen at run time) carry one row
per non-SiLU activation, alternating corners.

Row fields: kernel name, corner, D, C, hidden widths, activation, precision, mode -- "state" / "tangent" (f32: Hutchinson
and exact trace plan to the same divergence-capable instance) / "hutch" / "exact" (split: an instance per mode).
"""
from collections import namedtuple

import torch

Row = namedtuple("Row", "kernel corner D C units act prec mode")


def R(*a):
    return Row(*a)


ROWS = [
    R('mlp_ode_m32_h64_d4_c0_t0', 'top', 8, 0, (63, 64, 33, 64, 63), 'silu', 'f32', 'state'),
    R('mlp_ode_m32_h64_d4_c0_t0', 'bottom', 1, 0, (1,), 'silu', 'f32', 'state'),
    R('mlp_ode_m32_h64_d4_c0_t1', 'top', 8, 0, (63, 64, 33, 64, 63), 'silu', 'f32', 'tangent'),
    R('mlp_ode_m32_h64_d4_c0_t1', 'bottom', 1, 0, (1,), 'silu', 'f32', 'tangent'),
    R('mlp_ode_m32_h64_d4_c8_t0', 'top', 8, 16, (63, 64, 33, 64, 63), 'silu', 'f32', 'state'),
    R('mlp_ode_m32_h64_d4_c8_t0', 'bottom', 1, 1, (1,), 'silu', 'f32', 'state'),
    R('mlp_ode_m32_h64_d4_c8_t1', 'top', 8, 16, (63, 64, 33, 64, 63), 'silu', 'f32', 'tangent'),
    R('mlp_ode_m32_h64_d4_c8_t1', 'bottom', 1, 1, (1,), 'silu', 'f32', 'tangent'),
    R('mlp_ode_m32_h64_d8_c0_t0', 'top', 16, 0, (63, 64, 33, 64, 63), 'silu', 'f32', 'state'),
    R('mlp_ode_m32_h64_d8_c0_t0', 'bottom', 9, 0, (1,), 'silu', 'f32', 'state'),
    R('mlp_ode_m32_h64_d8_c0_t1', 'top', 16, 0, (63, 64, 33, 64, 63), 'silu', 'f32', 'tangent'),
    R('mlp_ode_m32_h64_d8_c0_t1', 'bottom', 9, 0, (1,), 'silu', 'f32', 'tangent'),
    R('mlp_ode_m32_h64_d8_c8_t0', 'top', 16, 16, (63, 64, 33, 64, 63), 'silu', 'f32', 'state'),
    R('mlp_ode_m32_h64_d8_c8_t0', 'bottom', 9, 1, (1,), 'silu', 'f32', 'state'),
    R('mlp_ode_m32_h64_d8_c8_t1', 'top', 16, 16, (63, 64, 33, 64, 63), 'silu', 'f32', 'tangent'),
    R('mlp_ode_m32_h64_d8_c8_t1', 'bottom', 9, 1, (1,), 'silu', 'f32', 'tangent'),
    R('mlp_ode_m32_h64_d16_c0_t0', 'top', 32, 0, (63, 64, 33, 64, 63), 'silu', 'f32', 'state'),
    R('mlp_ode_m32_h64_d16_c0_t0', 'bottom', 17, 0, (1,), 'silu', 'f32', 'state'),
    R('mlp_ode_m32_h64_d16_c0_t1', 'top', 32, 0, (63, 64, 33, 64, 63), 'silu', 'f32', 'tangent'),
    R('mlp_ode_m32_h64_d16_c0_t1', 'bottom', 17, 0, (1,), 'silu', 'f32', 'tangent'),
    R('mlp_ode_m32_h64_d16_c8_t0', 'top', 32, 16, (63, 64, 33, 64, 63), 'silu', 'f32', 'state'),
    R('mlp_ode_m32_h64_d16_c8_t0', 'bottom', 17, 1, (1,), 'silu', 'f32', 'state'),
    R('mlp_ode_m32_h64_d16_c8_t1', 'top', 32, 16, (63, 64, 33, 64, 63), 'silu', 'f32', 'tangent'),
    R('mlp_ode_m32_h64_d16_c8_t1', 'bottom', 17, 1, (1,), 'silu', 'f32', 'tangent'),
    R('mlp_ode_m32_h128_d16_c0_t0', 'top', 32, 0, (127, 128, 65, 128, 127), 'silu', 'f32', 'state'),
    R('mlp_ode_m32_h128_d16_c0_t0', 'bottom', 17, 0, (65,), 'silu', 'f32', 'state'),
    R('mlp_ode_m32_h128_d16_c0_t1', 'top', 32, 0, (127, 128, 65, 128, 127), 'silu', 'f32', 'tangent'),
    R('mlp_ode_m32_h128_d16_c0_t1', 'bottom', 17, 0, (65,), 'silu', 'f32', 'tangent'),
    R('mlp_ode_m32_h128_d16_c8_t0', 'top', 32, 16, (127, 128, 65, 128, 127), 'silu', 'f32', 'state'),
    R('mlp_ode_m32_h128_d16_c8_t0', 'bottom', 17, 1, (65,), 'silu', 'f32', 'state'),
    R('mlp_ode_m32_h128_d16_c8_t1', 'top', 32, 16, (127, 128, 65, 128, 127), 'silu', 'f32', 'tangent'),
    R('mlp_ode_m32_h128_d16_c8_t1', 'bottom', 17, 1, (65,), 'silu', 'f32', 'tangent'),
    R('mlp_ode_m16_h128_d4_c0_t0_w3', 'top', 16, 0, (127, 128, 65, 128, 127), 'silu', 'f32', 'state'),
    R('mlp_ode_m16_h128_d4_c0_t0_w3', 'bottom', 1, 0, (65,), 'silu', 'f32', 'state'),
    R('mlp_ode_m16_h128_d4_c0_t1_w3', 'top', 16, 0, (127, 128, 65, 128, 127), 'silu', 'f32', 'tangent'),
    R('mlp_ode_m16_h128_d4_c0_t1_w3', 'bottom', 1, 0, (65,), 'silu', 'f32', 'tangent'),
    R('mlp_ode_m16_h128_d4_c4_t0_w3', 'top', 16, 16, (127, 128, 65, 128, 127), 'silu', 'f32', 'state'),
    R('mlp_ode_m16_h128_d4_c4_t0_w3', 'bottom', 1, 1, (65,), 'silu', 'f32', 'state'),
    R('mlp_ode_m16_h128_d4_c4_t1_w3', 'top', 16, 16, (127, 128, 65, 128, 127), 'silu', 'f32', 'tangent'),
    R('mlp_ode_m16_h128_d4_c4_t1_w3', 'bottom', 1, 1, (65,), 'silu', 'f32', 'tangent'),
    R('mlp_ode_m16_h256_d4_c0_t0_w2', 'top', 16, 0, (255, 256, 129, 256, 255), 'silu', 'f32', 'state'),
    R('mlp_ode_m16_h256_d4_c0_t0_w2', 'bottom', 1, 0, (129,), 'silu', 'f32', 'state'),
    R('mlp_ode_m16_h256_d4_c0_t1_w2', 'top', 16, 0, (255, 256, 129, 256, 255), 'silu', 'f32', 'tangent'),
    R('mlp_ode_m16_h256_d4_c0_t1_w2', 'bottom', 1, 0, (129,), 'silu', 'f32', 'tangent'),
    R('mlp_ode_m16_h256_d4_c4_t0_w2', 'top', 16, 16, (255, 256, 129, 256, 255), 'silu', 'f32', 'state'),
    R('mlp_ode_m16_h256_d4_c4_t0_w2', 'bottom', 1, 1, (129,), 'silu', 'f32', 'state'),
    R('mlp_ode_m16_h256_d4_c4_t1_w2', 'top', 16, 16, (255, 256, 129, 256, 255), 'silu', 'f32', 'tangent'),
    R('mlp_ode_m16_h256_d4_c4_t1_w2', 'bottom', 1, 1, (129,), 'silu', 'f32', 'tangent'),
    R('mlp_ode_m16_h256_d8_c4_t0_w2', 'top', 32, 16, (255, 256, 129, 256, 255), 'silu', 'f32', 'state'),
    R('mlp_ode_m16_h256_d8_c4_t0_w2', 'bottom', 17, 0, (129,), 'silu', 'f32', 'state'),
    R('mlp_ode_m16_h256_d8_c4_t1_w2', 'top', 32, 16, (255, 256, 129, 256, 255), 'silu', 'f32', 'tangent'),
    R('mlp_ode_m16_h256_d8_c4_t1_w2', 'bottom', 17, 0, (129,), 'silu', 'f32', 'tangent'),
    R('mlp_ode_m16_h256_d8_c8_t0_w2', 'top', 32, 32, (255, 256, 129, 256, 255), 'silu', 'f32', 'state'),
    R('mlp_ode_m16_h256_d8_c8_t0_w2', 'bottom', 1, 17, (1,), 'silu', 'f32', 'state'),
    R('mlp_ode_m16_h256_d8_c8_t1_w2', 'top', 32, 32, (255, 256, 129, 256, 255), 'silu', 'f32', 'tangent'),
    R('mlp_ode_m16_h256_d8_c8_t1_w2', 'bottom', 1, 17, (1,), 'silu', 'f32', 'tangent'),
    R('mlp_ode_m16_h256_d16_c4_t0', 'top', 64, 16, (255, 256, 129, 256, 255), 'silu', 'f32', 'state'),
    R('mlp_ode_m16_h256_d16_c4_t0', 'bottom', 33, 0, (1,), 'silu', 'f32', 'state'),
    R('mlp_ode_m16_h256_d16_c4_t1', 'top', 64, 16, (255, 256, 129, 256, 255), 'silu', 'f32', 'tangent'),
    R('mlp_ode_m16_h256_d16_c4_t1', 'bottom', 33, 0, (1,), 'silu', 'f32', 'tangent'),
    R('mlp_ode_m16_h512_d16_c4_t0', 'top', 64, 16, (511, 512, 257, 512, 511), 'silu', 'f32', 'state'),
    R('mlp_ode_m16_h512_d16_c4_t0', 'bottom', 1, 0, (257,), 'silu', 'f32', 'state'),
    R('mlp_ode_m16_h512_d16_c4_t1', 'top', 64, 16, (511, 512, 257, 512, 511), 'silu', 'f32', 'tangent'),
    R('mlp_ode_m16_h512_d16_c4_t1', 'bottom', 1, 0, (257,), 'silu', 'f32', 'tangent'),
    R('mlp_ode_m32_h128_d16_c8_t0_a9', 'top', 32, 16, (127, 128, 65, 128, 127), 'tanh', 'f32', 'state'),
    R('mlp_ode_m32_h128_d16_c8_t0_a9', 'bottom', 1, 0, (1,), 'sigmoid', 'f32', 'state'),
    R('mlp_ode_m32_h128_d16_c8_t0_a9', 'top', 32, 16, (127, 128, 65, 128, 127), 'relu', 'f32', 'state'),
    R('mlp_ode_m32_h128_d16_c8_t0_a9', 'bottom', 1, 0, (1,), 'leaky_relu', 'f32', 'state'),
    R('mlp_ode_m32_h128_d16_c8_t0_a9', 'top', 32, 16, (127, 128, 65, 128, 127), 'elu', 'f32', 'state'),
    R('mlp_ode_m32_h128_d16_c8_t0_a9', 'bottom', 1, 0, (1,), 'softplus', 'f32', 'state'),
    R('mlp_ode_m32_h128_d16_c8_t0_a9', 'top', 32, 16, (127, 128, 65, 128, 127), 'gelu', 'f32', 'state'),
    R('mlp_ode_m32_h128_d16_c8_t0_a9', 'bottom', 1, 0, (1,), 'gelu_tanh', 'f32', 'state'),
    R('mlp_ode_m32_h128_d16_c8_t1_a9', 'top', 32, 16, (127, 128, 65, 128, 127), 'tanh', 'f32', 'tangent'),
    R('mlp_ode_m32_h128_d16_c8_t1_a9', 'bottom', 1, 0, (1,), 'sigmoid', 'f32', 'tangent'),
    R('mlp_ode_m32_h128_d16_c8_t1_a9', 'top', 32, 16, (127, 128, 65, 128, 127), 'relu', 'f32', 'tangent'),
    R('mlp_ode_m32_h128_d16_c8_t1_a9', 'bottom', 1, 0, (1,), 'leaky_relu', 'f32', 'tangent'),
    R('mlp_ode_m32_h128_d16_c8_t1_a9', 'top', 32, 16, (127, 128, 65, 128, 127), 'elu', 'f32', 'tangent'),
    R('mlp_ode_m32_h128_d16_c8_t1_a9', 'bottom', 1, 0, (1,), 'softplus', 'f32', 'tangent'),
    R('mlp_ode_m32_h128_d16_c8_t1_a9', 'top', 32, 16, (127, 128, 65, 128, 127), 'gelu', 'f32', 'tangent'),
    R('mlp_ode_m32_h128_d16_c8_t1_a9', 'bottom', 1, 0, (1,), 'gelu_tanh', 'f32', 'tangent'),
    R('mlp_ode_m16_h256_d8_c4_t0_a9', 'top', 32, 16, (255, 256, 129, 256, 255), 'tanh', 'f32', 'state'),
    R('mlp_ode_m16_h256_d8_c4_t0_a9', 'bottom', 1, 0, (129,), 'sigmoid', 'f32', 'state'),
    R('mlp_ode_m16_h256_d8_c4_t0_a9', 'top', 32, 16, (255, 256, 129, 256, 255), 'relu', 'f32', 'state'),
    R('mlp_ode_m16_h256_d8_c4_t0_a9', 'bottom', 1, 0, (129,), 'leaky_relu', 'f32', 'state'),
    R('mlp_ode_m16_h256_d8_c4_t0_a9', 'top', 32, 16, (255, 256, 129, 256, 255), 'elu', 'f32', 'state'),
    R('mlp_ode_m16_h256_d8_c4_t0_a9', 'bottom', 1, 0, (129,), 'softplus', 'f32', 'state'),
    R('mlp_ode_m16_h256_d8_c4_t0_a9', 'top', 32, 16, (255, 256, 129, 256, 255), 'gelu', 'f32', 'state'),
    R('mlp_ode_m16_h256_d8_c4_t0_a9', 'bottom', 1, 0, (129,), 'gelu_tanh', 'f32', 'state'),
    R('mlp_ode_m16_h512_d16_c4_t0_a9', 'top', 64, 16, (511, 512, 257, 512, 511), 'tanh', 'f32', 'state'),
    R('mlp_ode_m16_h512_d16_c4_t0_a9', 'bottom', 1, 0, (257,), 'sigmoid', 'f32', 'state'),
    R('mlp_ode_m16_h512_d16_c4_t0_a9', 'top', 64, 16, (511, 512, 257, 512, 511), 'relu', 'f32', 'state'),
    R('mlp_ode_m16_h512_d16_c4_t0_a9', 'bottom', 1, 0, (257,), 'leaky_relu', 'f32', 'state'),
    R('mlp_ode_m16_h512_d16_c4_t0_a9', 'top', 64, 16, (511, 512, 257, 512, 511), 'elu', 'f32', 'state'),
    R('mlp_ode_m16_h512_d16_c4_t0_a9', 'bottom', 1, 0, (257,), 'softplus', 'f32', 'state'),
    R('mlp_ode_m16_h512_d16_c4_t0_a9', 'top', 64, 16, (511, 512, 257, 512, 511), 'gelu', 'f32', 'state'),
    R('mlp_ode_m16_h512_d16_c4_t0_a9', 'bottom', 1, 0, (257,), 'gelu_tanh', 'f32', 'state'),
    R('mlp_ode_m16_h512_d16_c4_t1_a9', 'top', 64, 16, (511, 512, 257, 512, 511), 'tanh', 'f32', 'tangent'),
    R('mlp_ode_m16_h512_d16_c4_t1_a9', 'bottom', 1, 0, (257,), 'sigmoid', 'f32', 'tangent'),
    R('mlp_ode_m16_h512_d16_c4_t1_a9', 'top', 64, 16, (511, 512, 257, 512, 511), 'relu', 'f32', 'tangent'),
    R('mlp_ode_m16_h512_d16_c4_t1_a9', 'bottom', 1, 0, (257,), 'leaky_relu', 'f32', 'tangent'),
    R('mlp_ode_m16_h512_d16_c4_t1_a9', 'top', 64, 16, (511, 512, 257, 512, 511), 'elu', 'f32', 'tangent'),
    R('mlp_ode_m16_h512_d16_c4_t1_a9', 'bottom', 1, 0, (257,), 'softplus', 'f32', 'tangent'),
    R('mlp_ode_m16_h512_d16_c4_t1_a9', 'top', 64, 16, (511, 512, 257, 512, 511), 'gelu', 'f32', 'tangent'),
    R('mlp_ode_m16_h512_d16_c4_t1_a9', 'bottom', 1, 0, (257,), 'gelu_tanh', 'f32', 'tangent'),
    R('mlp_ode_m16_h256_d8_c4_t1_a1', 'top', 32, 16, (255, 256, 129, 256, 255), 'tanh', 'f32', 'tangent'),
    R('mlp_ode_m16_h256_d8_c4_t1_a1', 'bottom', 1, 0, (129,), 'tanh', 'f32', 'tangent'),
    R('mlp_ode_m16_h256_d8_c4_t1_a2', 'top', 32, 16, (255, 256, 129, 256, 255), 'sigmoid', 'f32', 'tangent'),
    R('mlp_ode_m16_h256_d8_c4_t1_a2', 'bottom', 1, 0, (129,), 'sigmoid', 'f32', 'tangent'),
    R('mlp_ode_m16_h256_d8_c4_t1_a3', 'top', 32, 16, (255, 256, 129, 256, 255), 'relu', 'f32', 'tangent'),
    R('mlp_ode_m16_h256_d8_c4_t1_a3', 'bottom', 1, 0, (129,), 'relu', 'f32', 'tangent'),
    R('mlp_ode_m16_h256_d8_c4_t1_a4', 'top', 32, 16, (255, 256, 129, 256, 255), 'leaky_relu', 'f32', 'tangent'),
    R('mlp_ode_m16_h256_d8_c4_t1_a4', 'bottom', 1, 0, (129,), 'leaky_relu', 'f32', 'tangent'),
    R('mlp_ode_m16_h256_d8_c4_t1_a5', 'top', 32, 16, (255, 256, 129, 256, 255), 'elu', 'f32', 'tangent'),
    R('mlp_ode_m16_h256_d8_c4_t1_a5', 'bottom', 1, 0, (129,), 'elu', 'f32', 'tangent'),
    R('mlp_ode_m16_h256_d8_c4_t1_a6', 'top', 32, 16, (255, 256, 129, 256, 255), 'softplus', 'f32', 'tangent'),
    R('mlp_ode_m16_h256_d8_c4_t1_a6', 'bottom', 1, 0, (129,), 'softplus', 'f32', 'tangent'),
    R('mlp_ode_m16_h256_d8_c4_t1_a7', 'top', 32, 16, (255, 256, 129, 256, 255), 'gelu', 'f32', 'tangent'),
    R('mlp_ode_m16_h256_d8_c4_t1_a7', 'bottom', 1, 0, (129,), 'gelu', 'f32', 'tangent'),
    R('mlp_ode_m16_h256_d8_c4_t1_a8', 'top', 32, 16, (255, 256, 129, 256, 255), 'gelu_tanh', 'f32', 'tangent'),
    R('mlp_ode_m16_h256_d8_c4_t1_a8', 'bottom', 1, 0, (129,), 'gelu_tanh', 'f32', 'tangent'),
    R('mlp_ode_m16_h1024_d32_c16_t0_wide', 'top', 128, 64, (1023, 1024, 513, 1024, 1023), 'silu', 'f32', 'state'),
    R('mlp_ode_m16_h1024_d32_c16_t0_wide', 'bottom', 1, 0, (513,), 'silu', 'f32', 'state'),
    R('mlp_ode_m16_h1024_d32_c16_t1_wide', 'top', 128, 64, (1023, 1024, 513, 1024, 1023), 'silu', 'f32', 'tangent'),
    R('mlp_ode_m16_h1024_d32_c16_t1_wide', 'bottom', 1, 0, (513,), 'silu', 'f32', 'tangent'),
    R('mlp_ode_split_h256_n1_t0', 'top', 16, 16, (256,), 'silu', 'bf16x3', 'state'),
    R('mlp_ode_split_h256_n1_t0', 'bottom', 1, 0, (1,), 'silu', 'bf16x3', 'state'),
    R('mlp_ode_split_h256_n2_t0', 'top', 16, 16, (256, 255), 'silu', 'bf16x3', 'state'),
    R('mlp_ode_split_h256_n2_t0', 'bottom', 1, 0, (1, 1), 'silu', 'bf16x3', 'state'),
    R('mlp_ode_split_h256_n3_t0', 'top', 16, 16, (256, 255, 129), 'silu', 'bf16x3', 'state'),
    R('mlp_ode_split_h256_n3_t0', 'bottom', 1, 0, (1, 1, 1), 'silu', 'bf16x3', 'state'),
    R('mlp_ode_split_h256_n4_t0', 'top', 16, 16, (256, 255, 129, 255), 'silu', 'bf16x3', 'state'),
    R('mlp_ode_split_h256_n4_t0', 'bottom', 1, 0, (1, 1, 1, 1), 'silu', 'bf16x3', 'state'),
    R('mlp_ode_split2_h256_n1_t0', 'top', 16, 16, (256,), 'silu', 'bf16x2', 'state'),
    R('mlp_ode_split2_h256_n1_t0', 'bottom', 1, 0, (129,), 'silu', 'bf16x2', 'state'),
    R('mlp_ode_split2_h256_n1_t1', 'top', 16, 16, (256,), 'silu', 'bf16x2', 'hutch'),
    R('mlp_ode_split2_h256_n1_t1', 'bottom', 1, 0, (129,), 'silu', 'bf16x2', 'hutch'),
    R('mlp_ode_split2_h256_n1_t2', 'top', 16, 16, (256,), 'silu', 'bf16x2', 'exact'),
    R('mlp_ode_split2_h256_n1_t2', 'bottom', 1, 0, (129,), 'silu', 'bf16x2', 'exact'),
    R('mlp_ode_split2_h256_n2_t0', 'top', 16, 16, (256, 255), 'silu', 'bf16x2', 'state'),
    R('mlp_ode_split2_h256_n2_t0', 'bottom', 1, 0, (129, 128), 'silu', 'bf16x2', 'state'),
    R('mlp_ode_split2_h256_n2_t1', 'top', 16, 16, (256, 255), 'silu', 'bf16x2', 'hutch'),
    R('mlp_ode_split2_h256_n2_t1', 'bottom', 1, 0, (129, 128), 'silu', 'bf16x2', 'hutch'),
    R('mlp_ode_split2_h256_n2_t2', 'top', 16, 16, (256, 255), 'silu', 'bf16x2', 'exact'),
    R('mlp_ode_split2_h256_n2_t2', 'bottom', 1, 0, (129, 128), 'silu', 'bf16x2', 'exact'),
    R('mlp_ode_split2_h256_n3_t0', 'top', 16, 16, (256, 255, 129), 'silu', 'bf16x2', 'state'),
    R('mlp_ode_split2_h256_n3_t0', 'bottom', 1, 0, (129, 128, 127), 'silu', 'bf16x2', 'state'),
    R('mlp_ode_split2_h256_n3_t1', 'top', 16, 16, (256, 255, 129), 'silu', 'bf16x2', 'hutch'),
    R('mlp_ode_split2_h256_n3_t1', 'bottom', 1, 0, (129, 128, 127), 'silu', 'bf16x2', 'hutch'),
    R('mlp_ode_split2_h256_n3_t2', 'top', 16, 16, (256, 255, 129), 'silu', 'bf16x2', 'exact'),
    R('mlp_ode_split2_h256_n3_t2', 'bottom', 1, 0, (129, 128, 127), 'silu', 'bf16x2', 'exact'),
    R('mlp_ode_split2_h256_n4_t0', 'top', 16, 16, (256, 255, 129, 255), 'silu', 'bf16x2', 'state'),
    R('mlp_ode_split2_h256_n4_t0', 'bottom', 1, 0, (129, 128, 127, 126), 'silu', 'bf16x2', 'state'),
    R('mlp_ode_split2_h256_n4_t1', 'top', 16, 16, (256, 255, 129, 255), 'silu', 'bf16x2', 'hutch'),
    R('mlp_ode_split2_h256_n4_t1', 'bottom', 1, 0, (129, 128, 127, 126), 'silu', 'bf16x2', 'hutch'),
    R('mlp_ode_split2_h256_n4_t2', 'top', 16, 16, (256, 255, 129, 255), 'silu', 'bf16x2', 'exact'),
    R('mlp_ode_split2_h256_n4_t2', 'bottom', 1, 0, (129, 128, 127, 126), 'silu', 'bf16x2', 'exact'),
    R('mlp_ode_split2_h256_d2_n1_t0', 'top', 32, 16, (256,), 'silu', 'bf16x2', 'state'),
    R('mlp_ode_split2_h256_d2_n1_t0', 'bottom', 17, 0, (1,), 'silu', 'bf16x2', 'state'),
    R('mlp_ode_split2_h256_d2_n2_t0', 'top', 32, 16, (256, 255), 'silu', 'bf16x2', 'state'),
    R('mlp_ode_split2_h256_d2_n2_t0', 'bottom', 17, 0, (1, 1), 'silu', 'bf16x2', 'state'),
    R('mlp_ode_split2_h256_d2_n3_t0', 'top', 32, 16, (256, 255, 129), 'silu', 'bf16x2', 'state'),
    R('mlp_ode_split2_h256_d2_n3_t0', 'bottom', 17, 0, (1, 1, 1), 'silu', 'bf16x2', 'state'),
    R('mlp_ode_split2_h256_d2_n4_t0', 'top', 32, 16, (256, 255, 129, 255), 'silu', 'bf16x2', 'state'),
    R('mlp_ode_split2_h256_d2_n4_t0', 'bottom', 17, 0, (1, 1, 1, 1), 'silu', 'bf16x2', 'state'),
    R('mlp_ode_split2_h128_n1_t0', 'top', 16, 16, (128,), 'silu', 'bf16x2', 'state'),
    R('mlp_ode_split2_h128_n1_t0', 'bottom', 1, 0, (1,), 'silu', 'bf16x2', 'state'),
    R('mlp_ode_split2_h128_n1_t1', 'top', 16, 16, (128,), 'silu', 'bf16x2', 'hutch'),
    R('mlp_ode_split2_h128_n1_t1', 'bottom', 1, 0, (1,), 'silu', 'bf16x2', 'hutch'),
    R('mlp_ode_split2_h128_n1_t2', 'top', 16, 16, (128,), 'silu', 'bf16x2', 'exact'),
    R('mlp_ode_split2_h128_n1_t2', 'bottom', 1, 0, (1,), 'silu', 'bf16x2', 'exact'),
    R('mlp_ode_split2_h128_n2_t0', 'top', 16, 16, (128, 127), 'silu', 'bf16x2', 'state'),
    R('mlp_ode_split2_h128_n2_t0', 'bottom', 1, 0, (1, 1), 'silu', 'bf16x2', 'state'),
    R('mlp_ode_split2_h128_n2_t1', 'top', 16, 16, (128, 127), 'silu', 'bf16x2', 'hutch'),
    R('mlp_ode_split2_h128_n2_t1', 'bottom', 1, 0, (1, 1), 'silu', 'bf16x2', 'hutch'),
    R('mlp_ode_split2_h128_n2_t2', 'top', 16, 16, (128, 127), 'silu', 'bf16x2', 'exact'),
    R('mlp_ode_split2_h128_n2_t2', 'bottom', 1, 0, (1, 1), 'silu', 'bf16x2', 'exact'),
    R('mlp_ode_split2_h128_n3_t0', 'top', 16, 16, (128, 127, 65), 'silu', 'bf16x2', 'state'),
    R('mlp_ode_split2_h128_n3_t0', 'bottom', 1, 0, (1, 1, 1), 'silu', 'bf16x2', 'state'),
    R('mlp_ode_split2_h128_n3_t1', 'top', 16, 16, (128, 127, 65), 'silu', 'bf16x2', 'hutch'),
    R('mlp_ode_split2_h128_n3_t1', 'bottom', 1, 0, (1, 1, 1), 'silu', 'bf16x2', 'hutch'),
    R('mlp_ode_split2_h128_n3_t2', 'top', 16, 16, (128, 127, 65), 'silu', 'bf16x2', 'exact'),
    R('mlp_ode_split2_h128_n3_t2', 'bottom', 1, 0, (1, 1, 1), 'silu', 'bf16x2', 'exact'),
    R('mlp_ode_split2_h128_n4_t0', 'top', 16, 16, (128, 127, 65, 127), 'silu', 'bf16x2', 'state'),
    R('mlp_ode_split2_h128_n4_t0', 'bottom', 1, 0, (1, 1, 1, 1), 'silu', 'bf16x2', 'state'),
    R('mlp_ode_split2_h128_n4_t1', 'top', 16, 16, (128, 127, 65, 127), 'silu', 'bf16x2', 'hutch'),
    R('mlp_ode_split2_h128_n4_t1', 'bottom', 1, 0, (1, 1, 1, 1), 'silu', 'bf16x2', 'hutch'),
    R('mlp_ode_split2_h128_n4_t2', 'top', 16, 16, (128, 127, 65, 127), 'silu', 'bf16x2', 'exact'),
    R('mlp_ode_split2_h128_n4_t2', 'bottom', 1, 0, (1, 1, 1, 1), 'silu', 'bf16x2', 'exact'),
]

# FF_ACT_* codes (include/flowfusion_amd.h) and the torch modules the rows run with: parameters that reach every branch
# -- a negative slope, an ELU alpha other than 1, a softplus beta and a threshold that pre-activations of these networks
# cross (beta * x > 3 at |x| > 1.5)
ACT_CODES = {"silu": 0, "tanh": 1, "sigmoid": 2, "relu": 3, "leaky_relu": 4, "elu": 5, "softplus": 6, "gelu": 7,
             "gelu_tanh": 8}


def act_module(name):
    return {"silu": lambda: torch.nn.SiLU(), "tanh": lambda: torch.nn.Tanh(), "sigmoid": lambda: torch.nn.Sigmoid(),
            "relu": lambda: torch.nn.ReLU(), "leaky_relu": lambda: torch.nn.LeakyReLU(0.2),
            "elu": lambda: torch.nn.ELU(0.7), "softplus": lambda: torch.nn.Softplus(beta=2.0, threshold=3.0),
            "gelu": lambda: torch.nn.GELU(), "gelu_tanh": lambda: torch.nn.GELU(approximate="tanh")}[name]()


def plan_modes(row):
    """FF_MODE_* values a row must plan to its instance under."""
    from flowfusion_amd import _native as N
    return {"state": [N.MODE_STATE], "tangent": [N.MODE_HUTCH, N.MODE_EXACT], "hutch": [N.MODE_HUTCH],
            "exact": [N.MODE_EXACT]}[row.mode]


def plan_row(row, mode, D=None, C=None, units=None):
    """The planner's pick for a row (or a shape next to it): kernel name, or None when no instance holds the shape."""
    from flowfusion_amd import _native as N
    from flowfusion_amd.fused import activation_spec
    try:
        p = N.make_plan(row.D if D is None else D, row.C if C is None else C, list(row.units if units is None else units),
                        mode, activation_spec(act_module(row.act)), N.PRECISIONS[row.prec])
    except NotImplementedError:
        return None
    return N.kernel_name(p)


def registry():
    """{kernel name: (family, has one-wavefront kernel, has cooperative twin, tangents, waves per SIMD)} as build.py declares
    it: family "f32" / "wide" / "split"; split tangents 0 / 1 / 2 (state / Hutchinson / exact trace)."""
    from flowfusion_amd import build as B
    out = {}
    for i in B.INSTANCES:
        out[B._inst_name(*i)] = ("f32", True, B._has_coop(i[1], i[7]), i[4], i[5])
    for i in B.WIDE_INSTANCES:
        out[B._wide_name(*i)] = ("wide", False, True, i[4], 1)
    for i in B.SPLIT_INSTANCES:
        out[B._split_name(*i)] = ("split", True, False, i[1], 1)
    return out


ONE_WAVE, TWIN, TAIL = "one_wave", "twin", "one_wave+twin"


def launch_kinds(entry):
    """The launch kinds an instance serves: its one-wavefront kernel (FF_COOP=0), its cooperative twin (FF_COOP=1) and, with
    both, the one-wavefront kernel with the leftover tiles on the twin (a batch just past whole rounds of the chip)."""
    family, one, coop = entry[:3]
    kinds = []
    if one:
        kinds.append(ONE_WAVE)
    if coop:
        kinds.append(TWIN)
    if one and coop:
        kinds.append(TAIL)
    return kinds


def solve_modes(entry, kind):
    """What the GPU test runs on an instance in a launch kind: fixed-grid state solve and Euler-Maruyama on state-only
    instances; Hutchinson and exact-trace forward solves and (f32; the Jacobian output runs no tail split) the Jacobian
    output on divergence-capable ones."""
    family, t = entry[0], entry[3]
    if family == "split":
        return [["rk4", "em"], ["hutch"], ["exact"]][t]
    if not t:
        return ["rk4", "em"]
    return ["hutch", "exact"] + ([] if kind == TAIL else ["jac"])


def chip_tiles(entry):
    """Tiles the chip runs at once on the one-wavefront kernel (1024 SIMDs x waves per SIMD): a launch of more tiles than
    this and a few leftover ones is the one that hands the leftovers to the twin."""
    return 1024 * entry[4]


def expected_coverage():
    """{(kernel name, launch kind, mode)} every instance must pass on the GPU."""
    return {(name, kind, mode) for name, e in registry().items() for kind in launch_kinds(e) for mode in solve_modes(e, kind)}
