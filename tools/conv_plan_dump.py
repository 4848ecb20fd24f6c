#!/usr/bin/env python3
"""The answers of the forward / data-gradient plan queries over a grid of shapes and hook settings, one text line per (hooks, descriptor): host logic only, no GPU.

    SEGLAND_LIB_PATH=/path/to/libsegland_a.so python tools/conv_plan_dump.py a.txt
    SEGLAND_LIB_PATH=/path/to/libsegland_b.so python tools/conv_plan_dump.py b.txt && diff a.txt b.txt

A line: hooks dtype B H W Cin Cout C1 k stride pad dil | sl_conv2d_tile_config_ex for every forward epilogue of FWD_EPI | the same for every data-gradient epilogue of
DGRAD_EPI | sl_conv2d_stat_rows, sl_conv2d_bwd_data_bnstat_rows, sl_conv2d_bwd_data_addend_bnstat_rows, sl_conv2d_bwd_data_addend_half_ok,
sl_conv2d_affine_fwd_workspace.  Two builds of the library dispatch the same way when their dumps are equal (profiles/ab_dgrad_plan.txt)."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from segland_amd import _lib  # noqa: E402

STATS, AFFINE, ADDEND, BITS, GATE, SPLITK, GELU = 1, 2, 4, 8, 16, 32, 64      # SL_EPI_* of include/segland_hip.h
FWD_EPI = (0, STATS, AFFINE, AFFINE | ADDEND, AFFINE | SPLITK, AFFINE | ADDEND | SPLITK)
DGRAD_EPI = (0, STATS, ADDEND, ADDEND | STATS, ADDEND | BITS, GATE, GATE | ADDEND, GELU)
# rows B * H * W on both sides of 32 (the <= 32-row kernel), of 256 x 96 = 24 576 (256-row tiles) and of 65 536 (pixel-stationary and 64 -> 64 3x3 kernels)
BATCHES = (1, 2, 3, 6, 8, 16)
MAPS = ((4, 8), (8, 8), (16, 16), (30, 30), (32, 32), (33, 31), (40, 52), (64, 64), (63, 65), (128, 128), (256, 256))
CHANNELS = (64, 128, 192, 256, 384, 512, 768, 1024, 2048)
WINDOWS = ((1, 1, 0, 1), (1, 2, 0, 1), (3, 1, 1, 1), (3, 1, 2, 2), (3, 1, 4, 4), (3, 2, 1, 1), (7, 2, 3, 1))      # k, stride, pad, dilation
HOOKS = (('default', None, 0), ('affine0', 'sl_debug_conv_affine', 0), ('p9off', 'sl_debug_conv_p9', 0), ('p8k1off', 'sl_debug_conv_p8_k1', 0),
         ('ring192off', 'sl_debug_conv_ring192', 0), ('ringn64off', 'sl_debug_conv_ringn64', 0), ('rowsoff', 'sl_debug_conv_rows_small', 0),
         ('parityoff', 'sl_debug_conv_parity', 0), ('smallk0', 'sl_debug_ring_small_k', 0), ('ring64off', 'sl_debug_ring64_max_tiles', 0))


def descriptors():
    for dtype in (_lib.SL_BF16, _lib.SL_F32):
        for B in BATCHES:
            for H, W in MAPS:
                for cin in CHANNELS:
                    for cout in CHANNELS:
                        for k, stride, pad, dil in WINDOWS:
                            Ho = (H + 2 * pad - dil * (k - 1) - 1) // stride + 1
                            Wo = (W + 2 * pad - dil * (k - 1) - 1) // stride + 1
                            if Ho <= 0 or Wo <= 0:
                                continue
                            for c1 in (cin, cin // 2):
                                if c1 % 64 == 0:
                                    yield _lib.SlConvDesc(dtype, B, H, W, cin, cout, k, k, stride, pad, dil, Ho, Wo, c1)


def main():
    L = _lib.lib()
    cfg = L.sl_conv2d_tile_config_ex
    n = 0
    with open(sys.argv[1], 'w') as f:
        for tag, hook, value in HOOKS:
            L.sl_debug_reset()
            if hook:
                getattr(L, hook)(value)
            for d in descriptors():
                r = C.byref(d)
                f.write('%s %s | %s | %s | %d %d %d %d %d\n' % (
                    tag, ' '.join(str(getattr(d, name)) for name, _ in d._fields_), ' '.join(str(cfg(r, 0, e)) for e in FWD_EPI), ' '.join(str(cfg(r, 1, e)) for e in DGRAD_EPI),
                    L.sl_conv2d_stat_rows(r), L.sl_conv2d_bwd_data_bnstat_rows(r), L.sl_conv2d_bwd_data_addend_bnstat_rows(r), L.sl_conv2d_bwd_data_addend_half_ok(r),
                    L.sl_conv2d_affine_fwd_workspace(r)))
                n += 1
        L.sl_debug_reset()
    print('%d lines (%d hook settings x %d descriptors) -> %s' % (n, len(HOOKS), n // len(HOOKS), sys.argv[1]))


if __name__ == '__main__':
    main()
