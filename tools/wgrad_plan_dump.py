#!/usr/bin/env python3
"""The answers of the four weight-gradient plan queries over a grid of shapes and hook settings, one text line per (hooks, descriptor): host logic only, no GPU.

    SEGLAND_LIB_PATH=/path/to/libsegland_a.so python tools/wgrad_plan_dump.py a.txt
    SEGLAND_LIB_PATH=/path/to/libsegland_b.so python tools/wgrad_plan_dump.py b.txt && diff a.txt b.txt

A line: hooks dtype B H W Cin Cout C1 k stride pad dil | sl_conv2d_wgrad_config, sl_conv2d_bwd_weight_workspace, sl_conv2d_bwd_weight_bias_rows at (0, 0) and at
(Cout - 32, Cin - 32), the return value and the eight outputs of sl_debug_wgrad3_plan.  Two builds of the library dispatch the same way when their dumps are equal
(profiles/ab_wgrad_plan.txt)."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from segland_amd import _lib  # noqa: E402

BATCHES = (1, 2, 8, 16)
MAPS = ((8, 8), (16, 16), (30, 30), (32, 32), (40, 52), (64, 64), (128, 128), (256, 256))
CHANNELS = (64, 128, 192, 256, 384, 512, 768, 1024, 2048)
WINDOWS = ((1, 1, 0, 1), (1, 2, 0, 1), (3, 1, 1, 1), (3, 1, 2, 2), (3, 1, 4, 4), (3, 2, 1, 1), (7, 2, 3, 1))      # k, stride, pad, dilation
HOOKS = (('default', None, 0), ('tr0', 'sl_debug_wgrad_tr', 0), ('w3off', 'sl_debug_wgrad3', 0), ('bias0', 'sl_debug_wgrad_bias', 0), ('pair4096', 'sl_debug_wgrad_pair_min', 4096))


def descriptors():
    for dtype in (_lib.SL_BF16, _lib.SL_F32):
        for B in BATCHES:
            for H, W in MAPS:
                for cin in CHANNELS:
                    for cout in CHANNELS:
                        for k, stride, pad, dil in WINDOWS:
                            Ho = (H + 2 * pad - dil * (k - 1) - 1) // stride + 1
                            Wo = (W + 2 * pad - dil * (k - 1) - 1) // stride + 1
                            for c1 in (cin, cin // 2):
                                if c1 % 64 == 0:
                                    yield _lib.SlConvDesc(dtype, B, H, W, cin, cout, k, k, stride, pad, dil, Ho, Wo, c1)


def main():
    L = _lib.lib()
    out8 = (C.c_int * 8)()
    n = 0
    with open(sys.argv[1], 'w') as f:
        for tag, hook, value in HOOKS:
            L.sl_debug_reset()
            if hook:
                getattr(L, hook)(value)
            for d in descriptors():
                r = C.byref(d)
                served = L.sl_debug_wgrad3_plan(r, out8)
                f.write('%s %s | %d %d %d %d %d %s\n' % (
                    tag, ' '.join(str(getattr(d, name)) for name, _ in d._fields_), L.sl_conv2d_wgrad_config(r), L.sl_conv2d_bwd_weight_workspace(r),
                    L.sl_conv2d_bwd_weight_bias_rows(r, 0, 0), L.sl_conv2d_bwd_weight_bias_rows(r, d.Cout - 32, d.Cin - 32), served, ' '.join(map(str, out8))))
                n += 1
        L.sl_debug_reset()
    print('%d lines (%d hook settings x %d descriptors) -> %s' % (n, len(HOOKS), n // len(HOOKS), sys.argv[1]))


if __name__ == '__main__':
    main()
