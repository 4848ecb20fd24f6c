"""Exact-integer convolution cases: the route table, the operand generator and the float64 reference shared by test_conv_exact_cpu.py and test_conv_exact_gpu.py
(a plain module: no fixtures, no hooks).

Method.  With operands in {-1, 0, 1} every product and every partial sum of a convolution is an integer far below 2^24, so the fp32 accumulator of ANY correct
kernel holds the exact result whatever its summation order, tile shape, K split or tap order; the expected output is the float64 reference rounded once to the
tensor type, bit for bit.  A missing, duplicated or misplaced term anywhere fails.  The bounds that make this true (integral values, magnitudes below 2^24, outputs of
at most 256 wherever a kernel consumes its own output again -- statistics, gated statistics, the dual form -- so that reducing the accumulator or the stored bf16 value
is the same number) are conditions on the INPUTS: check_bounds() asserts them on the reference alone, before anything is launched.

One table entry per launch: Case(code, dtype, B, H, W, cin, cout, k, stride, pad, dil, mode, epi, entry, hooks, wide, c1).
  code   what sl_conv2d_tile_config_ex (mode 0 forward / 1 data gradient) or sl_conv2d_wgrad_config (mode 2) must answer for the descriptor, with `hooks` set
  epi    the SL_EPI_* bits of the query
  entry  which segland_amd.ops call runs (ENTRIES below)
  hooks  ((sl_debug_* name, value), ...): a bit-identical alternative route, or the only way to a code
  wide   the second operand set (activations in -3..3, weights in -2..2): |y| passes 256 (asserted), the store phase's round-to-nearest-even is exercised; only y is
         compared.  2: the same ranges drawn with more weight on the ends, for a reduction too short (K = 256) to pass 256 with the uniform draw
  c1     channels of the first source of a virtual concat (weight gradients), None: one source
(B, H, W, cin, cout) are the CONV's: a data gradient reduces over cout and writes cin columns.  Shapes are the smallest that reach the code under the thresholds of
csrc/conv_gemm.hip (MIN_TILES256 = 96: 256-row tiles from 24 576 rows; RING128_MIN = 16: ring tiles from 2 048 rows; 65 536 rows for the pixel-stationary and the
64 -> 64 3x3 kernels; 32 768 for the 3x3 patch kernel; 24 576 rows per parity plane)."""
import collections
import functools
import os
import re

import torch
import torch.nn.functional as F

from oracle import formula as fm

STATS, AFFINE, ADDEND, BITS, GATE, SPLITK = 1, 2, 4, 8, 16, 32
BF, F32 = torch.bfloat16, torch.float32
TWO24 = float(1 << 24)

Case = collections.namedtuple('Case', 'code dtype B H W cin cout k stride pad dil mode epi entry hooks wide c1')

# entry -> (mode, epi bits of the query)
ENTRIES = {
    'fwd': (0, 0), 'fwd_stats': (0, STATS), 'affine': (0, AFFINE), 'affine_res': (0, AFFINE), 'affine_splitk': (0, AFFINE | SPLITK),
    'bwd': (1, 0), 'bwd_addend': (1, ADDEND), 'bwd_addend_bits': (1, ADDEND | BITS), 'bwd_bnstat': (1, GATE), 'bwd_addend_bnstat': (1, GATE | ADDEND),
    'bwd_addend_half': (1, ADDEND), 'bwd_addend_half_stats': (1, GATE | ADDEND), 'bwd_addend_bnstat2': (1, GATE | ADDEND),
    'wgrad': (2, 0), 'wgrad_off': (2, 0), 'wgrad_clip': (2, 0), 'wgrad_bias': (2, 0),
}
TILE16 = (7016016, 8256256, 18256256)          # partial row = one 16 x 16-pixel tile (b, y / 16, x / 16); every other code: BM consecutive rows
PARITY_HW = 64                                 # the parity-plane cases (stride-2 3x3 data gradients on 64 x 64 inputs)


def case_id(c):
    s = '%d-%s-%dx%dx%d-%dto%d-k%ds%dd%d-%s' % (c.code, 'bf16' if c.dtype == BF else 'f32', c.B, c.H, c.W, c.cin, c.cout, c.k, c.stride, c.dil, c.entry)
    if c.c1:
        s += '-x2'
    if c.wide:
        s += '-wide' if c.wide is True else '-wide%d' % c.wide
    for n, v in c.hooks:
        s += '-%s%d' % (n.replace('sl_debug_', ''), v)
    return s


def is_parity(c):
    return c.mode == 1 and c.stride == 2 and c.k == 3


def _case(code, dtype, shape, cin, cout, k, stride, dil, entry, hooks=(), wide=False, c1=None, pad=None):
    mode, epi = ENTRIES[entry]
    B, H, W = shape
    return Case(code, dtype, B, H, W, cin, cout, k, stride, dil * (k // 2) if pad is None else pad, dil, mode, epi, entry, tuple(hooks), wide, c1)


def _table():
    T = []

    def add(code, dtype, shape, cin, cout, entries, k=1, stride=1, dil=1, hooks=(), wide=False, c1=None):
        for e in ([entries] if isinstance(entries, str) else entries):
            T.append(_case(code, dtype, shape, cin, cout, k, stride, dil, e, hooks, wide, c1))
    S, R = (2, 32, 32), (1, 36, 60)                      # 2 048 rows: the ring tiles' first shape; 2 160 rows: a ragged last row block
    L, LR = (6, 64, 64), (6, 64, 65)                     # 24 576 rows: the 256-row tiles' first shape; 24 960 rows: ragged
    # ---- two-stage kernel, 128-row blocks (below 2 048 rows); 144 rows: one full and one ragged block
    add(2128064, BF, (1, 12, 12), 64, 64, ['fwd_stats', 'bwd'])
    add(2128064, BF, (1, 12, 12), 64, 64, 'fwd_stats', k=3)
    add(2128064, BF, (1, 12, 12), 128, 64, 'fwd_stats', k=3, wide=True)
    add(2128128, BF, (1, 12, 12), 64, 128, 'fwd_stats')
    add(2128128, BF, (1, 12, 12), 64, 128, 'fwd_stats', k=3)
    add(2128128, BF, (1, 12, 12), 128, 128, 'fwd_stats', k=3, wide=True)
    add(2128128, BF, (1, 12, 12), 128, 64, ['bwd', 'bwd_addend', 'bwd_addend_bits'])
    add(2128128, BF, (1, 16, 16), 128, 64, 'bwd_bnstat')                                  # 256 rows: full blocks, the gated store phase
    # ---- ring kernel, 128 x 128 tiles (statistics or a gate keep a launch off the 64-row tiles)
    add(4128128, BF, S, 64, 128, 'fwd_stats')
    add(4128128, BF, R, 64, 128, 'fwd_stats')
    add(4128128, BF, S, 64, 128, 'fwd_stats', k=3)
    add(4128128, BF, S, 64, 128, 'fwd_stats', k=3, wide=True)
    add(4128128, BF, S, 128, 64, 'bwd_bnstat')
    # ---- ring kernel, 64 x 128 tiles: the same shapes without statistics; with the hook at 0 they are 128 x 128 tiles again
    add(4064128, BF, S, 64, 128, ['fwd', 'affine', 'affine_res'])
    add(4064128, BF, R, 64, 128, 'affine')
    add(4064128, BF, S, 64, 128, 'fwd', k=3)
    add(4064128, BF, S, 64, 128, 'fwd', k=3, wide=True)
    add(4064128, BF, S, 128, 64, ['bwd', 'bwd_addend', 'bwd_addend_bits'])
    add(4064128, BF, S, 64, 128, 'affine', hooks=[('sl_debug_conv_affine', 0)])
    add(4128128, BF, S, 64, 128, 'affine', hooks=[('sl_debug_ring64_max_tiles', 0)])
    add(4128128, BF, S, 128, 64, 'bwd', hooks=[('sl_debug_ring64_max_tiles', 0)])
    # ---- ring kernel, 128 x 64 tiles (64-column inference layers) and 128 x 192 tiles
    add(4128064, BF, S, 128, 64, ['fwd', 'affine'])
    add(4128064, BF, R, 128, 64, 'affine')
    add(4128064, BF, S, 64, 128, 'bwd')
    add(4128064, BF, S, 128, 64, 'affine_res', k=3)
    add(4128064, BF, S, 128, 64, 'fwd', k=3, wide=True)
    add(4128192, BF, S, 64, 192, ['fwd_stats', 'affine'])
    add(4128192, BF, R, 64, 192, 'fwd_stats')
    add(4128192, BF, S, 192, 64, ['bwd', 'bwd_addend'])
    add(4128192, BF, S, 64, 192, 'fwd', k=3, wide=True)
    # ---- many rows, short reduction: 128 x 128 ring tiles by the small-K rule
    add(4128128, BF, L, 128, 384, 'fwd')
    # ---- 256-row tiles
    add(2256064, BF, L, 64, 64, ['fwd_stats', 'bwd_bnstat'])
    add(2256064, BF, LR, 64, 64, 'fwd_stats')
    add(2256064, BF, L, 64, 64, 'fwd_stats', k=3)
    add(2256064, BF, L, 64, 64, 'fwd_stats', k=3, wide=True)
    add(4256128, BF, L, 256, 128, 'fwd_stats')
    add(4256128, BF, LR, 256, 128, 'fwd_stats')
    add(4256128, BF, L, 64, 128, 'fwd_stats', k=3)
    add(4256128, BF, L, 64, 128, 'fwd_stats', k=3, wide=True)
    add(4256128, BF, L, 128, 256, 'bwd_bnstat')
    add(4256256, BF, LR, 256, 64, 'bwd', stride=2)                                        # 24 960 rows: ragged last block
    add(4256256, BF, L, 256, 64, ['bwd', 'bwd_addend'], stride=2)                         # a stride-2 1x1 data gradient has no affine row map: not the half-tile kernel
    # ---- half-tile kernel
    add(5256256, BF, L, 64, 256, ['fwd_stats', 'affine_res'])
    add(5256256, BF, L, 64, 256, 'fwd_stats', hooks=[('sl_debug_conv_p8_k1', 0)])
    add(5256256, BF, LR, 64, 256, 'fwd_stats')
    add(5256256, BF, (7, 60, 64), 64, 256, 'fwd_stats', k=3)                              # H = 60: the patch kernel refuses the shape
    add(5256256, BF, (7, 60, 64), 64, 256, 'fwd_stats', k=3, wide=True)
    add(5256256, BF, L, 256, 64, ['bwd', 'bwd_addend_bits', 'bwd_bnstat'])
    # ---- 3x3 patch kernel, d = 1, 2, 4, forward and data gradient (flipped window), lean and generic K-tile loop
    P = (8, 64, 64)
    for d in (1, 2, 4):
        add(8256256, BF, P, 64, 256, 'fwd_stats', k=3, dil=d)
        add(8256256, BF, P, 64, 256, 'fwd_stats', k=3, dil=d, hooks=[('sl_debug_conv_p9_lean', 0)])
        add(8256256, BF, P, 256, 64, 'bwd', k=3, dil=d)
        add(8256256, BF, P, 256, 64, 'bwd', k=3, dil=d, hooks=[('sl_debug_conv_p9_lean', 0)])
    add(8256256, BF, P, 64, 256, 'affine_res', k=3, dil=4)
    add(8256256, BF, P, 64, 256, 'fwd_stats', k=3, dil=1, wide=True)
    add(8256256, BF, P, 256, 64, 'bwd_addend_bits', k=3, dil=1)
    add(8256256, BF, P, 256, 64, 'bwd_bnstat', k=3, dil=2)
    # ---- the same kernel split along K through the workspace (four parts of four 64-channel chunks)
    for d in (1, 2):
        add(18256256, BF, (1, 16, 16), 1024, 256, 'affine_splitk', k=3, dil=d)
        add(18256256, BF, (1, 16, 16), 1024, 256, 'affine_splitk', k=3, dil=d, hooks=[('sl_debug_conv_p9_lean', 0)])
    # (no wide case: split-K is planned for the affine forms only, and every affine epilogue is applied to the accumulator ALREADY rounded to the tensor type --
    # conv_splitk_finish_kernel, as the tile kernels' staging does -- so past 256 the result is rounded twice by design; the wide set is for plain stores)
    # ---- 64 -> 64 3x3 patch kernel: full and ragged 16 x 16 tiles
    for shape in ((16, 64, 64), (17, 60, 68)):
        add(7016016, BF, shape, 64, 64, ['fwd_stats', 'bwd', 'bwd_bnstat'], k=3)
    add(7016016, BF, (16, 64, 64), 64, 64, 'fwd_stats', k=3, wide=True)
    # ---- pixel-stationary kernel, K = 64 / 128 / 256
    Q = (16, 64, 64)
    for K in (64, 128, 256):
        add(6256064, BF, Q, K, 256, 'fwd_stats')
        add(6256064, BF, Q, 256, K, ['bwd', 'bwd_addend_bnstat'])
    add(6256064, BF, Q, 256, 64, 'fwd_stats')
    add(6256064, BF, Q, 256, 64, ['bwd_addend', 'bwd_addend_bits', 'bwd_addend_half', 'bwd_addend_half_stats', 'bwd_addend_bnstat2'])
    add(6256064, BF, Q, 128, 128, 'bwd_addend_bits')
    add(6256064, BF, Q, 256, 256, 'fwd_stats', wide=2)                                    # K = 256 is too short for the uniform draw to pass 256: edge-weighted draw
    # ---- <= 32 rows
    add(3032032, BF, (3, 1, 5), 512, 512, 'fwd')
    add(3032032, BF, (3, 1, 5), 512, 512, 'fwd', wide=True)
    add(3032032, BF, (3, 1, 5), 512, 512, 'bwd')
    # ---- stride-2 3x3 data gradients as four parity planes of the ring kernel (24 576 rows per plane)
    add(4256128, BF, (24, PARITY_HW, PARITY_HW), 128, 128, ['bwd', 'bwd_addend', 'bwd_bnstat'], k=3, stride=2)
    add(4256256, BF, (24, PARITY_HW, PARITY_HW), 256, 128, ['bwd', 'bwd_bnstat'], k=3, stride=2)
    add(4256256, BF, (24, PARITY_HW, PARITY_HW), 256, 128, 'bwd', k=3, stride=2, wide=True)      # bf16 reaches the code by data gradients only: its plain store past 256
    # ---- fp32: the six ring / two-stage codes at the same smallest shapes, Cin a multiple of 32
    add(2128064, F32, (1, 12, 12), 32, 64, 'fwd_stats')
    add(2128064, F32, (1, 12, 12), 32, 64, 'fwd_stats', k=3)
    add(2128128, F32, (1, 12, 12), 32, 128, 'fwd_stats')
    add(2128128, F32, (1, 12, 12), 128, 32, ['bwd', 'bwd_addend_bits'])
    add(4128128, F32, S, 32, 128, ['fwd_stats', 'affine_res'])
    add(4128128, F32, R, 32, 128, 'fwd_stats')
    add(4128128, F32, S, 32, 128, 'fwd_stats', k=3)
    add(4128128, F32, S, 128, 32, ['bwd', 'bwd_bnstat'])
    add(2256064, F32, L, 32, 64, 'fwd_stats')
    add(2256064, F32, LR, 32, 64, 'fwd_stats')
    add(4256128, F32, L, 32, 128, 'fwd_stats')
    add(4256128, F32, LR, 32, 128, 'fwd_stats')
    add(4256256, F32, L, 32, 256, 'fwd_stats')
    add(4256256, F32, LR, 32, 256, 'fwd_stats')
    add(4256256, F32, L, 32, 256, 'fwd_stats', k=3)
    # ---- weight gradients: one shape per answer of sl_conv2d_wgrad_config, each with the call forms plan_wgrad admits on that route: virtual concat (c1), the wider-dw
    # window, the clipped call, the bias rows under both sl_debug_wgrad_bias settings where the hook moves them (glds tiles other than 256 x 256, 1x1).
    # Refused by the plan, so absent: a second source on routes 1, 2 and on pixel pairs (all need c2 == 0: the call plans another tile); a dw window or a clip on route 1
    # (c64k3_eligible / `full`: the call runs as pixel pairs); a clip on route 3 (`full`: the call runs on the 128 x 128 tiles -- the case below names that plan with the hook
    # that gives it, sl_debug_wgrad3(0), set for the query AND the launch).
    W_ALL = ['wgrad', 'wgrad_off', 'wgrad_clip', 'wgrad_bias']
    NO_KB = [('sl_debug_wgrad_bias', 0)]
    add(1, BF, (16, 64, 64), 64, 64, ['wgrad', 'wgrad_bias'], k=3)                        # 64 -> 64 3x3 kernel
    add(1, BF, (17, 60, 68), 64, 64, 'wgrad', k=3)
    add(2, BF, (16, 64, 64), 64, 256, W_ALL)                                              # 64-channel 1x1 kernel (its flat reduce clips)
    add(2, BF, (16, 64, 64), 64, 64, 'wgrad')
    add(3, BF, (2, 64, 64), 128, 128, ['wgrad', 'wgrad_off', 'wgrad_bias'], k=3)          # nine-tap kernel
    add(3, BF, (2, 64, 64), 128, 128, 'wgrad', k=3, dil=2)
    add(3, BF, (2, 64, 64), 128, 128, 'wgrad', k=3, c1=64)
    add(10128128, BF, (2, 64, 64), 128, 128, 'wgrad_clip', k=3, hooks=[('sl_debug_wgrad3', 0)])
    add(10128128, BF, (1, 32, 32), 128, 384, W_ALL)
    add(10128128, BF, (1, 32, 32), 128, 384, ['wgrad', 'wgrad_bias'], hooks=[('sl_debug_wgrad_tr', 0)])
    add(10128128, BF, (1, 32, 32), 128, 384, 'wgrad_bias', hooks=NO_KB)
    add(10128128, BF, (1, 32, 32), 256, 384, 'wgrad', c1=128)
    add(10128128, BF, (2, 16, 16), 128, 128, 'wgrad', k=3, stride=2)                      # per-tap slabs
    add(10128256, BF, (1, 32, 32), 256, 128, W_ALL)
    add(10128256, BF, (1, 32, 32), 256, 128, 'wgrad_bias', hooks=NO_KB)
    add(10128256, BF, (1, 32, 32), 512, 128, 'wgrad', c1=256)
    add(10256128, BF, (1, 32, 32), 128, 256, W_ALL)
    add(10256128, BF, (1, 32, 32), 128, 256, 'wgrad_bias', hooks=NO_KB)
    add(10256128, BF, (1, 32, 32), 256, 256, 'wgrad', c1=128)
    add(10256256, BF, (1, 32, 32), 512, 768, W_ALL)                                       # (no bias instantiation: the hook changes nothing)
    add(10256256, BF, (1, 32, 32), 512, 768, 'wgrad', c1=256)
    add(10628128, BF, (1, 128, 128), 192, 192, W_ALL)                                     # pixel pairs
    add(10628128, BF, (1, 128, 128), 192, 192, 'wgrad_bias', hooks=NO_KB)
    add(10628128, BF, (2, 16, 16), 64, 64, 'wgrad', k=3)                                  # pixel pairs of a 3x3 layer
    add(20064064, BF, (1, 32, 32), 64, 64, W_ALL)                                         # register-staged kernel (bias always in the reduce launch)
    add(20064064, BF, (1, 32, 32), 64, 64, 'wgrad', hooks=[('sl_debug_wgrad_tr', 0)])
    add(20064064, BF, (1, 32, 32), 128, 64, 'wgrad', c1=64)
    add(20128064, BF, (1, 32, 32), 64, 128, W_ALL)
    add(20128064, BF, (1, 32, 32), 128, 128, 'wgrad', c1=64)
    add(20064128, BF, (1, 32, 32), 128, 64, W_ALL)
    add(20064128, BF, (1, 32, 32), 256, 64, 'wgrad', c1=128)
    add(20064064, F32, (1, 32, 32), 64, 64, W_ALL)
    add(20064064, F32, (1, 32, 32), 128, 64, 'wgrad', c1=64)
    add(10128128, F32, (1, 32, 32), 128, 128, W_ALL)
    add(10128128, F32, (1, 32, 32), 128, 128, 'wgrad_bias', hooks=NO_KB)
    add(10128128, F32, (1, 32, 32), 256, 128, 'wgrad', c1=128)
    return T


TABLE = _table()
IDS = [case_id(c) for c in TABLE]
assert len(set(IDS)) == len(IDS)


# ---------------------------------------------------------------------------------------------------- operands
def ints(tag, shape, density):
    """float64 tensor in {-1, 0, 1}: -1 and 1 with probability density / 2 each (oracle/formula.py's hash)."""
    n = 1
    for s in shape:
        n *= s
    u = fm.uniform01(tag, n)
    return ((u > 1.0 - density / 2).to(torch.float64) - (u < density / 2).to(torch.float64)).reshape(shape)


def span(tag, shape, r):
    """float64 integers uniform in [-r, r]."""
    n = 1
    for s in shape:
        n *= s
    return (torch.floor(fm.uniform01(tag, n) * (2 * r + 1)) - r).reshape(shape)


def pick_t(tag, shape, values):
    """float64 tensor drawn uniformly from the LIST `values` (repeats weight a value): the wide set's ranges with more mass at the ends."""
    n = 1
    for d in shape:
        n *= d
    return pick(tag, n, values).reshape(shape)


def pick(tag, n, values):
    v = torch.tensor(values, dtype=torch.float64)
    return v[torch.floor(fm.uniform01(tag, n) * len(values)).long()]


class Problem:
    """Operands and float64 references of one (shape, operand set), NCHW on the CPU; each piece is made once."""

    def __init__(self, key):
        self.key = key
        (self.B, self.H, self.W, self.cin, self.cout, self.k, self.stride, self.pad, self.dil, self.wide) = key
        self.tag = 'exact/%s' % (key,)
        f = lambda n: (n + 2 * self.pad - self.dil * (self.k - 1) - 1) // self.stride + 1
        self.Ho, self.Wo = f(self.H), f(self.W)
        self._c = {}

    def _get(self, name, make):
        if name not in self._c:
            self._c[name] = make()
        return self._c[name]

    def _dens(self):
        """(activations and gradients, weights).  Both reductions of the problem (forward over cin k^2, data gradient over cout k^2 terms) keep a variance of
        K * 0.5 * min(0.5, 4096 / K) <= 2048: sigma <= 45.3, and 256 is at least 5.6 sigma away (check_bounds asserts the bound itself on every reference)."""
        K = max(self.cin, self.cout) * self.k * self.k
        return 0.5, min(0.5, 4096.0 / K)

    def _act(self, name, shape):
        if self.wide == 2:
            return pick_t(self.tag + name, shape, (-3, -3, -2, -1, 0, 1, 2, 3, 3))
        return span(self.tag + name, shape, 3) if self.wide else ints(self.tag + name, shape, self._dens()[0])

    @property
    def x(self):
        return self._get('x', lambda: self._act('/x', (self.B, self.cin, self.H, self.W)))

    @property
    def w(self):
        shape = (self.cout, self.cin, self.k, self.k)
        if self.wide == 2:
            return self._get('w', lambda: pick_t(self.tag + '/w', shape, (-2, -2, -1, 0, 1, 2, 2)))
        return self._get('w', lambda: span(self.tag + '/w', shape, 2) if self.wide else ints(self.tag + '/w', shape, self._dens()[1]))

    @property
    def dy(self):
        return self._get('dy', lambda: self._act('/dy', (self.B, self.cout, self.Ho, self.Wo)))

    @property
    def y(self):
        return self._get('y', lambda: F.conv2d(self.x, self.w, None, self.stride, self.pad, self.dil))

    @property
    def dx(self):
        return self._get('dx', lambda: torch.nn.grad.conv2d_input((self.B, self.cin, self.H, self.W), self.w, self.dy, self.stride, self.pad, self.dil))

    @property
    def dw(self):
        return self._get('dw', lambda: torch.nn.grad.conv2d_weight(self.x, (self.cout, self.cin, self.k, self.k), self.dy, self.stride, self.pad, self.dil))

    def small(self, name, shape, density=0.5):
        """an addend / residual / gate source / BatchNorm input in {-1, 0, 1}, NCHW"""
        return self._get(name, lambda: ints(self.tag + '/' + name, shape, density))

    def vec(self, name, n, values):
        return self._get(name, lambda: pick(self.tag + '/' + name, n, values))


@functools.lru_cache(maxsize=2)
def _problem(key):
    return Problem(key)


def problem(c):
    return _problem((c.B, c.H, c.W, c.cin, c.cout, c.k, c.stride, c.pad, c.dil, c.wide))


SCALES, SHIFTS, INVSTDS = (0.5, 1.0, 2.0), tuple(float(v) for v in range(-4, 5)), (0.25, 0.5, 1.0)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def block_sums(v, c):
    """v: float64 [B, H, W, C] -> [partial rows, C], the sums over the rows each partial row of the case's plan covers; None for parity planes (totals only)."""
    if is_parity(c):
        return None
    B, H, W, C = v.shape
    if c.code in TILE16:
        Hp, Wp = (H + 15) // 16 * 16, (W + 15) // 16 * 16
        v = F.pad(v, (0, 0, 0, Wp - W, 0, Hp - H))
        return v.reshape(B, Hp // 16, 16, Wp // 16, 16, C).sum((2, 4)).reshape(-1, C)
    bm = (c.code // 1000) % 1000
    v = v.reshape(-1, C)
    rows = (v.shape[0] + bm - 1) // bm
    v = F.pad(v, (0, 0, 0, rows * bm - v.shape[0]))
    return v.reshape(rows, bm, C).sum(1)


def expected(c):
    """The float64 reference of the case, NHWC: dict with 'out' (the output tensor, or dw in OIHW), optionally 'stats' = list of [2][...] float64 tensors the partials
    are sums of (per element, NHWC: the test reduces them per block and in total), 'bias' (column sums of dy), and the auxiliary operands the launch needs (NHWC)."""
    p = problem(c)
    e = {}
    if c.mode == 2:
        e['out'] = p.dw
        if c.entry == 'wgrad_bias':
            e['bias'] = p.dy.sum((0, 2, 3))
        return e
    if c.mode == 0:
        y = nhwc(p.y)
        if c.entry in ('fwd', 'fwd_stats'):
            e['out'] = y
            if c.entry == 'fwd_stats' and not c.wide:
                e['stats'] = [(y, y * y)]
            return e
        e['scale'], e['shift'] = p.vec('scale', c.cout, SCALES), p.vec('shift', c.cout, SHIFTS)
        v = y
        if c.entry == 'affine_res':
            e['pre'], e['res'] = nhwc(p.small('pre', tuple(p.y.shape))), nhwc(p.small('res', tuple(p.y.shape)))
            v = v + e['pre']
        v = v * e['scale'] + e['shift']
        if c.entry == 'affine_res':
            v = v + e['res']
        e['out'] = torch.relu(v)
        return e
    dx = nhwc(p.dx)
    shape = (c.B, c.cin, c.H, c.W)
    if c.entry in ('bwd_addend', 'bwd_addend_bits', 'bwd_addend_bnstat', 'bwd_addend_bnstat2'):
        e['addend'] = nhwc(p.small('addend', shape))
    if c.entry in ('bwd_addend_half', 'bwd_addend_half_stats'):
        e['addend_half'] = nhwc(p.small('addend_half', (c.B, c.cin, c.H // 2, c.W // 2)))
        up = torch.zeros_like(dx)
        up[:, ::2, ::2] = e['addend_half']
        dx = dx + up
    if c.entry in ('bwd_addend', 'bwd_addend_bnstat', 'bwd_addend_bnstat2'):
        dx = dx + e['addend']
    if c.epi & (BITS | GATE):
        e['gate'] = nhwc(p.small('gate', shape))                                        # its ReLU bits (ops.bn_act(..., want_mask=True)) gate the launch
    if c.entry == 'bwd_addend_bits':
        dx = dx + e['addend'] * (e['gate'] > 0)
    if c.epi & GATE:
        dx = dx * (e['gate'] > 0)
        e['stats'] = []
        for s in ('', '2')[:2 if c.entry == 'bwd_addend_bnstat2' else 1]:
            e['bn_x' + s] = nhwc(p.small('bn_x' + s, shape))
            e['mean' + s], e['invstd' + s] = p.vec('mean' + s, c.cin, SHIFTS), p.vec('invstd' + s, c.cin, INVSTDS)
            e['stats'].append((dx, dx * ((e['bn_x' + s] - e['mean' + s]) * e['invstd' + s])))
    e['out'] = dx
    return e


def check_bounds(c, e):
    """The conditions that make the comparison exact, asserted on the reference alone.  -> dict of the reference's maximum magnitudes."""
    out = e['out']
    unit = 0.25 if c.entry.startswith('affine') else 1.0
    assert torch.equal(out, torch.round(out / unit) * unit), 'reference values are not multiples of %g' % unit
    mx = float(out.abs().max())
    assert mx < TWO24
    rec = {'max_out': mx}
    if c.wide:
        assert mx > 256, 'the wide operand set is there to pass 256'
        return rec
    if c.mode == 0:
        p = problem(c)
        assert float(p.y.abs().max()) <= 256, 'conv result beyond 256: bf16 would round before the epilogue consumers see it'
    if 'stats' in e:
        assert mx <= 256, 'an output that the kernel reduces again must be exact in bf16'
        worst = 0.0
        for a, b in e['stats']:
            for t in (a, b):
                assert torch.equal(t, torch.round(t * 4) / 4)
                blocks = block_sums(t.abs(), c)
                m = float((blocks if blocks is not None else t.abs().reshape(-1, t.shape[-1]).sum(0)).max())      # parity planes: the whole column bounds every partial
                worst = max(worst, m)
        assert 4 * worst < TWO24, 'a statistics partial (in units of 0.25) could pass 2^24'
        rec['max_partial'] = worst
    if c.mode == 2:
        p = problem(c)
        assert c.B * p.Ho * p.Wo < TWO24                                                  # the term count of a weight-gradient element bounds every slab sum
        if 'bias' in e:
            assert float(e['bias'].abs().max()) < TWO24
    return rec


def to_dtype(ref, dtype):
    """The expected tensor in its type: one round-to-nearest-even from the exact value (what f2bf of csrc/common.h does); exact for fp32."""
    return ref.to(torch.float32).to(dtype)


# ---------------------------------------------------------------------------------------------------- host queries
def desc(c):
    from segland_amd import _lib
    Ho = (c.H + 2 * c.pad - c.dil * (c.k - 1) - 1) // c.stride + 1
    Wo = (c.W + 2 * c.pad - c.dil * (c.k - 1) - 1) // c.stride + 1
    return _lib.SlConvDesc(_lib.SL_BF16 if c.dtype == BF else _lib.SL_F32, c.B, c.H, c.W, c.cin, c.cout, c.k, c.k, c.stride, c.pad, c.dil, Ho, Wo, c.c1 or c.cin)


def query(lib, c):
    """What the dispatch answers for the case's descriptor with the case's hooks set (host logic; the debug record is put back).  The call-level fields of a weight
    gradient (dw window, clip, bias) are not part of the descriptor: 'wgrad_off' / 'wgrad_clip' / 'wgrad_bias' entries carry the code of the plain call of their
    shape; where such a call leaves the route of the plain one, the table either omits it or names the plan it takes together with the hook that gives it."""
    import ctypes as C
    d = desc(c)
    lib.sl_debug_reset()
    for name, v in c.hooks:
        getattr(lib, name)(v)
    try:
        if c.mode == 2:
            return lib.sl_conv2d_wgrad_config(C.byref(d))
        return lib.sl_conv2d_tile_config_ex(C.byref(d), c.mode, c.epi)
    finally:
        lib.sl_debug_reset()


def _chain_body():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'segland_amd', 'csrc', 'conv_gemm.hip')).read()
    a = src.index('static Plan choose_kernel(')
    return re.sub(r'//[^\n]*', '', src[a:src.index('static long long stat_rows', a)])


def _literals(text):
    return sorted({int(m) for m in re.findall(r'(?<![\w.])(\d{7,8})(?![\w.])', text)})


def chain_codes():
    """The 7- and 8-digit literals choose_kernel (csrc/conv_gemm.hip) can return, read from the source."""
    return _literals(_chain_body())


def fp32_codes():
    """The ones an fp32 launch can reach: what is left of the function without its `if (dtype == SL_BF16) { ... }` blocks and its statements conditioned on bf16."""
    body = re.sub(r'\n  if \(dtype == SL_BF16\) \{.*?\n  \}', '\n', _chain_body(), flags=re.S)
    return _literals('\n'.join(l for l in body.split('\n') if 'SL_BF16' not in l))


def wgrad_codes():
    """The codes plan_wgrad (csrc/conv_wgrad.hip) can report: the special routes of enum WgradRoute and, for WG_TILES, every tile the launch switch instantiates."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'segland_amd', 'csrc', 'conv_wgrad.hip')).read()
    enum = re.search(r'enum WgradRoute \{([^}]*)\}', src).group(1)
    routes = {n.strip(): int(v) for n, v in re.findall(r'(\w+)\s*=\s*(\d+)', enum)}
    tiles = routes.pop('WG_TILES')
    assert tiles == max(routes.values()) + 1
    glds = {(int(a), int(b)) for a, b in re.findall(r'launch_wgrad_glds<T, (\d+), (\d+),', src)}
    staged = {(int(a), int(b)) for a, b in re.findall(r'WG_LAUNCH\((\d+), (\d+)\);', src)}
    return sorted(routes.values()), sorted(glds), sorted(staged)
