"""The Swin kernels of csrc/swin.hip restated with torch's own ops in float64 on the CPU, the input generators, the route tables and the elementwise comparators of
tests/test_swin_reference_cpu.py and tests/test_swin_parity_gpu.py.  Nothing here restates a kernel's index arithmetic: LayerNorm / GELU / conv / unfold / interpolate are
torch's, the window partition is pad + torch.roll + view / permute with oracle.swin_oracle.shift_mask, gradients come from autograd or from a closed form that
test_swin_reference_cpu.py checks against autograd.  Every reference takes the kernel's own inputs AFTER rounding to the kernel's input type, so input rounding costs no
tolerance, and every reference takes `dt`: float64 is the reference, float32 the CPU yardstick the constants below are set from.

Comparators.  |kernel - reference| <= bound elementwise, bound = K * 2^-24 * R_abs (+ the terms below), R_abs the same reference evaluated on absolute values (the sum
of |terms|: the quantity a rounding of any partial result is relative to).  None is taken from a kernel's output.  K is set per family from torch's own FLOAT32 evaluation
of the same plain reference against the float64 one on the CPU (worst ratio over every case of the tables below, printed by test_swin_reference_cpu.py), times a margin
of 8 for a different summation order and the fast exponential, rounded up to a power of two; floor 4 (an expression of up to four roundings).  Measured (torch 2.10 CPU):

    family          worst fp32 / (2^-24 R_abs)     K
    ln_fwd          %(ln_fwd)s
    ln_fwd_offset   %(ln_fwd_offset)s
    ln_bwd          %(ln_bwd)s
    ln_cols         %(ln_cols)s
    gelu            %(gelu)s
    patch           %(patch)s
    bilinear        %(bilinear)s
    attn_fwd        %(attn_fwd)s
    attn_bwd        %(attn_bwd)s
    table           %(table)s

* bf16 outputs add 2^-8 |ref| for the final rounding (half a bf16 ulp is at most 2^-9 of the value's binade, i.e. at most 2^-8 of the value).
* LayerNorm: R_abs = |x - mean| rstd |gamma| + |beta|.  The subtraction x - mean is exact only to the ulp of x: the mean carries the rounding of a sum of values of size
  max|x| and x - mean one more, together delta = 2^-23 max_row|x|; every x_hat is off by delta * rstd, which adds delta * rstd * |gamma| to y whatever the size of
  x - mean (the family x = 100 + randn lives on this term; a one-pass E[x^2] - mean^2 variance would be off by 2^-24 * 100^2 * rstd^2 relative and is rejected there).
  The offset family has a constant of its own (ln_fwd_offset): torch's float32 mean of 96 values near 100 is itself off by up to 2^-23 max|x| (half an ulp of each
  partial sum near 9 600 is 5e-4), so on the elements next to the mean, where R_abs is small, the K term has to carry what the delta term leaves.
  The statistics: the mean to 24 * 2^-24 max|x| (worst case of a sum of C values, <= 12 additions in a lane, <= 6 shuffle levels, each relative to a partial sum);
  rstd to K 2^-24 rstd + rstd^3 / 2 * (2 d mean|x - mean| + d^2) with that d (the error of var, through d rstd = rstd^3 d var / 2).
  Backward, g = dy gamma, x_hat = (x - mean) rstd:  dx: R_abs = rstd (|g| + mean|g| + |x_hat| mean|g x_hat|) + |addend|; every x_hat is off by delta rstd, which moves dx by at
  most rstd * delta rstd * (|x_hat| mean|g| + mean|g x_hat| + mean|g|).
  dgamma: R_abs = sum_rows |dy| |x_hat| plus sum_rows |dy| delta rstd; dbeta: R_abs = sum_rows |dy|.  The scaled copy is round_T(dx) * row_scale[b], rounded once more:
  the dx bound times |row_scale| plus the output rounding; a sample with scale 0 is exactly 0.
* GELU: near the negative tail 1 + erf cancels, a bound relative to the result would be void: K 2^-24 |x| absolutely plus one ulp of the result (2^-23 |ref| fp32,
  2^-8 |ref| bf16).  bf16 tensors use the Abramowitz-Stegun erf (|error| < 6.1e-7, csrc/common.h): 3.05e-7 |x| more.  Backward: K 2^-24 |dy| (1 + |x| pdf(x)) (the cdf is
  bounded by 1 absolutely), 3.05e-7 |dy| more in bf16, plus the output rounding.
* patch embedding: R_abs = |bias| + sum |w| |img| (a 48-term fma chain).  Its weight gradient is the MFMA weight-gradient GEMM over the im2col: R_abs = sum_tokens |dy| |col|;
  in bf16 the im2col rounds the image once (2^-8 R_abs more, the unit roundoff of bf16 as below); bias gradient R_abs = sum_tokens |dy|.
* bilinear: the kernels form the source coordinate in fp32, a few ulp of the COORDINATE, so a weight is off absolutely and the error is relative to the neighbouring taps, not
  to the (possibly tiny) weighted sum: K 2^-24 max(R_abs) over the tensor, R_abs = interpolate(|x|) (+ |base|); same for the backward with R_abs = its autograd on |dy|
  (+ |previous content| under accumulate).  A wrong tap, weight, border or window is 4 orders above.
* window attention (q k^T / sqrt 32 + bias + mask, softmax, P v).  out: R_abs = sum_j P_ij |v_j|.  With dP_abs = |dO| . |v| and A = P (dP_abs + sum_j P dP_abs) bounding
  |dS|: dq: R_abs = sum_j A_ij |k_j| / sqrt 32; dk: sum_i A_ij |q_i| / sqrt 32; dv: sum_i P_ij |dO_i|; d rel_bias: sum over windows of A; the pad-token share of
  d qkv_bias: the sum of the dk / dv R_abs over the pad tokens.  A masked pair has P = e^-100 = 4e-44, below the smallest normal fp32 number: each P may be
  lost to underflow, 2^-126 times what it multiplies ('*_floor': the same sums with P replaced by 1) is added to the bounds of dqkv, d rel_bias and the pad share.
  The MFMA kernels round operands to bf16 between their two MFMA stages, counted from the code:
    forward    P before O^T = V^T P^T                                                   1 rounding of out
    backward   dS before dQ^T = K^T dS and before dK^T = Q^T dS^T, P before dV^T = dO^T P^T     1 rounding each of dq, dk, dv and of the pad-token sums (taken from dk / dv)
               the sum of dS over windows is taken from the fp32 registers              0 roundings of d rel_bias
  (q, k, v, dO are the bf16 inputs themselves), each 2^-8 R_abs: bf16 has 8 significant bits, so a rounding moves a value by up to 2^-8 of itself (half the spacing 2^-7 at the
  bottom of a binade; 2^-9 holds only at the top of one).  Replaying exactly these roundings in otherwise exact float64 arithmetic (mut = 'mfma-roundings') reaches 1.39 times a
  2^-9 R_abs + 2^-8 |ref| bound on the windows that are mostly pad tokens, and the MI355X kernels give the same figures to three digits.
  Pad tokens carry the qkv bias rounded to the tensor type, as the qkv GEMM would have stored it.
* position-table gradient: R_abs = sum over the pair list of |d bias|; d qkv_bias = colsum + pad share is one addition: 2^-24 |ref|.
* kernels that only move or select data (merge gather / scatter, im2col, scale_add with scales in {0, 0.5, 1, 2}, every zero channel pad): bit for bit, on inputs whose
  results are exact in bf16 (check_exact, on the reference alone)."""
import math
import zlib

import torch
import torch.nn.functional as F

from oracle import swin_oracle as so

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
DTYPES = {'f32': F32, 'bf16': BF16}
WS, WN, HD = 7, 49, 32

# family: (worst CPU float32 ratio measured, K = pow2ceil(8 * ratio), floor 4)
MEASURED = {'ln_fwd': (2.77, 32), 'ln_fwd_offset': (185.0, 2048), 'ln_bwd': (1.69, 16), 'ln_cols': (1.8, 16), 'gelu': (4.04, 64), 'patch': (3.73, 32), 'bilinear': (26.2, 256),
            'attn_fwd': (16.2, 256), 'attn_bwd': (13.4, 128), 'table': (2.59, 32)}
K = {f: k for f, (_, k) in MEASURED.items()}
__doc__ = __doc__ % {f: '%-30.3g %d' % v for f, v in MEASURED.items()}
E24 = 2.0 ** -24
BF16_U = 2.0 ** -8              # unit roundoff of bf16 (8 significant bits): one rounding moves a value by at most this fraction of itself


def k_from(ratio):
    """The rule of the constants: 8 x the CPU float32 ratio, rounded up to a power of two, at least 4."""
    return max(4, 2 ** math.ceil(math.log2(max(8.0 * ratio, 1e-30))))


def vec(dtype):
    """Elements of a 16-byte vector."""
    return 8 if dtype == BF16 else 4


# ------------------------------------------------------------------------------------------------------------ inputs
def gen(tag):
    g = torch.Generator()
    g.manual_seed(zlib.crc32(tag.encode()))
    return g


def randn(tag, shape, dtype=F32, scale=1.0):
    """Normal values rounded to `dtype` (the kernel's input type)."""
    return (torch.randn(shape, generator=gen(tag), dtype=F32) * scale).to(dtype)


def rand(tag, shape, lo=0.0, hi=1.0):
    return torch.rand(shape, generator=gen(tag), dtype=F32) * (hi - lo) + lo


def ints(tag, shape, dtype, lo=-3, hi=3, step=1.0):
    """Integer multiples of `step` (a power of two) in [lo, hi] * step: exact in bf16 and fp32."""
    return (torch.randint(lo, hi + 1, shape, generator=gen(tag)).to(F32) * step).to(dtype)


def padded(t, P):
    """[..., C] -> [..., P] with a zero channel pad."""
    if t.shape[-1] == P:
        return t.contiguous()
    out = torch.zeros(t.shape[:-1] + (P,), dtype=t.dtype)
    out[..., :t.shape[-1]] = t
    return out


def check_exact(ref, what=''):
    """The condition of a bit-for-bit comparison, on the reference alone: the float64 result is a bf16 number (so it is exact in either type, whatever the order)."""
    r = ref.to(F64)
    assert bool((r.to(BF16).to(F64) == r).all()), what + ': reference is not exact in bf16'


# ------------------------------------------------------------------------------------------------------------ comparators
def worst_ratio(what, got, ref, bound):
    """max over the elements of |got - ref| / bound (bound: a float64 tensor broadcastable to ref, or a number); an element with bound 0 must be exact.  Prints the figure."""
    got, ref = got.to(F64), ref.to(F64)
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    assert bool(torch.isfinite(got).all()), what + ': non-finite result'
    err = (got - ref).abs()
    b = (bound if isinstance(bound, torch.Tensor) else torch.full_like(ref, float(bound))).to(F64).expand_as(ref)
    ratio = torch.where(b > 0, err / b.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float('inf')), torch.zeros_like(err)))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print('%s: worst error/bound %.3g (max error %.3g, max |ref| %.3g)' % (what, worst, float(err.max()) if err.numel() else 0.0, float(ref.abs().max()) if ref.numel() else 0.0))
    return worst


def bit_equal(what, got, ref):
    """Bit for bit against a float64 reference that check_exact has accepted; prints and returns the number of differing elements."""
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    n = int((got.to(F64) != ref.to(F64)).sum())
    print('%s: %d of %d elements differ' % (what, n, ref.numel()))
    return n


def out_rounding(ref, dtype):
    """The one final rounding of a bf16 output: 2^-8 |ref|; nothing for fp32."""
    return BF16_U * ref.abs() if dtype == BF16 else torch.zeros_like(ref)


# ------------------------------------------------------------------------------------------------------------ LayerNorm
LN_EPS = 1e-5
LN_FAMILIES = ('randn', 'offset100', 'near-constant')


def ln_input(tag, family, shape, C, dtype):
    """[..., P] with a zero pad past C.  offset100: x = 100 + randn.  near-constant: 1 + 2^-7 * {0, 1} (exact in bf16, variance near eps), row 0 exactly constant."""
    if family == 'randn':
        x = randn(tag, shape[:-1] + (C,), F32) * 2 + 0.5
    elif family == 'offset100':
        x = randn(tag, shape[:-1] + (C,), F32) + 100.0
    else:
        x = 1.0 + 2.0 ** -7 * torch.randint(0, 2, shape[:-1] + (C,), generator=gen(tag)).to(F32)
        x.view(-1, C)[0] = 1.0
    return padded(x.to(dtype), shape[-1])


def ln_stats(x, C, dt=F64, eps=LN_EPS, divisor=None):
    xd = x[..., :C].to(dt)
    n = C if divisor is None else divisor
    mean = xd.sum(-1, keepdim=True) / n
    var = ((xd - mean) ** 2).sum(-1, keepdim=True) / n
    return xd, mean, (var + eps).rsqrt()


def ln_fwd(x, gamma, beta, C, dt=F64, eps=LN_EPS):
    """F.layer_norm over the first C channels -> (y [..., C], mean [...], rstd [...]).  The float32 yardstick is the two-pass expression (x - mean) rstd gamma + beta
    with torch's ops: ATen's CPU float32 layer_norm folds the mean into an offset, x rstd - mean rstd, and loses 2^-24 |x| rstd to the cancellation (196 in the units of
    the table above on the near-constant family), which is no yardstick for a two-pass kernel.  In float64 the two agree to 1e-12 (test_swin_reference_cpu.py)."""
    xd, mean, rstd = ln_stats(x, C, dt, eps)
    y = F.layer_norm(xd, (C,), gamma.to(dt), beta.to(dt), eps) if dt == F64 else (xd - mean) * rstd * gamma.to(dt) + beta.to(dt)
    return y, mean[..., 0], rstd[..., 0]


def ln_fwd_wrong(x, gamma, beta, C, divisor=None, eps=LN_EPS):
    """A wrong kernel: statistics over `divisor` channels (the pitch) instead of C, or another eps."""
    xd, mean, rstd = ln_stats(x, C, F64, eps, divisor)
    return (xd - mean) * rstd * gamma.to(F64) + beta.to(F64)


def ln_delta(x, C):
    return 2.0 ** -23 * x[..., :C].to(F64).abs().amax(-1, keepdim=True)


def ln_fwd_bound(x, gamma, beta, C, ref, dtype, family='randn'):
    xd, mean, rstd = ln_stats(x, C)
    g = gamma.to(F64).abs()
    return K['ln_fwd_offset' if family == 'offset100' else 'ln_fwd'] * E24 * ((xd - mean).abs() * rstd * g + beta.to(F64).abs()) + ln_delta(x, C) * rstd * g + out_rounding(ref, dtype)


def ln_stats_bounds(x, C):
    xd, mean, rstd = ln_stats(x, C)
    d = 12 * ln_delta(x, C)                                                # 24 * 2^-24 max|x|: the worst case of the summation tree (module docstring)
    dvar = 2 * d * (xd - mean).abs().mean(-1, keepdim=True) + d * d
    return d[..., 0], (K['ln_fwd'] * E24 * rstd + 0.5 * rstd ** 3 * dvar)[..., 0]


def ln_bwd(dy, x, gamma, C, addend=None, dt=F64, eps=LN_EPS):
    """Autograd of F.layer_norm -> (dx [..., C] (+ addend), dgamma [C], dbeta [C])."""
    xd = x[..., :C].to(dt).clone().requires_grad_(True)
    g = gamma.to(dt).clone().requires_grad_(True)
    b = torch.zeros(C, dtype=dt, requires_grad=True)
    y = F.layer_norm(xd, (C,), g, b, eps)
    dx, dg, db = torch.autograd.grad(y, (xd, g, b), dy[..., :C].to(dt))
    if addend is not None:
        dx = dx + addend[..., :C].to(dt)
    return dx, dg, db


def ln_bwd_bounds(dy, x, gamma, C, addend, refs, dtype):
    """(dx bound [..., C], dgamma bound [C], dbeta bound [C])."""
    xd, mean, rstd = ln_stats(x, C)
    xh = ((xd - mean) * rstd).abs()
    dya = dy[..., :C].to(F64).abs()
    g = dya * gamma.to(F64).abs()
    mg, mgx = g.mean(-1, keepdim=True), (g * xh).mean(-1, keepdim=True)
    r_abs = rstd * (g + mg + xh * mgx) + (addend[..., :C].to(F64).abs() if addend is not None else 0.0)
    dxh = ln_delta(x, C) * rstd                                           # what every x_hat is off by
    bdx = K['ln_bwd'] * E24 * r_abs + rstd * dxh * (mg * xh + mgx + mg) + out_rounding(refs[0], dtype)
    flat = lambda t: t.reshape(-1, C)
    bdg = K['ln_cols'] * E24 * flat(dya * xh).sum(0) + flat(dya * dxh).sum(0)
    bdb = K['ln_cols'] * E24 * flat(dya).sum(0)
    return bdx, bdg, bdb


def ln_fwd_route(dtype, C, py):
    """launch_ln_fwd: (lanes per row, channel vectors a lane keeps in registers; 0 = streaming) by the vectors of a row incl. the output pitch's pad."""
    nvp = max(py // vec(dtype), C // vec(dtype))
    return (16, 1) if nvp <= 16 else (32, 1) if nvp <= 32 else (64, 1) if nvp <= 64 else (64, 2) if nvp <= 128 else (64, 3) if nvp <= 192 else (64, 0)


def ln_fwd_trips(dtype, rows, C, py):
    """(grid, trips of a block's grid-stride loop): a block takes 4 * 64 / LPR rows per trip, the grid is capped at 16 384 blocks."""
    rpb = 4 * (64 // ln_fwd_route(dtype, C, py)[0])
    grid = min(16384, max(1, -(-rows // rpb)))
    return grid, -(-rows // (grid * rpb))


def ln_bwd_blocks(dtype, rows, pdx):
    """sl_layernorm_bwd_rows: the partial rows of the column sums (= the grid of the fused form)."""
    nvp = pdx // vec(dtype)
    if nvp > 192:
        return min(1024, max(1, -(-rows // 256)))
    rpb = 4 * (64 // (16 if nvp <= 16 else 32 if nvp <= 32 else 64))
    want = rows // 16 + 1
    if want < 512:
        want = min(-(-rows // rpb), 512)
    return min(2048, max(1, want))


def ln_bwd_route(dtype, rows, C, pdx, want_param_grads):
    """launch_ln_bwd: ('fused' | 'cols' | 'dx-only', LPR, NV, grid, trips).  fused: the column sums ride in the lanes' registers (rows of at most 192 vectors); cols: NV = 0
    and layernorm_bwd_cols_kernel; dx-only: NV = 0, no partials."""
    nvec, nvp = C // vec(dtype), pdx // vec(dtype)
    if want_param_grads and nvp <= 192:
        lpr, nv = (16, 1) if nvp <= 16 else (32, 1) if nvp <= 32 else (64, 1) if nvp <= 64 else (64, 2) if nvp <= 128 else (64, 3)
        grid = ln_bwd_blocks(dtype, rows, pdx)
        kind = 'fused'
    else:
        lpr, nv = 16 if nvec <= 16 else 32 if nvec <= 32 else 64, 0
        grid = min(8192, rows // 16 + 1)
        kind = 'cols' if want_param_grads else 'dx-only'
    return kind, lpr, nv, grid, -(-rows // (grid * 4 * (64 // lpr)))


# name: (dtype, B, rows per sample, C, px, py = pdx, family, options).  Options: nostats, noparam, noaddend, rowscale, fwdonly
LN_CASES = {
    'f32-c64-1row':            ('f32', 1, 1, 64, 64, 64, 'randn', ()),
    'bf16-c96-p128':           ('bf16', 5, 37, 96, 128, 128, 'randn', ()),
    'f32-c96-p128-3rows':      ('f32', 1, 3, 96, 128, 128, 'randn', ()),
    'bf16-c192':               ('bf16', 5, 37, 192, 192, 192, 'randn', ()),
    'f32-c192':                ('f32', 5, 37, 192, 192, 192, 'randn', ()),
    'bf16-c384-3rows':         ('bf16', 3, 1, 384, 384, 384, 'randn', ('rowscale',)),
    'f32-c384':                ('f32', 5, 37, 384, 384, 384, 'randn', ()),
    'bf16-c768-1row':          ('bf16', 1, 1, 768, 768, 768, 'randn', ()),
    'f32-c768':                ('f32', 5, 37, 768, 768, 768, 'randn', ()),
    'bf16-c1536':              ('bf16', 5, 37, 1536, 1536, 1536, 'randn', ()),
    'f32-c1536-cols':          ('f32', 5, 37, 1536, 1536, 1536, 'randn', ()),
    'f32-c1536-cols-1row':     ('f32', 1, 1, 1536, 1536, 1536, 'randn', ()),
    'bf16-c2048-cols':         ('bf16', 5, 37, 2048, 2048, 2048, 'randn', ()),
    'f32-c192-2051rows':       ('f32', 1, 2051, 192, 192, 192, 'randn', ()),
    'f32-c96-4099rows':        ('f32', 1, 4099, 96, 128, 128, 'randn', ()),
    'bf16-c96-32771rows':      ('bf16', 1, 32771, 96, 128, 128, 'randn', ()),
    'f32-c192-65539rows-fwd':  ('f32', 1, 65539, 192, 192, 192, 'randn', ('fwdonly',)),
    'bf16-c96-px96-py128':     ('bf16', 5, 37, 96, 96, 128, 'randn', ()),
    'f32-c96-px128-py96':      ('f32', 5, 37, 96, 128, 96, 'randn', ()),
    'f32-c64-nostats-dxonly':  ('f32', 5, 37, 64, 64, 64, 'randn', ('nostats', 'noparam')),
    'f32-c128-dxonly':         ('f32', 5, 37, 128, 128, 128, 'randn', ('noparam', 'noaddend')),
    'bf16-c384-dxonly':        ('bf16', 5, 37, 384, 384, 384, 'randn', ('noparam',)),
    'bf16-c96-dxonly':         ('bf16', 5, 37, 96, 128, 128, 'randn', ('noparam',)),
    'bf16-c192-dxonly':        ('bf16', 5, 37, 192, 192, 192, 'randn', ('noparam', 'nostats')),
    'f32-c384-dxonly':         ('f32', 1, 3, 384, 384, 384, 'randn', ('noparam',)),
    'bf16-c96-noaddend':      ('bf16', 5, 37, 96, 128, 128, 'randn', ('noaddend',)),
    'f32-c96-rowscale':        ('f32', 3, 61, 96, 128, 128, 'randn', ('rowscale',)),
    'bf16-c96-rowscale':       ('bf16', 3, 61, 96, 128, 128, 'randn', ('rowscale',)),
    'f32-c96-offset100':       ('f32', 5, 37, 96, 128, 128, 'offset100', ()),
    'bf16-c192-offset100':     ('bf16', 5, 37, 192, 192, 192, 'offset100', ()),
    'f32-c96-near-constant':   ('f32', 5, 37, 96, 128, 128, 'near-constant', ()),
    'bf16-c96-near-constant':  ('bf16', 5, 37, 96, 128, 128, 'near-constant', ()),
}
ROW_SCALE = (0.0, 1.0, 1.0 / 0.9)


def ln_case(name):
    """The shared, unmodified inputs of a case."""
    d, B, n, C, px, py, family, opts = LN_CASES[name]
    dtype = DTYPES[d]
    c = dict(dtype=dtype, B=B, n=n, rows=B * n, C=C, px=px, py=py, opts=opts, family=family)
    c['x'] = ln_input('ln/x/' + name, family, (B, n, px), C, dtype)
    c['gamma'] = rand('ln/g/' + name, (C,), 0.5, 1.5)
    c['beta'] = randn('ln/b/' + name, (C,))
    c['dy'] = padded(randn('ln/dy/' + name, (B, n, C), dtype), py)          # the gradient and the addend live at the dx pitch
    c['addend'] = None if 'noaddend' in opts else padded(randn('ln/add/' + name, (B, n, C), dtype), py)
    c['row_scale'] = torch.tensor(ROW_SCALE, dtype=F32) if 'rowscale' in opts else None
    return c


# ------------------------------------------------------------------------------------------------------------ GELU, scale_add
def gelu_input(tag, n, dtype):
    """A grid over [-8, 8] followed by random values, n elements."""
    grid = torch.linspace(-8, 8, min(n, 4097))
    return torch.cat([grid, randn(tag, (n - grid.numel(),)) * 2]).to(dtype)


def gelu_fwd(h, dt=F64):
    return F.gelu(h.to(dt))


def gelu_bwd(h, dy, dt=F64):
    x = h.to(dt).clone().requires_grad_(True)
    return torch.autograd.grad(F.gelu(x), x, dy.to(dt))[0]


AS_ERF = 0.5 * 6.1e-7          # the Abramowitz-Stegun erf of the bf16 kernels, times the 1/2 of GELU


def gelu_fwd_bound(h, ref, dtype):
    x = h.to(F64).abs()
    return K['gelu'] * E24 * x + (2.0 ** -8 * ref.abs() + AS_ERF * x if dtype == BF16 else 2.0 ** -23 * ref.abs())


def gelu_bwd_bound(h, dy, ref, dtype):
    x, g = h.to(F64), dy.to(F64).abs()
    pdf = torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)
    return K['gelu'] * E24 * g * (1 + x.abs() * pdf) + (AS_ERF * g if dtype == BF16 else 0.0) + out_rounding(ref, dtype)


# elements (a multiple of 8): 2 vectors; a vector count that is no multiple of 256; the second grid-stride trip past ew_grid's 16 384 blocks (bf16 only)
GELU_SIZES = {'16': 16, '9000': 9000, 'second-trip': (16384 * 256 + 37) * 8}
EW_CAP = 16384


def ew_trips(nvec):
    """Trips of an elementwise kernel's grid-stride loop: 256 threads per block, ew_grid caps the grid at 16 384 blocks."""
    grid = min(EW_CAP, max(1, -(-nvec // 256)))
    return -(-nvec // (grid * 256))


SCALES = (0.0, 0.5, 1.0, 2.0)


def scale_add(x, scale, addend, C, per_channel, dt=F64):
    """x [B, rows, P]: addend + x * scale[b] (DropPath) or addend + x * scale[b][c] with the channel pad forced to zero (Dropout2d); a broadcast multiply and add."""
    B, P = x.shape[0], x.shape[-1]
    s = scale.to(dt)
    if per_channel:
        s = padded(s.view(B, C), P).view((B,) + (1,) * (x.dim() - 2) + (P,))
    else:
        s = s.view((B,) + (1,) * (x.dim() - 1))
    out = x.to(dt) * s
    return out + addend.to(dt) if addend is not None else out


# name: (B, rows per sample, C, P, per_channel, with addend)
SCALE_ADD_CASES = {
    'droppath': (4, 37, 96, 128, False, False),
    'droppath-addend': (4, 37, 96, 128, False, True),
    'dropout2d': (4, 37, 96, 128, True, False),
    'dropout2d-addend': (4, 37, 96, 128, True, True),
    'droppath-c192': (3, 5, 192, 192, False, True),
}
SCALE_ADD_BIG = (1, 16384 * 256 + 37, 8, 8, False, True)                   # bf16: that many 8-element vectors


def scale_add_case(name, dtype, spec=None):
    B, rows, C, P, per_channel, with_add = spec or SCALE_ADD_CASES[name]
    x = ints('sa/x/' + name, (B, rows, P), dtype)
    add = ints('sa/a/' + name, (B, rows, P), dtype) if with_add else None
    sc = torch.tensor(SCALES)[torch.randint(0, 4, (B * C if per_channel else B,), generator=gen('sa/s/' + name))]
    if not per_channel:
        sc[:min(B, 4)] = torch.tensor(SCALES)[-min(B, 4):]             # four samples or more: every scale occurs; one sample: 2
    return x, sc.contiguous(), add, C, per_channel


# ------------------------------------------------------------------------------------------------------------ patch embedding
def patch_pad(img, dt=F64):
    H, W = img.shape[2:]
    return F.pad(img.to(dt), (0, (4 - W % 4) % 4, 0, (4 - H % 4) % 4))


def patch_embed_fwd(img, w, b, dt=F64):
    """conv 4x4 stride 4 of the zero-padded NCHW image -> NHWC [B, Ho, Wo, C]."""
    return F.conv2d(patch_pad(img, dt), w.to(dt), b.to(dt), stride=4).permute(0, 2, 3, 1).contiguous()


def patch_embed_abs(img, w, b):
    return patch_embed_fwd(img.abs(), w.abs(), b.abs())


def patch_im2col(img, dt=F64):
    """[tokens, 64]: F.unfold of the padded image (column ci*16 + ky*4 + kx), columns 48..63 zero."""
    u = F.unfold(patch_pad(img, dt), 4, stride=4)                        # [B, 48, L]
    return padded(u.transpose(1, 2).reshape(-1, 48), 64)


def patch_embed_bwd(img, dy, C, dt=F64):
    """Autograd of the conv: (dw [C, 3, 4, 4], db [C]) for dy NHWC [B, Ho, Wo, >= C]."""
    w = torch.zeros(C, 3, 4, 4, dtype=dt, requires_grad=True)
    b = torch.zeros(C, dtype=dt, requires_grad=True)
    y = F.conv2d(patch_pad(img, dt), w, b, stride=4)
    return torch.autograd.grad(y, (w, b), dy[..., :C].to(dt).permute(0, 3, 1, 2))


def patch_bwd_bounds(img, dy, C, dtype):
    dwa, dba = patch_embed_bwd(img.abs(), dy.abs(), C)
    return (K['patch'] * E24 + (BF16_U if dtype == BF16 else 0.0)) * dwa, K['patch'] * E24 * dba


# name: (B, H, W, C, pitch)
PATCH_CASES = {
    'c32-30x37': (1, 30, 37, 32, 128),
    'c96-30x37-b2': (2, 30, 37, 96, 128),
    'c128-5x3': (1, 5, 3, 128, 128),
    'c192-one-token': (1, 3, 2, 192, 256),
    'c96-64-tokens': (1, 32, 32, 96, 128),
    'c192-33x61': (3, 33, 61, 192, 192),
}


# ------------------------------------------------------------------------------------------------------------ patch merging
def merge_gather(x, C, dt=F64):
    """PatchMerging's 2x2 space-to-depth on the zero-padded map, the quarters in oracle.swin_oracle.patch_merging's order.  x [B, H, W, >= C] -> [B, H2, W2, 4C]."""
    B, H, W, _ = x.shape
    x = F.pad(x[..., :C].to(dt), (0, 0, 0, W % 2, 0, H % 2))
    return torch.cat([x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]], -1)


def merge_gather_wrong(x, C, swap=False, pad_value=0.0):
    B, H, W, _ = x.shape
    x = F.pad(x[..., :C].to(F64), (0, 0, 0, W % 2, 0, H % 2), value=pad_value)
    q = [x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]]
    if swap:
        q[1], q[2] = q[2], q[1]
    return torch.cat(q, -1)


def merge_scatter(dxm, shape, C, dt=F64):
    """Autograd of the gather: [B, H2, W2, 4C] -> [B, H, W, P] with a zero channel pad."""
    B, H, W, P = shape
    x = torch.zeros(B, H, W, C, dtype=dt, requires_grad=True)
    g, = torch.autograd.grad(merge_gather(x, C, dt), x, dxm.to(dt))
    return padded(g, P)


# name: (B, H, W, C, P)
MERGE_CASES = {'odd-odd-c96': (2, 5, 7, 96, 128), 'odd-even-c192': (2, 5, 6, 192, 192), 'even-odd-c96': (1, 4, 3, 96, 128), '1x1-c96': (1, 1, 1, 96, 128), '1x1-c192': (3, 1, 1, 192, 192)}


# ------------------------------------------------------------------------------------------------------------ bilinear
def bilinear_fwd(x, size, align, Cn=None, src_off=0, dt=F64):
    """F.interpolate(bilinear) of the channel window [src_off, src_off + Cn) of an NHWC map -> [B, H, W, Cn]."""
    Cn = x.shape[-1] if Cn is None else Cn
    xs = x[..., src_off:src_off + Cn].to(dt).permute(0, 3, 1, 2)
    return F.interpolate(xs, size=tuple(size), mode='bilinear', align_corners=align).permute(0, 2, 3, 1).contiguous()


def bilinear_bwd(dy, src_hw, align, Cn=None, dy_off=0, dt=F64):
    """Autograd of F.interpolate wrt its source for the channel window of dy -> [B, h, w, Cn]."""
    B, H, W, _ = dy.shape
    Cn = dy.shape[-1] if Cn is None else Cn
    x = torch.zeros(B, Cn, src_hw[0], src_hw[1], dtype=dt, requires_grad=True)
    y = F.interpolate(x, size=(H, W), mode='bilinear', align_corners=align)
    g, = torch.autograd.grad(y, x, dy[..., dy_off:dy_off + Cn].to(dt).permute(0, 3, 1, 2))
    return g.permute(0, 2, 3, 1).contiguous()


def window_put(prefill, y, off, accumulate=False):
    """What a kernel writing the channel window [off, off + Cn) of `prefill` must leave: plain slicing and adds."""
    out = prefill.to(y.dtype).clone()
    w = out[..., off:off + y.shape[-1]]
    out[..., off:off + y.shape[-1]] = w + y if accumulate else y
    return out


def bilinear_bound(ref, ref_abs, dtype):
    return K['bilinear'] * E24 * float(ref_abs.max()) + out_rounding(ref, dtype)


def bilinear_bwd_route(dy_dtype, B, h, w, H, W, Cn):
    """sl_bilinear_bwd: a block per source pixel when there are few source pixels under a map of at least 4x their number and the channel vectors divide a block."""
    nv = Cn // vec(dy_dtype)
    return 'small' if B * h * w <= 2048 and H * W >= 4 * h * w and nv <= 128 and 256 % nv == 0 else 'general'


BIL_TYPES = {'f32/f32': (F32, F32), 'bf16/bf16': (BF16, BF16), 'bf16/f32': (BF16, F32)}          # (large map T, small map TS)
# geometry name: (B, h, w, H, W)
BIL_GEOM = {'up-4x5-8x10': (2, 4, 5, 8, 10), 'up-2x3-16x20': (2, 2, 3, 16, 20), 'src-1x1': (2, 1, 1, 7, 9), 'src-one-row': (1, 1, 6, 5, 13), 'down-9x12-5x6': (2, 9, 12, 5, 6),
            'identity-6x6': (1, 6, 6, 6, 6), 'to-1x1': (1, 3, 4, 1, 1)}
# backward: name: (geometry (B, h, w, H, W), channel vectors of dy, route, options).  Options: window (dy_off, out_off in wider tensors), accumulate
BIL_BWD_CASES = {
    'small-nv2': ((2, 2, 3, 16, 20), 2, 'small', ()),
    'small-nv128': ((1, 2, 3, 5, 6), 128, 'small', ()),
    'small-nv2-window-accumulate': ((2, 2, 3, 16, 20), 2, 'small', ('window', 'accumulate')),
    'small-src-1x1': ((2, 1, 1, 7, 9), 4, 'small', ()),
    'small-exactly-4x': ((1, 4, 5, 8, 10), 2, 'small', ()),
    'small-2048-sources': ((2, 32, 32, 64, 64), 2, 'small', ()),
    'general-nv12': ((2, 2, 3, 16, 20), 12, 'general', ()),
    'general-nv24-window-accumulate': ((2, 2, 3, 16, 20), 24, 'general', ('window', 'accumulate')),
    'general-2052-sources': ((2, 27, 38, 54, 76), 2, 'general', ()),
    'general-under-4x': ((1, 4, 5, 8, 9), 2, 'general', ()),
    'general-down-9x12-5x6': ((2, 9, 12, 5, 6), 2, 'general', ()),
    'general-identity': ((1, 6, 6, 6, 6), 4, 'general', ('window',)),
    'general-src-one-row-nv12': ((1, 1, 6, 5, 13), 12, 'general', ()),
    'general-window': ((2, 4, 5, 8, 9), 2, 'general', ('window',)),
}


# ------------------------------------------------------------------------------------------------------------ window attention
def attn_geom(H, W):
    Hp, Wp = -(-H // WS) * WS, -(-W // WS) * WS
    return Hp, Wp, (Hp // WS) * (Wp // WS)


def band_mask(Hp, Wp, shift, d7=0, d3=0):
    """oracle.swin_oracle.shift_mask with the two band boundaries (Hp - 7, Hp - 3) of the ROWS movable by d7 / d3: the wrong kernels of the sharpness tests.
    test_swin_reference_cpu.py asserts that it equals shift_mask at d7 = d3 = 0; the references below use shift_mask itself."""
    band = lambda n, a, b: torch.where(torch.arange(n) < n - WS + a, 0, torch.where(torch.arange(n) < n - shift + b, 1, 2))
    ids = (3 * band(Hp, d7, d3)[:, None] + band(Wp, 0, 0)[None, :]).float()
    w = ids.view(Hp // WS, WS, Wp // WS, WS).permute(0, 2, 1, 3).reshape(-1, WN)
    diff = w[:, None, :] - w[:, :, None]
    return torch.where(diff != 0, torch.full_like(diff, -100.0), torch.zeros_like(diff))


def _partition(t):
    """[Hp, Wp, X] -> [nW, 49, X] (swintransformer.py's window_partition)."""
    Hp, Wp, X = t.shape
    return t.view(Hp // WS, WS, Wp // WS, WS, X).permute(0, 2, 1, 3, 4).reshape(-1, WN, X)


def _reverse(w, Hp, Wp):
    return w.view(Hp // WS, Wp // WS, WS, WS, -1).permute(0, 2, 1, 3, 4).reshape(Hp, Wp, -1)


def _heads(t, heads):
    """[nW, 49, heads * 32] -> [nW, heads, 49, 32]"""
    return t.view(t.shape[0], WN, heads, HD).transpose(1, 2)


def _unheads(t):
    return t.transpose(1, 2).reshape(t.shape[0], WN, -1)


MUTANTS = ('no-mask', 'mask-row-7', 'mask-row-3', 'roll-reversed', 'pad-zero', 'relb-transposed', 'last-window-missing', 'window-to-neighbour')


def _attn_sample(x, pad_bias, relb, C, heads, shift, mut, dO=None, last=False):
    """One sample.  x [H, W, 3C] (dt, may require grad), pad_bias [3C] -> out [H, W, C]; with dO [H, W, C] also the closed-form backward and every R_abs."""
    H, W, _ = x.shape
    Hp, Wp, nW = attn_geom(H, W)
    dt = x.dtype
    fill = torch.zeros_like(pad_bias) if mut == 'pad-zero' else pad_bias
    canvas = torch.cat([torch.cat([x, fill.expand(H, Wp - W, 3 * C)], 1), fill.expand(Hp - H, Wp, 3 * C)], 0)
    sh = (shift, shift) if mut == 'roll-reversed' else (-shift, -shift)
    roll = (lambda t: torch.roll(t, sh, (0, 1))) if shift else (lambda t: t)
    unroll = (lambda t: torch.roll(t, (-sh[0], -sh[1]), (0, 1))) if shift else (lambda t: t)
    xw = _partition(roll(canvas))
    q, k, v = (_heads(xw[..., i * C:(i + 1) * C], heads) for i in range(3))
    scale = HD ** -0.5
    rb = relb.to(dt)
    s = (q * scale) @ k.transpose(-2, -1) + (rb.transpose(-1, -2) if mut == 'relb-transposed' else rb)[None]
    if shift and mut != 'no-mask':
        m = so.shift_mask(Hp, Wp, WS, shift) if mut not in ('mask-row-7', 'mask-row-3') else band_mask(Hp, Wp, shift, int(mut == 'mask-row-7'), int(mut == 'mask-row-3'))
        s = s + m.to(dt)[:, None]
    P = torch.softmax(s, -1)
    rnd = (lambda t: t.to(BF16).to(dt)) if mut == 'mfma-roundings' else (lambda t: t)      # the MFMA kernels' operand roundings, in otherwise exact arithmetic
    o = _unheads(rnd(P) @ v)
    if mut == 'window-to-neighbour' and nW > 1:
        o = torch.cat([o[:1], o[:1], o[2:]], 0)
    out = unroll(_reverse(o, Hp, Wp))[:H, :W]
    if dO is None:
        return out
    r = {'out': out, 'out_abs': unroll(_reverse(_unheads(P @ v.abs()), Hp, Wp))[:H, :W]}
    g = _heads(_partition(roll(F.pad(dO, (0, 0, 0, Wp - W, 0, Hp - H)))), heads)          # outputs of pad queries are cropped: their gradient is zero
    dP, dPa = g @ v.transpose(-2, -1), g.abs() @ v.abs().transpose(-2, -1)
    dS = P * (dP - (P * dP).sum(-1, keepdim=True))
    A = P * (dPa + (P * dPa).sum(-1, keepdim=True))
    parts = (scale * (rnd(dS) @ k), scale * (rnd(dS).transpose(-2, -1) @ q), rnd(P).transpose(-2, -1) @ g)
    parts_abs = (scale * (A @ k.abs()), scale * (A.transpose(-2, -1) @ q.abs()), P.transpose(-2, -1) @ g.abs())
    U = (dPa + (P * dPa).sum(-1, keepdim=True)).expand_as(P)              # what a probability lost to underflow would have multiplied in dS
    parts_floor = (scale * (U @ k.abs()), scale * (U.transpose(-2, -1) @ q.abs()), torch.ones_like(P) @ g.abs())
    real = torch.zeros(Hp, Wp, 1, dtype=dt)
    real[:H, :W] = 1
    keep = torch.ones(nW, 1, 1, dtype=dt)
    if last and mut == 'last-window-missing':
        keep[-1] = 0                                                       # a wrong kernel: the last window's share of the two sums is lost
    for name, ps in (('', parts), ('_abs', parts_abs), ('_floor', parts_floor)):
        dwin = torch.cat([_unheads(p) for p in ps], -1)                     # [nW, 49, 3C]
        dcan = unroll(_reverse(dwin, Hp, Wp))
        r['dqkv' + name] = dcan[:H, :W]
        r['dpad' + name] = (unroll(_reverse(dwin * keep, Hp, Wp)) * (1 - real)).sum((0, 1))
    r['drel'], r['drel_abs'] = (dS * keep[:, None]).sum(0), (A * keep[:, None]).sum(0)
    r['drel_floor'] = U.sum(0)
    return r


def pad_bias_of(bias, dtype):
    """What a pad token carries: the qkv bias as the qkv GEMM would have stored it in the tensor type."""
    return bias.to(dtype).to(F32)


def attn_forward(qkv, pad_bias, relb, C, heads, shift, dt=F64, mut=None):
    """The plain, differentiable forward: qkv [B, H, W, >= 3C] -> out [B, H, W, C]."""
    x, pb = qkv[..., :3 * C].to(dt), pad_bias.to(dt)
    return torch.stack([_attn_sample(x[b], pb, relb, C, heads, shift, mut) for b in range(x.shape[0])], 0)


def attention(qkv, pad_bias, relb, dout, C, heads, shift, dt=F64, mut=None):
    """Forward and closed-form backward, sample by sample -> dict of out, dqkv [B, H, W, 3C], drel [heads, 49, 49], dpad [3C] and their R_abs ('*_abs')."""
    B = qkv.shape[0]
    acc = {}
    with torch.no_grad():
        for b in range(B):
            r = _attn_sample(qkv[b, ..., :3 * C].to(dt), pad_bias.to(dt), relb, C, heads, shift, mut, dout[b, ..., :C].to(dt), last=(b == B - 1))
            for key, t in r.items():
                if key.startswith(('drel', 'dpad')):                       # sums over the samples
                    acc[key] = acc[key] + t if key in acc else t
                else:
                    acc.setdefault(key, []).append(t)
    return {key: (torch.stack(t, 0) if isinstance(t, list) else t) for key, t in acc.items()}


def attn_bounds(ref, route, dtype):
    """route: 'valu' (fp32 arithmetic) or 'mfma' (one bf16 rounding of out, dq, dk, dv and the pad sums; none of d rel_bias)."""
    nb, tiny = BF16_U if route == 'mfma' else 0.0, 2.0 ** -126
    return {'out': (K['attn_fwd'] * E24 + nb) * ref['out_abs'] + out_rounding(ref['out'], dtype),
            'dqkv': (K['attn_bwd'] * E24 + nb) * ref['dqkv_abs'] + tiny * ref['dqkv_floor'] + out_rounding(ref['dqkv'], dtype),
            'drel': K['attn_bwd'] * E24 * ref['drel_abs'] + tiny * ref['drel_floor'],
            'dpad': (K['attn_bwd'] * E24 + nb) * ref['dpad_abs'] + tiny * ref['dpad_floor']}


def attn_tasks(B, H, W, heads):
    return B * attn_geom(H, W)[2] * heads


def win_wpb(tasks):
    """Windows a block of the VALU backward walks."""
    return min(16, max(1, tasks // 2048))


def win_wpw(tasks):
    """Windows a WAVEFRONT of the MFMA backward walks (four wavefronts, i.e. four windows, per trip)."""
    return (win_wpb(tasks) + 3) // 4


def attn_route(route, B, H, W, heads):
    """dict: nwin, wpb / wpw, chunks (= sl_window_attention_bwd_chunks), windows of the last chunk, and for MFMA the live wavefronts of the last trip (4 = no tail)."""
    nwin, tasks = B * attn_geom(H, W)[2], attn_tasks(B, H, W, heads)
    if route == 'mfma':
        wpw = win_wpw(tasks)
        per = 4 * wpw
        chunks = -(-nwin // per)
        last = nwin - (chunks - 1) * per
        return dict(nwin=nwin, wpw=wpw, chunks=chunks, last_chunk=last, last_trips=-(-last // 4), tail_waves=last - (last - 1) // 4 * 4)
    wpb = win_wpb(tasks)
    chunks = -(-nwin // wpb)
    return dict(nwin=nwin, wpb=wpb, chunks=chunks, last_chunk=nwin - (chunks - 1) * wpb)


ATTN_ROUTES = {'f32-valu': (F32, 'valu'), 'bf16-valu': (BF16, 'valu'), 'bf16-mfma': (BF16, 'mfma')}
# name: (B, H, W, heads)
ATTN_CASES = {
    'one-window-h1': (1, 7, 7, 1),
    'below-window-4x4': (2, 4, 4, 3),
    'below-window-1x5-h24': (1, 1, 5, 24),
    'nwin1-pad-both-5x6': (1, 5, 6, 3),
    'nwin2-7x14': (1, 7, 14, 3),
    'nwin3-b3-7x7-h12': (3, 7, 7, 12),
    'nwin5-7x35': (1, 7, 35, 3),
    'nwin6-b2-7x15': (2, 7, 15, 3),
    'nwin12-b2-10x15': (2, 10, 15, 3),
    'pad-rows-10x14': (1, 10, 14, 3),
    'pad-cols-14x10-h1': (1, 14, 10, 1),
    'nwin8-b2-10x13': (2, 10, 13, 3),
}
# the two large cases: (B, H, W, heads), routes.  Their values are bf16 numbers in either dtype and their bias is a bf16 number, so one reference serves every route
ATTN_BIG = {
    'wpb2-171-windows': ((1, 61, 130, 24), ('f32-valu', 'bf16-valu')),
    'wpw2-429-windows': ((3, 75, 88, 24), ('bf16-mfma',)),
}


def attn_inputs(name, shape, dtype, exact_bf16=False):
    """qkv [B, H, W, P3] and dout [B, H, W, P] in dtype with zero channel pads, bias [3C], rel_bias [heads, 49, 49] (fp32)."""
    B, H, W, heads = shape
    C = heads * HD
    P, P3 = pad_to(C), pad_to(3 * C)
    src = BF16 if exact_bf16 else dtype
    qkv = padded(randn('attn/qkv/' + name, (B, H, W, 3 * C), src).to(dtype), P3)
    dout = padded(randn('attn/do/' + name, (B, H, W, C), src).to(dtype), P)
    bias = randn('attn/b/' + name, (3 * C,), BF16 if exact_bf16 else F32, 0.5).to(F32)
    relb = randn('attn/rb/' + name, (heads, WN, WN), F32, 0.5)
    return qkv, dout, bias, relb, C, P


def pad_to(c, m=128):
    """The channel pitch of a C-channel map (segland_amd.ops_swin.pad_to)."""
    return c if c % 64 == 0 else (c + m - 1) // m * m


# ------------------------------------------------------------------------------------------------------------ position-table gradient
def table_grad(dbias, dt=F64, pairs_short=False):
    """d relative_position_bias_table [169, heads] from d bias [heads, 49 * 49]: index_add_ through relative_position_index."""
    heads = dbias.shape[0]
    idx = so.relative_position_index(WS).reshape(-1)
    src = dbias.to(dt).t().contiguous()                                   # [pairs, heads]
    if pairs_short:                                                        # a wrong kernel: every pair list short by its last entry
        lastpos = torch.zeros(169, dtype=torch.long).scatter_reduce(0, idx, torch.arange(idx.numel()), 'amax')
        src = src.clone()
        src[lastpos] = 0
    return torch.zeros(169, heads, dtype=dt).index_add_(0, idx, src)


def qkv_bias_grad(dbq_colsum, dpad, heads, dt=F64, wrong_order=False):
    """d qkv.bias [3 * heads * 32] = column sums + the pad-token share dpad [heads, 3, 32] in the bias' (3, heads, 32) order."""
    p = dpad.to(dt).view(heads, 3, HD)
    p = p.reshape(3, heads, HD) if wrong_order else p.permute(1, 0, 2)
    return dbq_colsum.to(dt) + p.reshape(-1)
