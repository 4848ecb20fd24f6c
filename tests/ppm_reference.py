"""The pyramid-pooling kernels of csrc/ppm.hip (and the layout kernels of csrc/conv_weight_prep.hip that feed them) restated with torch's own ops in float64 on the CPU,
the input generators and the elementwise comparators of tests/test_ppm_reference_cpu.py and tests/test_ppm_parity_gpu.py.  Nothing here restates the kernels' index
arithmetic: bins come from F.adaptive_avg_pool*, bilinear weights from F.interpolate applied to an identity, gradients from autograd or from the same matrices transposed.

Layouts (include/segland_hip.h): activations are NHWC; the pooled / stage tensors are rows [sum_l B*s_l*s_l][C], level after level, (b, i, j) row-major inside a level;
the factorised prior operand q has the same rows and columns (ky*3 + kx)*N + n.

Every reference takes the kernel's own inputs AFTER rounding to the kernel's input type (a bf16 tensor is passed as it is and widened here), so input rounding costs no
tolerance.  The comparators bound |kernel - reference| elementwise and are derived from the arithmetic, never from a kernel's output:

* pool forward: integer inputs in -3..3 (exact in bf16) make every cell and bin sum an exact integer below 2^24 (check_pool_input), so the division by the bin area is the
  only rounding: 2^-23 |ref| (one fp32 ulp), exactly 0 where the reference is 0.  A missing or doubled pixel moves a result by >= 1/area.
* pool backward: a sum of the direct gradient and one term per bin that holds the pixel, <= 3 roundings per term: 2^-20 (|dcat| + sum |dpooled_bin| / area), the
  reference evaluated on absolute values; bf16 outputs add 2^-8 |ref| for the final rounding (half a bf16 ulp is 2^-9 of the binade).
* bilinear kernels (upsample, its backward, gather, scatter): 2^-18 max(R_abs) with R_abs the reference on absolute inputs (all weights are >= 0, so it bounds the sum of
  |terms|); the kernels form the source coordinate scale * (dst + 0.5) - 0.5 in fp32, a few ulp of the coordinate.  torch's own fp32 F.interpolate stays inside
  2^-20 max(R_abs) on the CPU (test_ppm_reference_cpu.py), so the bound is neither vacuous nor knife-edge; a wrong cell, weight or border mask is >= 4 orders above it.
  bf16 outputs add 2^-8 |ref|.
* stage BatchNorm + ReLU backward and the rows weight gradient: 1e-5 of the reference tensor's maximum per level (the number of the tests they supplement).
* layout kernels: bit for bit."""
import zlib

import torch
import torch.nn.functional as F

SIZES = (1, 2, 3, 6)
F64 = torch.float64


# ------------------------------------------------------------------------------------------------------------ inputs
def gen(tag):
    g = torch.Generator()
    g.manual_seed(zlib.crc32(tag.encode()))
    return g


def randn(tag, shape, dtype=torch.float32):
    """Normal values rounded to `dtype` (the kernel's input type)."""
    return torch.randn(shape, generator=gen(tag), dtype=torch.float32).to(dtype)


def pool_input(tag, shape, dtype):
    """Integers in -3..3: exact in bf16 and fp32."""
    return torch.randint(-3, 4, shape, generator=gen(tag)).to(dtype)


def rows(B, sizes):
    return B * sum(s * s for s in sizes)


def level_slices(B, sizes):
    out, off = [], 0
    for s in sizes:
        out.append(slice(off, off + B * s * s))
        off += B * s * s
    return out


def to_maps(t_rows, B, sizes):
    """rows [sum B*s*s][C] -> per level NCHW [B][C][s][s] (views)."""
    return [t_rows[sl].reshape(B, s, s, -1).permute(0, 3, 1, 2) for sl, s in zip(level_slices(B, sizes), sizes)]


def to_rows(maps):
    """per level NCHW [B][C][s][s] -> rows."""
    return torch.cat([m.permute(0, 2, 3, 1).reshape(-1, m.shape[1]) for m in maps], 0)


# ------------------------------------------------------------------------------------------------------------ geometry, from torch's own ops
def bin_membership(s, n):
    """[s][n] 0/1 matrix: pixel k lies in bin i of AdaptiveAvgPool(s) over n pixels -- read off F.adaptive_avg_pool1d of an identity."""
    a = F.adaptive_avg_pool1d(torch.eye(n, dtype=F64)[None], s)[0]        # [n (pixel as channel)][s]
    return (a > 0).to(F64).t().contiguous()


def bin_area(s, H, W):
    """[s][s] pixel count of every bin."""
    return bin_membership(s, H).sum(1)[:, None] * bin_membership(s, W).sum(1)[None, :]


def cell_count(sizes, n):
    """Cells of the common refinement of all levels' bin boundaries along an axis of n pixels: runs of pixels with the same bin membership in every level."""
    m = torch.cat([bin_membership(s, n) for s in sizes], 0)              # [sum s][n]
    return 1 + int((m[:, 1:] != m[:, :-1]).any(0).sum())


def interp_matrix(s, n, align_corners=False):
    """U_(s,n) [n][s]: the bilinear resampling of s cells to n pixels, as F.interpolate itself applies it to an identity in float64."""
    e = torch.eye(s, dtype=F64)[None, :, :, None]                        # [1][c = cell][s][1]
    u = F.interpolate(e, size=(n, 1), mode='bilinear', align_corners=align_corners)[0, :, :, 0]      # [cell][n]
    return u.t().contiguous()


def tap_matrices(s, n, interp=interp_matrix, masked=True):
    """S_k [n][s], k = 0..2: row y is U[y + k - 1], zero where y + k - 1 falls outside the map (the 3x3 conv's zero padding).  masked=False clamps instead (a wrong kernel)."""
    u = interp(s, n)
    z = torch.zeros(1, s, dtype=F64)
    p = torch.cat([z if masked else u[:1], u, z if masked else u[-1:]], 0)
    return [p[k:k + n] for k in range(3)]


# ------------------------------------------------------------------------------------------------------------ pool
def pool_fwd(x, sizes):
    """x NHWC (any float dtype) -> pooled rows, float64."""
    xc = x.to(F64).permute(0, 3, 1, 2)
    return to_rows([F.adaptive_avg_pool2d(xc, s) for s in sizes])


def check_pool_input(x, sizes):
    """The input conditions of the pool-forward comparator, on the reference alone: integer inputs with sum |x| over a whole map below 2^24 (so every partial sum of a
    cell or a bin, in any order, is an exact fp32 integer), and reference * bin area an integer."""
    xd = x.to(F64)
    assert bool((xd == xd.round()).all()) and float(xd.abs().max()) <= 3
    B, H, W, _ = x.shape
    assert float(xd.abs().sum((1, 2)).max()) < 2 ** 24                    # any cell / bin partial sum is below this
    ref = pool_fwd(x, sizes)
    for sl, s in zip(level_slices(B, sizes), sizes):
        sums = ref[sl].reshape(B, s, s, -1) * bin_area(s, H, W)[None, :, :, None]
        assert float((sums - sums.round()).abs().max()) < 1e-9


def pool_bwd(dpooled, x_shape, sizes, dcat=None, cat_off=0):
    """Gradient wrt x of <pool_fwd(x), dpooled>, plus the concat slice dcat[..., cat_off : cat_off + C]; float64 NHWC."""
    B, H, W, C = x_shape
    x = torch.zeros(B, C, H, W, dtype=F64, requires_grad=True)
    pooled = to_rows([F.adaptive_avg_pool2d(x, s) for s in sizes])
    g, = torch.autograd.grad(pooled, x, dpooled.to(F64))
    g = g.permute(0, 2, 3, 1)
    if dcat is not None:
        g = g + dcat.to(F64)[..., cat_off:cat_off + C]
    return g.contiguous()


# ------------------------------------------------------------------------------------------------------------ upsample
def upsample_fwd(stage, x_shape, sizes):
    """stage rows [.][Cs] -> priors NHWC [B][H][W][nl*Cs], level-major channels; F.interpolate(bilinear, align_corners=False) in float64."""
    B, H, W, _ = x_shape
    ups = [F.interpolate(m, size=(H, W), mode='bilinear', align_corners=False) for m in to_maps(stage.to(F64), B, sizes)]
    return torch.cat(ups, 1).permute(0, 2, 3, 1).contiguous()


def upsample_bwd(dcat, x_shape, sizes, Cs):
    """Gradient wrt the stage rows of <upsample_fwd(stage), dcat[..., : nl*Cs]>, by autograd of F.interpolate."""
    B, H, W, _ = x_shape
    stage = torch.zeros(rows(B, sizes), Cs, dtype=F64, requires_grad=True)
    g, = torch.autograd.grad(upsample_fwd(stage, x_shape, sizes), stage, dcat.to(F64)[..., :len(sizes) * Cs])
    return g


def upsample_fwd_mat(stage, x_shape, sizes, interp=interp_matrix):
    """upsample_fwd written with the matrices U (the form the gather builds on); `interp` may be a deliberately wrong matrix in the sharpness tests."""
    B, H, W, _ = x_shape
    outs = []
    for m, s in zip(to_maps(stage.to(F64), B, sizes), sizes):
        outs.append(torch.einsum('yi,xj,bcij->byxc', interp(s, H), interp(s, W), m))
    return torch.cat(outs, 3)


# ------------------------------------------------------------------------------------------------------------ factorised prior gather / scatter
def fact_gather(q, x_shape, sizes, N, taps=tap_matrices):
    """out[b,y,x,n] = sum_l sum_(ky,kx) sum_(i,j) Sy_ky[y,i] Sx_kx[x,j] q_l[b,i,j,ky,kx,n]; float64 NHWC."""
    B, H, W, _ = x_shape
    out = torch.zeros(B, H, W, N, dtype=F64)
    for sl, s in zip(level_slices(B, sizes), sizes):
        ql = q[sl].to(F64).reshape(B, s, s, 3, 3, N)
        sy, sx = taps(s, H), taps(s, W)
        for ky in range(3):
            for kx in range(3):
                out += torch.einsum('yi,xj,bijn->byxn', sy[ky], sx[kx], ql[:, :, :, ky, kx])
    return out


def fact_scatter(dcb, x_shape, sizes, taps=tap_matrices):
    """The exact transpose: gq_l[b,i,j,ky,kx,n] = sum_(y,x) Sy_ky[y,i] Sx_kx[x,j] dcb[b,y,x,n]; float64 rows [.][9N]."""
    B, H, W, _ = x_shape
    d = dcb.to(F64)
    N = d.shape[-1]
    out = []
    for s in sizes:
        sy, sx = taps(s, H), taps(s, W)
        g = torch.zeros(B, s, s, 3, 3, N, dtype=F64)
        for ky in range(3):
            for kx in range(3):
                g[:, :, :, ky, kx] = torch.einsum('yi,xj,byxn->bijn', sy[ky], sx[kx], d)
        out.append(g.reshape(B * s * s, 9 * N))
    return torch.cat(out, 0)


# ------------------------------------------------------------------------------------------------------------ stage BatchNorm + ReLU backward
def stage_bn_inputs(tag, B, C, sizes, trains, no_gamma=()):
    """fp32 x, dy, y = relu(gamma * xhat + beta) and per level mean / invstd / gamma (None for the levels in no_gamma).  Train levels carry the batch statistics of their
    rows, eval levels arbitrary 'running' ones."""
    n = rows(B, sizes)
    x, dy = randn(tag + '/x', (n, C)), randn(tag + '/dy', (n, C))
    y = torch.empty_like(x)
    means, invs, gammas = [], [], []
    for l, sl in enumerate(level_slices(B, sizes)):
        if trains[l]:
            m, v = x[sl].mean(0), x[sl].var(0, unbiased=False)
        else:
            m, v = 0.3 * randn('%s/rm%d' % (tag, l), (C,)), torch.rand(C, generator=gen('%s/rv%d' % (tag, l))) + 0.5
        i = (v + 1e-5).rsqrt()
        g = None if l in no_gamma else torch.rand(C, generator=gen('%s/g%d' % (tag, l))) + 0.5
        y[sl] = torch.relu((x[sl] - m) * i * (g if g is not None else 1.0) + 0.1)
        means.append(m.contiguous()); invs.append(i.contiguous()); gammas.append(g)
    return x, dy, y, means, invs, gammas


def stage_bn_bwd(dy, y, x, B, sizes, means, invs, gammas, trains):
    """The closed form in float64 from the fp32 tensors the kernel receives -> (dx rows, [dgamma per level], [dbeta per level])."""
    dx = torch.empty(x.shape, dtype=F64)
    dgs, dbs = [], []
    for l, sl in enumerate(level_slices(B, sizes)):
        mu, is_ = means[l].to(F64), invs[l].to(F64)
        gm = gammas[l].to(F64) if gammas[l] is not None else torch.ones_like(mu)
        g = dy[sl].to(F64) * (y[sl] > 0)
        xhat = (x[sl].to(F64) - mu) * is_
        n = g.shape[0]
        dbeta, dgamma = g.sum(0), (g * xhat).sum(0)
        dx[sl] = gm * is_ * (g - dbeta / n - xhat * dgamma / n) if trains[l] else gm * is_ * g
        dgs.append(dgamma); dbs.append(dbeta)
    return dx, dgs, dbs


def rows_wgrad(a, x, B, sizes):
    """dw[l][n][k] = sum over level l's rows of a[r][n] x[r][k]; float64."""
    return [torch.einsum('rn,rk->nk', a[sl].to(F64), x[sl].to(F64)) for sl in level_slices(B, sizes)]


# ------------------------------------------------------------------------------------------------------------ layout kernels (bit for bit)
def wq_layouts(w, Cs, nl):
    """OIHW [N][Ctot][3][3] -> wq_f [nl][9N][Cs] with wq_f[l][tap*N+n][c] = W[n][l*Cs+c][tap], and wq_b [nl][Cs][9N] holding the same values."""
    N = w.shape[0]
    v = w[:, :nl * Cs].reshape(N, nl, Cs, 9)                             # [n][l][c][tap]
    wq_f = v.permute(1, 3, 0, 2).reshape(nl, 9 * N, Cs).contiguous()
    return wq_f, wq_f.permute(0, 2, 1).contiguous()


def dwq_scatter(dwq, dw, Cs, nl):
    """dw[n][l*Cs+c][tap] = dwq[l][tap*N+n][c]; the columns >= nl*Cs of dw stay as they are.  Returns a new tensor."""
    N = dw.shape[0]
    out = dw.clone()
    out[:, :nl * Cs] = dwq.reshape(nl, 9, N, Cs).permute(2, 0, 3, 1).reshape(N, nl * Cs, 9).reshape(N, nl * Cs, 3, 3)
    return out


def slice_layouts(w, dtype, ci_off, ci_cnt):
    """The input-channel slice of an OIHW weight as wf [O][KH][KW][ci] and wb [ci][KH][KW][O], rounded once to dtype."""
    v = w[:, ci_off:ci_off + ci_cnt].to(dtype)
    return v.permute(0, 2, 3, 1).contiguous(), v.permute(1, 2, 3, 0).contiguous()


# ------------------------------------------------------------------------------------------------------------ comparators
def worst_ratio(what, got, ref, bound):
    """max over the elements of |got - ref| / bound (bound: a float64 tensor like ref, or a number); an element with bound 0 must be exact.  Prints the figure."""
    got, ref = got.to(F64), ref.to(F64)
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    assert bool(torch.isfinite(got).all()), what + ': non-finite result'
    err = (got - ref).abs()
    b = bound if isinstance(bound, torch.Tensor) else torch.full_like(ref, float(bound))
    ratio = torch.where(b > 0, err / b.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float('inf')), torch.zeros_like(err)))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print('%s: worst error/bound %.3g (max error %.3g, max |ref| %.3g)' % (what, worst, float(err.max()), float(ref.abs().max())))
    return worst


def out_rounding(ref, dtype):
    """The one final rounding of a bf16 output: 2^-8 |ref|; nothing for fp32."""
    return 2.0 ** -8 * ref.abs() if dtype == torch.bfloat16 else torch.zeros_like(ref)


def pool_fwd_bound(ref):
    return 2.0 ** -23 * ref.abs()


def pool_bwd_bound(ref, ref_abs, dtype):
    return 2.0 ** -20 * ref_abs + out_rounding(ref, dtype)


def bilinear_bound(ref, ref_abs, dtype=torch.float32):
    return 2.0 ** -18 * float(ref_abs.max()) + out_rounding(ref, dtype)


def max_bound(ref, tol=1e-5):
    return tol * float(ref.abs().max())


def stage_bn_dx_bound(ref, dy, y, inv, gamma, train):
    """1e-5 of the level's maximum.  A one-row level in train mode has the reference 0 identically: xhat = 0 and g - dbeta/1 = 0.  The kernel forms
    dx = cA g + cB (x - mean) + cC with cA = fl(gamma is), cC = fl(-gamma is dbeta / 1), dbeta = g and x - mean = 0 exactly, i.e. gamma is g [(1+e1)(1+e2) - (1+e3)] with
    |e| <= 2^-24: at most 3 * 2^-24 |gamma is g|, bounded here by 2^-22 |gamma is g| elementwise."""
    if train and ref.shape[0] == 1:
        assert float(ref.abs().max()) == 0.0
        gm = gamma.to(F64) if gamma is not None else 1.0
        return 2.0 ** -22 * (gm * inv.to(F64) * dy.to(F64) * (y > 0)).abs()
    return max_bound(ref)


# ------------------------------------------------------------------------------------------------------------ cases: id -> shape, and the route each one reaches
# Dispatch conditions as csrc/ppm.hip and csrc/conv_weight_prep.hip state them, evaluated in plain Python so that a case id's route is checked, not assumed.
DTYPES = {'f32': torch.float32, 'bf16': torch.bfloat16}


def pool_fwd_route(dtype, B, H, W, C, sizes):
    """sl_ppm_pool_fwd: bf16 with fewer than 262144 (cell, 8-channel vector) pairs -> ppm_cells_rows_kernel, else ppm_cells_kernel<T>."""
    vecs = B * cell_count(sizes, H) * cell_count(sizes, W) * (C // 8)
    return 'rows' if dtype == torch.bfloat16 and vecs < 256 * 1024 else 'cells'


def pool_bwd_route(C, sizes):
    """ppm_pool_bwd_cells_kernel: the wavefront-shuffle route needs C % 64 == 0 and at most 64 bins."""
    return 'wave' if C % 64 == 0 and sum(s * s for s in sizes) <= 64 else 'scalar'


def scatter_route(dtype, H, W, N, sizes, walk_hook=True):
    """sl_ppm_fact_scatter: the sliding-window kernels need the hook on, W <= 64, an even N and no level finer than the map; the general stage A shares weights across a
    wavefront when N / (elements per 16 bytes) % 64 == 0, the general stage B when N % 64 == 0."""
    if walk_hook and W <= 64 and N % 2 == 0 and all(s <= W and s <= H for s in sizes):
        return 'walk'
    v = 8 if dtype == torch.bfloat16 else 4
    return 'general:A-%s:B-%s' % ('wave' if (N // v) % 64 == 0 else 'scalar', 'wave' if N % 64 == 0 else 'scalar')


def slice_route(O, ci_off, ci_cnt, taps):
    """sl_weight_prep_slice: 64 x 32 tiles when O % 64 == 0, ci_cnt % 32 == 0, ci_off % 4 == 0 and at most 9 taps; else one thread per element."""
    return 'tiled' if O % 64 == 0 and ci_cnt % 32 == 0 and ci_off % 4 == 0 and taps <= 9 else 'scalar'


def stage_bn_trips(B, s):
    """ppm_stage_bn_bwd_kernel sums a level's rows 128 per trip (32 row lanes x 4 rows in flight): (trips, rows of the last trip)."""
    n = B * s * s
    return (n + 127) // 128, n - (n - 1) // 128 * 128


# (B, H, W, C), sizes, {dtype name: route}
POOL_FWD_CASES = {
    'one-pixel': ((1, 1, 1, 8), SIZES, {'f32': 'cells', 'bf16': 'rows'}),
    'bins-overlap-nv9': ((2, 5, 4, 72), SIZES, {'f32': 'cells', 'bf16': 'rows'}),
    'ragged-11x10-cells': ((3, 13, 22, 128), SIZES, {'f32': 'cells', 'bf16': 'rows'}),
    'row-lanes-wrap': ((1, 64, 40, 64), SIZES, {'f32': 'cells', 'bf16': 'rows'}),
    'b8-below-threshold': ((8, 13, 13, 2048), SIZES, {'f32': 'cells', 'bf16': 'rows'}),
    'b9-above-threshold': ((9, 13, 13, 2048), SIZES, {'f32': 'cells', 'bf16': 'cells'}),
}
# (B, H, W, C), sizes, route of ppm_pool_bwd_cells_kernel
POOL_BWD_CASES = {
    'one-pixel-scalar': ((1, 1, 1, 8), SIZES, 'scalar'),
    'bins-overlap-c72-scalar': ((2, 5, 4, 72), SIZES, 'scalar'),
    'bins-overlap-c64-wave': ((2, 5, 4, 64), SIZES, 'wave'),
    'ragged-c128-wave': ((3, 13, 22, 128), SIZES, 'wave'),
    'ragged-c72-scalar': ((3, 13, 22, 72), SIZES, 'scalar'),
    'tall-cells-c64-wave': ((1, 64, 40, 64), SIZES, 'wave'),
    '78-bins-c64-scalar': ((2, 13, 22, 64), (1, 2, 3, 8), 'scalar'),
    'w260-fill-loop-wave': ((1, 2, 260, 64), SIZES, 'wave'),
}
POOL_BWD_DCAT = {'none': None, 'off0': 0, 'off64': 64}                    # concat offset; the pitch is cat_off + C + 24
# (B, H, W)
UPSAMPLE_MAPS = {'5x4': (2, 5, 4), '6x6-identity-level': (2, 6, 6), '13x22': (2, 13, 22), '1x1': (2, 1, 1), '64x40': (1, 64, 40)}
UPSAMPLE_CS = (8, 64)
# (B, H, W), {dtype name: N}, walk hook, {dtype name: route}
FACT_CASES = {
    'walk-6x6-n8': ((1, 6, 6), {'f32': 8, 'bf16': 8}, True, {'f32': 'walk', 'bf16': 'walk'}),
    'walk-7x9': ((2, 7, 9), {'f32': 64, 'bf16': 64}, True, {'f32': 'walk', 'bf16': 'walk'}),
    'walk-w64-full-table': ((1, 64, 64), {'f32': 64, 'bf16': 64}, True, {'f32': 'walk', 'bf16': 'walk'}),
    'walk-h66': ((1, 66, 6), {'f32': 64, 'bf16': 64}, True, {'f32': 'walk', 'bf16': 'walk'}),
    'general-scalar-AB-n72': ((2, 5, 4), {'f32': 72, 'bf16': 72}, True, {'f32': 'general:A-scalar:B-scalar', 'bf16': 'general:A-scalar:B-scalar'}),
    'general-wave-B': ((2, 5, 4), {'f32': 64, 'bf16': 64}, True, {'f32': 'general:A-scalar:B-wave', 'bf16': 'general:A-scalar:B-wave'}),
    'general-wave-A-two-chunks-w66': ((1, 6, 66), {'f32': 256, 'bf16': 512}, True, {'f32': 'general:A-wave:B-wave', 'bf16': 'general:A-wave:B-wave'}),
    'general-by-hook-wave-B-two-chunks-h66': ((1, 66, 6), {'f32': 64, 'bf16': 64}, False, {'f32': 'general:A-scalar:B-wave', 'bf16': 'general:A-scalar:B-wave'}),
}
# B, C, train flag per level, levels without gamma
STAGE_BN_CASES = {
    # B = 1: the first level is one row (count = 1).  In eval mode it is an ordinary level; in train mode the gradient of a BatchNorm over one value is 0 identically
    # (torch refuses that forward), 1e-5 of the tensor's maximum is then 0 and stage_bn_dx_bound states what the kernel's three-term form can keep instead
    'b1-c32-one-row-level': (1, 32, (False, True, True, True), ()),
    'b1-c32-one-row-level-train': (1, 32, (True, True, False, True), ()),
    'b5-c128': (5, 128, (True, False, True, True), ()),
    'b16-c96-five-trips': (16, 96, (True, True, False, True), ()),
    'b16-c96-all-train-no-gamma-level2': (16, 96, (True, True, True, True), (2,)),
}
ROWS_WGRAD_CASES = {'b1-one-row-level': (1, 128, 64), 'b16': (16, 128, 64)}          # B, N, K
WQ_CASES = {'n64-cs32-4-levels': (64, 32, 4, 160), 'n128-cs64-3-of-5-slices': (128, 64, 3, 256 + 64)}      # N, Cs, nl, Ctot
# O, CinTot, ci_off, ci_cnt, route
SLICE_CASES = {
    'tiled': (64, 192, 128, 32, 'tiled'),
    'scalar-o48': (48, 192, 128, 32, 'scalar'),
    'scalar-off6-cnt40': (64, 192, 6, 40, 'scalar'),
}
