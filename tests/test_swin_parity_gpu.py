"""Every route of the Swin kernels (csrc/swin.hip) through segland_amd.ops_swin against the float64 references of tests/swin_reference.py on the kernel's own (rounded)
inputs, inside the derived elementwise bounds stated there (data-moving kernels: bit for bit).  The case tables, with the dispatch condition of every route, live in
swin_reference.py; tests/test_swin_reference_cpu.py checks those conditions, the references and the comparators' sharpness without a GPU.  Each test prints its worst
error / bound ratio (SEGLAND_PARITY_LOG collects them: profiles/parity_swin.txt)."""
import ctypes as C

import pytest
import torch

import swin_reference as sr
from swin_reference import BF16, F32, F64

pytestmark = pytest.mark.gpu
DEV = 'cuda'
DT = sorted(sr.DTYPES)
_cache = {}


def cached(key, make):
    """References and inputs are built once per key, shared and never modified."""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def dev(t):
    return None if t is None else t.to(DEV).contiguous()


def cpu(t):
    return t.detach().cpu()


def zero_pad(what, t, C):
    """The channel pad of an output is exactly zero."""
    n = int((cpu(t)[..., C:] != 0).sum()) if t.shape[-1] > C else 0
    print('%s: %d nonzero pad elements' % (what, n))
    return n == 0


# ------------------------------------------------------------------------------------------------------------ the route tables against the library
def test_route_restatements_equal_the_library(hip):
    from segland_amd import ops_swin as osw
    from segland_amd.ops import dt
    for name, (d, B, n, Cn, px, py, family, opts) in sr.LN_CASES.items():
        dtype = sr.DTYPES[d]
        assert hip.sl_layernorm_bwd_rows(dt(dtype), B * n, Cn, py) == sr.ln_bwd_blocks(dtype, B * n, py), name
    cases = list(sr.ATTN_CASES.items()) + [(k, v[0]) for k, v in sr.ATTN_BIG.items()]
    for name, (B, H, W, heads) in cases:
        Cn = heads * 32
        for route, (dtype, kind) in sr.ATTN_ROUTES.items():
            d = osw.win_desc(dtype, B, H, W, Cn, heads, sr.pad_to(3 * Cn), sr.pad_to(Cn), 3)
            if route == 'bf16-valu':
                hip.sl_debug_attn_valu(1)
            try:
                chunks, nwin = hip.sl_window_attention_bwd_chunks(C.byref(d)), hip.sl_window_attention_windows(C.byref(d))
            finally:
                hip.sl_debug_attn_valu(-1)
            r = sr.attn_route(kind, B, H, W, heads)
            assert (chunks, nwin) == (r['chunks'], r['nwin']), (name, route, chunks, nwin, r)


# ------------------------------------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize('name', sorted(sr.LN_CASES))
def test_layernorm(hip, name):
    """layernorm_fwd_kernel<T, LPR, NVL>, layernorm_bwd_kernel<T, LPR, NV> (+ layernorm_bwd_cols_kernel) against F.layer_norm and its autograd in float64."""
    from segland_amd import ops_swin as osw
    c = cached(('ln', name), lambda: sr.ln_case(name))
    x, g, b, Cn, dtype, opts, py = c['x'], c['gamma'], c['beta'], c['C'], c['dtype'], c['opts'], c['py']
    tag = 'layernorm %s fwd%s' % (name, sr.ln_fwd_route(dtype, Cn, py))
    ref = cached(('ln/fwd', name), lambda: sr.ln_fwd(x, g, b, Cn))
    y, st = osw.layernorm_fwd(dev(x), dev(g), dev(b), Cn, out_pitch=py, want_stats='nostats' not in opts)
    assert y.dtype == dtype and tuple(y.shape) == (c['B'], c['n'], py)
    ok = sr.worst_ratio(tag + ' y', cpu(y)[..., :Cn], ref[0], sr.ln_fwd_bound(x, g, b, Cn, ref[0], dtype, c['family'])) <= 1
    ok &= zero_pad(tag + ' y', y, Cn)
    if 'nostats' in opts:
        assert st is None
    else:
        bm, br = sr.ln_stats_bounds(x, Cn)
        s = cpu(st).view(c['B'], c['n'], 2)
        ok &= sr.worst_ratio(tag + ' mean', s[..., 0], ref[1], bm) <= 1
        ok &= sr.worst_ratio(tag + ' rstd', s[..., 1], ref[2], br) <= 1
    assert ok
    if 'fwdonly' in opts:
        return
    kind, lpr, nv, grid, trips = sr.ln_bwd_route(dtype, c['rows'], Cn, py, 'noparam' not in opts)
    tag = 'layernorm %s bwd %s (%d, %d) %d blocks %d trips' % (name, kind, lpr, nv, grid, trips)
    dy, add, rs = c['dy'], c['addend'], c['row_scale']
    refs = cached(('ln/bwd', name), lambda: sr.ln_bwd(dy, x, g, Cn, add))
    bdx, bdg, bdb = sr.ln_bwd_bounds(dy, x, g, Cn, add, refs, dtype)
    stats = torch.stack([ref[1], ref[2]], -1).to(F32).view(-1, 2)            # the float64 statistics rounded to the kernel's input type
    dx, dg, db = osw.layernorm_bwd(dev(dy), dev(x), dev(g), dev(stats), Cn, addend=dev(add), want_param_grads='noparam' not in opts, dx_pitch=py, row_scale=dev(rs))
    dx2 = None
    if rs is not None:
        dx, dx2 = dx
    assert dx.dtype == dtype and tuple(dx.shape) == (c['B'], c['n'], py)
    ok = sr.worst_ratio(tag + ' dx', cpu(dx)[..., :Cn], refs[0], bdx) <= 1
    ok &= zero_pad(tag + ' dx', dx, Cn)
    if 'noparam' in opts:
        assert dg is None and db is None
    else:
        ok &= sr.worst_ratio(tag + ' dgamma', cpu(dg), refs[1], bdg) <= 1
        ok &= sr.worst_ratio(tag + ' dbeta', cpu(db), refs[2], bdb) <= 1
    if rs is not None:
        scale = rs.to(F64).view(-1, 1, 1)
        r2 = refs[0].to(dtype).to(F64) * scale
        ok &= sr.worst_ratio(tag + ' dx * row_scale', cpu(dx2)[..., :Cn], r2, bdx * scale.abs() + sr.out_rounding(r2, dtype)) <= 1
        ok &= zero_pad(tag + ' dx * row_scale', dx2, Cn)
        assert float(cpu(dx2)[0].abs().max()) == 0.0 and torch.equal(cpu(dx2)[1], cpu(dx)[1])          # scale 0 and scale 1 are exact
    assert ok


# ------------------------------------------------------------------------------------------------------------ GELU, scale_add
@pytest.mark.parametrize('size,d', [(s, d) for s in sorted(sr.GELU_SIZES) for d in DT if (s, d) != ('second-trip', 'f32')])
def test_gelu(hip, size, d):
    """gelu_fwd_kernel / gelu_bwd_kernel against F.gelu and its autograd in float64; the second grid-stride trip once, in bf16."""
    from segland_amd import ops_swin as osw
    dtype, n = sr.DTYPES[d], sr.GELU_SIZES[size]
    assert (sr.ew_trips(n // sr.vec(dtype)) == 2) == (size == 'second-trip')
    h = cached(('gelu/h', size, d), lambda: sr.gelu_input('gelu/%s/%s' % (size, d), n, dtype))
    dy = cached(('gelu/dy', size, d), lambda: sr.randn('gelu/dy/%s/%s' % (size, d), (n,), dtype))
    ref, refb = sr.gelu_fwd(h), sr.gelu_bwd(h, dy)
    hg = dev(h)
    ok = sr.worst_ratio('gelu forward %s %s' % (size, d), cpu(osw.gelu_fwd(hg)), ref, sr.gelu_fwd_bound(h, ref, dtype)) <= 1
    ok &= sr.worst_ratio('gelu backward %s %s' % (size, d), cpu(osw.gelu_bwd(hg, dev(dy))), refb, sr.gelu_bwd_bound(h, dy, refb, dtype)) <= 1
    assert ok


@pytest.mark.parametrize('name,d', [(n, d) for n in sorted(sr.SCALE_ADD_CASES) for d in DT] + [('second-trip', 'bf16')])
def test_scale_add(hip, name, d):
    """scale_add_kernel in both modes, bit for bit on exact inputs; the channel pad of the per-channel mode is zero (it is part of the reference)."""
    from segland_amd import ops_swin as osw
    dtype = sr.DTYPES[d]
    spec = None
    if name == 'second-trip':
        spec = sr.SCALE_ADD_BIG
        assert sr.ew_trips(spec[0] * spec[1] * spec[3] // sr.vec(dtype)) == 2
    x, sc, add, Cn, pc = cached(('sa', name, d), lambda: sr.scale_add_case(name, dtype, spec))
    ref = sr.scale_add(x, sc, add, Cn, pc)
    sr.check_exact(ref, name)
    got = osw.scale_add(dev(x), dev(sc), dev(add), per_channel=pc, Cn=Cn)
    assert got.dtype == dtype and sr.bit_equal('scale_add %s %s' % (name, d), cpu(got), ref) == 0


# ------------------------------------------------------------------------------------------------------------ patch embedding, im2col, patch merging
@pytest.mark.parametrize('d', DT)
@pytest.mark.parametrize('name', sorted(sr.PATCH_CASES))
def test_patch_embed(hip, name, d):
    """patch_embed_fwd_kernel against F.conv2d of the padded image; patch_im2col_kernel bit for bit; patch_embed_bwd (im2col + weight-gradient GEMM) against autograd."""
    from segland_amd import _lib
    from segland_amd import ops_swin as osw
    from segland_amd.ops import _p, _s, dt
    B, H, W, Cn, P = sr.PATCH_CASES[name]
    dtype = sr.DTYPES[d]
    img, w, b = cached(('pe', name), lambda: (sr.randn('pe/i/' + name, (B, 3, H, W)), sr.randn('pe/w/' + name, (Cn, 3, 4, 4), F32, 0.2), sr.randn('pe/b/' + name, (Cn,))))
    ref, ra = cached(('pe/ref', name), lambda: (sr.patch_embed_fwd(img, w, b), sr.patch_embed_abs(img, w, b)))
    y = osw.patch_embed_fwd(dev(img), dev(w), dev(b), dtype, P)
    assert y.dtype == dtype and tuple(y.shape) == tuple(ref.shape[:3]) + (P,)
    ok = sr.worst_ratio('patch_embed forward %s %s' % (name, d), cpu(y)[..., :Cn], ref, sr.K['patch'] * sr.E24 * ra + sr.out_rounding(ref, dtype)) <= 1
    ok &= zero_pad('patch_embed forward %s %s' % (name, d), y, Cn)
    # im2col, bit for bit on quarter-integers
    qi = cached(('pe/qi', name), lambda: sr.ints('ic/' + name, (B, 3, H, W), F32, -64, 64, 0.25))
    cref = sr.patch_im2col(qi)
    sr.check_exact(cref, name)
    col = torch.full((cref.shape[0], 64), 7.0, dtype=dtype, device=DEV)
    _lib.check(_lib.lib().sl_patch_im2col(dt(dtype), _p(dev(qi)), _p(col), B, H, W, _s()), 'patch_im2col')
    ok &= sr.bit_equal('patch_im2col %s %s' % (name, d), cpu(col), cref) == 0
    # weight and bias gradient end to end
    dy = cached(('pe/dy', name, d), lambda: sr.padded(sr.randn('pe/dy/' + name, tuple(ref.shape[:3]) + (Cn,), dtype), P))
    rw, rb = cached(('pe/bwd', name, d), lambda: sr.patch_embed_bwd(img, dy, Cn))
    bw, bb = sr.patch_bwd_bounds(img, dy, Cn, dtype)
    dw, db = osw.patch_embed_bwd(dev(img), dev(dy), Cn)
    ok &= sr.worst_ratio('patch_embed backward dw %s %s' % (name, d), cpu(dw), rw, bw) <= 1
    ok &= sr.worst_ratio('patch_embed backward db %s %s' % (name, d), cpu(db), rb, bb) <= 1
    assert ok


@pytest.mark.parametrize('d', DT)
@pytest.mark.parametrize('name', sorted(sr.MERGE_CASES))
def test_patch_merge(hip, name, d):
    """merge_gather_kernel / merge_scatter_kernel bit for bit against the reference module's slicing and its autograd; scatter's channel pad is zero."""
    from segland_amd import ops_swin as osw
    B, H, W, Cn, P = sr.MERGE_CASES[name]
    dtype = sr.DTYPES[d]
    x = cached(('mg/x', name, d), lambda: sr.padded(sr.ints('mg/' + name, (B, H, W, Cn), dtype), P))
    ref = sr.merge_gather(x, Cn)
    sr.check_exact(ref, name)
    got = osw.merge_gather(dev(x), Cn)
    assert got.dtype == dtype
    ok = sr.bit_equal('merge gather %s %s' % (name, d), cpu(got), ref) == 0
    dxm = cached(('mg/d', name, d), lambda: sr.ints('ms/' + name, (B, (H + 1) // 2, (W + 1) // 2, 4 * Cn), dtype))
    refs = sr.merge_scatter(dxm, (B, H, W, P), Cn)
    sr.check_exact(refs, name)
    gots = osw.merge_scatter(dev(dxm), (B, H, W, P), Cn)
    ok &= sr.bit_equal('merge scatter %s %s (pad included)' % (name, d), cpu(gots), refs) == 0
    assert ok


# ------------------------------------------------------------------------------------------------------------ bilinear
def _window_bound(shape, inner, off):
    """A bound for a whole tensor whose channel window [off, off + Cn) was written: `inner` inside, 0 (bit-exact, untouched) outside."""
    b = torch.zeros(shape, dtype=F64)
    b[..., off:off + inner.shape[-1]] = inner
    return b


@pytest.mark.parametrize('align', [False, True])
@pytest.mark.parametrize('types', sorted(sr.BIL_TYPES))
def test_bilinear_forward(hip, types, align):
    """bilinear_fwd_kernel<T, TS> against F.interpolate in float64: every geometry plain, then channel windows, accumulate and base on one of them."""
    from segland_amd import ops_swin as osw
    T, TS = sr.BIL_TYPES[types]
    ok, plain = True, {}
    for name, (B, h, w, H, W) in sr.BIL_GEOM.items():
        x = cached(('bl/x', name, TS), lambda: sr.randn('bl/' + name, (B, h, w, 32), TS))
        ref, ra = cached(('bl/ref', name, TS, align), lambda: (sr.bilinear_fwd(x, (H, W), align), sr.bilinear_fwd(x.abs(), (H, W), align)))
        plain[name] = (x, ref, ra)
        out = torch.full((B, H, W, 32), 7.0, dtype=T, device=DEV)
        osw.bilinear_fwd(dev(x), (H, W), align, out=out)
        ok &= sr.worst_ratio('bilinear forward %s %s align %d' % (name, types, align), cpu(out), ref, sr.bilinear_bound(ref, ra, T)) <= 1
    B, h, w, H, W = sr.BIL_GEOM['up-4x5-8x10']
    x, ref, ra = plain['up-4x5-8x10']
    refw, raw = sr.bilinear_fwd(x, (H, W), align, 16, 8), sr.bilinear_fwd(x.abs(), (H, W), align, 16, 8)
    pre = cached(('bl/pre', T), lambda: sr.randn('bl/pre', (B, H, W, 48), T))
    for acc in (False, True):
        out = dev(pre).clone()
        osw.bilinear_fwd(dev(x), (H, W), align, out=out, out_off=16, Cn=16, src_off=8, accumulate=acc)
        want = sr.window_put(pre.to(F64), refw, 16, acc)
        inner = sr.bilinear_bound(want[..., 16:32], raw + (pre.to(F64)[..., 16:32].abs() if acc else 0.0), T)
        ok &= sr.worst_ratio('bilinear forward window src 8 dst 16 accumulate %d %s align %d' % (acc, types, align), cpu(out), want, _window_bound(want.shape, inner, 16)) <= 1
    base = cached(('bl/base', T), lambda: sr.randn('bl/base', (B, H, W, 32), T))
    out = torch.full((B, H, W, 32), 7.0, dtype=T, device=DEV)
    osw.bilinear_fwd(dev(x), (H, W), align, out=out, base=dev(base))
    want = base.to(F64) + ref
    ok &= sr.worst_ratio('bilinear forward base %s align %d' % (types, align), cpu(out), want, sr.bilinear_bound(want, ra + base.to(F64).abs(), T)) <= 1
    assert ok


@pytest.mark.parametrize('align', [False, True])
@pytest.mark.parametrize('types', sorted(sr.BIL_TYPES))
@pytest.mark.parametrize('name', sorted(sr.BIL_BWD_CASES))
def test_bilinear_backward(hip, name, types, align):
    """bilinear_bwd_small_kernel<T, TS> / bilinear_bwd_kernel<T, TS> against the autograd of F.interpolate in float64."""
    from segland_amd import ops_swin as osw
    (B, h, w, H, W), nv, route, opts = sr.BIL_BWD_CASES[name]
    T, TS = sr.BIL_TYPES[types]
    Cn = nv * sr.vec(T)
    assert sr.bilinear_bwd_route(T, B, h, w, H, W, Cn) == route
    dy_off, out_off = (16, 8) if 'window' in opts else (0, 0)
    Pd, Po = (Cn + 32, Cn + 16) if 'window' in opts else (Cn, Cn)
    acc = 'accumulate' in opts
    dy = cached(('blb/dy', name, T), lambda: sr.randn('blb/' + name, (B, H, W, Pd), T))
    pre = cached(('blb/pre', name, TS), lambda: sr.randn('blb/pre/' + name, (B, h, w, Po), TS))
    ref, ra = cached(('blb/ref', name, T, align), lambda: (sr.bilinear_bwd(dy, (h, w), align, Cn, dy_off), sr.bilinear_bwd(dy.abs(), (h, w), align, Cn, dy_off)))
    out = dev(pre).clone()
    osw.bilinear_bwd(dev(dy), (h, w), align, out=out, out_off=out_off, Cn=Cn, dy_off=dy_off, accumulate=acc)
    want = sr.window_put(pre.to(F64), ref, out_off, acc)
    inner = sr.bilinear_bound(want[..., out_off:out_off + Cn], ra + (pre.to(F64)[..., out_off:out_off + Cn].abs() if acc else 0.0), TS)
    assert sr.worst_ratio('bilinear backward %s [%s] %s align %d' % (name, route, types, align), cpu(out), want, _window_bound(want.shape, inner, out_off)) <= 1


# ------------------------------------------------------------------------------------------------------------ window attention
def _attention(hip, name, shape, route, shift, exact=False):
    from segland_amd import ops_swin as osw
    dtype, kind = sr.ATTN_ROUTES[route]
    B, H, W, heads = shape
    qkv, dout, bias, relb, Cn, P = cached(('at/in', name, 'exact' if exact else dtype), lambda: sr.attn_inputs(name, shape, dtype, exact))
    if exact:                                                              # bf16 numbers in either type: one reference for every route
        qkv, dout = qkv.to(dtype), dout.to(dtype)
    ref = cached(('at/ref', name, shift, 'exact' if exact else dtype), lambda: sr.attention(qkv, sr.pad_bias_of(bias, dtype), relb, dout, Cn, heads, shift))
    bounds = sr.attn_bounds(ref, kind, dtype)
    r = sr.attn_route(kind, B, H, W, heads)
    tag = 'window attention %s shift %d [%s %s]' % (name, shift, route, ' '.join('%s %d' % kv for kv in sorted(r.items())))
    if route == 'bf16-valu':
        hip.sl_debug_attn_valu(1)
    try:
        out = osw.window_attention_fwd(dev(qkv), dev(bias), dev(relb), Cn, heads, shift, P)
        dqkv, drel, dpad = osw.window_attention_bwd(dev(qkv), dev(bias), dev(relb), dev(dout), Cn, heads, shift)
    finally:
        hip.sl_debug_attn_valu(-1)
    assert out.dtype == dtype and dqkv.dtype == dtype and tuple(dqkv.shape) == tuple(qkv.shape)
    ok = sr.worst_ratio(tag + ' out', cpu(out)[..., :Cn], ref['out'], bounds['out']) <= 1
    ok &= zero_pad(tag + ' out', out, Cn)
    ok &= sr.worst_ratio(tag + ' dqkv', cpu(dqkv)[..., :3 * Cn], ref['dqkv'], bounds['dqkv']) <= 1
    ok &= zero_pad(tag + ' dqkv', dqkv, 3 * Cn)
    ok &= sr.worst_ratio(tag + ' drel', cpu(drel), ref['drel'], bounds['drel']) <= 1
    ok &= sr.worst_ratio(tag + ' dpad', cpu(dpad), ref['dpad'], bounds['dpad']) <= 1
    assert ok


@pytest.mark.parametrize('route', sorted(sr.ATTN_ROUTES))
@pytest.mark.parametrize('shift', [0, 3])
@pytest.mark.parametrize('name', sorted(sr.ATTN_CASES))
def test_window_attention(hip, name, shift, route):
    """window_attention_{fwd,bwd}_kernel<float>, <bf16_t> (debug hook) and the MFMA kernels against the plain float64 attention and its closed-form backward."""
    _attention(hip, name, sr.ATTN_CASES[name], route, shift)


@pytest.mark.parametrize('name,route', [(n, r) for n in sorted(sr.ATTN_BIG) for r in sr.ATTN_BIG[n][1]])
def test_window_attention_many_windows(hip, name, route):
    """4 104 tasks: two windows per block of the VALU backward, a one-window last chunk; 10 296 tasks: two trips per wavefront of the MFMA backward, one live wavefront
    in the last block's second trip."""
    _attention(hip, name, sr.ATTN_BIG[name][0], route, 3, exact=True)


# ------------------------------------------------------------------------------------------------------------ position-table gradient
@pytest.mark.parametrize('heads', [3, 24])
def test_relpos_table_grad(hip, heads):
    """relpos_table_grad_kernel through both entry points, with the real pair lists, against index_add_ through relative_position_index in float64."""
    from oracle import swin_oracle as so
    from segland_amd import ops_swin as osw
    from segland_amd.functional_swin import _rel_pairs
    pairs = _rel_pairs(so.make_block(32 * heads, heads).attn, 169)
    assert pairs.dtype == torch.int32 and pairs.shape[0] == 169
    db = cached(('tg/db', heads), lambda: sr.randn('tg/%d' % heads, (heads, 49 * 49)))
    ref, bound = sr.table_grad(db), sr.K['table'] * sr.E24 * sr.table_grad(db.abs())
    ok = sr.worst_ratio('table gradient heads %d' % heads, cpu(osw.relpos_table_grad(dev(db), dev(pairs), 169)), ref, bound) <= 1
    cs, dp = sr.randn('tg/cs%d' % heads, (3 * heads * 32,)), sr.randn('tg/dp%d' % heads, (heads, 3, 32))
    table, dbq = osw.relpos_table_grad(dev(db), dev(pairs), 169, qkv_bias=(dev(cs), dev(dp)))
    ok &= sr.worst_ratio('table gradient heads %d (with the bias entry point)' % heads, cpu(table), ref, bound) <= 1
    rq = sr.qkv_bias_grad(cs, dp, heads)
    ok &= sr.worst_ratio('qkv bias gradient heads %d' % heads, cpu(dbq), rq, sr.E24 * rq.abs()) <= 1
    assert ok
