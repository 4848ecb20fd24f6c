"""Proves tests/swin_reference.py without a GPU: the references against autograd and against oracle/swin_oracle.py (pinned to the reference implementation), the route
tables (every route named there is taken, through the plain-Python restatements of the launchers' predicates), the bounds (torch's own float32 evaluation of every case
lies inside every fp32 bound; the worst ratios printed here are what the constants K are set from) and the comparators' sharpness (every wrong kernel listed below is
rejected)."""
import pytest
import torch
import torch.nn.functional as F

import swin_reference as sr
from oracle import swin_oracle as so
from swin_reference import BF16, F32, F64

_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def needed_k(family, what, err, bound_fn):
    """The smallest K of `family` with err <= bound everywhere: the bound is affine in K, bound = K a + e, so two evaluations give a and e.  Prints it, asserts K suffices."""
    old = sr.K[family]
    try:
        sr.K[family] = 1
        b1 = bound_fn()
        sr.K[family] = 2
        b2 = bound_fn()
    finally:
        sr.K[family] = old
    a, e = (b2 - b1).expand_as(err), (2 * b1 - b2).expand_as(err)
    over = (err - e).clamp_min(0)
    need = torch.where(a > 0, over / a.clamp_min(1e-300), torch.where(over > 0, torch.full_like(over, float('inf')), torch.zeros_like(over)))
    need = float(need.max())
    print('%s %s: float32 evaluation needs K = %.3g (K = %d, rule gives %d)' % (family, what, need, old, sr.k_from(need)))
    assert need <= old, (family, what, need)
    return need


def err(a, b):
    return (a.to(F64) - b.to(F64)).abs()


# ------------------------------------------------------------------------------------------------------------ references
@pytest.mark.parametrize('shift', [0, 3])
def test_closed_form_attention_backward_equals_autograd(shift):
    B, H, W, heads = 2, 10, 13, 3
    qkv, dout, bias, relb, C, P = sr.attn_inputs('cf%d' % shift, (B, H, W, heads), F32)
    q = qkv[..., :3 * C].to(F64).requires_grad_(True)
    b = bias.to(F64).requires_grad_(True)
    r = relb.to(F64).requires_grad_(True)
    out = sr.attn_forward(q, b, r, C, heads, shift)
    gq, gb, gr = torch.autograd.grad(out, (q, b, r), dout[..., :C].to(F64))
    ref = sr.attention(qkv, bias, relb, dout, C, heads, shift)
    for name, a, w in (('out', ref['out'], out.detach()), ('dqkv', ref['dqkv'], gq), ('drel', ref['drel'], gr), ('dpad', ref['dpad'], gb)):
        e = float(err(a, w).max())
        print('closed form vs autograd, shift %d, %s: %.3g' % (shift, name, e))
        assert e <= 1e-12, (name, e)
    # every R_abs dominates its reference
    for name in ('out', 'dqkv', 'drel', 'dpad'):
        assert bool((ref[name + '_abs'] >= ref[name].abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize('shift', [0, 3])
def test_attention_reference_equals_oracle(shift):
    """oracle.swin_oracle.window_attention (float32) on the windows of an unpadded 14 x 21 map, identity projection, against the float64 reference on qkv = Linear(x)."""
    B, H, W, heads, C = 2, 14, 21, 3, 96
    torch.manual_seed(11 + shift)
    a = so.make_block(C, heads).attn
    with torch.no_grad():
        a.relative_position_bias_table.normal_(0, 0.5)
        a.proj.weight.copy_(torch.eye(C)); a.proj.bias.zero_()
        x = sr.randn('or/x', (B, H, W, C))
        y = torch.roll(x, shifts=(-shift, -shift), dims=(1, 2)) if shift else x
        yw = y.view(B, H // 7, 7, W // 7, 7, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, 49, C)
        o = so.window_attention(yw, a, heads, so.shift_mask(H, W, 7, 3) if shift else None)
        o = o.view(B, H // 7, W // 7, 7, 7, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, C)
        want = torch.roll(o, shifts=(shift, shift), dims=(1, 2)) if shift else o
        qkv = F.linear(x.to(F64), a.qkv.weight.to(F64), a.qkv.bias.to(F64))
        relb = a.relative_position_bias_table[a.relative_position_index.view(-1)].view(49, 49, heads).permute(2, 0, 1)
        ref = sr.attn_forward(qkv, a.qkv.bias, relb, C, heads, shift)
    e = float(err(ref, want).max())
    print('float64 attention reference vs oracle window_attention in float32, shift %d: %.3g' % (shift, e))
    assert e <= 1e-5 * float(ref.abs().max())


@pytest.mark.parametrize('shift', [0, 3])
def test_attention_reference_equals_oracle_block(shift):
    """The whole oracle block (norm1, qkv, attention, proj, residual) with the MLP silenced, against LayerNorm + Linear + the attention reference + Linear in float64."""
    B, H, W, heads, C = 2, 10, 13, 3, 96
    torch.manual_seed(5 + shift)
    blk = so.make_block(C, heads)
    blk.shift, blk.index, blk.drop_path_p = shift, 0, 0.0
    with torch.no_grad():
        blk.attn.relative_position_bias_table.normal_(0, 0.5)
        blk.mlp.fc2.weight.zero_(); blk.mlp.fc2.bias.zero_()
    x = sr.randn('blk/x', (B, H * W, C))
    Hp, Wp, _ = sr.attn_geom(H, W)
    holder = type('M', (), {'drop_path_scale': staticmethod(lambda i, B, p: None)})
    with torch.no_grad():
        want = so.block_forward(holder, blk, x, H, W, so.shift_mask(Hp, Wp, 7, 3))
        d = lambda t: t.detach().to(F64)
        y, _, _ = sr.ln_fwd(x, blk.norm1.weight.detach(), blk.norm1.bias.detach(), C)
        qkv = F.linear(y, d(blk.attn.qkv.weight), d(blk.attn.qkv.bias)).view(B, H, W, 3 * C)
        a = blk.attn
        relb = a.relative_position_bias_table.detach()[a.relative_position_index.view(-1)].view(49, 49, heads).permute(2, 0, 1)
        o = sr.attn_forward(qkv, d(a.qkv.bias), relb, C, heads, shift)
        got = x.to(F64) + F.linear(o.reshape(B, H * W, C), d(a.proj.weight), d(a.proj.bias))
    e = float(err(got, want).max())
    print('LayerNorm + attention reference vs oracle block_forward, shift %d: %.3g' % (shift, e))
    assert e <= 1e-5 * float(want.abs().max())


def test_merge_patch_bilinear_references_equal_oracle():
    for name, (B, H, W, C, P) in sr.MERGE_CASES.items():
        x = sr.ints('mo/' + name, (B, H, W, P), F32)
        ds = so._Box()
        ds.norm = torch.nn.LayerNorm(4 * C)
        ds.reduction = torch.nn.Linear(4 * C, 2 * C, bias=False)
        with torch.no_grad():
            want = so.patch_merging(ds, x[..., :C].reshape(B, H * W, C), H, W)
            xm = sr.merge_gather(x, C)
            got = F.linear(F.layer_norm(xm.reshape(B, -1, 4 * C), (4 * C,), ds.norm.weight.to(F64), ds.norm.bias.to(F64), 1e-5), ds.reduction.weight.to(F64))
        assert float(err(got, want).max()) <= 1e-5 * max(1.0, float(want.abs().max())), name
    # patch embedding = the first lines of swin_forward: pad to a multiple of 4, conv stride 4
    for name, (B, H, W, C, P) in sr.PATCH_CASES.items():
        img, w, b = sr.randn('po/i/' + name, (B, 3, H, W)), sr.randn('po/w/' + name, (C, 3, 4, 4), F32, 0.2), sr.randn('po/b/' + name, (C,))
        want = F.conv2d(F.pad(img, (0, (4 - W % 4) % 4, 0, (4 - H % 4) % 4)), w, b, stride=4).permute(0, 2, 3, 1)
        assert float(err(sr.patch_embed_fwd(img, w, b), want).max()) <= 1e-5 * float(want.abs().max()), name
        # the im2col times the flattened weight is the same conv
        col = sr.patch_im2col(img)
        assert float(col[:, 48:].abs().max()) == 0
        got = (col[:, :48] @ w.to(F64).reshape(C, 48).t() + b.to(F64)).reshape(want.shape)
        assert float(err(got, sr.patch_embed_fwd(img, w, b)).max()) <= 1e-12 * float(want.abs().max()), name
    for name, (B, h, w, H, W) in sr.BIL_GEOM.items():
        x = sr.randn('bo/' + name, (B, h, w, 8))
        want = so._up(x.permute(0, 3, 1, 2), (H, W)).permute(0, 2, 3, 1)
        assert float(err(sr.bilinear_fwd(x, (H, W), True), want).max()) <= 1e-5 * float(want.abs().max()), name


def test_two_pass_layernorm_equals_f_layer_norm_in_float64():
    """The float32 yardstick of the LayerNorm forward is the two-pass expression, not ATen's float32 kernel (swin_reference.ln_fwd): in float64 they are the same function."""
    for name in ('f32-c96-offset100', 'bf16-c96-near-constant', 'f32-c192'):
        c = sr.ln_case(name)
        y, mean, rstd = sr.ln_fwd(c['x'], c['gamma'], c['beta'], c['C'])
        xd, m, r = sr.ln_stats(c['x'], c['C'])
        two_pass = (xd - m) * r * c['gamma'].to(F64) + c['beta'].to(F64)
        assert float(err(two_pass, y).max()) <= 1e-12 * float(y.abs().max()), name


def test_band_mask_equals_oracle_mask():
    for Hp, Wp in ((7, 7), (14, 21), (21, 14)):
        assert torch.equal(sr.band_mask(Hp, Wp, 3), so.shift_mask(Hp, Wp, 7, 3))


# ------------------------------------------------------------------------------------------------------------ routes
def test_layernorm_routes_are_all_taken():
    fwd, bwd, trips_f, trips_b = set(), set(), {}, {}
    for name, (d, B, n, C, px, py, family, opts) in sr.LN_CASES.items():
        dtype, rows = sr.DTYPES[d], B * n
        fwd.add((d,) + sr.ln_fwd_route(dtype, C, py))
        trips_f[name] = sr.ln_fwd_trips(dtype, rows, C, py)
        if 'fwdonly' not in opts:
            kind, lpr, nv, grid, trips = sr.ln_bwd_route(dtype, rows, C, py, 'noparam' not in opts)
            bwd.add((d, kind, lpr, nv))
            trips_b[name] = (kind, lpr, grid, trips)
    for d in ('f32', 'bf16'):
        for inst in ((16, 1), (32, 1), (64, 1), (64, 2), (64, 3), (64, 0)):
            assert (d,) + inst in fwd, ('forward', d, inst)
        for inst in (('fused', 16, 1), ('fused', 32, 1), ('fused', 64, 1), ('fused', 64, 2), ('fused', 64, 3), ('cols', 64, 0), ('dx-only', 16, 0), ('dx-only', 32, 0), ('dx-only', 64, 0)):
            assert (d,) + inst in bwd, ('backward', d, inst)
    # the multi-trip cases of the fused backward, one per lanes-per-row, each with a partial last trip; the benchmark's stage-1 route at its block cap
    assert trips_b['f32-c192-2051rows'] == ('fused', 64, 512, 2) and trips_b['f32-c96-4099rows'] == ('fused', 32, 512, 2)
    assert trips_b['bf16-c96-32771rows'] == ('fused', 16, 2048, 2)
    assert trips_f['f32-c192-65539rows-fwd'] == (16384, 2)                 # past the forward's 16 384-block cap
    multi = ('f32-c192-2051rows', 'f32-c96-4099rows', 'bf16-c96-32771rows')
    assert all(t[3] == 1 for k, t in trips_b.items() if k not in multi and t[0] == 'fused')
    opts = set(o for c in sr.LN_CASES.values() for o in c[7])
    assert opts == {'nostats', 'noparam', 'noaddend', 'rowscale', 'fwdonly'}
    assert any(c[4] != c[5] for c in sr.LN_CASES.values()) and set(c[6] for c in sr.LN_CASES.values()) == set(sr.LN_FAMILIES)
    assert {1, 3, 185} <= set(c[1] * c[2] for c in sr.LN_CASES.values())


def test_bilinear_backward_routes_are_all_taken():
    seen = set()
    for name, ((B, h, w, H, W), nv, route, opts) in sr.BIL_BWD_CASES.items():
        for t, (T, TS) in sr.BIL_TYPES.items():
            assert sr.bilinear_bwd_route(T, B, h, w, H, W, nv * sr.vec(T)) == route, (name, t)
            seen.add((route, t))
    assert seen == {(r, t) for r in ('small', 'general') for t in sr.BIL_TYPES}
    nvs = {r: set(c[1] for c in sr.BIL_BWD_CASES.values() if c[2] == r) for r in ('small', 'general')}
    assert {2, 128} <= nvs['small'] and {12, 24} <= nvs['general']
    assert sr.BIL_BWD_CASES['general-2052-sources'][0][0] * 27 * 38 == 2052 and sr.BIL_BWD_CASES['small-2048-sources'][0][0] * 32 * 32 == 2048


def test_attention_routes_are_all_taken():
    tails = set()
    for name, (B, H, W, heads) in sr.ATTN_CASES.items():
        r = sr.attn_route('mfma', B, H, W, heads)
        assert r['wpw'] == 1 and sr.attn_route('valu', B, H, W, heads)['wpb'] == 1
        tails.add(r['tail_waves'])
    assert tails == {1, 2, 3, 4}                                          # the MFMA tail: 1, 2 and 3 live wavefronts in the last block, and none idle
    assert {sr.attn_geom(H, W)[2] * B for B, H, W, _ in sr.ATTN_CASES.values()} >= {1, 2, 3, 5, 6}
    assert {h for _, _, _, h in sr.ATTN_CASES.values()} == {1, 3, 12, 24}
    (B, H, W, heads), routes = sr.ATTN_BIG['wpb2-171-windows']
    r = sr.attn_route('valu', B, H, W, heads)
    assert sr.attn_tasks(B, H, W, heads) == 4104 and r == dict(nwin=171, wpb=2, chunks=86, last_chunk=1)
    (B, H, W, heads), routes = sr.ATTN_BIG['wpw2-429-windows']
    r = sr.attn_route('mfma', B, H, W, heads)
    assert sr.attn_tasks(B, H, W, heads) == 10296 and r == dict(nwin=429, wpw=2, chunks=54, last_chunk=5, last_trips=2, tail_waves=1)


def test_elementwise_and_patch_cases_cover_their_edges():
    assert sr.ew_trips(sr.GELU_SIZES['second-trip'] // 8) == 2 and sr.ew_trips(sr.GELU_SIZES['9000'] // 4) == 1 and (sr.GELU_SIZES['9000'] // 4) % 256 != 0
    B, rows, C, P, _, _ = sr.SCALE_ADD_BIG
    assert sr.ew_trips(B * rows * P // 8) == 2
    toks = {n: B * -(-H // 4) * -(-W // 4) for n, (B, H, W, C, P) in sr.PATCH_CASES.items()}
    assert toks['c192-one-token'] == 1 and toks['c96-64-tokens'] == 64 and any(t % 64 for t in toks.values()) and any(t > 64 for t in toks.values())
    assert {c[3] for c in sr.PATCH_CASES.values()} == {32, 96, 128, 192} and any(c[4] > c[3] for c in sr.PATCH_CASES.values())
    assert any(H % 2 and W % 2 for _, H, W, _, _ in sr.MERGE_CASES.values()) and any(H % 2 != W % 2 for _, H, W, _, _ in sr.MERGE_CASES.values())


def test_no_case_is_skipped():
    import os
    here = os.path.dirname(os.path.abspath(__file__))
    for f in ('swin_reference.py', 'test_swin_parity_gpu.py'):
        with open(os.path.join(here, f), encoding='utf-8') as fh:
            text = fh.read()
        assert 'xfail' not in text and 'pytest.skip' not in text and 'mark.skip' not in text, f


# ------------------------------------------------------------------------------------------------------------ bounds: torch's float32 evaluation
def test_float32_layernorm_is_inside_the_bounds():
    worst = {'ln_fwd': 0.0, 'ln_fwd_offset': 0.0, 'ln_bwd': 0.0, 'ln_cols': 0.0}
    for name in sr.LN_CASES:
        c = sr.ln_case(name)
        x, g, b, C = c['x'], c['gamma'], c['beta'], c['C']
        y, mean, rstd = sr.ln_fwd(x, g, b, C)
        y32, m32, r32 = sr.ln_fwd(x, g, b, C, dt=F32)
        fam = 'ln_fwd_offset' if c['family'] == 'offset100' else 'ln_fwd'
        worst[fam] = max(worst[fam], needed_k(fam, name, err(y32, y), lambda: sr.ln_fwd_bound(x, g, b, C, y, F32, c['family'])))
        bm, br = sr.ln_stats_bounds(x, C)
        assert bool((err(m32, mean) <= bm).all()) and bool((err(r32, rstd) <= br).all()), name
        if 'fwdonly' in c['opts']:
            continue
        refs = sr.ln_bwd(c['dy'], x, g, C, c['addend'])
        r32 = sr.ln_bwd(c['dy'], x, g, C, c['addend'], dt=F32)
        bounds = lambda: sr.ln_bwd_bounds(c['dy'], x, g, C, c['addend'], refs, F32)
        worst['ln_bwd'] = max(worst['ln_bwd'], needed_k('ln_bwd', name, err(r32[0], refs[0]), lambda: bounds()[0]))
        worst['ln_cols'] = max(worst['ln_cols'], needed_k('ln_cols', name + ' dgamma', err(r32[1], refs[1]), lambda: bounds()[1]),
                               needed_k('ln_cols', name + ' dbeta', err(r32[2], refs[2]), lambda: bounds()[2]))
    for f, w in worst.items():
        print('YARDSTICK %s: worst float32 ratio %.3g -> K = %d (in use: %d)' % (f, w, sr.k_from(w), sr.K[f]))


def test_float32_gelu_patch_bilinear_table_are_inside_the_bounds():
    w = 0.0
    for d, dtype in sr.DTYPES.items():
        h = sr.gelu_input('gelu/' + d, sr.GELU_SIZES['9000'], dtype)
        dy = sr.randn('gelu/dy/' + d, h.shape, dtype)
        ref, refb = sr.gelu_fwd(h), sr.gelu_bwd(h, dy)
        w = max(w, needed_k('gelu', 'forward ' + d, err(sr.gelu_fwd(h, F32), ref), lambda: sr.gelu_fwd_bound(h, ref, F32)),
                needed_k('gelu', 'backward ' + d, err(sr.gelu_bwd(h, dy, F32), refb), lambda: sr.gelu_bwd_bound(h, dy, refb, F32)))
    print('YARDSTICK gelu: worst float32 ratio %.3g -> K = %d (in use: %d)' % (w, sr.k_from(w), sr.K['gelu']))
    w = 0.0
    for name, (B, H, W, C, P) in sr.PATCH_CASES.items():
        img, wt, b = sr.randn('pe/i/' + name, (B, 3, H, W)), sr.randn('pe/w/' + name, (C, 3, 4, 4), F32, 0.2), sr.randn('pe/b/' + name, (C,))
        ref = sr.patch_embed_fwd(img, wt, b)
        w = max(w, needed_k('patch', name, err(sr.patch_embed_fwd(img, wt, b, F32), ref), lambda: sr.K['patch'] * sr.E24 * sr.patch_embed_abs(img, wt, b)))
        dy = sr.randn('pe/dy/' + name, ref.shape[:3] + (P,))
        rw, rb = sr.patch_embed_bwd(img, dy, C)
        gw, gb = sr.patch_embed_bwd(img, dy, C, F32)
        w = max(w, needed_k('patch', name + ' dw', err(gw, rw), lambda: sr.patch_bwd_bounds(img, dy, C, F32)[0]),
                needed_k('patch', name + ' db', err(gb, rb), lambda: sr.patch_bwd_bounds(img, dy, C, F32)[1]))
    print('YARDSTICK patch: worst float32 ratio %.3g -> K = %d (in use: %d)' % (w, sr.k_from(w), sr.K['patch']))
    w = 0.0
    for align in (True, False):
        for name, (B, h, ww, H, W) in sr.BIL_GEOM.items():
            x = sr.randn('bl/' + name, (B, h, ww, 16))
            ref, ra = sr.bilinear_fwd(x, (H, W), align), sr.bilinear_fwd(x.abs(), (H, W), align)
            w = max(w, needed_k('bilinear', '%s align %d' % (name, align), err(sr.bilinear_fwd(x, (H, W), align, dt=F32), ref), lambda: sr.bilinear_bound(ref, ra, F32)))
        for name, ((B, h, ww, H, W), nv, route, opts) in sr.BIL_BWD_CASES.items():
            dy = sr.randn('blb/' + name, (B, H, W, 8))
            ref, ra = sr.bilinear_bwd(dy, (h, ww), align), sr.bilinear_bwd(dy.abs(), (h, ww), align)
            w = max(w, needed_k('bilinear', 'backward %s align %d' % (name, align), err(sr.bilinear_bwd(dy, (h, ww), align, dt=F32), ref), lambda: sr.bilinear_bound(ref, ra, F32)))
    print('YARDSTICK bilinear: worst float32 ratio %.3g -> K = %d (in use: %d)' % (w, sr.k_from(w), sr.K['bilinear']))
    w = 0.0
    for heads in (3, 24):
        db = sr.randn('tg/%d' % heads, (heads, 49 * 49))
        ref = sr.table_grad(db)
        w = max(w, needed_k('table', 'heads %d' % heads, err(sr.table_grad(db, F32), ref), lambda: sr.K['table'] * sr.E24 * sr.table_grad(db.abs())))
    print('YARDSTICK table: worst float32 ratio %.3g -> K = %d (in use: %d)' % (w, sr.k_from(w), sr.K['table']))


def _attn_yardstick(name, shape, dtype, shift, exact=False):
    qkv, dout, bias, relb, C, P = sr.attn_inputs(name, shape, dtype, exact)
    pb = sr.pad_bias_of(bias, dtype)
    ref = sr.attention(qkv, pb, relb, dout, C, shape[3], shift)
    r32 = sr.attention(qkv, pb, relb, dout, C, shape[3], shift, dt=F32)
    tag = '%s shift %d %s' % (name, shift, dtype)
    f = needed_k('attn_fwd', tag, err(r32['out'], ref['out']), lambda: sr.attn_bounds(ref, 'valu', F32)['out'])
    b = max(needed_k('attn_bwd', tag + ' ' + key, err(r32[key], ref[key]), lambda: sr.attn_bounds(ref, 'valu', F32)[key]) for key in ('dqkv', 'drel', 'dpad'))
    return f, b


def test_float32_attention_is_inside_the_bounds():
    wf = wb = 0.0
    for name, shape in sr.ATTN_CASES.items():
        for shift in (0, 3):
            for dtype in (F32, BF16):
                f, b = _attn_yardstick(name, shape, dtype, shift)
                wf, wb = max(wf, f), max(wb, b)
    for name, (shape, routes) in sr.ATTN_BIG.items():
        f, b = _attn_yardstick(name, shape, BF16, 3, exact=True)
        wf, wb = max(wf, f), max(wb, b)
    print('YARDSTICK attn_fwd: worst float32 ratio %.3g -> K = %d (in use: %d)' % (wf, sr.k_from(wf), sr.K['attn_fwd']))
    print('YARDSTICK attn_bwd: worst float32 ratio %.3g -> K = %d (in use: %d)' % (wb, sr.k_from(wb), sr.K['attn_bwd']))


def test_constants_follow_the_rule():
    """K = 8 x the recorded CPU ratio rounded up to a power of two, at least 4 (the recorded ratios are the ones the tests above print)."""
    for f, (ratio, k) in sr.MEASURED.items():
        assert k == sr.k_from(ratio), (f, ratio, k)


def test_exact_input_conditions():
    for d, dtype in sr.DTYPES.items():
        for name, (B, H, W, C, P) in sr.MERGE_CASES.items():
            x = sr.padded(sr.ints('mg/' + name, (B, H, W, C), dtype), P)
            sr.check_exact(sr.merge_gather(x, C), name)
            sr.check_exact(sr.merge_scatter(sr.ints('ms/' + name, (B, (H + 1) // 2, (W + 1) // 2, 4 * C), dtype), (B, H, W, P), C), name)
        for name in sr.SCALE_ADD_CASES:
            x, sc, add, C, pc = sr.scale_add_case(name, dtype)
            assert set(sc.tolist()) <= set(sr.SCALES) and (pc or set(sc.tolist()) >= set(sr.SCALES[-min(4, x.shape[0]):]))
            sr.check_exact(sr.scale_add(x, sc, add, C, pc), name)
        for name, (B, H, W, C, P) in sr.PATCH_CASES.items():
            sr.check_exact(sr.patch_im2col(sr.ints('ic/' + name, (B, 3, H, W), F32, -64, 64, 0.25)), name)
    with pytest.raises(AssertionError):
        sr.check_exact(torch.tensor([1.0 + 2.0 ** -9]))


# ------------------------------------------------------------------------------------------------------------ the comparators reject wrong kernels
def _attn_mutant_case(dtype, route):
    shape = (2, 12, 13, 3)                                                 # 12 rows: the middle band of the shifted map (rows Hp - 7 .. Hp - 4) holds real tokens
    qkv, dout, bias, relb, C, P = cached(('am/in', dtype), lambda: sr.attn_inputs('mutant', shape, dtype))
    pb = sr.pad_bias_of(bias, dtype)
    ref = cached(('am/ref', dtype), lambda: sr.attention(qkv, pb, relb, dout, C, 3, 3))
    return qkv, dout, pb, relb, C, ref, sr.attn_bounds(ref, route, dtype)


@pytest.mark.parametrize('route', sorted(sr.ATTN_ROUTES))
@pytest.mark.parametrize('mut', sr.MUTANTS)
def test_attention_comparator_rejects(mut, route):
    dtype, kind = sr.ATTN_ROUTES[route]
    qkv, dout, pb, relb, C, ref, bounds = _attn_mutant_case(dtype, kind)
    assert all(sr.worst_ratio('the reference itself ' + k, ref[k], ref[k], bounds[k]) == 0 for k in bounds)
    bad = sr.attention(qkv, pb, relb, dout, C, 3, 3, mut=mut)
    keys = {'last-window-missing': ('drel', 'dpad'), 'window-to-neighbour': ('out',)}.get(mut, ('out', 'dqkv', 'drel', 'dpad'))
    for k in keys:
        assert sr.worst_ratio('%s [%s] %s' % (mut, route, k), bad[k], ref[k], bounds[k]) > 1, (mut, k)


def test_mfma_operand_roundings_fill_the_mfma_bound():
    """The MFMA kernels' bf16 operand roundings (P before P v; dS and P before the three gradient products) replayed in otherwise exact arithmetic, outputs rounded to
    bf16: inside the MFMA bound on every case, outside a bound that counted each rounding as 2^-9 (what the windows of mostly pad tokens exposed), and outside the
    VALU bound, so the count is neither short nor slack."""
    worst, worst9 = 0.0, 0.0
    for name, shape in sr.ATTN_CASES.items():
        for shift in (0, 3):
            qkv, dout, bias, relb, C, P = sr.attn_inputs(name, shape, BF16)
            pb = sr.pad_bias_of(bias, BF16)
            ref = sr.attention(qkv, pb, relb, dout, C, shape[3], shift)
            em = sr.attention(qkv, pb, relb, dout, C, shape[3], shift, mut='mfma-roundings')
            bounds, valu = sr.attn_bounds(ref, 'mfma', BF16), sr.attn_bounds(ref, 'valu', BF16)
            for k in ('out', 'dqkv', 'dpad'):
                got = em[k].to(BF16).to(F64) if k != 'dpad' else em[k]
                r = sr.worst_ratio('replayed roundings %s shift %d %s' % (name, shift, k), got, ref[k], bounds[k])
                worst = max(worst, r)
                if k != 'dpad':
                    half = bounds[k] - 2.0 ** -9 * ref[k + '_abs']               # each operand rounding counted as 2^-9 R_abs
                    worst9 = max(worst9, sr.worst_ratio('... against 2^-9 per rounding', got, ref[k], half))
                    assert sr.worst_ratio('... against the VALU bound', got, ref[k], valu[k]) > 1
            assert float(err(em['drel'], ref['drel']).max()) == 0.0           # the position-bias gradient sees no rounding
    print('replayed MFMA roundings: worst ratio %.3g of the bound, %.3g of a 2^-9 bound' % (worst, worst9))
    assert worst <= 1 < worst9


def test_layernorm_comparators_reject():
    for d in ('f32', 'bf16'):
        c = sr.ln_case(d + '-c96-rowscale')
        x, g, b, C, dtype = c['x'], c['gamma'], c['beta'], 96, c['dtype']
        y, _, _ = sr.ln_fwd(x, g, b, C)
        bound = sr.ln_fwd_bound(x, g, b, C, y, dtype)
        assert sr.worst_ratio('divisor P', sr.ln_fwd_wrong(x, g, b, C, divisor=128), y, bound) > 1
        refs = sr.ln_bwd(c['dy'], x, g, C, c['addend'])
        bdx, bdg, bdb = sr.ln_bwd_bounds(c['dy'], x, g, C, c['addend'], refs, dtype)
        assert sr.worst_ratio('addend dropped', sr.ln_bwd(c['dy'], x, g, C, None)[0], refs[0], bdx) > 1
        # the column sums without the rows of a last trip: the last 3 rows of the map
        dy_short = c['dy'].clone()
        dy_short.view(-1, dy_short.shape[-1])[-3:] = 0
        short = sr.ln_bwd(dy_short, x, g, C, c['addend'])
        assert sr.worst_ratio('dgamma without the last trip', short[1], refs[1], bdg) > 1 and sr.worst_ratio('dbeta without the last trip', short[2], refs[2], bdb) > 1
        # the scaled copy with row / rows_per_sample off by one at the sample boundaries
        rs = c['row_scale'].to(F64)
        rows = torch.arange(c['rows'])
        good, bad = rs[rows // c['n']].view(3, -1, 1), rs[((rows + 1) // c['n']).clamp_max(2)].view(3, -1, 1)
        r2 = refs[0].to(dtype).to(F64) * good
        assert sr.worst_ratio('dx2 wrong sample', refs[0].to(dtype).to(F64) * bad, r2, bdx * good.abs() + sr.out_rounding(r2, dtype)) > 1
        # eps omitted at near-constant rows
        c = sr.ln_case(d + '-c96-near-constant')
        x, g, b = c['x'], c['gamma'], c['beta']
        y, _, _ = sr.ln_fwd(x, g, b, C)
        xs = x.view(-1, x.shape[-1])[1:]                                    # (row 0 is exactly constant: without eps it is 0 / 0)
        assert sr.worst_ratio('eps omitted', sr.ln_fwd_wrong(xs, g, b, C, eps=0.0), y.view(-1, C)[1:], sr.ln_fwd_bound(xs, g, b, C, y.view(-1, C)[1:], dtype)) > 1
        # a one-pass variance in float32 at the offset family
        c = sr.ln_case('f32-c96-offset100')
        x, g, b = c['x'], c['gamma'], c['beta']
        y, _, _ = sr.ln_fwd(x, g, b, C)
        x32 = x[..., :C]
        m = x32.mean(-1, keepdim=True)
        one_pass = (x32 - m) * ((x32 * x32).mean(-1, keepdim=True) - m * m + 1e-5).rsqrt() * g + b
        assert sr.worst_ratio('one-pass variance', one_pass, y, sr.ln_fwd_bound(x, g, b, C, y, F32, 'offset100')) > 1


def test_bilinear_comparators_reject():
    for t, (T, TS) in sr.BIL_TYPES.items():
        B, h, w, H, W = sr.BIL_GEOM['up-4x5-8x10']
        x = sr.randn('bm/x', (B, h, w, 32), TS)
        for align in (True, False):
            ref, ra = sr.bilinear_fwd(x, (H, W), align, 16, 8), sr.bilinear_fwd(x.abs(), (H, W), align, 16, 8)
            bound = sr.bilinear_bound(ref, ra, T)
            assert sr.worst_ratio('align swapped', sr.bilinear_fwd(x, (H, W), not align, 16, 8), ref, bound) > 1
            assert sr.worst_ratio('window off by a vector', sr.bilinear_fwd(x, (H, W), align, 16, 8 + sr.vec(T)), ref, bound) > 1
            base = sr.randn('bm/base', (B, H, W, 16), T)
            acc = sr.window_put(base, ref, 0, True)
            ba = sr.bilinear_bound(acc, ra + base.to(F64).abs(), T)
            assert sr.worst_ratio('accumulate overwrites', sr.window_put(base, ref, 0, False), acc, ba) > 1
            # backward: one candidate row of the destination missing at the border
            dy = sr.randn('bm/dy', (B, H, W, 16), T)
            refb, rab = sr.bilinear_bwd(dy, (h, w), align), sr.bilinear_bwd(dy.abs(), (h, w), align)
            for row in (0, H - 1):
                cut = dy.clone()
                cut[:, row] = 0
                assert sr.worst_ratio('candidate row %d missing' % row, sr.bilinear_bwd(cut, (h, w), align), refb, sr.bilinear_bound(refb, rab, TS)) > 1


def test_move_kernel_comparators_reject():
    B, H, W, C, P = sr.MERGE_CASES['odd-odd-c96']
    x = sr.padded(sr.ints('mm/x', (B, H, W, C), BF16), P)
    ref = sr.merge_gather(x, C)
    assert sr.bit_equal('the reference itself', ref, ref) == 0
    assert sr.bit_equal('middle quarters swapped', sr.merge_gather_wrong(x, C, swap=True), ref) > 0
    assert sr.bit_equal('odd-size pad not zero', sr.merge_gather_wrong(x, C, pad_value=1.0), ref) > 0
    B, H, W, C, P = sr.PATCH_CASES['c96-30x37-b2']
    img, w, b = sr.randn('mm/i', (B, 3, H, W)), sr.randn('mm/w', (C, 3, 4, 4), F32, 0.2), sr.randn('mm/b', (C,))
    ref = sr.patch_embed_fwd(img, w, b)
    for dtype in (F32, BF16):
        bound = sr.K['patch'] * sr.E24 * sr.patch_embed_abs(img, w, b) + sr.out_rounding(ref, dtype)
        assert sr.worst_ratio('ky / kx swapped', sr.patch_embed_fwd(img, w.transpose(2, 3), b), ref, bound) > 1
        edge = F.conv2d(F.pad(img.to(F64), (0, 3, 0, 2), mode='replicate'), w.to(F64), b.to(F64), stride=4).permute(0, 2, 3, 1)
        assert sr.worst_ratio('border not zero', edge, ref, bound) > 1
    col = sr.patch_im2col(sr.ints('mm/ic', (B, 3, H, W), F32, -64, 64, 0.25))
    assert sr.bit_equal('im2col ky / kx swapped', col.view(-1, 4, 4, 4)[:, :3].transpose(2, 3).reshape(-1, 48), col[:, :48]) > 0
    for heads in (3, 24):
        db = sr.randn('mm/tg%d' % heads, (heads, 49 * 49))
        ref = sr.table_grad(db)
        assert sr.worst_ratio('pair lists short', sr.table_grad(db, pairs_short=True), ref, sr.K['table'] * sr.E24 * sr.table_grad(db.abs())) > 1
        cs, dp = sr.randn('mm/cs%d' % heads, (3 * heads * 32,)), sr.randn('mm/dp%d' % heads, (heads, 3, 32))
        ref = sr.qkv_bias_grad(cs, dp, heads)
        assert sr.worst_ratio('dpad in (3, heads) order', sr.qkv_bias_grad(cs, dp, heads, wrong_order=True), ref, sr.E24 * ref.abs()) > 1
    x, sc, add, C, pc = sr.scale_add_case('dropout2d-addend', BF16)
    ref = sr.scale_add(x, sc, add, C, pc)
    assert sr.bit_equal('addend dropped', sr.scale_add(x, sc, None, C, pc), ref) > 0 and sr.bit_equal('per-sample instead of per-channel', sr.scale_add(x, sc[:x.shape[0]].contiguous(), add, C, False), ref) > 0
