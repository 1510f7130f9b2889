"""What the entry layer of the two fp16 families (csrc/conv_api.hip) refuses by the VALUE of an argument, without a GPU: the fourteen forward entries of
fp16x2 ('h2') and fp16x1 ('h1') run one body per layer shape, so every row holds for both families with the same code.  The addresses are made up and never
dereferenced: every case returns inside the entry layer (or the launcher's host-side argument check) before any HIP call -- a case that passed would try to
launch, so this file holds refusals and B == 0 only.

The split-K rows are the reason the file exists: the reduce kernel behind that entry reads the slabs and the bias and writes y as float4, and the first
launch (destination: the workspace, no bias) never shows y or bias to the launcher's validation.  The alignment check once stood in the h1 entry alone."""
import ctypes as C

import pytest

INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -4
X, AX, W_, AW, BIAS, Y, AY, WS, POOLED, CODES, HW, OUT = (0x10000 * i for i in range(1, 13))     # 64 KiB apart: each 16-byte aligned
B, H, W, CIN, COUT, KS = 1, 16, 16, 32, 32, 2


def _p(v):
    return None if v is None else C.c_void_p(v)


def _call(name, fam, *args):
    from pnnp_amd import ops
    fn = getattr(ops._prep(), name.replace('FAM', fam))
    return fn(*[a if isinstance(a, (C.c_int, C.c_int64)) else _p(a) for a in args])


def _i(*v):
    return [C.c_int(x) for x in v]


def _bits(fam):
    return [None] if fam == 'h2' else []             # the h2 entries' bits_y; the h1 entries have no such argument


def splitk(fam, y=Y, bias=BIAS, ws=WS, amax_y=AY, b=B, cout=COUT, ks=KS, ws_floats=None):
    if ws_floats is None:
        ws_floats = ks * b * H * W * cout
    return _call('pnnp_conv3x3_FAM_fwd_splitk_f32', fam, X, C.c_int(CIN), AX, None, C.c_int(0), None, W_, AW, bias, y, amax_y, *_bits(fam),
                 *_i(b, H, W, cout, 1, ks), ws, C.c_int64(ws_floats), None)


@pytest.mark.parametrize('fam', ['h2', 'h1'])
@pytest.mark.parametrize('kw,want', [
    (dict(y=Y + 4), INVALID), (dict(bias=BIAS + 4), INVALID), (dict(ws=WS + 4), INVALID), (dict(amax_y=AY + 1), INVALID),
    (dict(ws_floats=KS * B * H * W * COUT - 1), WORKSPACE), (dict(b=0), 0), (dict(cout=48), INVALID),
    (dict(ks=2, b=1 << 19, ws_floats=1 << 40), UNSUPPORTED)],
    ids=['y+4', 'bias+4', 'ws+4', 'odd amax_y', 'workspace too small', 'B=0', 'Cout=48', 'ksplit*B>=2^20'])
def test_splitk_entry_refuses_by_value(fam, kw, want):
    assert splitk(fam, **kw) == want


@pytest.mark.parametrize('fam', ['h2', 'h1'])
def test_head_pool_and_pointwise_entries_refuse_by_value(fam):
    src = (X, C.c_int(CIN), AX, None, C.c_int(0), None, W_, AW, BIAS)
    # head: Cout != 32
    assert _call('pnnp_conv3x3_FAM_fwd_head_f32', fam, *src, Y, AY, *_bits(fam), HW, None, None, OUT, *_i(B, H, W, 64, 1), None) == UNSUPPORTED
    # pool: odd height
    assert _call('pnnp_conv3x3_FAM_fwd_pool_f32', fam, *src, Y, POOLED, CODES, AY, *_bits(fam), *_i(B, 15, W, COUT, 1), None) == INVALID
    # 1x1: no amax slot for x1
    assert _call('pnnp_conv1x1_FAM_fwd_f32', fam, X, C.c_int(CIN), None, None, C.c_int(0), None, W_, AW, BIAS, None, Y, AY, *_i(B, H, W, COUT, 0), None) == INVALID
    # stride 2: odd height
    s2 = 'pnnp_conv3x3s2_h2_fwd_f32' if fam == 'h2' else 'pnnp_conv_s2_h1_fwd_f32'
    assert _call(s2, fam, X, C.c_int(CIN), AX, W_, AW, BIAS, Y, AY, *_i(B, 15, W, COUT, 0), None) == INVALID
    # ConvTranspose2d: Cin = 16 (K % 32)
    ct = 'pnnp_convt2x2_h2_fwd_f32' if fam == 'h2' else 'pnnp_convt_h1_fwd_f32'
    assert _call(ct, fam, X, C.c_int(16), AX, W_, AW, BIAS, Y, AY, *_i(B, H, W, COUT), None) == INVALID


def test_h1_wrappers_refuse_sign_bits_before_any_call():
    """ops: the shared wrappers take the family; fp16x1 writes no sign bits, and says so before it touches a tensor"""
    from pnnp_amd import ops
    from pnnp_amd._lib import PnnpError
    for fn, n in ((ops.conv_h1_fwd, 9), (ops.conv_h1_fwd_splitk, 11), (ops.conv_h1_fwd_head, 12), (ops.conv_h1_fwd_pool, 11)):
        with pytest.raises(PnnpError, match='sign bits'):
            fn(*[None] * n, bits_y=object())
    with pytest.raises(PnnpError, match='not an fp16 family'):
        ops.conv_f16_fwd('x3', *[None] * 9)
