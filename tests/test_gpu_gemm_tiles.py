"""Every instantiation of the pointwise GEMM kernel (csrc/gemm_s.h: 12 of the bf16x3 scheme, csrc/gemm_x3s.hip, and 12 of the fp16x2 scheme, csrc/gemm_h2s.hip),
op by op against float64: the ops of ConvTranspose2d(2, 2), Conv2d 1x1 and Conv2d 3x3 stride 2 at shapes that PICK each tile -- ragged maps, 32 .. 128
channels, and for each (scheme, tile) one map with more tiles than compute units, so that a workgroup walks a second tile and its cursor carries in x, y and image.
The two dispatch rules are restated below; every case asserts the instantiation it is labelled with."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

FWD, BWD, GEN, BWDB = 0, 1, 2, 3                                     # the epilogue a kernel carries (csrc/gemm_s.h)
E_FWD, E_BWD = 6e-7, 8e-7                                            # relative L2 against float64: the bars of tests/test_gpu_gemm_h2.py, for both families


def _tile_h2(N):
    """pnnp_gemm_h2s_launch: by the GEMM's columns alone."""
    return (128, 64) if N % 128 == 0 else ((64, 32) if N % 64 == 0 else (32, 32))


def _tile_x3(B, DH, DW, N, cus):
    """pnnp_gemm_x3s_launch: the widest tile that still gives 3/4 of the compute units a tile."""
    cols = (DW + 31) // 32
    rows8, rows16 = cols * ((DH + 7) // 8) * B, cols * ((DH + 15) // 16) * B
    if N % 128 == 0 and rows8 * (N // 128) * 4 >= cus * 3:
        return (128, 64)
    if N % 64 == 0:
        return (64, 64) if rows16 * (N // 64) * 4 >= cus * 3 else (64, 32)
    return (32, 32)


def _tiles(tile, B, DH, DW, N, fam):
    th = 16 if (fam == 'x3' and tile in ((64, 64), (32, 32))) else 8     # 512-pixel tiles: bf16x3's one-wave-wide ones
    return ((DW + 31) // 32) * ((DH + th - 1) // th) * B * ((N + tile[0] - 1) // tile[0])


def _epilogue(residual=False, accum=False, masked=False, bits=False, act=0, bias=False):
    """launch_gs_ek."""
    plain = not residual and not accum
    if plain and not masked:
        return FWD
    if bits:
        return BWDB
    return BWD if plain and not act and not bias else GEN


# (name, op, (B, H, W) of the TILE DOMAIN, channels, options, expected (BN, WN) of bf16x3 on 256 compute units)
#   convt_fwd: (Cin, Cout), N = 4 Cout      convt_bwd: (Cout, Cin), N = Cin      c1_fwd: (C1, C2, Cout), N = Cout      c1_bwd: (Cout, C1, C2), N = C1 + C2
#   s2_fwd: (Cin, Cout), N = Cout, the input map is twice the domain      s2_bwd: (Cout, Cin), N = Cin, four launches (one per parity class of dx) over the domain
BIG8, BIG16, MID, SMALL = (3, 61, 370), (3, 125, 370), (1, 197, 370), (2, 13, 40)
CASES = [
    ('convT fwd 32->32 wide', 'convt_fwd', BIG8, (32, 32), {}, (128, 64)),                                        # 12 x 8 x 3 = 288 tiles of 256 px x 128
    ('1x1 dgrad 32->64+64 masks wide', 'c1_bwd', BIG8, (32, 64, 64), dict(mask=(1, 2)), (128, 64)),                # n_split = 64: a wave's two block pairs go to different tensors
    ('1x1 fwd 32->128 residual wide', 'c1_fwd', BIG8, (32, 0, 128), dict(residual=True, act=1), (128, 64)),
    ('1x1 fwd 32+32->64 tall', 'c1_fwd', BIG16, (32, 32, 64), dict(act=2), (64, 64)),                               # two K segments; 288 tiles of 512 px x 64 / 576 of 256 px x 64
    ('1x1 dgrad 32->64 mask tall', 'c1_bwd', BIG16, (32, 64, 0), dict(mask=(1, 0)), (64, 64)),
    ('1x1 dgrad 32->32+32 accum tall', 'c1_bwd', BIG16, (32, 32, 32), dict(mask=(0, 1), accum=True), (64, 64)),
    ('s2 fwd 32->64', 's2_fwd', (2, 13, 41), (32, 64), dict(act=1), (64, 32)),
    ('convT dgrad 32->64 mask', 'convt_bwd', SMALL, (32, 64), dict(mask=1, bits=True), (64, 32)),
    ('s2 dgrad 32->64 accum', 's2_bwd', (2, 13, 41), (32, 64), dict(accum=True), (64, 32)),
    ('1x1 fwd 32->64 many small tiles', 'c1_fwd', MID, (32, 0, 64), {}, (64, 32)),                                  # 12 x 25 = 300 tiles of 256 px x 64, 156 of 512 px: below 3/4 x 256
    ('1x1 fwd 64->32 tall', 'c1_fwd', BIG16, (64, 0, 32), {}, (32, 32)),                                            # 288 tiles of 512 px x 32 / 576 of 256 px x 32
    ('convT dgrad 32->32 mask', 'convt_bwd', SMALL, (32, 32), dict(mask=1, bits=True), (32, 32)),
    ('1x1 fwd 32+32->32 residual', 'c1_fwd', SMALL, (32, 32, 32), dict(residual=True, act=1), (32, 32)),
    ('convT dgrad 32->128 mask', 'convt_bwd', SMALL, (32, 128), dict(mask=1, bits=True), (64, 32)),
]


def _columns(op, ch):
    return dict(convt_fwd=lambda: 4 * ch[1], convt_bwd=lambda: ch[1], c1_fwd=lambda: ch[2], c1_bwd=lambda: ch[1] + ch[2], s2_fwd=lambda: ch[1], s2_bwd=lambda: ch[1])[op]()


def _labels(case, cus=256):
    """{family: [(BN, WN, EK), ...]} of the launches of a case."""
    name, op, (B, H, W), ch, o, _ = case
    N = _columns(op, ch)
    if op in ('convt_fwd', 's2_fwd'):
        eks = [_epilogue(act=o.get('act', 0), bias=True)]
    elif op == 'c1_fwd':
        eks = [_epilogue(residual=o.get('residual', False), act=o.get('act', 0), bias=True)]
    elif op == 'convt_bwd':
        eks = [_epilogue(masked=bool(o.get('mask')))]
    else:
        eks = [_epilogue(masked=any(o.get('mask', (0, 0))) if op == 'c1_bwd' else False, accum=o.get('accum', False))]
    lab = {'x3': [_tile_x3(B, H, W, N, cus) + (e,) for e in eks], 'h2': [_tile_h2(N) + (e,) for e in eks]}
    if op == 'convt_bwd' and o.get('bits'):
        lab['h2'].append(_tile_h2(N) + (BWDB,))
    return lab


def test_the_cases_reach_all_24_instantiations_and_walk_a_second_tile():
    got = {'x3': set(), 'h2': set()}
    many = set()
    for case in CASES:
        name, op, (B, H, W), ch, o, x3_tile = case
        lab = _labels(case)
        assert lab['x3'][0][:2] == x3_tile, name                   # the bf16x3 tile a case is labelled with (256 compute units)
        for fam in got:
            got[fam] |= set(lab[fam])
            if _tiles(lab[fam][0][:2], B, H, W, _columns(op, ch), fam) > 256:
                many.add((fam,) + lab[fam][0][:2])
    assert got['x3'] == {(bn, wn, ek) for bn, wn in ((128, 64), (64, 64), (64, 32), (32, 32)) for ek in (FWD, BWD, GEN)}
    assert got['h2'] == {(bn, wn, ek) for bn, wn in ((128, 64), (64, 32), (32, 32)) for ek in (FWD, BWD, GEN, BWDB)}
    assert many == {('x3', 128, 64), ('x3', 64, 64), ('x3', 64, 32), ('x3', 32, 32), ('h2', 128, 64), ('h2', 64, 32), ('h2', 32, 32)}


def _slot(t=None):
    from pnnp_amd import ops
    s = torch.zeros(1, dtype=torch.int32, device='cuda')
    return ops.amax(t, s) if t is not None else s


def _nan(*shape):
    return torch.full(shape, float('nan'), device='cuda')


def _act(t, act):
    return t if act == 0 else (F.leaky_relu(t, 0.2) if act == 1 else F.relu(t))


def _masked(t, mask, mode):
    return t if not mode else torch.where(mask > 0, t, (0.2 if mode == 1 else 0.0) * t)


def _nchw(t):
    return t.permute(0, 3, 1, 2).double()


def _bits_of(below_shape, gen):
    """An activation map [B, H, W, C] and its sign bits as a 3x3 fp16x2 forward layer stores them (tests/test_gpu_gemm_h2.py)."""
    from pnnp_amd import ops
    B, H, W, C = below_shape
    xin = torch.randn(B, H, W, 32, device='cuda', generator=gen)
    w3 = torch.randn(C, 32, 3, 3, device='cuda', generator=gen) * 0.1
    jobs = ops.PackJobs(); f3 = torch.zeros(ops.h2_weight_bytes(32, C), dtype=torch.uint8, device='cuda'); s3 = jobs.add_h2(w3, f3, None, cin_pad=32); jobs.run()
    below = torch.empty(B, H, W, C, device='cuda'); bits = torch.zeros(ops.h2_bits_words(B, H, W, C), dtype=torch.int32, device='cuda')
    ops.conv_h2_fwd(xin, None, f3, s3, None, below, C, 1, _slot(xin), bits_y=bits)
    return below, bits


def run_case(case, families=('x3', 'h2')):
    """The op of `case` on each family: {'ref': [float64 references], family: ([outputs], [amax slot of output 0 or None]), 'h2 bits': ...}, and the bar."""
    from pnnp_amd import ops
    name, op, (B, H, W), ch, o, _ = case
    gen = torch.Generator(device='cuda').manual_seed(sum(map(ord, name)))
    rnd = lambda *s: torch.randn(*s, device='cuda', generator=gen)
    bytes_of = dict(x3=ops.x3mat_bytes, h2=ops.h2mat_bytes)
    buf = lambda n: torch.zeros(n, dtype=torch.uint8, device='cuda')
    jobs = ops.PackJobs()
    out = {}
    act = o.get('act', 0)
    if op in ('convt_fwd', 'convt_bwd'):
        Ci, Co = ch if op == 'convt_fwd' else ch[::-1]               # the layer's ConvTranspose2d(Ci -> Co); the domain is its INPUT map
        w = rnd(Ci, Co, 2, 2) * 0.1
        pk = {f: (buf(bytes_of[f](Ci, 4 * Co)), buf(bytes_of[f](4 * Co, Ci))) for f in families}
        sw = {f: (jobs.add_x3_convt if f == 'x3' else jobs.add_h2_convt)(w, *pk[f]) for f in families}
        jobs.run()
        if op == 'convt_fwd':
            x = rnd(B, H, W, Ci); bias = rnd(Co)
            out['ref'] = [F.conv_transpose2d(_nchw(x), w.double(), bias.double(), stride=2).permute(0, 2, 3, 1)]
            for f in families:
                y, s = _nan(B, 2 * H, 2 * W, Co), _slot()
                if f == 'x3': ops.convt_x3_fwd(x, pk[f][0], bias, y, Co, amax_y=s)
                else: ops.convt_h2_fwd(x, _slot(x), pk[f][0], sw[f], bias, y, Co, amax_y=s)
                out[f] = ([y], s)
            return out, E_FWD
        g = rnd(B, 2 * H, 2 * W, Co)
        if o.get('bits'):
            mask, bits = _bits_of((B, H, W, Ci), gen)
        else:
            mask, bits = rnd(B, H, W, Ci), None
        out['ref'] = [_masked(F.conv2d(_nchw(g), w.double(), stride=2).permute(0, 2, 3, 1), mask, o['mask'])]
        for f in families:
            dx, s = _nan(B, H, W, Ci), _slot()
            if f == 'x3': ops.convt_x3_bwd_data(g, pk[f][1], dx, mask=mask, mode=o['mask'], amax_dx=s)
            else: ops.convt_h2_bwd_data(g, _slot(g), pk[f][1], sw[f], dx, mask=mask, mode=o['mask'], amax_dx=s)
            out[f] = ([dx], s)
        if bits is not None and 'h2' in families:
            dx, s = _nan(B, H, W, Ci), _slot()
            ops.convt_h2_bwd_data(g, _slot(g), pk['h2'][1], sw['h2'], dx, mask=None, mode=o['mask'], amax_dx=s, bits=bits)
            out['h2 bits'] = ([dx], s)
        return out, E_BWD
    if op in ('c1_fwd', 'c1_bwd'):
        (C1, C2, Co) = ch if op == 'c1_fwd' else (ch[1], ch[2], ch[0])
        w = rnd(Co, C1 + C2, 1, 1) * 0.1
        pk = {f: (buf(bytes_of[f](C1 + C2, Co)), buf(bytes_of[f](Co, C1 + C2))) for f in families}
        sw = {f: (jobs.add_x3_1x1 if f == 'x3' else jobs.add_h2_1x1)(w, *pk[f]) for f in families}
        jobs.run()
        w2 = w[:, :, 0, 0].double()
        if op == 'c1_fwd':
            x1 = rnd(B, H, W, C1); x2 = rnd(B, H, W, C2) * 3 if C2 else None
            bias = rnd(Co); res = rnd(B, H, W, Co) if o.get('residual') else None
            xin = torch.cat([x1, x2], 3) if C2 else x1
            r = torch.einsum('bhwi,oi->bhwo', xin.double(), w2) + bias.double()
            out['ref'] = [_act(r + res.double() if res is not None else r, act)]
            for f in families:
                y = _nan(B, H, W, Co)
                if f == 'x3':
                    ops.conv1x1_x3_fwd(x1, x2, pk[f][0], bias, y, Co, act, residual=res); s = None
                else:
                    s = _slot(); ops.conv1x1_h2_fwd(x1, _slot(x1), x2, _slot(x2) if C2 else None, pk[f][0], sw[f], bias, y, Co, act, residual=res, amax_y=s)
                out[f] = ([y], s)
            return out, E_FWD
        g = rnd(B, H, W, Co)
        m1, m2 = o.get('mask', (0, 0)); accum = int(o.get('accum', False))
        k1 = rnd(B, H, W, C1) if m1 else None; k2 = rnd(B, H, W, C2) if (C2 and m2) else None
        b1 = rnd(B, H, W, C1); b2 = rnd(B, H, W, C2) if C2 else None
        full = torch.einsum('bhwo,oi->bhwi', g.double(), w2)
        out['ref'] = [_masked(full[..., :C1], k1, m1) + (b1.double() if accum else 0)]
        if C2: out['ref'].append(_masked(full[..., C1:], k2, m2) + (b2.double() if accum else 0))
        for f in families:
            d1 = b1.clone() if accum else _nan(B, H, W, C1)
            d2 = (b2.clone() if accum else _nan(B, H, W, C2)) if C2 else None
            if f == 'x3':
                ops.conv1x1_x3_bwd_data(g, pk[f][1], d1, mask1=k1, mode1=m1, accum1=accum, dx2=d2, mask2=k2, mode2=m2, accum2=accum); s = None
            else:
                s = _slot(); ops.conv1x1_h2_bwd_data(g, _slot(g), pk[f][1], sw[f], d1, mask1=k1, mode1=m1, accum1=accum, amax_dx1=s, dx2=d2, mask2=k2, mode2=m2, accum2=accum)
            out[f] = ([d1] + ([d2] if C2 else []), s)
        return out, E_BWD
    Ci, Co = ch if op == 's2_fwd' else ch[::-1]                       # Conv2d(Ci -> Co, 3, stride 2, pad 1) on a [2 H, 2 W] map
    w = rnd(Co, Ci, 3, 3) * 0.05
    pk = {f: (buf(bytes_of[f](9 * Ci, Co)), buf(9 * bytes_of[f](Co, Ci))) for f in families}
    sw = {f: (jobs.add_x3_s2 if f == 'x3' else jobs.add_h2_s2)(w, *pk[f]) for f in families}
    jobs.run()
    if op == 's2_fwd':
        x = rnd(B, 2 * H, 2 * W, Ci); bias = rnd(Co)
        out['ref'] = [_act(F.conv2d(_nchw(x), w.double(), bias.double(), stride=2, padding=1).permute(0, 2, 3, 1), act)]
        for f in families:
            y, s = _nan(B, H, W, Co), _slot()
            if f == 'x3': ops.conv_s2_x3_fwd(x, pk[f][0], bias, y, Co, act, amax_y=s)
            else: ops.conv_s2_h2_fwd(x, _slot(x), pk[f][0], sw[f], bias, y, Co, act, amax_y=s)
            out[f] = ([y], s)
        return out, E_FWD
    g = rnd(B, H, W, Co); base = rnd(B, 2 * H, 2 * W, Ci)
    out['ref'] = [base.double() + F.conv_transpose2d(_nchw(g), w.double(), stride=2, padding=1, output_padding=1).permute(0, 2, 3, 1)]
    for f in families:
        dx, s = base.clone(), _slot()
        if f == 'x3': ops.conv_s2_x3_bwd_data(g, pk[f][1], dx, accum=1, amax_dx=s)
        else: ops.conv_s2_h2_bwd_data(g, _slot(g), pk[f][1], sw[f], dx, accum=1, amax_dx=s)
        out[f] = ([dx], s)
    return out, E_BWD


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_pointwise_gemm_instantiation_vs_float64(case):
    from pnnp_amd import _lib
    name, op, (B, H, W), ch, o, x3_tile = case
    cus = _lib.lib().pnnp_device_cus()
    lab = _labels(case, cus)
    # the bf16x3 tile of a case is the one of 256 compute units; elsewhere the fp16x2 half (whose tile does not depend on the device) still runs
    families = ['x3', 'h2'] if lab['x3'][0][:2] == x3_tile else ['h2']
    out, bar = run_case(case, families)
    for key, (ys, slot) in ((k, v) for k, v in out.items() if k != 'ref'):
        for i, (y, ref) in enumerate(zip(ys, out['ref'])):
            assert torch.isfinite(y).all(), (name, key, i)
            e = float((y.double() - ref).norm() / ref.norm())
            print(f'{name} [{key}] output {i}: rel L2 vs float64 {e:.2e} (bar {bar:.0e})')
            assert e < bar, (name, key, i, e)
        if slot is not None:
            amax, top = slot.view(torch.float32).item(), float(ys[0].abs().max())
            assert top <= amax <= 1.0001 * top, (name, key, amax, top)
    if 'h2 bits' in out:                                             # EK_BWDB must be bit-equal to EK_BWD on the same inputs
        assert torch.equal(out['h2 bits'][0][0], out['h2'][0][0]) and torch.equal(out['h2 bits'][1], out['h2'][1]), name
    if 'x3' not in families:
        pytest.skip(f'{cus} compute units: the bf16x3 dispatch picks {lab["x3"][0][:2]}, not {x3_tile}; the shape is made for 256 (the fp16x2 half passed)')
