"""The opt-in fp16x1 eval forwards -- 'fp16' (ConvPolicy.h1_eval, csrc/conv_h1s.hip: the stride-1 3x3 layers) and 'fp16_all' (+ h1_pointwise,
csrc/gemm_h1s.hip: ConvTranspose2d, 1x1 and stride-2 layers as well) -- against the default fp16x2 one: time and accuracy.

    python tools/h1_eval_bench.py [--out profiles/r7/h1_pointwise.txt] [--reps 5]

Everything runs in ONE process.  Three networks with the same weights, one per mode (so that no weight
re-pack falls into a timed region), are called alternately -- h2 h1 all h2 h1 all ... -- inside every round, after warm-up rounds; device
events around back-to-back eval forwards only.  Per call: median [min .. max] over the rounds; a ratio is quoted beside the spread of
its baseline, and the baseline of every ratio is the fp16x2 path measured in this same run.

Workloads (those of tools/tiled_eval_bench.py / profiles/r7/tiled_eval.txt): UNetSeeInDark nf = 32 on one 4x512x512 crop, on 16 crops, on
the whole 4x1424x2128 SID frame and through forward_tiled (20 tiles of 512); ResUnet nf = 32 on the 16-crop batch.  A per-layer split of
the 3x3 launches (the wrappers' own device events, pnnp_amd.ops.PROFILE) says which levels gain, and one of the pointwise launches
which of those gain from one piece (the yardstick of the 'fp16_all' column is the 'fp16' column of the same run).

Accuracy: a synthetic SID-like frame (rand^2.2 * 0.1 with 0.1 % saturated pixels, as tests/test_gpu_soak.py builds its crops) + noise
through variance-preserving random weights: PSNR of the fp16x1 output against a float64 forward of the same weights (tests/_h1_ref.py,
on a 512 x 512 crop) and against the fp16x2 output (whole frame), and what `evaluate` reports for both precisions."""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
import numpy as np
import torch

from oracle import net_torch as O
from pnnp_amd import ops
from pnnp_amd.archs import ResUnet, UNetSeeInDark
from pnnp_amd.evaluate import evaluate, forward_tiled

H, W, P, BASE = 1424, 2128, 512, 64


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / inner            # us per call


def rounds(forms, reps, inner, warm=2):
    out = {k: [] for k in forms}
    for r in range(warm + reps):
        for k, fn in forms.items():
            t = timed(fn, inner)
            if r >= warm:
                out[k].append(t)
    return out


def stat(v):
    return f'{np.median(v):10.1f} us [{min(v):.1f} .. {max(v):.1f}]'


def make(arch, res=False):
    shapes = O.unet_param_shapes(nf=32) if arch == 'unet' else O.resunet_param_shapes(nf=32)
    sd = O.init_state_he(shapes, seed=5, res_scale=0.5, head_scale=0.05, head_bias=0.1)
    nets = []
    for h1, pw in ((False, False), (True, False), (True, True)):
        net = (UNetSeeInDark if arch == 'unet' else ResUnet)(dict(nframes=1, res=res, nf=32, in_nc=4, out_nc=4))
        net.load_state_dict({k: v.clone() for k, v in sd.items()})
        net = net.cuda().eval()
        net.engine.set_policy(h1_eval=h1, h1_pointwise=pw)
        nets.append(net)
    return nets[0], nets[1], nets[2], sd


def sid_like(shape, gen):
    hr = torch.rand(*shape, device='cuda', generator=gen) ** 2.2 * 0.1
    sat = torch.rand(*shape, device='cuda', generator=gen) < 1e-3
    return torch.where(sat, torch.ones_like(hr), hr)


def psnr(a, b):
    return float(-10.0 * torch.log10(((a.double() - b.double()) ** 2).mean()))


CONV3 = ('conv9_fwd_h1', 'conv9_fwd_h2')
POINTWISE = tuple(f'{k}_fwd_{f}' for k in ('convt', 'conv1', 'conv9s2') for f in ('h1', 'h2'))


def per_layer(net, x, names, reps=5, kinds=CONV3):
    """{layer: median us} of the launches of ``kinds`` of one eval forward, in launch order (ops.PROFILE: events around every wrapper call)"""
    acc = {n: [] for n in names}
    for _ in range(reps + 1):
        ops.PROFILE = []
        with torch.no_grad():
            net.engine.forward(x, False)
        torch.cuda.synchronize()
        recs = [r for r in ops.PROFILE if r[0] in kinds]
        ops.PROFILE = None
        assert len(recs) == len(names), (len(recs), len(names))
        for n, r in zip(names, recs):
            acc[n].append(r[3].elapsed_time(r[4]) * 1e3)
    return {n: float(np.median(v[1:])) for n, v in acc.items()}


def act16_main(a):
    """'fp16_act' (ConvPolicy.h1_act16: every map a convolution writes and a convolution reads stored as fp16) alternated with 'fp32' / 'fp16' / 'fp16_all' in
    one process; the yardstick of the new column is the 'fp16_all' column of the SAME run.  UNet only: ResUnet's plan is its fp16_all plan."""
    out = a.out
    g = torch.Generator(device='cuda').manual_seed(1)
    u2, u1, ua, sd = make('unet')
    uc = UNetSeeInDark(dict(nframes=1, res=False, nf=32, in_nc=4, out_nc=4))
    uc.load_state_dict({k: v.clone() for k, v in sd.items()})
    uc = uc.cuda().eval()
    uc.engine.set_policy(h1_eval=True, h1_pointwise=True, h1_act16=True)
    hr = sid_like((1, 4, H, W), g)
    frame = (hr + 0.02 * torch.randn(1, 4, H, W, device='cuda', generator=g)).clamp(0, 1)
    crop1 = frame[:, :, 400:912, 800:1312].contiguous()
    crops16 = torch.cat([frame[:, :, 64 * i:64 * i + 512, 100 * i:100 * i + 512] for i in range(14)] + [crop1, crop1.flip(-1)]).contiguous()
    L = [f"fp16 storage of the activations ('fp16_act') against 'fp16_all', 'fp16' and 'fp32' on {torch.cuda.get_device_name(0)}; UNet nf = 32; random variance-preserving weights",
         f'per call, median [min .. max] over {a.reps} rounds, the four modes alternated inside every round (four engines, same weights: no re-pack is timed); device events', '']

    def fwd(net, x):
        def f():
            with torch.no_grad():
                net.engine.forward(x, False)
        return f
    nets = {'fp32': u2, 'fp16': u1, 'fp16_all': ua, 'fp16_act': uc}
    work = [('1 crop 4x512x512', lambda n: fwd(n, crop1), 20), ('16 crops 4x512x512', lambda n: fwd(n, crops16), 4), (f'whole frame 4x{H}x{W}', lambda n: fwd(n, frame), 4),
            ('forward_tiled, 20 tiles of 512', lambda n: (lambda: forward_tiled(n, frame, P, BASE)), 3)]
    L.append('(a) eval forward')
    for name, mk, inner in work:
        res = rounds({k: mk(n) for k, n in nets.items()}, a.reps, inner)
        ma, mc = np.median(res['fp16_all']), np.median(res['fp16_act'])
        L.append(f'  {name}')
        for k in nets:
            L.append(f'    {k:9s}{stat(res[k])}')
        L.append(f'    fp16_all / fp16_act = {ma / mc:.3f} x  (spread of the fp16_all rounds: {100 * (max(res["fp16_all"]) - min(res["fp16_all"])) / ma:.1f} % of their median)')
    assert uc.engine._plan.act16 and not ua.engine._plan.act16
    L.append('')
    order = [f'conv{i}_{j}' for i in range(1, 6) for j in (1, 2)]
    for i in range(6, 10):
        order += [f'upv{i}', f'conv{i}_1', f'conv{i}_2']
    show = ('conv1_1', 'conv1_2', 'upv9', 'conv9_1', 'conv9_2', 'conv5_1', 'conv5_2', 'upv6', 'conv6_1')
    for label, x in (('16 crops 4x512x512', crops16), (f'whole frame 4x{H}x{W}', frame)):
        ta = per_layer(ua, x, order, kinds=('conv9_fwd_h1', 'convt_fwd_h1'))
        tc = per_layer(uc, x, order, kinds=('conv9_fwd_h1a', 'convt_fwd_h1a'))
        L.append(f'(b) {label}: launches one by one (events around every launch: sums exceed (a)); conv9_2 carries the head')
        for n in show:
            L.append(f'    {n:8s} {uc.engine._plan[n].fwd:10s} fp16_all {ta[n]:8.1f} us   fp16_act {tc[n]:8.1f} us   fp16_all / fp16_act = {ta[n] / tc[n]:.3f} x')
        L.append(f'    all 22 launches: fp16_all {sum(ta.values()):.1f} us, fp16_act {sum(tc.values()):.1f} us')
    L.append('')
    with torch.no_grad():
        ya, yc = ua(crop1), uc(crop1)
    L.append(f'(c) 512 x 512 crop, fp16_act against fp16_all: PSNR {psnr(yc, ya):.1f} dB, max |difference| {float((yc - ya).abs().max()):.2e} of outputs up to {float(ya.abs().max()):.2f}')
    rng = uc.engine.act16_range()
    L.append(f'    act16_range: largest map amax {max(r["amax"] for r in rng):.3g} ({max(rng, key=lambda r: r["amax"])["name"]}), overflow flags {sum(r["overflow"] for r in rng)}')
    text = '\n'.join(L) + '\n'
    print(text)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, 'w') as f:
        f.write(text)


def act16_res_main(a):
    """'fp16_act_res' (ConvPolicy.h1_act16_res: fp16 storage of ResUnet's 31 maps) alternated with 'fp32' / 'fp16' / 'fp16_all' in one process; the yardstick of
    the new column is the 'fp16_all' column of the SAME run.  ResUnet nf = 32 on 16 crops of 512 and on one crop; then the launches one by one."""
    out = a.out
    g = torch.Generator(device='cuda').manual_seed(1)
    r2, r1, ra, sd = make('resunet')
    rc = ResUnet(dict(nframes=1, res=False, nf=32, in_nc=4, out_nc=4))
    rc.load_state_dict({k: v.clone() for k, v in sd.items()})
    rc = rc.cuda().eval()
    rc.engine.set_policy(h1_eval=True, h1_pointwise=True, h1_act16=True, h1_act16_res=True)
    hr = sid_like((1, 4, H, W), g)
    frame = (hr + 0.02 * torch.randn(1, 4, H, W, device='cuda', generator=g)).clamp(0, 1)
    crop1 = frame[:, :, 400:912, 800:1312].contiguous()
    crops16 = torch.cat([frame[:, :, 64 * i:64 * i + 512, 100 * i:100 * i + 512] for i in range(14)] + [crop1, crop1.flip(-1)]).contiguous()
    L = [f"fp16 storage of ResUnet's activations ('fp16_act_res') against 'fp16_all', 'fp16' and 'fp32' on {torch.cuda.get_device_name(0)}; ResUnet nf = 32; random variance-preserving weights",
         f'per call, median [min .. max] over {a.reps} rounds, the four modes alternated inside every round (four engines, same weights: no re-pack is timed); device events', '']

    def fwd(net, x):
        def f():
            with torch.no_grad():
                net.engine.forward(x, False)
        return f
    nets = {'fp32': r2, 'fp16': r1, 'fp16_all': ra, 'fp16_act_res': rc}
    L.append('(a) eval forward')
    for name, x, inner in (('16 crops 4x512x512', crops16, 4), ('1 crop 4x512x512', crop1, 20)):
        res = rounds({k: fwd(n, x) for k, n in nets.items()}, a.reps, inner)
        ma, mc = np.median(res['fp16_all']), np.median(res['fp16_act_res'])
        spread = max((max(res[k]) - min(res[k])) / np.median(res[k]) for k in ('fp16_all', 'fp16_act_res'))
        L.append(f'  {name}')
        for k in nets:
            L.append(f'    {k:13s}{stat(res[k])}')
        gain = ma / mc
        verdict = 'a gain beyond the spread' if gain - 1.0 > spread else ('SLOWER beyond the spread' if 1.0 - gain > spread else 'NO difference beyond the spread')
        L.append(f'    fp16_all / fp16_act_res = {gain:.3f} x  (larger spread of the two columns\' rounds: {100 * spread:.1f} % of the median): {verdict}')
    assert rc.engine._plan.act16 and not ra.engine._plan.act16
    L.append('')
    order = ['conv_in']
    for l in range(1, 6):
        order += [f'b{l}_0', f'b{l}_1'] + ([f'pool{l}'] if l < 5 else [])
    for i in range(6, 10):
        order += [f'upv{i}', f'b{i}_0', f'sc{i}', f'b{i}_1']
    order.append('conv10')
    show = ('conv_in', 'b1_0', 'b1_1', 'pool1', 'b5_0', 'b5_1', 'upv6', 'b6_0', 'sc6', 'b6_1', 'upv9', 'b9_0', 'sc9', 'b9_1', 'conv10')
    k_all = ('first_fwd', 'conv9_fwd_h1', 'conv9s2_fwd_h1', 'convt_fwd_h1', 'conv1_fwd_h1', 'head_fwd')
    k_act = ('first_fwd_et', 'conv9_fwd_h1a', 'conv9s2_fwd_h1a', 'convt_fwd_h1a', 'conv1_fwd_h1a', 'head_fwd_et')
    for label, x in (('16 crops 4x512x512', crops16), ('1 crop 4x512x512', crop1)):
        ta = per_layer(ra, x, order, kinds=k_all)
        tc = per_layer(rc, x, order, kinds=k_act)
        L.append(f'(b) {label}: launches one by one (events around every launch: sums exceed (a))')
        for n in show:
            L.append(f'    {n:8s} {rc.engine._plan[n].fwd:6s} fp16_all {ta[n]:8.1f} us   fp16_act_res {tc[n]:8.1f} us   fp16_all / fp16_act_res = {ta[n] / tc[n]:.3f} x')
        L.append(f'    all {len(order)} launches: fp16_all {sum(ta.values()):.1f} us, fp16_act_res {sum(tc.values()):.1f} us, ratio {sum(ta.values()) / sum(tc.values()):.3f}')
    L.append('')
    with torch.no_grad():
        ya, yc = ra(crop1), rc(crop1)
    L.append(f'(c) 512 x 512 crop, fp16_act_res against fp16_all: PSNR {psnr(yc, ya):.1f} dB, max |difference| {float((yc - ya).abs().max()):.2e} of outputs up to {float(ya.abs().max()):.2f}')
    rng = rc.engine.act16_range()
    L.append(f'    act16_range: {len(rng)} maps, largest amax {max(r["amax"] for r in rng):.3g} ({max(rng, key=lambda r: r["amax"])["name"]}), overflow flags {sum(r["overflow"] for r in rng)}')
    text = '\n'.join(L) + '\n'
    print(text)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, 'w') as f:
        f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None, help='default: profiles/r7/h1_pointwise.txt, profiles/r7/act16.txt with --act16, profiles/r7/act16_resunet.txt with --act16-res')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--act16', action='store_true', help="the 'fp16_act' column (fp16 storage of the activations, UNet) beside the three others -> profiles/r7/act16.txt")
    ap.add_argument('--act16-res', action='store_true', help="the 'fp16_act_res' column (fp16 storage of the activations, ResUnet) beside the three others -> profiles/r7/act16_resunet.txt")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('h1_eval_bench needs the GPU: nothing here is measured without one')
    a.out = a.out or os.path.join(REPO, 'profiles', 'r7', 'act16_resunet.txt' if a.act16_res else 'act16.txt' if a.act16 else 'h1_pointwise.txt')
    if a.act16_res:
        return act16_res_main(a)
    if a.act16:
        return act16_main(a)
    g = torch.Generator(device='cuda').manual_seed(1)
    u2, u1, ua, sd_u = make('unet')
    r2, r1, ra, _ = make('resunet')
    hr = sid_like((1, 4, H, W), g)
    frame = (hr + 0.02 * torch.randn(1, 4, H, W, device='cuda', generator=g)).clamp(0, 1)
    crop1 = frame[:, :, 400:912, 800:1312].contiguous()
    crops16 = torch.cat([frame[:, :, 64 * i:64 * i + 512, 100 * i:100 * i + 512] for i in range(14)] + [crop1, crop1.flip(-1)]).contiguous()
    L = [f"fp16x1 eval forwards -- 'fp16' (h1_eval: the stride-1 3x3 layers) and 'fp16_all' (+ h1_pointwise: ConvTranspose2d / 1x1 / stride-2 too) -- against fp16x2 "
         f'on {torch.cuda.get_device_name(0)}; nf = 32; random variance-preserving weights',
         f'per call, median [min .. max] over {a.reps} rounds, the three modes alternated inside every round (three engines, same weights: no re-pack is timed); device events', '']

    def fwd(net, x):
        def f():
            with torch.no_grad():
                net.engine.forward(x, False)
        return f
    work = [('UNet, 1 crop 4x512x512', fwd(u2, crop1), fwd(u1, crop1), fwd(ua, crop1), 20),
            ('UNet, 16 crops 4x512x512', fwd(u2, crops16), fwd(u1, crops16), fwd(ua, crops16), 4),
            (f'UNet, whole frame 4x{H}x{W}', fwd(u2, frame), fwd(u1, frame), fwd(ua, frame), 4),
            ('UNet, forward_tiled, 20 tiles of 512', lambda: forward_tiled(u2, frame, P, BASE), lambda: forward_tiled(u1, frame, P, BASE),
             lambda: forward_tiled(ua, frame, P, BASE), 3),
            ('ResUnet, 16 crops 4x512x512', fwd(r2, crops16), fwd(r1, crops16), fwd(ra, crops16), 4)]
    L.append("(a) eval forward: fp16x2 ('fp32', the default), fp16x1 on the 3x3 layers ('fp16') and on every layer that has a one-piece kernel ('fp16_all')")
    for name, f2, f1, fa, inner in work:
        res = rounds({'h2': f2, 'h1': f1, 'all': fa}, a.reps, inner)
        m2, m1, ma = np.median(res['h2']), np.median(res['h1']), np.median(res['all'])
        spread = 100 * (max(res['h2']) - min(res['h2'])) / m2
        spread1 = 100 * (max(res['h1']) - min(res['h1'])) / m1
        L.append(f'  {name}')
        L.append(f'    fp32     {stat(res["h2"])}')
        L.append(f'    fp16     {stat(res["h1"])}   fp32 / fp16 = {m2 / m1:.3f} x  (spread of the fp32 rounds: {spread:.1f} % of their median)')
        L.append(f'    fp16_all {stat(res["all"])}   fp16 / fp16_all = {m1 / ma:.3f} x, fp32 / fp16_all = {m2 / ma:.3f} x  (spread of the fp16 rounds: {spread1:.1f} %)')
    L.append('')

    names = [f'conv{i}_{j}' for i in range(1, 10) for j in (1, 2)]
    for label, x in (('16 crops 4x512x512', crops16), (f'whole frame 4x{H}x{W}', frame)):
        t2, t1 = per_layer(u2, x, names), per_layer(u1, x, names)
        plan = u1.engine._plan
        L.append(f'(b) UNet, {label}: the 3x3 launches one by one (events around every launch: sums exceed (a)); level = 1 full resolution .. 5')
        L.append('    layer     level  launch          fp16x2 us   fp16x1 us   ratio')
        lv2, lv1 = {}, {}
        for n in names:
            i = int(n[4])
            lvl = i if i <= 5 else 10 - i
            lv2[lvl] = lv2.get(lvl, 0.0) + t2[n]; lv1[lvl] = lv1.get(lvl, 0.0) + t1[n]
            L.append(f'    {n:9s} {lvl:5d}  {plan[n].fwd:12s} {t2[n]:11.1f} {t1[n]:11.1f} {t2[n] / t1[n]:7.2f}')
        for lvl in sorted(lv2):
            L.append(f'    level {lvl}: fp16x2 {lv2[lvl]:9.1f} us, fp16x1 {lv1[lvl]:9.1f} us, ratio {lv2[lvl] / lv1[lvl]:.2f}')
        L.append(f'    all 3x3 launches: fp16x2 {sum(t2.values()):.1f} us, fp16x1 {sum(t1.values()):.1f} us, ratio {sum(t2.values()) / sum(t1.values()):.2f}')
        L.append('')

    # ---- the pointwise launches one by one: fp16x2 (what 'fp16' runs them on: the yardstick) against fp16x1
    upv = [f'upv{i}' for i in range(6, 10)]
    res_names = [f'pool{i}' for i in range(1, 5)] + [n for i in range(6, 10) for n in (f'upv{i}', f'sc{i}')]
    for label, n1, na, x, names in (('UNet, 16 crops 4x512x512', u1, ua, crops16, upv), (f'UNet, whole frame 4x{H}x{W}', u1, ua, frame, upv),
                                    ('ResUnet, 16 crops 4x512x512', r1, ra, crops16, res_names)):
        t1, ta = per_layer(n1, x, names, kinds=POINTWISE), per_layer(na, x, names, kinds=POINTWISE)
        plan = na.engine._plan
        L.append(f"(d) {label}: the pointwise launches one by one, 'fp16' (fp16x2 kernel) against 'fp16_all' (fp16x1 kernel); K per segment -> N of the GEMM")
        L.append('    layer   kernel   fp16x2 us   fp16x1 us   ratio')
        for n in names:
            L.append(f'    {n:7s} {plan[n].fwd:6s} {t1[n]:11.1f} {ta[n]:11.1f} {t1[n] / ta[n]:7.2f}')
        L.append(f'    all pointwise launches: fp16x2 {sum(t1.values()):.1f} us, fp16x1 {sum(ta.values()):.1f} us, ratio {sum(t1.values()) / sum(ta.values()):.2f}')
        L.append('')

    # ---- accuracy
    from _h1_ref import h1_unet_forward
    with torch.no_grad():
        y2, y1, ya = u2(crop1).clone(), u1(crop1).clone(), ua(crop1).clone()
        f2, f1, fa = u2(frame).clone(), u1(frame).clone(), ua(frame).clone()
    sd64 = {k: v.double().cuda() for k, v in sd_u.items()}
    exact = h1_unet_forward(sd64, crop1)
    rel = lambda p, q: float((p.double() - q.double()).norm() / q.double().norm())
    L.append('(c) accuracy, UNet on the synthetic SID-like frame (outputs in [0, 1] units; PSNR = -10 log10 MSE)')
    L.append(f'  512 x 512 crop against the float64 forward of the same weights: fp16x1 PSNR {psnr(y1, exact):.1f} dB (relative L2 {rel(y1, exact):.2e}), '
             f'fp16x2 PSNR {psnr(y2, exact):.1f} dB (relative L2 {rel(y2, exact):.2e})')
    L.append(f'  whole frame, fp16x1 against fp16x2: PSNR {psnr(f1, f2):.1f} dB, relative L2 {rel(f1, f2):.2e}, max |difference| {float((f1 - f2).abs().max()):.2e} (max |output| {float(f2.abs().max()):.2e})')
    L.append(f'  512 x 512 crop against the float64 forward: fp16_all PSNR {psnr(ya, exact):.1f} dB (relative L2 {rel(ya, exact):.2e})')
    L.append(f'  whole frame, fp16_all against fp16x2: PSNR {psnr(fa, f2):.1f} dB, relative L2 {rel(fa, f2):.2e}, max |difference| {float((fa - f2).abs().max()):.2e}; '
             f'fp16_all against fp16: PSNR {psnr(fa, f1):.1f} dB')
    ma = evaluate(ua, frame, hr)['metrics'].cpu().tolist()
    L.append(f'  evaluate(frame, target): fp16_all PSNR {ma[0]:.4f} dB SSIM {ma[1]:.6f}')
    m2 = evaluate(u2, frame, hr)['metrics'].cpu().tolist()
    m1 = evaluate(u1, frame, hr)['metrics'].cpu().tolist()
    L.append(f'  evaluate(frame, target) with untrained weights: fp16x2 PSNR {m2[0]:.4f} dB SSIM {m2[1]:.6f}; fp16x1 PSNR {m1[0]:.4f} dB SSIM {m1[1]:.6f}; '
             f'change {m1[0] - m2[0]:+.4f} dB, {m1[1] - m2[1]:+.6f}')
    text = '\n'.join(L) + '\n'
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
