"""The restatement of the reference's pure-tensor ISP (data_process/process.py:104-184) and of the trainers' preview strip
(trainer_SID.py:150-158, trainer_NF_SID.py:166-180) that csrc/isp.hip is tested against; tests/test_host_isp.py pins it to the reference's
own outputs (tests/golden/isp.npz).

Per pixel, float32, every operation rounded on its own:

    x * wb;  clamp [0,1];  g = (g1 + g2) / 2;  (r c0 + g c1) + b c2 per matrix row;  clamp [0,1]            -> ``linear``
    p = max(v, 1e-8) ** float32(1/2.2);  level = clamp(int(p * 255), 0, 255);  result level / 255           -> ``levels`` / ``levels_once``

``levels`` raises with torch's CPU float32 pow (what the reference ran); ``levels_once`` evaluates the power in float64 on the float32
operands and rounds once to float32 (what the kernel does); ``pre`` is the float64 value 255 v^e before any rounding or truncation, the
quantity the agreement rule looks at.  All return numpy arrays; levels are int64.

The agreement rule (``disagreements``): a level must equal the golden level, or differ by exactly one level where ``pre`` lies within
PRE_TOL of an integer.  PRE_TOL: one float32 ulp of the power below 1 is 6e-8, times 255 = 1.5e-5; the product's rounding adds at most
7.6e-6; the reference's pow is within 1 ulp, the device's within 0.5: under 4e-5 in sum, so 1e-4 has margin and is 5 000 times narrower than
a level.  The share of values that use the exception is capped at CAP per case: a condition that keeps the exception from hiding a wrong
kernel, not a tolerance."""
import numpy as np
import torch

EXPONENT = np.float32(1.0 / 2.2)
PRE_TOL = 1e-4
CAP = 0.005

SONY_WB = np.array([2.13, 1.0, 1.57, 1.0], np.float32)
SONY_CCM = np.array([[1.9712269, -0.6789218, -0.29230508],                      # utils/isp_ops.py:151-153
                     [-0.29104823, 1.748401, -0.45735288],
                     [0.02051281, -0.5380369, 1.5175241]], np.float32)


def linear(x, wb, ccm):
    """[N,4,H,W], wb [4] / [1,4] / [N,4], ccm [3,3] / [1,3,3] / [N,3,3] -> float32 torch [N,3,H,W]: the pipeline up to the second clamp"""
    x = torch.as_tensor(np.asarray(x, np.float32))
    N = x.shape[0]
    wb = torch.as_tensor(np.asarray(wb, np.float32)).reshape(-1, 4).expand(N, 4)
    ccm = torch.as_tensor(np.asarray(ccm, np.float32)).reshape(-1, 3, 3).expand(N, 3, 3)
    v = torch.clamp(x * wb.reshape(N, 4, 1, 1), 0.0, 1.0)
    r, g, b = v[:, 0], (v[:, 1] + v[:, 3]) / 2, v[:, 2]
    rows = [(r * ccm[:, c, 0].view(N, 1, 1) + g * ccm[:, c, 1].view(N, 1, 1)) + b * ccm[:, c, 2].view(N, 1, 1) for c in range(3)]
    return torch.clamp(torch.stack(rows, dim=1), 0.0, 1.0)


def _trunc(s):
    """(x * 255).int() then clamp(0, 255), NaN -> 0"""
    s = np.nan_to_num(np.asarray(s, np.float64), nan=0.0, posinf=255.0, neginf=0.0)
    return np.clip(np.trunc(s), 0, 255).astype(np.int64)


def levels(v, floor=True):
    """torch CPU float32 pow, as the reference ran it"""
    v = torch.as_tensor(np.asarray(v, np.float32))
    m = torch.clamp(v, min=1e-8) if floor else v
    return _trunc(((m ** (1 / 2.2)) * 255).numpy())


def levels_once(v, floor=True):
    """the power in float64 on the float32 operands, rounded once to float32"""
    v = np.asarray(v, np.float32)
    m = np.where(v < np.float32(1e-8), np.float32(1e-8), v) if floor else v
    with np.errstate(invalid='ignore'):
        p = (m.astype(np.float64) ** np.float64(EXPONENT)).astype(np.float32)
    return _trunc(p * np.float32(255))


def pre(v, floor=True):
    """float64 255 v^e before any rounding"""
    v = np.asarray(v, np.float32)
    m = np.where(v < np.float32(1e-8), np.float32(1e-8), v) if floor else v
    with np.errstate(invalid='ignore'):
        return 255.0 * m.astype(np.float64) ** np.float64(EXPONENT)


def process_levels(x, wb, ccm, once=False):
    v = linear(x, wb, ccm).numpy()
    return (levels_once if once else levels)(v)


def process_pre(x, wb, ccm):
    return pre(linear(x, wb, ccm).numpy())


def preview_linear(inputs, output, target, wb, add_inputs_to_output=False):
    """the float32 strip before the power, [H,3W,3] BGR, clipped to [0,1]"""
    wb = np.asarray(wb, np.float32)
    i = np.asarray(inputs, np.float32).clip(0, 1)
    o = np.asarray(output, np.float32)
    if add_inputs_to_output:
        o = o + i
    t = np.concatenate((i, o, np.asarray(target, np.float32)), axis=2)[:3].copy()
    t[0] = t[0] * wb[0]
    t[2] = t[2] * wb[2]
    return t.transpose(1, 2, 0)[:, :, ::-1].clip(0, 1)


def to_levels(out_f32):
    """a float render k / 255 -> k, asserting it is exactly such a value"""
    out = np.asarray(out_f32, np.float32)
    k = np.rint(out.astype(np.float64) * 255).astype(np.int64)
    assert np.array_equal((k.astype(np.float32) / np.float32(255)).view(np.uint32), out.view(np.uint32)), 'not k / 255 in float32'
    return k


def disagreements(got, golden, pre_value):
    """-> (values that differ from the golden, how many of those the rule does not excuse)"""
    got, golden = np.asarray(got, np.int64), np.asarray(golden, np.int64)
    assert got.shape == golden.shape == np.shape(pre_value), (got.shape, golden.shape, np.shape(pre_value))
    diff = got != golden
    near = np.abs(pre_value - np.rint(pre_value)) <= PRE_TOL
    bad = diff & ~((np.abs(got - golden) == 1) & near)
    return int(diff.sum()), int(bad.sum())


def assert_agrees(got, golden, pre_value, what=''):
    """the agreement rule with its cap; -> the number of values that used the one-level exception"""
    n_diff, n_bad = disagreements(got, golden, pre_value)
    print(f'isp agreement {what}: {n_diff} of {np.size(golden)} values used the one-level exception, {n_bad} not excused')
    assert n_bad == 0, f'{what}: {n_bad} values differ from the golden outside the one-level exception'
    assert n_diff <= CAP * np.size(golden), f'{what}: {n_diff} of {np.size(golden)} values used the exception (cap {CAP})'
    return n_diff
