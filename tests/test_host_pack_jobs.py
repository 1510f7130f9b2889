"""The weight-pack job tables (_EngineBase._build_pack_jobs -> ops.PackJobs) without a GPU: the builder only records pointers and shapes, so it
runs on CPU tensors.  Per case -- both networks (nf = 32, 4 -> 4 channels), the four FAMILIES of tests/test_host_plan.py, train and eval --
the number of jobs and of amax jobs and a SHA-256 over both tables and over self._wp, every pointer normalised: a source as (parameter name,
byte offset), a destination as (ordinal of the first appearance of the packed tensor that contains it, that tensor's byte size, byte offset
inside it), an amax slot as its index.  The digest depends neither on addresses nor on how the engine keys its packed buffers; it pins the
order of the jobs (the pack launches), the slot indices and which pack every layer is handed.  A tensor in self._wp that no job writes counts
as no pack (None).  The constants were recorded from the builders as they were before the two engines shared one."""
import ctypes
import hashlib
import os

import pytest
import torch

from test_host_plan import FAMILIES

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (arch, family, train): (jobs, amax jobs, digest)
EXPECTED = {
    ('unet', 'h2', True): (69, 22, '7d6272fa30348aac5171b520deff8021605be4ac0b38d801f25c488ed03b3109'),
    ('unet', 'h2', False): (35, 22, '50f4dedf5435cbbca27e80e4b8da20e3080c8f0026c1df557562488025798e2c'),
    ('unet', 'x3', True): (69, 0, '2eb02f6a8fb98ba18d45be52377d66a6b608b1f24e60899c0ab77f8216a5f1ba'),
    ('unet', 'x3', False): (35, 0, 'c62fb0f785f0195d5945bc51bc94507c624776f717dd8a65be89bb8dbf7347c2'),
    ('unet', 'wino', True): (69, 0, 'e584fa832f17f5cb784989d305367206234b3767e37b5ec2cef29f62c305ff82'),
    ('unet', 'wino', False): (35, 0, 'f4efe0deee97bab1434fa45bc3a22f4b924a042f48f9da1589bccbc50ca3fa9c'),
    ('unet', 'direct', True): (69, 0, 'ce68904ccdbe9e8ad2589e47924b8e396d93e9ee7736eb3f6c40713ceb19b7f1'),
    ('unet', 'direct', False): (35, 0, '2adda6c0fd07efa0899deeaece5f1aabe535c322d019dea1979e597d0314ab47'),
    ('resunet', 'h2', True): (151, 31, 'fc0cf488b702b3dcf015c9ec305139af7957fdaf2525f773b08d9ee60d0ac194'),
    ('resunet', 'h2', False): (76, 31, '808ccffcab4addd77405430b507c03176de905480e1305a002ef849e77c0739c'),
    ('resunet', 'x3', True): (151, 0, '607a3c16fde9b94d025811f44c608852f8ca0a6fa15c605a1c235977a41ac790'),
    ('resunet', 'x3', False): (76, 0, 'f9d18350d838a222d20c85b5ec03aaa7215153919ea04d45c3c01caeab851f19'),
    ('resunet', 'wino', True): (119, 0, 'a8adf143cb9705c78a27ac4799960e55b4780a7f3f5ec51d87ba2ababc3e058f'),
    ('resunet', 'wino', False): (44, 0, 'd86d8d9cb047bb9f0ade3fd88686b5a2d58696194019fcd849f07295cd121686'),
    ('resunet', 'direct', True): (119, 0, '06f13e09d669162d0bb50477112ee228619e549bc298b98451a33a29afdbebad'),
    ('resunet', 'direct', False): (44, 0, 'e4d19c820bd42a4a598847399d79a2aaeb75b3656df6f07868cbc9c37a0345a7'),
}


def describe(arch, family, train):
    from pnnp_amd import ops
    from pnnp_amd.archs import ResUnet, UNetSeeInDark
    net = (UNetSeeInDark if arch == 'unet' else ResUnet)(dict(nframes=1, res=False, nf=32, in_nc=4, out_nc=4))
    e = net.engine
    e.set_policy(**FAMILIES[family])
    cpu = torch.device('cpu')
    e.params.ensure(cpu)
    P = dict(net.named_parameters())
    jobs = e._build_pack_jobs(train, cpu, P, e._plan_for(2, 96, 160, train))
    params = [(p.data_ptr(), p.numel() * p.element_size(), n) for n, p in P.items()]
    packed = {}
    for t in jobs.keep:
        if t is not None and not any(lo <= t.data_ptr() < lo + nb for lo, nb, _ in params) and (jobs.wslots is None or t.data_ptr() != jobs.wslots.data_ptr()):
            packed[t.data_ptr()] = t.numel() * t.element_size()
    order = {}                                   # base address of a packed tensor -> ordinal of its first appearance as a destination

    def src(p):
        return next((n, p - lo) for lo, nb, n in params if lo <= p < lo + nb)

    def dst(p, new=True):
        for lo, nb in packed.items():
            if lo <= p < lo + nb:
                if lo not in order:
                    if not new:
                        return None
                    order[lo] = len(order)
                return (order[lo], nb, p - lo)
        return None

    def slot(p):
        if not p:
            return None
        off = p - jobs.wslots.data_ptr()
        assert off % 4 == 0 and 0 <= off < 4 * jobs.wslots.numel()
        return off // 4

    scalars = [f for f, _ in ops.PackJob._fields_ if f not in ('src', 'dst', 'amax')]
    rows = []
    for i in range(jobs.n.value):
        j = jobs.jobs[i]
        rows.append(('job', src(j.src), dst(j.dst), slot(j.amax)) + tuple(getattr(j, f) for f in scalars))
    for i in range(jobs.n_amax.value):
        j = jobs.amax_jobs[i]
        rows.append(('amax', src(j.src), slot(j.dst), slot(j.amax)) + tuple(getattr(j, f) for f in scalars))
    for name in sorted(e._wp):
        f, d, s = e._wp[name]
        rows.append(('wp', name, None if f is None else dst(f.data_ptr(), new=False), None if d is None else dst(d.data_ptr(), new=False),
                     None if s is None else slot(s.data_ptr())))
    return jobs.n.value, jobs.n_amax.value, hashlib.sha256(repr(rows).encode()).hexdigest()


CASES = [(a, f, t) for a in ('unet', 'resunet') for f in ('h2', 'x3', 'wino', 'direct') for t in (True, False)]


@pytest.fixture(scope='module')
def built():
    so = os.path.join(REPO, 'pnnp_amd', 'libpnnp_hip.so')
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    if ctypes.CDLL(so).pnnp_device_cus() != 256:
        pytest.skip('the plans behind these tables are stated for 256 compute units')


@pytest.mark.parametrize('arch,family,train', CASES, ids=[f'{a}-{f}-{"train" if t else "eval"}' for a, f, t in CASES])
def test_pack_jobs_match_recorded_tables(built, arch, family, train):
    got = describe(arch, family, train)
    print(arch, family, train, got)
    assert got[:2] == EXPECTED[(arch, family, train)][:2]
    assert got[2] == EXPECTED[(arch, family, train)][2]
