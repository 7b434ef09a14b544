"""adamw8.hip on the GPU: the AdamW kernel with 8-bit block-quantised moments, the standalone
quantise / dequantise kernels, their bindings' argument checks, and AdamW8bit / make_optimizer / the
SFT job on top of them.

Reference and units are those of tests/test_optim_kernels_gpu.py (imported as ``base``): ref64() is
AdamW in float64 on the ten uploaded hyper values, here fed the DEQUANTISED old moments
(table[code] * absmax, the state the kernel starts from); the floor is the worst error of fp32
ops/_ref.py::adamw_ on the same inputs in units of 2^-23 times the magnitude of the terms summed; the
bound is MARGIN = 4 x the floor (ulp_bf16 / 2 more for bf16 parameters without a master copy). Every
view sits in a frame of sentinels, the code and absmax buffers included.

Per step, beside p (and the master copy):
  absmax   each block's new absmax against max |m64| / max |v64| over the block, to the largest m / v
           bound in the block (|max a - max b| <= max |a - b|);
  codes    |table[code] * absmax - float64 value| <= half the larger gap to a neighbouring entry * absmax
           + the m / v bound: true for either neighbour at a tie, false for a quantiser that takes the
           entry below instead of the nearest on most elements (the table's gaps are 0.7 % and more of
           a value, the m / v bounds 1e-6 of it).
The number of codes that differ from the host reference's (ops/_ref.py::quantize_blockwise8 of the fp32
_ref.adamw_ moments) is printed: the kernel's moments differ from the host's in the last bits, and the
fast variant normalises with v_rcp_f32, so a value within a few ulp of a midpoint may take the other
neighbour.
"""
import os
import subprocess
import sys
import time

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:  # the child process starts from this file, not from pytest
        sys.path.insert(0, _p)

import test_optim_kernels_gpu as base  # noqa: E402  (ref64, floor32, make_hyper, ulp_bf16, MARGIN, ...)
from gke_ray_train_amd.ops import _ref  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
MARGIN, LR, WD, HSCALE, GS1 = base.MARGIN, base.LR, base.WD, base.HSCALE, base.GS1
SIZES = (1, 255, 256, 257, 1053, 4381)  # 1053: four blocks, three 8-wide groups and a 5-element tail;
#                                         4381: more than two workgroups of eight blocks
QB = _ref.Q8_BLOCK
CHILD_TIMEOUT = 20  # the child of test_optim_kernels_gpu.py takes 2.4-2.8 s; this one launches about as much


def _C():
    from gke_ray_train_amd import _native
    return _native.kernels()


def _half_gap(signed):
    t = _ref.q8_table(signed).double()
    gap = t[1:] - t[:-1]
    return torch.maximum(torch.cat([gap[:1], gap]), torch.cat([gap, gap[-1:]])) / 2


HALF = {True: _half_gap(True), False: _half_gap(False)}


# ----------------------------------------------------------------------------- framed operands
class Frame:
    """x inside a buffer with `pad` sentinel elements on both sides."""

    def __init__(self, x, dtype, pad):
        self.n, self.pad = x.numel(), pad
        self.sentinel = 7
        self.buf = torch.full((self.n + 2 * pad,), self.sentinel, dtype=dtype, device=DEV)
        self.view = self.buf[pad:pad + self.n]
        self.view.copy_(x.to(dtype))

    def intact(self):
        return bool((self.buf[:self.pad] == self.sentinel).all()) and bool((self.buf[self.pad + self.n:] == self.sentinel).all())


class State8:
    """One flat parameter with its gradient and quantised moments on the device, every view framed.
    shift: p and g start 8 bytes into a 16-byte aligned buffer (bf16 only)."""

    def __init__(self, p0, m0, v0, pdt, master=False, shift=False):
        n = p0.numel()
        self.n, self.pdt, self.shift = n, pdt, shift
        lo = 4 if shift else 8
        self.f = {}
        if master:
            self.f["master"] = Frame(p0, F32, 4)
            self.f["p"] = Frame(torch.zeros(n), pdt, lo)  # the step must read the master copy, not p
        else:
            self.f["p"] = Frame(p0, pdt, lo)
        self.f["g"] = Frame(torch.zeros(n), pdt, lo)
        for key, x, signed in (("m", m0, True), ("v", v0, False)):
            codes, absmax = _ref.quantize_blockwise8(x, signed)
            self.f["c" + key] = Frame(codes, U8, 8)  # code arrays are 8-byte aligned
            self.f["a" + key] = Frame(absmax, F32, 3)
        self.p, self.g = self.f["p"].view, self.f["g"].view
        self.mas = self.f["master"].view if master else None
        self.cm, self.am, self.cv, self.av = (self.f[k].view for k in ("cm", "am", "cv", "av"))

    def set_grad(self, g):
        self.g.copy_(g.to(self.pdt))

    def moments(self):
        """(m, v) dequantised on the host: fp32, what the kernel starts from."""
        return (_ref.dequantize_blockwise8(self.cm.cpu(), self.am.cpu(), True),
                _ref.dequantize_blockwise8(self.cv.cpu(), self.av.cpu(), False))

    def value(self):
        return (self.mas if self.mas is not None else self.p).cpu().float().clone()

    def launch(self, hyper, gsc, max_blocks=0, ioff=0):
        _C().adamw8(self.p, self.g, self.cm, self.am, self.cv, self.av, self.mas, hyper, gsc, max_blocks, ioff)

    def broken_frames(self):
        return [k for k, f in self.f.items() if not f.intact()]


def _block_max(x, n):
    return torch.stack([b.max() for b in x.split(QB)])


def floor32(p, g, m, v, h, gs1, ref, units):
    """base.floor32 (the worst normalised error of fp32 _ref.adamw_ on the same inputs), over the elements
    whose unit is not zero: an element of an all-zero block has zero terms, a zero unit and a bound of
    zero, which asks for the exact result."""
    pc, mc, vc = p.clone(), m.clone(), v.clone()
    _ref.adamw_(pc, g, mc, vc, h[9], h[0], h[1], h[2], h[3], h[4], grad_scale=h[7] * gs1)
    return [((x.double() - r).abs()[s > 0] / s[s > 0]).max().item() for x, r, s in zip((pc, mc, vc), ref, units)]


def _worst(err, unit):
    return (err[unit > 0] / unit[unit > 0]).max().item() if bool((err[unit == 0] == 0).all()) else float("inf")


def verify_step(s, before, g_cpu, h, gs1, sr=False):
    """One launched step of State8 s against ref64 from `before` = (value, m, v) fp32. Returns
    (floors, worst p/m-absmax/v-absmax/m-codes/v-codes in bound units, fails, codes differing from the host's)."""
    n = s.n
    ref, units = base.ref64(before[0].double(), g_cpu.double(), before[1].double(), before[2].double(), h, gs1)
    fl = floor32(before[0], g_cpu, before[1], before[2], h, gs1, ref, units)
    fails = []
    out = s.value().double()
    err = (out - ref[0]).abs()
    if s.pdt == BF16 and s.mas is None:
        if sr:  # one of the two bf16 neighbours of the float64 value
            err = (err - base.ulp_bf16(torch.maximum(out.abs(), ref[0].abs()))).clamp_min(0.0)
        else:  # the correctly rounded bf16 of the float64 value
            err = (err - base.ulp_bf16(ref[0]) / 2).clamp_min(0.0)
    if s.mas is not None and not torch.equal(s.p.cpu(), s.mas.cpu().to(s.pdt)):
        fails.append("p is not the rounded master copy")
    worst = [_worst(err, units[0])]
    if not worst[0] <= MARGIN * fl[0]:
        fails.append(f"p is {worst[0]:.2f} units off, bound {MARGIN} x {fl[0]:.2f}")
    blk = torch.arange(n) // QB
    host = [before[0].clone(), before[1].clone(), before[2].clone()]
    _ref.adamw_(host[0], g_cpu, host[1], host[2], h[9], h[0], h[1], h[2], h[3], h[4], grad_scale=h[7] * gs1)
    differ = []
    code_worst = []
    for i, (codes, absmax, signed, what) in enumerate(((s.cm, s.am, True, "m"), (s.cv, s.av, False, "v")), start=1):
        codes, absmax = codes.cpu().long(), absmax.cpu().double()
        bound = MARGIN * fl[i] * units[i]
        # absmax
        big = _block_max(ref[i].abs(), n)
        w = ((absmax - big).abs() / _block_max(bound, n).clamp_min(1e-300)).max().item() if float(big.max()) > 0 else 0.0
        worst.append(w)
        if not bool(((absmax - big).abs() <= _block_max(bound, n)).all()):
            fails.append(f"absmax of {what} is off: {w:.2f} of the bound")
        # codes
        a = absmax[blk]
        deq = _ref.q8_table(signed).double()[codes] * a
        lim = HALF[signed][codes] * a + bound
        e = (deq - ref[i]).abs()
        code_worst.append(((e - HALF[signed][codes] * a).clamp_min(0.0) / bound.clamp_min(1e-300)).max().item())
        bad = int((~(e <= lim)).sum())
        if bad:
            fails.append(f"{bad} of {n} codes of {what} are not the nearest entry")
        differ.append(int((codes != _ref.quantize_blockwise8(host[i], signed)[0].long()).sum()))
    for k in s.broken_frames():
        fails.append(f"the kernel wrote outside the {k} view")
    return fl, worst + code_worst, fails, differ


def _initial(n, seed=1234):
    gen = torch.Generator().manual_seed(seed)
    return gen, torch.randn(n, generator=gen), 0.01 * torch.randn(n, generator=gen), 0.01 * torch.rand(n, generator=gen)


def check_trajectory(n, pdt, master, shift, max_blocks):
    """Steps 4, 5, 6 from random non-zero quantised moments, each against ref64 from the state the
    kernel left."""
    gen, p0, m0, v0 = _initial(n)
    s = State8(p0, m0, v0, pdt, master, shift)
    gsc = torch.tensor([123.0, GS1], dtype=F32).to(DEV)
    gs1 = float(gsc[1])
    fails, tot_diff, worst_all = [], [0, 0], [0.0] * 5
    for step in (4, 5, 6):
        s.set_grad(3 * torch.randn(n, generator=gen))
        hyper = base.make_hyper(LR, WD, step, gscale=HSCALE).to(DEV)
        before = (s.value(), *s.moments())
        s.launch(hyper, gsc, max_blocks)
        fl, worst, f, differ = verify_step(s, before, s.g.cpu(), hyper.cpu().double().tolist(), gs1)
        fails += [f"step {step}: {x}" for x in f]
        tot_diff = [a + b for a, b in zip(tot_diff, differ)]
        worst_all = [max(a, b) for a, b in zip(worst_all, worst)]
    tag = f"n={n} {base._name(pdt)} master={int(master)} shift={int(shift)} max_blocks={max_blocks}"
    print(f"trajectory8 {tag}: p {worst_all[0]:.2f} units; codes differing from the host's over 3 steps: "
          f"m {tot_diff[0]} v {tot_diff[1]} of {3 * n}; code excess over the half gap, in bounds: "
          f"m {worst_all[3]:.2f} v {worst_all[4]:.2f}")
    assert not fails, f"{tag}: " + "; ".join(fails)


VARIANTS = {"bf16": (BF16, False), "bf16-master": (BF16, True), "f32": (F32, False)}
TRAJECTORY_CASES = [(n, v, mb) for v in VARIANTS for n in SIZES for mb in (0, 1)]


@pytest.mark.parametrize("n,variant,max_blocks", TRAJECTORY_CASES,
                         ids=[f"{v}-n{n}-blocks{mb}" for n, v, mb in TRAJECTORY_CASES])
def test_adamw8_trajectory(n, variant, max_blocks):
    pdt, master = VARIANTS[variant]
    check_trajectory(n, pdt, master, False, max_blocks)


SHIFT_CASES = [(n, master) for n in (1053, 4381) for master in (False, True)]


@pytest.mark.parametrize("n,master", SHIFT_CASES, ids=[f"n{n}-{'master' if m else 'nomaster'}" for n, m in SHIFT_CASES])
def test_adamw8_plus4_view(n, master):
    """p and g views 8 but not 16 bytes aligned."""
    check_trajectory(n, BF16, master, True, 0)


# ----------------------------------------------------------------------------- edge cases
def _one_step(s, g, step=4, sr=0.0, max_blocks=0, ioff=0):
    s.set_grad(g)
    hyper = base.make_hyper(LR, WD, step, gscale=HSCALE, sr=sr).to(DEV)
    gsc = torch.tensor([123.0, GS1], dtype=F32).to(DEV)
    before = (s.value(), *s.moments())
    s.launch(hyper, gsc, max_blocks, ioff)
    return before, hyper.cpu().double().tolist(), float(gsc[1])


def check_zero_block():
    """Block 1 of three: zero gradient on zero moments. Zero codes, absmax 0, p = p * decay, all finite."""
    n = 700
    gen, p0, m0, v0 = _initial(n, 5)
    m0[256:512] = 0
    v0[256:512] = 0
    g = 3 * torch.randn(n, generator=gen)
    g[256:512] = 0
    s = State8(p0, m0, v0, F32)
    before, h, gs1 = _one_step(s, g)
    _fl, _w, fails, _d = verify_step(s, before, s.g.cpu(), h, gs1)
    assert not fails, fails
    assert bool((s.cm[256:512] == _ref.Q8_ZERO_CODE[True]).all()) and bool((s.cv[256:512] == _ref.Q8_ZERO_CODE[False]).all())
    assert s.am[1].item() == 0.0 and s.av[1].item() == 0.0
    decay = torch.tensor(1.0, dtype=F32) - torch.tensor(LR, dtype=F32) * torch.tensor(WD, dtype=F32)
    assert torch.equal(s.p[256:512].cpu(), p0[256:512] * decay)
    for t in (s.p, s.am, s.av):
        assert bool(t.isfinite().all())


def check_outlier_block():
    """One element 1e4 x the rest of its block: the others fall into the lowest decades or to zero."""
    n = 600
    gen, p0, m0, v0 = _initial(n, 6)
    g = 3 * torch.randn(n, generator=gen)
    g[300] = 3e4
    for pdt in (BF16, F32):
        s = State8(p0, m0, v0, pdt)
        before, h, gs1 = _one_step(s, g)
        _fl, _w, fails, _d = verify_step(s, before, s.g.cpu(), h, gs1)
        assert not fails, fails
        assert s.cm[300].item() == 255 and s.cv[300].item() == 255  # the entry 1.0


def check_nan_gradient():
    """A NaN gradient stays visible: the element's p and its block's two absmax become non-finite."""
    n = 700
    gen, p0, m0, v0 = _initial(n, 7)
    g = 3 * torch.randn(n, generator=gen)
    g[300] = float("nan")
    for pdt, master in ((BF16, False), (BF16, True), (F32, False)):
        s = State8(p0, m0, v0, pdt, master)
        _one_step(s, g)
        val = s.value()
        assert not bool(val[300].isfinite()) and not bool(s.p[300].isfinite())
        assert not bool(s.am[1].isfinite()) and not bool(s.av[1].isfinite())
        others = torch.ones(n, dtype=torch.bool)
        others[300] = False
        assert bool(val[others].isfinite().all())
        assert bool(s.am[[0, 2]].isfinite().all()) and bool(s.av[[0, 2]].isfinite().all())
        assert not s.broken_frames()


def check_slices_match_whole():
    """Two launches over block-aligned slices with matching index offsets, stochastic rounding on:
    bitwise the single launch over the whole."""
    n = 4381
    gen, p0, m0, v0 = _initial(n, 8)
    g = 3 * torch.randn(n, generator=gen)
    big = (1 << 33) + 512
    hyper = base.make_hyper(LR, WD, 4, gscale=HSCALE, sr=1.0).to(DEV)
    whole = State8(p0, m0, v0, BF16)
    whole.set_grad(g)
    whole.launch(hyper, None, 0, big)
    parts = State8(p0, m0, v0, BF16)
    parts.set_grad(g)
    C = _C()
    for a, b in ((0, 1024), (1024, n)):
        ba, bb = a // QB, (b + QB - 1) // QB
        C.adamw8(parts.p[a:b], parts.g[a:b], parts.cm[a:b], parts.am[ba:bb], parts.cv[a:b], parts.av[ba:bb], None,
                 hyper, None, 0, big + a)
    for k in ("p", "cm", "am", "cv", "av"):
        assert torch.equal(whole.f[k].buf, parts.f[k].buf), k
    other = State8(p0, m0, v0, BF16)
    other.set_grad(g)
    other.launch(hyper, None, 0, 512)
    assert not torch.equal(whole.p, other.p), "index_offset 2^33 + 512 rounds like index_offset 512"
    assert torch.equal(whole.cm, other.cm) and torch.equal(whole.av, other.av)  # the moments do not depend on it


def check_sr_neighbours():
    n = 4381
    gen, p0, m0, v0 = _initial(n, 9)
    s = State8(p0, m0, v0, BF16)
    before, h, gs1 = _one_step(s, 3 * torch.randn(n, generator=gen), sr=1.0, ioff=256)
    fl, worst, fails, _d = verify_step(s, before, s.g.cpu(), h, gs1, sr=True)
    assert not fails, fails
    ref, _ = base.ref64(before[0].double(), s.g.cpu().double(), before[1].double(), before[2].double(), h, gs1)
    assert not torch.equal(s.p.cpu(), ref[0].to(BF16)), "stochastic rounding rounded to nearest everywhere"


def check_lds_patterns():
    """The kernel reads only what it wrote of the LDS: NaN-filled and zero-filled LDS give the same bits."""
    n = 4381
    gen, p0, m0, v0 = _initial(n, 10)
    g = 3 * torch.randn(n, generator=gen)
    outs = []
    for pattern in (0x7fc00000, 0):
        s = State8(p0, m0, v0, BF16)
        s.set_grad(g)
        hyper = base.make_hyper(LR, WD, 4, gscale=HSCALE, sr=1.0).to(DEV)
        _C().lds_fill(pattern, torch.cuda.current_device())
        s.launch(hyper, None)
        outs.append({k: f.buf.clone() for k, f in s.f.items()})
    for k in outs[0]:
        assert torch.equal(outs[0][k].view(U8), outs[1][k].view(U8)), k


EDGE_CHECKS = [check_zero_block, check_outlier_block, check_nan_gradient, check_slices_match_whole,
               check_sr_neighbours, check_lds_patterns]


@pytest.mark.parametrize("check", EDGE_CHECKS, ids=[c.__name__[6:] for c in EDGE_CHECKS])
def test_adamw8_edge(check):
    check()


# ----------------------------------------------------------------------------- the IEEE variants
def _sr_pattern():
    """Rounding decisions of a fixed input: the fast and the IEEE variant draw them from other hashes."""
    n = 256
    s = State8(torch.ones(n), torch.zeros(n), torch.zeros(n), BF16)
    hyper = base.make_hyper(2.0 ** -5, 2.0 ** -5, 4, sr=1.0).to(DEV)
    s.launch(hyper, None)
    return "".join("1" if x else "0" for x in s.p.float().ne(1.0).tolist())


def run_variant_checks():
    for n, v, mb in TRAJECTORY_CASES:
        check_trajectory(n, *VARIANTS[v], False, mb)
    for n, master in SHIFT_CASES:
        check_trajectory(n, BF16, master, True, 0)
    for c in EDGE_CHECKS:
        c()
    print("sr pattern " + _sr_pattern())


def test_adamw8_ieee_variants_in_child():
    """GRT_ADAMW_FASTMATH is read once per process, so the IEEE kernels run in one fresh child."""
    env = dict(os.environ, GRT_ADAMW_FASTMATH="0")
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=CHILD_TIMEOUT)
    print(r.stdout)
    print(f"the child took {time.perf_counter() - t0:.1f} s")
    assert r.returncode == 0, f"child exited with {r.returncode}:\n{r.stdout}"
    assert "variant checks passed" in r.stdout, r.stdout
    if os.environ.get("GRT_ADAMW_FASTMATH", "1")[:1] != "0":
        assert "sr pattern " + _sr_pattern() not in r.stdout, "the child ran the fast variant"


# ----------------------------------------------------------------------------- quantise / dequantise kernels
@pytest.mark.parametrize("signed", [True, False], ids=["signed", "unsigned"])
def test_quantize_dequantize_kernels(signed):
    C = _C()
    table = _ref.q8_table(signed)
    # the kernels' tables are the host's: every code with absmax 1, and every entry back to its code
    codes = Frame(torch.arange(256), U8, 8)
    one = Frame(torch.ones(1), F32, 3)
    out = Frame(torch.zeros(256), F32, 4)
    C.dequantize_blockwise8(codes.view, one.view, out.view, signed)
    assert torch.equal(out.view.cpu(), table)
    back = Frame(torch.zeros(256), U8, 8)
    amax = Frame(torch.zeros(1), F32, 3)
    C.quantize_blockwise8(out.view, back.view, amax.view, signed)
    assert torch.equal(back.view.cpu(), torch.arange(256, dtype=U8)) and amax.view.item() == 1.0
    # where the quantiser decides: every midpoint and every edge of its lookup cells (|x| with the low
    # 16 bits zero, from 2^-24 up), each with its two fp32 neighbours, in blocks led by 1.0 (absmax 1,
    # so x / absmax is x). The kernel divides as the host does: the codes are the host's exactly.
    t64 = table.double()
    mids = ((t64[1:] + t64[:-1]) / 2).to(F32)
    edges = (torch.arange((127 - 24) << 7, (127 << 7) + 1, dtype=torch.int32) << 16).view(F32)
    pts = torch.cat([mids, edges, -edges] if signed else [mids.abs(), edges])
    pts = torch.cat([pts, torch.nextafter(pts, torch.full_like(pts, 2.0)), torch.nextafter(pts, torch.full_like(pts, -2.0))])
    pts = pts.clamp(-1.0 if signed else 0.0, 1.0)
    pts = torch.cat([pts, torch.zeros((-pts.numel()) % 255)]).view(-1, 255)
    x = torch.cat([torch.ones(pts.shape[0], 1), pts], dim=1).reshape(-1)
    xf, cf, af = Frame(x, F32, 4), Frame(torch.zeros(x.numel()), U8, 8), Frame(torch.zeros(pts.shape[0]), F32, 3)
    C.quantize_blockwise8(xf.view, cf.view, af.view, signed)
    hc, ha = _ref.quantize_blockwise8(x, signed)
    assert bool((ha == 1).all()) and torch.equal(af.view.cpu(), ha)
    wrong = (cf.view.cpu() != hc).nonzero().flatten()
    assert wrong.numel() == 0, (wrong.numel(), x[wrong[:5]].tolist(), cf.view.cpu()[wrong[:5]].tolist(), hc[wrong[:5]].tolist())
    for n in SIZES:
        gen = torch.Generator().manual_seed(n)
        x = torch.randn(n, generator=gen) * torch.exp(4 * torch.randn(n, generator=gen))
        x = x if signed else x.abs()
        if n > 300:
            x[256:512] = 0  # an all-zero block
        xf, cf, af = Frame(x, F32, 4), Frame(torch.zeros(n), U8, 8), Frame(torch.zeros(_ref.q8_blocks(n)), F32, 3)
        C.quantize_blockwise8(xf.view, cf.view, af.view, signed)
        hc, ha = _ref.quantize_blockwise8(x, signed)
        c, a = cf.view.cpu(), af.view.cpu()
        assert torch.equal(a, ha), n
        ab = a.double()[torch.arange(n) // QB]
        err = (table.double()[c.long()] * ab - x.double()).abs()
        assert bool((err <= HALF[signed][c.long()] * ab + 2.0 ** -24 * x.double().abs()).all()), n
        print(f"quantize n={n}: {int((c != hc).sum())} codes differ from the host's")
        df = Frame(torch.zeros(n), F32, 4)
        C.dequantize_blockwise8(cf.view, af.view, df.view, signed)
        assert torch.equal(df.view.cpu(), _ref.dequantize_blockwise8(c, a, signed)), n  # one fp32 product
        # requantisation is the identity on the device too
        c2, a2 = Frame(torch.zeros(n), U8, 8), Frame(torch.zeros(_ref.q8_blocks(n)), F32, 3)
        C.quantize_blockwise8(df.view, c2.view, a2.view, signed)
        assert torch.equal(c2.view, cf.view) and torch.equal(a2.view, af.view), n
        for f in (xf, cf, af, df, c2, a2):
            assert f.intact(), n


# ----------------------------------------------------------------------------- argument checks
# Every operand stays inside a live device allocation for whatever a kernel without the guard would
# read or write, so a missing guard fails the test without a fault.
def _ops8(n=512, pdt=BF16):
    big = {k: torch.zeros(2 * n + 64, dtype=dt, device=DEV) for k, dt in
           (("p", pdt), ("g", pdt), ("cm", U8), ("cv", U8), ("am", F32), ("av", F32))}
    nb = n // QB
    return big, dict(p=big["p"][:n], g=big["g"][:n], cm=big["cm"][:n], am=big["am"][:nb], cv=big["cv"][:n],
                     av=big["av"][:nb], master=None, hyper=base.make_hyper(LR, WD, 4).to(DEV), gscale=None)


def _call8(o, max_blocks=0, ioff=0):
    _C().adamw8(o["p"], o["g"], o["cm"], o["am"], o["cv"], o["av"], o["master"], o["hyper"], o["gscale"], max_blocks, ioff)


def test_adamw8_refuses_bad_operands():
    n = 512
    big, good = _ops8(n)
    _call8(good)  # the operands as they are pass
    for k in big:
        big[k].zero_()
    f32 = torch.zeros(2 * n, dtype=F32, device=DEV)
    small = base._bad_small
    bad = [
        ("p and g", dict(g=f32[:n])), ("p and g", dict(p=f32[:n])),                  # mixed dtypes
        ("p and g", dict(p=big["p"][:n].to(torch.float16), g=big["g"][:n].to(torch.float16))),
        ("size mismatch", dict(g=big["g"][:n - 8])),
        ("contiguous", dict(p=big["p"][::2][:n])), ("contiguous", dict(g=big["g"][::2][:n])),
        ("contiguous", dict(cm=big["cm"][::2][:n])), ("contiguous", dict(av=big["av"][::2][:n // QB])),
        ("exp_avg: codes", dict(cm=big["cm"][:n - 1])), ("exp_avg_sq: codes", dict(cv=big["cv"][:n + 8])),
        ("exp_avg: codes", dict(cm=big["cm"][:n].to(torch.int8))),
        ("exp_avg: absmax", dict(am=big["am"][:1])), ("exp_avg_sq: absmax", dict(av=big["av"][:3])),
        ("exp_avg_sq: absmax", dict(av=big["av"][:2].double())),
        ("8-byte aligned", dict(cm=big["cm"][4:n + 4])), ("8-byte aligned", dict(cv=big["cv"][1:n + 1])),
        ("vector aligned", dict(p=big["p"][1:n + 1])), ("vector aligned", dict(g=big["g"][2:n + 2])),
        ("master", dict(master=f32[:n - 1])), ("master", dict(master=f32[:n].double())),
        ("master", dict(master=f32[1:n + 1])), ("contiguous", dict(master=f32[::2][:n])),
        ("GPU tensor", dict(p=torch.zeros(n, dtype=BF16))), ("GPU tensor", dict(cm=torch.zeros(n, dtype=U8))),
        ("GPU tensor", dict(hyper=base.make_hyper(LR, WD, 4))),
    ]
    for which in ("short", "strided", "float64"):
        bad.append(("hyper", dict(hyper=small(10)[which])))
        bad.append(("gscale", dict(gscale=small(2)[which])))
    for match, change in bad:
        with pytest.raises(RuntimeError, match=match):
            _call8(dict(good, **change))
    for ioff in (-256, 4, 128, 255, 257):
        with pytest.raises(RuntimeError, match="index_offset"):
            _call8(good, 0, ioff)
    # fp32 parameters take no master copy
    big32, good32 = _ops8(n, F32)
    with pytest.raises(RuntimeError, match="master"):
        _call8(dict(good32, master=f32[:n]))
    # refused before any launch
    for b in (big, big32):
        for k, t in b.items():
            assert not bool(t.any()), k
    assert not bool(f32.any())


def test_quantize_kernels_refuse_bad_operands():
    C = _C()
    n = 512
    x = torch.ones(2 * n, dtype=F32, device=DEV)
    codes = torch.zeros(2 * n, dtype=U8, device=DEV)
    absmax = torch.zeros(8, dtype=F32, device=DEV)
    for signed in (True, False):
        for match, a in (("fp32", (x[:n].to(BF16), codes[:n], absmax[:2])), ("codes", (x[:n], codes[:n - 1], absmax[:2])),
                         ("absmax", (x[:n], codes[:n], absmax[:1])), ("absmax", (x[:n], codes[:n], absmax[:3])),
                         ("contiguous", (x[::2][:n], codes[:n], absmax[:2])), ("8-byte", (x[:n], codes[4:n + 4], absmax[:2])),
                         ("GPU tensor", (x[:n].cpu(), codes[:n], absmax[:2]))):
            with pytest.raises(RuntimeError, match=match):
                C.quantize_blockwise8(*a, signed)
        out = torch.zeros(2 * n, dtype=F32, device=DEV)
        for match, a in (("fp32", (codes[:n], absmax[:2], out[:n].to(BF16))), ("codes", (codes[:n + 1], absmax[:2], out[:n])),
                         ("codes", (codes[:n].to(torch.int8), absmax[:2], out[:n])), ("absmax", (codes[:n], absmax[:4], out[:n])),
                         ("contiguous", (codes[:n], absmax[:2], out[::2][:n])), ("GPU tensor", (codes[:n].cpu(), absmax[:2], out[:n]))):
            with pytest.raises(RuntimeError, match=match):
                C.dequantize_blockwise8(*a, signed)
        assert not bool(codes.any()) and not bool(absmax.any()) and not bool(out.any())


# ----------------------------------------------------------------------------- the optimizer
TINY_STEPS = 20
# |final loss(AdamW8bit) - final loss(FusedAdamW)| of tiny_llama_final_loss() with the host reference
# (_ref.adamw8_ / _ref.adamw_ on CPU parameters), seeds 0, 1, 2: see test_tiny_llama_tracks_fused_adamw
TINY_CPU_DIFFS = (0.0157, 0.1039, 0.0475)
TINY_BOUND = 2 * max(TINY_CPU_DIFFS)


def tiny_llama_final_loss(cls, device, seed):
    """The tiny Llama in bf16, TINY_STEPS steps of lr 1e-3 on one fixed batch per step (round to nearest:
    the host reference has no stochastic rounding), then the loss on a held-out batch."""
    from gke_ray_train_amd.models import build_llama
    m = build_llama("llama-tiny", device=device, dtype=BF16, seed=seed)
    opt = cls([p for p in m.parameters() if p.requires_grad], lr=1e-3, weight_decay=0.01, stochastic_rounding=False)
    gen = torch.Generator().manual_seed(1000 + seed)
    batches = [torch.randint(0, 512, (4, 32), generator=gen) for _ in range(4)]
    held = torch.randint(0, 512, (4, 32), generator=gen).to(device)
    for s in range(TINY_STEPS):
        ids = batches[s % 4].to(device)
        m(ids, labels=ids)["loss"].backward()
        opt.step()
        opt.zero_grad(set_to_none=True)
    with torch.no_grad():
        first = m(batches[0].to(device), labels=batches[0].to(device))["loss"].float().item()
        return first, m(held, labels=held)["loss"].float().item(), opt


def test_tiny_llama_tracks_fused_adamw():
    """The tiny Llama in bf16, 20 steps, AdamW8bit against FusedAdamW from the same seed: the final loss
    (on the first training batch) differs by no more than twice the worst difference the host reference
    shows. Measured with _ref.adamw8_ / _ref.adamw_ on CPU parameters, the same function, seeds 0, 1, 2:
    final loss 3.2276 / 3.2434, 3.1271 / 3.2310, 3.4417 / 3.3942 (8-bit / 32-bit), differences 0.0157,
    0.1039, 0.0475; bound 2 x 0.1039 = 0.2078. (The loss falls from ln 512 = 6.24 to about 3.3 in these
    20 steps, so the bound is 7 % of the descent.)"""
    from gke_ray_train_amd.ops import AdamW8bit, FusedAdamW
    seed = 0
    t8, h8, opt8 = tiny_llama_final_loss(AdamW8bit, DEV, seed)
    t32, h32, _ = tiny_llama_final_loss(FusedAdamW, DEV, seed)
    print(f"final loss on a training batch: 8-bit {t8:.5f}, 32-bit {t32:.5f}, difference {abs(t8 - t32):.5f}; "
          f"held out: {h8:.5f} / {h32:.5f}; bound {TINY_BOUND}")
    assert t32 < 6.0, "20 steps must have learned the training batches"  # ln(512) = 6.24 at the start
    assert abs(t8 - t32) <= TINY_BOUND
    # optimizer-state bytes: 2 n + 8 ceil(n / 256) per 8-bit tensor, 8 n for the small ones
    n8 = 0
    for p, st in opt8.state.items():
        n = p.numel()
        held = sum(v.numel() * v.element_size() for k, v in st.items() if k != "step")
        if n >= opt8.min_8bit_size:
            n8 += 1
            assert set(st) == {"step", "exp_avg_q", "exp_avg_absmax", "exp_avg_sq_q", "exp_avg_sq_absmax"}
            assert held <= 2 * n + 8 * ((n + 255) // 256), (n, held)
        else:
            assert held == 8 * n
    assert n8 > 0 and opt8.state_bytes() < 0.27 * 8 * sum(p.numel() for p in opt8.state)


def _synthetic_steps(opt, params, steps):
    for s in steps:
        gen = torch.Generator().manual_seed(2000 + s)
        for p in params:
            p.grad = torch.randn(p.shape, generator=gen).to(p.dtype).to(DEV)
        opt.step()


def test_save_reload_continues_bit_for_bit():
    """Save at step 10, load into a fresh optimizer: step 11 is bitwise the uninterrupted run's (stochastic
    rounding on, its stream is keyed by the step; bf16 with and without a master copy; a small fp32-moment tensor)."""
    from gke_ray_train_amd.ops import AdamW8bit, FusedAdamW
    for master in (False, True):
        gen = torch.Generator().manual_seed(3)
        shapes = ((70, 70), (4381,), (70,))
        ps = [torch.nn.Parameter(torch.randn(s, generator=gen).to(BF16).to(DEV)) for s in shapes]
        opt = AdamW8bit(ps, lr=1e-2, master_weights=master)
        _synthetic_steps(opt, ps, range(10))
        sd = opt.state_dict()
        assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"} | ({"master"} if master else set())
        assert sd["state"][0]["exp_avg"].shape == (70, 70) and sd["state"][0]["exp_avg"].dtype == F32
        sd = {"state": {i: {k: v.clone() for k, v in st.items()} for i, st in sd["state"].items()},
              "param_groups": sd["param_groups"]}
        ps2 = [torch.nn.Parameter(p.detach().clone()) for p in ps]
        opt2 = AdamW8bit(ps2, lr=1e-2, master_weights=master)
        opt2.load_state_dict(sd)
        for p, q in zip(ps, ps2):
            for k, v in opt.state[p].items():
                assert torch.equal(v, opt2.state[q][k]), k
        _synthetic_steps(opt, ps, range(10, 11))
        _synthetic_steps(opt2, ps2, range(10, 11))
        for p, q in zip(ps, ps2):
            assert torch.equal(p, q)
            for k, v in opt.state[p].items():
                assert torch.equal(v, opt2.state[q][k]), k
        # the same state dict loads into the 32-bit optimizer
        ps3 = [torch.nn.Parameter(p.detach().clone()) for p in ps]
        opt3 = FusedAdamW(ps3, lr=1e-2, master_weights=master)
        opt3.load_state_dict(sd)
        assert opt3.state[ps3[1]]["exp_avg"].dtype == F32 and opt3.state[ps3[1]]["exp_avg"].is_cuda


def test_make_optimizer_builds_adamw8bit_on_gpu_parameters():
    from gke_ray_train_amd.ops import AdamW8bit, make_optimizer
    ps = [torch.nn.Parameter(torch.zeros(5000, dtype=BF16, device=DEV))]
    for name in ("paged_adamw_8bit", "adamw_8bit", "adamw_bnb_8bit"):
        opt = make_optimizer(name, [{"params": ps, "weight_decay": 0.0}], lr=1e-3, weight_decay=0.0)
        assert type(opt) is AdamW8bit
    with pytest.raises(ValueError, match="8-bit"):
        make_optimizer("adamw_8bit", ps + [torch.nn.Parameter(torch.zeros(4))], lr=1e-3, weight_decay=0.0)
    with pytest.raises(ValueError, match="8-bit"):
        make_optimizer("adamw_8bit", ps, lr=1e-3, weight_decay=0.0, offload=True)
    with pytest.raises(RuntimeError, match="step"):
        opt.prepare_gpu_step()


# ----------------------------------------------------------------------------- the SFT job
def test_sft_job_with_paged_adamw_8bit(tmp_path):
    """Full fine-tuning of the tiny model with OPTIM=paged_adamw_8bit at world 1: AdamW8bit on the plain
    step(grad_scale=...) path, checkpoint-<step>/optimizer.pt in the per-parameter layout (fp32 moments),
    and a resume from it that ends where the uninterrupted run ends. The optimizer state resumes exactly
    (requantisation is the identity on the same flat layout), so the bound is that of the 32-bit resume
    test in tests/test_gpu_jobs.py: 1e-2 of a tensor's largest magnitude, bf16 rounding through three steps."""
    from gke_ray_train_amd.models import build_llama
    from gke_ray_train_amd.ops import AdamW8bit
    from gke_ray_train_amd.trainer import SFTConfig, SFTTrainer
    rows = [{"text": "select a, b from t%d where c > %d order by b" % (i, 3 * i)} for i in range(48)]

    def make(out):
        torch.manual_seed(0)
        m = build_llama("llama-tiny-gqa", device="cuda", dtype=BF16, seed=3)
        tr = SFTTrainer(m, SFTConfig(output_dir=str(out), per_device_train_batch_size=2, gradient_accumulation_steps=2,
                                     learning_rate=1e-3, max_steps=6, logging_steps=2, save_steps=3,
                                     save_strategy="steps", max_seq_length=64, optim="paged_adamw_8bit",
                                     report_to="none", seed=1), train_dataset=rows)
        assert type(tr.optimizer) is AdamW8bit
        return m, tr

    ma, ta = make(tmp_path / "a")
    ta.train()
    torch.cuda.synchronize()
    losses = [h["loss"] for h in ta.state["log_history"] if "loss" in h]
    assert losses[-1] < losses[0], losses
    big = ta.optimizer.param_groups[0]["params"][0]
    assert ta.optimizer.state[big]["exp_avg_q"].dtype == U8
    ref = {k: v.float().clone() for k, v in ma.state_dict().items()}
    sd = torch.load(tmp_path / "a" / "checkpoint-3" / "optimizer.pt", weights_only=True)
    named = [(n, p) for n, p in ma.named_parameters() if p.requires_grad]
    assert sd["grt_param_names"] == [n for n, _ in named] and set(sd["state"]) == set(range(len(named)))
    for i, (_n, p) in enumerate(named):
        assert sd["state"][i]["exp_avg"].shape == p.shape and sd["state"][i]["exp_avg"].dtype == F32
        assert sd["state"][i]["exp_avg_sq"].dtype == F32 and float(sd["state"][i]["step"]) == 3
    mb, tb = make(tmp_path / "b")
    tb.train(resume_from_checkpoint=str(tmp_path / "a" / "checkpoint-3"))
    torch.cuda.synchronize()
    assert tb.state["global_step"] == 6
    worst = max((v.float() - ref[k]).abs().max().item() / max(1e-3, ref[k].abs().max().item())
                for k, v in mb.state_dict().items())
    print(f"resumed run against the uninterrupted one: worst relative difference {worst:.2e}")
    assert worst <= 1e-2, worst


if __name__ == "__main__":
    if sys.argv[1:] != ["--child"]:
        sys.exit("usage: test_adamw8_gpu.py --child (started by test_adamw8_ieee_variants_in_child)")
    run_variant_checks()
    print("variant checks passed")
