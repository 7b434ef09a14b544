"""The optimizer kernels (optim.hip: sumsq, clip_finalize, adamw, adamw_t, scale_) against float64
references, on the paths the sibling tests in test_kernels_gpu.py do not reach. Those anchor AdamW to
one step from zero moments, where Adam is degenerate (the update is lr * g / (|g| + eps) whatever
b1, b2 or the bias corrections do), and otherwise compare the kernel with itself.

Which test launches which path:

  fp32 master copy (master != nullptr) .......... test_adamw_trajectory[bf16-*-master-*]
  mixed dtypes <bf16, float> / <float, bf16> .... test_adamw_trajectory[bf16-f32-*], [f32-bf16-*]
  IEEE variants (GRT_ADAMW_FASTMATH=0), with the
    64-bit stochastic-rounding hash ............. test_ieee_variants_in_child (every check of this
                                                  file that launches adamw / adamw_t, in one child)
  max_blocks > 0, > 1 grid-stride iteration ..... test_adamw_trajectory[*-blocks2] (and the 4-wide
                                                  kernel at blocks0: 1027 groups on 768 threads)
  hyper[7] with gscale[1], steps from non-zero
    m, v, exp_avg_sq compared ................... test_adamw_trajectory, test_adamw_t_float64
  clip_finalize: prescale != 1, max_norm <= 0,
    norm below max_norm, all-zero gradients ..... test_sumsq_clip_finalize_float64
  scale_ and clip_grad_norm_(apply=True) ........ test_scale_bit_exact, test_clip_grad_norm_apply
  stochastic rounding away from p = 1.0 ......... test_sr_neighbours_and_mean (negative values, all
                                                  exponents of randn), test_sr_lanes_independent,
                                                  test_sr_index_offset_above_2_32,
                                                  test_adamw_t_float64[*-sr]
  the bindings' argument checks ................. test_*_refuses_*

Instantiations: a launch takes the 4-wide kernel only when an operand is 8- but not 16-byte aligned,
and the binding admits that for 2-byte elements alone. With fp32 parameters AND fp32 gradients every
operand is fp32, so adamw_kernel<float, float, 4, FAST / IEEE> cannot be reached through the
binding (the "+4 view" of that case starts 16 bytes in and runs the 8-wide kernel again); the other
14 of the 16 instantiations are launched here.

Reference and bound. ref64() is AdamW with decoupled decay in float64 on the ten hyper values as
uploaded (fp32 values taken as exact, bc1 / bc2 from the buffer), the gradient times
hyper[7] * gscale[1]. Every step is compared on its own: the reference starts from the state the
kernel left. Errors are normalised per element by 2^-23 times the magnitude of the terms summed:

  p: |d| / (2^-23 (|p decay| + |update|))   m: |d| / (2^-23 (|b1 m| + |(1 - b1) g|))
  v: |d| / (2^-23 |v_ref|)

and the bound is 4x the worst such error of fp32 ops/_ref.py::adamw_ on the CPU on the same inputs
(the floor; 4x covers the kernel's other fused-multiply-add order and the 1-ulp v_sqrt_f32 /
v_rcp_f32 of the fast variant), on every element. bf16 parameters without a master copy must be
within ulp_bf16(p_ref) / 2 + bound of the float64 value: the correctly rounded result. Learning rate
1e-2: large enough that a relative error of 1e-4 in the update term of a typical element (|p| ~ 1,
|update| ~ lr) exceeds the bound on p, 4 x 1.1 x 2^-23 |p|.

Measured on an MI355X over the 24 trajectory cases x 3 steps (p / m / v, in the units above; the
floors differ a little between the two runs because each starts its steps from its own kernel's state):

                      floors (fp32 _ref.adamw_)        kernel, worst case
  fast (default)      1.07-1.10 / 0.85-0.88 / 1.05-1.17   1.10 / 1.18 / 1.36
  GRT_ADAMW_FASTMATH=0  1.07-1.16 / 0.85-0.88 / 1.05-1.17   1.05 / 1.18 / 1.36

so both variants sit at about 1x the floor, well inside the 4x bound. For bf16 parameters without a
master copy the excess over ulp_bf16 / 2 is at most 0.09 units (both variants). adamw_t (one step):
floors 1.10-1.98 / 0.86-0.87 / 1.09-1.26, kernel excess 0.00 (fast) and 0.60 (IEEE) / 1.18 / 1.43.
Stochastic rounding, 2^16 elements: mean of (out - exact) / ulp at +0.75 sigma (fast) and +0.16 sigma
(IEEE); lane and step correlations at most 0.0047 against the bound 6 / sqrt(n) = 0.0234.
"""
import math
import os
import subprocess
import sys
import time

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:  # the child process starts from this file, not from pytest
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
N = 4109  # 8 * 513 + 5: three workgroups, an 8-wide body and a 5-element scalar tail
MARGIN = 4.0
LR, WD, HSCALE, GS1 = 1e-2, 0.01, 0.5, 0.37
SENTINEL = 7.0  # around every operand view: nothing outside the view may change
# the child imports torch, loads the extension and launches ~150 small kernels: 2.4-2.8 s observed on
# an MI355X host (2.8 s as the first process after a fresh checkout); 3x that, rounded up
CHILD_TIMEOUT = 10


def _C():
    from gke_ray_train_amd import _native
    return _native.kernels()


def _name(dt):
    return "bf16" if dt == BF16 else "f32"


# ----------------------------------------------------------------------------- references
def make_hyper(lr, wd, step, gscale=1.0, sr=0.0, b1=0.9, b2=0.999, eps=1e-8):
    """The ten values in the order the kernels read them. The bias corrections come from the betas as
    rounded to fp32, so that ref64 (which reads bc1 / bc2 from the buffer) and _ref.adamw_ (which derives
    them from the betas it is given) see the same ones to within their fp32 rounding; with bc2 from
    the unrounded 0.999 the two would differ by 1e-5 at step 4."""
    b1, b2 = (torch.tensor(b, dtype=F32).item() for b in (b1, b2))
    return torch.tensor([lr, b1, b2, eps, wd, 1.0 - b1 ** step, 1.0 - b2 ** step, gscale, sr, step], dtype=F32)


def ref64(p, g, m, v, h, gs1):
    """One AdamW step in float64. p, g, m, v: float64 tensors; h: the uploaded hyper values as Python
    floats; gs1: gscale[1]. Returns the new (p, m, v) and the per-element error units of each."""
    lr, b1, b2, eps, wd, bc1, bc2, h7 = h[:8]
    gf = g * (h7 * gs1)
    m2 = b1 * m + (1.0 - b1) * gf
    v2 = b2 * v + (1.0 - b2) * gf * gf
    decay = 1.0 - lr * wd
    update = (lr / bc1) * m2 / (v2.sqrt() / math.sqrt(bc2) + eps)
    p2 = p * decay - update
    u = 2.0 ** -23
    units = (u * ((p * decay).abs() + update.abs()), u * ((b1 * m).abs() + ((1.0 - b1) * gf).abs()), u * v2.abs())
    return (p2, m2, v2), units


def floor32(p, g, m, v, h, gs1, ref, units):
    """Worst normalised error of fp32 _ref.adamw_ on the CPU on the same inputs: p, m, v fp32 tensors, g in
    its own dtype."""
    from gke_ray_train_amd.ops import _ref
    pc, mc, vc = p.clone(), m.clone(), v.clone()
    _ref.adamw_(pc, g, mc, vc, h[9], h[0], h[1], h[2], h[3], h[4], grad_scale=h[7] * gs1)
    return [((x.double() - r).abs() / s).max().item() for x, r, s in zip((pc, mc, vc), ref, units)]


def ulp_bf16(x):
    """Spacing of bf16 (8 significant bits) at |x|, float64."""
    _, e = torch.frexp(x.abs())  # |x| = f * 2^e with f in [0.5, 1)
    return torch.ldexp(torch.ones_like(x), e - 8)


def _worst(err, unit):
    return (err / unit).max().item()


# ----------------------------------------------------------------------------- adamw: trajectory
def _framed(x, dtype, lo):
    """x inside a buffer of len(x) + 8 sentinels, lo elements in; returns (buffer, view)."""
    buf = torch.full((x.numel() + 8,), SENTINEL, dtype=dtype, device=DEV)
    view = buf[lo:lo + x.numel()]
    view.copy_(x.to(dtype))
    return buf, view


def _frame_intact(buf, lo, n):
    return bool((buf[:lo] == SENTINEL).all()) and bool((buf[lo + n:] == SENTINEL).all())


def check_trajectory(pdt, gdt, master, shift, max_blocks):
    """Three consecutive steps (hyper[9] = 4, 5, 6) from random non-zero moments, each compared with
    ref64 started from the state the kernel left. Returns (floors, worst) as [p, m, v]."""
    C = _C()
    gen = torch.Generator().manual_seed(1234)
    lo = 4 if shift else 0
    p0 = torch.randn(N, generator=gen)
    bufs = {}
    if master:
        # the parameter itself starts as zeros: the step must read the master copy, not p
        bufs["master"], mas = _framed(p0, F32, lo)
        bufs["p"], p = _framed(torch.zeros(N), pdt, lo)
    else:
        mas = None
        bufs["p"], p = _framed(p0, pdt, lo)
    bufs["m"], m = _framed(0.01 * torch.randn(N, generator=gen), F32, lo)
    bufs["v"], v = _framed(0.01 * torch.rand(N, generator=gen), F32, lo)
    gsc = torch.tensor([123.0, GS1], dtype=F32).to(DEV)
    gs1 = float(gsc[1])
    floors, worst, fails = [0.0] * 3, [0.0] * 3, []
    steps = []
    for step in (4, 5, 6):
        bufs["g"], g = _framed(3 * torch.randn(N, generator=gen), gdt, lo)
        hyper = make_hyper(LR, WD, step, gscale=HSCALE).to(DEV)
        h = hyper.cpu().double().tolist()
        before = [(mas if master else p).cpu().float().clone(), m.cpu().clone(), v.cpu().clone()]
        C.adamw(p, g, m, v, mas, hyper, gsc, max_blocks, 0)
        gc = g.cpu()
        ref, units = ref64(before[0].double(), gc.double(), before[1].double(), before[2].double(), h, gs1)
        fl = floor32(before[0], gc, before[1], before[2], h, gs1, ref, units)
        floors = [max(a, b) for a, b in zip(floors, fl)]
        steps.append((step, ref, units, (mas if master else p).cpu().double(), m.cpu().double(), v.cpu().double(),
                      p.cpu().clone(), None if mas is None else mas.cpu().clone()))
        for k, b in bufs.items():
            if not _frame_intact(b, lo, N):
                fails.append(f"step {step}: the kernel wrote outside the {k} view")
    for step, ref, units, pk, mk, vk, p_raw, mas_raw in steps:
        errs = [(pk - ref[0]).abs(), (mk - ref[1]).abs(), (vk - ref[2]).abs()]
        if pdt == BF16 and not master:  # the correctly rounded bf16 of the float64 value
            errs[0] = (errs[0] - ulp_bf16(ref[0]) / 2).clamp_min(0.0)
        if master and not torch.equal(p_raw, mas_raw.to(pdt)):
            fails.append(f"step {step}: p is not the rounded master copy")
        for i, what in enumerate("pmv"):
            w = _worst(errs[i], units[i])
            worst[i] = max(worst[i], w)
            if not w <= MARGIN * floors[i]:
                fails.append(f"step {step}: {what} is {w:.2f} units off, bound {MARGIN} x {floors[i]:.2f}")
    tag = f"{_name(pdt)}/{_name(gdt)} master={int(master)} shift={int(shift)} max_blocks={max_blocks}"
    print(f"trajectory {tag}: floors p/m/v " + " ".join(f"{x:.2f}" for x in floors) +
          "  kernel " + " ".join(f"{x:.2f}" for x in worst))
    assert not fails, f"{tag}: " + "; ".join(fails)
    return floors, worst


TRAJECTORY_CASES = [(pdt, gdt, master, shift, mb)
                    for pdt, gdt in ((BF16, BF16), (BF16, F32), (F32, BF16), (F32, F32))
                    for master in ((False, True) if pdt == BF16 else (False,))
                    for shift in (False, True)
                    for mb in (0, 2)]


def _traj_id(c):
    return f"{_name(c[0])}-{_name(c[1])}-{'master' if c[2] else 'nomaster'}-{'plus4' if c[3] else 'aligned'}-blocks{c[4]}"


@pytest.mark.parametrize("case", TRAJECTORY_CASES, ids=_traj_id)
def test_adamw_trajectory(case):
    check_trajectory(*case)


# ----------------------------------------------------------------------------- adamw: stochastic rounding
def _sr_decay_only(p_cpu, lr, wd, step, ioff=0, cuts=None):
    """One stochastically rounded step with g = 0 and m = v = 0 (bf16, no master copy): the fp32 result
    is exactly p * (1 - lr * wd). Launched over the slices cuts of the buffer (default: the whole)."""
    C = _C()
    n = p_cpu.numel()
    p = p_cpu.clone().to(DEV)
    g = torch.zeros(n, dtype=BF16, device=DEV)
    m = torch.zeros(n, dtype=F32, device=DEV)
    v = torch.zeros(n, dtype=F32, device=DEV)
    hyper = make_hyper(lr, wd, step, sr=1.0).to(DEV)
    cuts = cuts or [0, n]
    for a, b in zip(cuts[:-1], cuts[1:]):
        C.adamw(p[a:b], g[a:b], m[a:b], v[a:b], None, hyper, None, 0, ioff + a)
    assert not bool(m.any()) and not bool(v.any()), "zero gradient and moments must leave zero moments"
    return p.cpu()


def _bits(x):
    return x.float().view(torch.int32).to(torch.int64) & 0xffffffff


def _sr_events(p_cpu, out, decay):
    """(exact fp32 value's bf16 neighbours hold the output, rounded-away-from-zero event, fraction)."""
    exact = p_cpu.float() * decay  # 8 x 7 significant bits: exact in fp32
    assert torch.equal(exact.double(), p_cpu.double() * decay)
    u, o = _bits(exact), _bits(out)
    low = u & 0xffff
    down = u - low  # truncation towards zero: the neighbour of smaller magnitude
    ok = (o == down) | ((o == down + 0x10000) & (low != 0))
    return ok, (o != down), low.double() / 65536.0


def check_sr_neighbours_and_mean():
    n = 1 << 16
    p = torch.randn(n, generator=torch.Generator().manual_seed(77)).to(BF16)
    out = _sr_decay_only(p, 2.0 ** -3, 2.0 ** -4, 4)
    ok, up, frac = _sr_events(p, out, 1.0 - 2.0 ** -7)
    assert bool(ok.all()), f"{int((~ok).sum())} outputs are not a bf16 neighbour of the exact value"
    assert (frac > 0).double().mean().item() > 0.9, "the inputs must fall between two bf16 values"
    # (out - exact) / ulp is 1 - f with probability f and -f otherwise (towards / away from zero): mean 0,
    # variance f (1 - f) per element; signed by the value's sign and unsigned (a bias towards zero
    # cancels in the signed sum of a symmetric sample)
    d = up.double() - frac
    sigma = (frac * (1 - frac)).sum().sqrt().item() / n
    signed = (d * torch.sign(p.double())).mean().item()
    unsigned = d.mean().item()
    print(f"sr mean: signed {signed / sigma:+.2f} sigma, by magnitude {unsigned / sigma:+.2f} sigma")
    assert abs(signed) <= 6 * sigma and abs(unsigned) <= 6 * sigma, (signed, unsigned, sigma)


def _corr(a, b):
    a, b = a.double() - a.double().mean(), b.double() - b.double().mean()
    return ((a * b).mean() / (a.pow(2).mean().sqrt() * b.pow(2).mean().sqrt())).item()


def check_sr_lanes_independent():
    """p = 1, decay 1 - 2^-10: the exact value lies 1/4 of the bf16 spacing below 1.0, so an element
    rounds down (to 1 - 2^-8) with probability 1/4. The four 16-bit lanes cut from one hash, and the
    same element at two steps, must decide independently."""
    n = 1 << 16
    p = torch.ones(n, dtype=BF16)
    down = {}
    for step in (4, 5):
        out = _sr_decay_only(p, 2.0 ** -5, 2.0 ** -5, step).float()
        assert bool(((out == 1.0) | (out == 1.0 - 2.0 ** -8)).all())
        down[step] = out != 1.0
        rate = down[step].double().mean().item()
        assert abs(rate - 0.25) <= 6 * (0.25 * 0.75 / n) ** 0.5, f"step {step}: rounds down at rate {rate}"
    bound = 6 / n ** 0.5
    cs = [_corr(down[4][:-k], down[4][k:]) for k in (1, 2, 3)] + [_corr(down[4], down[5])]
    print("sr correlations (i, i+1..3; steps 4, 5): " + " ".join(f"{c:+.4f}" for c in cs) + f"  bound {bound:.4f}")
    assert all(abs(c) <= bound for c in cs), (cs, bound)


def check_sr_index_offset():
    """The random stream is keyed by the 64-bit flat index: bits above 2^32 count, and slices launched
    with matching offsets (the second one 8-byte aligned: the 4-wide kernel) round like the whole."""
    p = torch.randn(N, generator=torch.Generator().manual_seed(78)).to(BF16)
    big = (1 << 33) + 8
    whole = _sr_decay_only(p, 2.0 ** -3, 2.0 ** -4, 4, ioff=big)
    ok, _, _ = _sr_events(p, whole, 1.0 - 2.0 ** -7)
    assert bool(ok.all())
    small = _sr_decay_only(p, 2.0 ** -3, 2.0 ** -4, 4, ioff=8)
    assert not torch.equal(whole, small), "index_offset 2^33 + 8 rounds like index_offset 8"
    sliced = _sr_decay_only(p, 2.0 ** -3, 2.0 ** -4, 4, ioff=big, cuts=[0, 1028, N])
    assert torch.equal(whole, sliced), "two slices with matching offsets differ from the whole"


def test_sr_neighbours_and_mean():
    check_sr_neighbours_and_mean()


def test_sr_lanes_independent():
    check_sr_lanes_independent()


def test_sr_index_offset_above_2_32():
    check_sr_index_offset()


# ----------------------------------------------------------------------------- adamw_t
def check_adamw_t(rows, cols, off, sr):
    C = _C()
    gen = torch.Generator().manual_seed(4321)
    p0 = torch.randn(rows, cols, generator=gen).to(BF16)
    g = (3 * torch.randn(rows, cols, generator=gen)).to(BF16)
    m0 = 0.01 * torch.randn(rows, cols, generator=gen)
    v0 = 0.01 * torch.rand(rows, cols, generator=gen)
    hyper = make_hyper(LR, WD, 4, gscale=HSCALE, sr=float(sr)).to(DEV)
    gsc = torch.tensor([123.0, GS1], dtype=F32).to(DEV)
    h, gs1 = hyper.cpu().double().tolist(), float(gsc[1])
    p, m, v = p0.clone().to(DEV), m0.clone().to(DEV), v0.clone().to(DEV)
    pt = torch.full((cols, rows), SENTINEL, dtype=BF16, device=DEV)
    C.adamw_t(p, g.to(DEV), m, v, hyper, gsc, pt, off)
    assert torch.equal(pt, p.t()), "pt is not the transpose of the updated p"
    ref, units = ref64(p0.double(), g.double(), m0.double(), v0.double(), h, gs1)
    floors = floor32(p0.float(), g, m0, v0, h, gs1, ref, units)
    errs = [(x.cpu().double() - r).abs() for x, r in zip((p, m, v), ref)]
    if sr:  # one of the two bf16 neighbours of the fp32 value, itself within the bound of ref
        out = p.cpu().double()
        errs[0] = (errs[0] - ulp_bf16(torch.maximum(out.abs(), ref[0].abs()))).clamp_min(0.0)
        assert not torch.equal(p.cpu(), ref[0].to(BF16)), "stochastic rounding rounded to nearest everywhere"
    else:
        errs[0] = (errs[0] - ulp_bf16(ref[0]) / 2).clamp_min(0.0)
    worst = [_worst(e, s) for e, s in zip(errs, units)]
    print(f"adamw_t {rows}x{cols} sr={int(sr)}: floors p/m/v " + " ".join(f"{x:.2f}" for x in floors) +
          "  kernel " + " ".join(f"{x:.2f}" for x in worst))
    for w, f, what in zip(worst, floors, "pmv"):
        assert w <= MARGIN * f, f"{what} is {w:.2f} units off, bound {MARGIN} x {f:.2f}"


ADAMW_T_CASES = [(64, 128, 0), (128, 256, 1 << 20)]  # one tile; four tiles at a non-zero index offset


@pytest.mark.parametrize("sr", [False, True], ids=["rne", "sr"])
@pytest.mark.parametrize("rows,cols,off", ADAMW_T_CASES, ids=["1tile", "4tiles"])
def test_adamw_t_float64(rows, cols, off, sr):
    check_adamw_t(rows, cols, off, sr)


# ----------------------------------------------------------------------------- the IEEE variants
def _sr_pattern():
    """Rounding decisions of a fixed input: the fast and the IEEE variant draw them from other hashes."""
    out = _sr_decay_only(torch.ones(256, dtype=BF16), 2.0 ** -5, 2.0 ** -5, 4)
    return "".join("1" if x else "0" for x in out.float().ne(1.0).tolist())


def run_variant_checks():
    """Every check of this file that launches adamw / adamw_t, for whichever variant this process runs."""
    floors, worst = [0.0] * 3, [0.0] * 3
    for case in TRAJECTORY_CASES:
        f, w = check_trajectory(*case)
        floors = [max(a, b) for a, b in zip(floors, f)]
        worst = [max(a, b) for a, b in zip(worst, w)]
    print("trajectory, all cases: floors p/m/v " + " ".join(f"{x:.2f}" for x in floors) +
          "  kernel " + " ".join(f"{x:.2f}" for x in worst))
    check_sr_neighbours_and_mean()
    check_sr_lanes_independent()
    check_sr_index_offset()
    for rows, cols, off in ADAMW_T_CASES:
        for sr in (False, True):
            check_adamw_t(rows, cols, off, sr)
    print("sr pattern " + _sr_pattern())


def test_ieee_variants_in_child():
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
        # the child ran other kernels than this process: 256 decisions drawn from another hash
        assert "sr pattern " + _sr_pattern() not in r.stdout, "the child ran the fast variant"


# ----------------------------------------------------------------------------- sumsq + clip_finalize
CLIP_SIZES = ((1, BF16), (7, F32), (2061, BF16))  # tail only; tail only; 8-wide body + 5-element tail


def _clip_run(grads, max_norm, prescale):
    C = _C()
    nb = C.sumsq_blocks()
    ws = torch.full((len(grads) * nb,), float("nan"), dtype=F32, device=DEV)  # every partial must be written
    out = torch.full((2,), float("nan"), dtype=F32, device=DEV)
    for i, g in enumerate(grads):
        C.sumsq(g, ws, i)
    C.clip_finalize(ws, len(grads) * nb, max_norm, prescale, out)
    return out.cpu()


def test_sumsq_clip_finalize_float64():
    gen = torch.Generator().manual_seed(9)
    grads = [torch.randn(n, generator=gen).to(dt) for n, dt in CLIP_SIZES]
    dev = [g.to(DEV) for g in grads]
    prescale = 0.125
    norm64 = math.sqrt(sum(g.double().pow(2).sum().item() for g in grads)) * prescale
    assert norm64 > 0.3
    out = _clip_run(dev, 0.3, prescale)
    coef64 = min(1.0, 0.3 / (norm64 + 1e-6)) * prescale
    print(f"norm {out[0].item():.9g} vs {norm64:.9g}, coefficient {out[1].item():.9g} vs {coef64:.9g}")
    assert abs(out[0].item() - norm64) <= 1e-5 * norm64
    assert abs(out[1].item() - coef64) <= 1e-5 * coef64
    for max_norm in (1e9, 0.0):  # no clipping: the norm is below max_norm / clipping is off
        out = _clip_run(dev, max_norm, prescale)
        assert abs(out[0].item() - norm64) <= 1e-5 * norm64
        assert out[1].item() == prescale, (max_norm, out[1].item())
    for max_norm in (0.3, 0.0):
        out = _clip_run([torch.zeros_like(g) for g in dev], max_norm, prescale)
        assert out[0].item() == 0.0 and out[1].item() == prescale, (max_norm, out.tolist())


SCALE_SIZES = (1, 255, 771)


@pytest.mark.parametrize("n", SCALE_SIZES)
@pytest.mark.parametrize("dtype", [BF16, F32], ids=_name)
def test_scale_bit_exact(dtype, n):
    """scale_ is one fp32 multiply and one rounding, with the factor as an argument or read from the device."""
    C = _C()
    x0 = torch.randn(n, generator=torch.Generator().manual_seed(n)).to(dtype)
    for factor, by_pointer in ((0.3, False), (-1.7, True)):
        s = torch.tensor(factor, dtype=F32)
        buf, x = _framed(x0, dtype, 0)
        if by_pointer:  # the argument is ignored
            C.scale_(x, 123.0, torch.tensor([99.0, factor], dtype=F32).to(DEV)[1:2])
        else:
            C.scale_(x, factor, None)
        assert torch.equal(x.cpu(), (x0.float() * s).to(dtype)), (factor, by_pointer)
        assert _frame_intact(buf, 0, n)


@pytest.mark.parametrize("n", SCALE_SIZES)
@pytest.mark.parametrize("dtype", [BF16, F32], ids=_name)
def test_clip_grad_norm_apply(dtype, n):
    from gke_ray_train_amd.ops import clip_grad_norm_
    gen = torch.Generator().manual_seed(100 + n)
    g0 = [(2 * torch.randn(n, generator=gen)).to(dtype), torch.randn(5, generator=gen).to(dtype)]
    grads = [g.to(DEV) for g in g0]
    st = clip_grad_norm_(grads, 0.3, prescale=0.5, apply=True)
    norm64 = math.sqrt(sum(g.double().pow(2).sum().item() for g in g0)) * 0.5
    coef64 = min(1.0, 0.3 / (norm64 + 1e-6)) * 0.5
    buf = st.buf.cpu()
    assert abs(buf[0].item() - norm64) <= 1e-5 * norm64 and abs(buf[1].item() - coef64) <= 1e-5 * coef64
    for g, g_in in zip(grads, g0):
        assert torch.equal(g.cpu(), (g_in.float() * buf[1]).to(dtype))


# ----------------------------------------------------------------------------- argument checks
# Every operand below stays inside a live device allocation for whatever a kernel without the guard
# would read or write, so a missing guard fails the test without a fault.
def _adamw_operands(n=64, shape=None):
    shape = shape or (n,)
    p = torch.ones(shape, dtype=BF16, device=DEV)
    g = torch.ones(shape, dtype=BF16, device=DEV)
    m = torch.zeros(shape, dtype=F32, device=DEV)
    v = torch.zeros(shape, dtype=F32, device=DEV)
    return p, g, m, v


def _bad_small(min_numel):
    """Views of a 64-element buffer that must be refused where min_numel fp32 values are required."""
    big = torch.ones(64, dtype=F32, device=DEV)
    return {"short": big[:min_numel - 1], "strided": big[::2][:min_numel],
            "float64": torch.ones(64, dtype=F64, device=DEV)[:min_numel]}


@pytest.mark.parametrize("which", ["short", "strided", "float64"])
def test_adamw_refuses_bad_gscale_and_hyper(which):
    C = _C()
    p, g, m, v = _adamw_operands()
    hyper = make_hyper(LR, WD, 4).to(DEV)
    good_gs = torch.ones(2, dtype=F32, device=DEV)
    with pytest.raises(RuntimeError, match="gscale"):
        C.adamw(p, g, m, v, None, hyper, _bad_small(2)[which], 0, 0)
    with pytest.raises(RuntimeError, match="hyper"):
        C.adamw(p, g, m, v, None, _bad_small(10)[which], good_gs, 0, 0)
    p2, g2, m2, v2 = _adamw_operands(shape=(64, 128))
    pt = torch.zeros(128, 64, dtype=BF16, device=DEV)
    with pytest.raises(RuntimeError, match="gscale"):
        C.adamw_t(p2, g2, m2, v2, hyper, _bad_small(2)[which], pt, 0)
    with pytest.raises(RuntimeError, match="hyper"):
        C.adamw_t(p2, g2, m2, v2, _bad_small(10)[which], good_gs, pt, 0)
    for t in (p, p2):  # refused before any launch
        assert bool((t == 1).all())
    assert not bool(m.any()) and not bool(m2.any()) and not bool(pt.any())


def test_clip_finalize_refuses_bad_operands():
    C = _C()
    big = torch.ones(4096, dtype=F32, device=DEV)
    ws = big[:1024]
    out = torch.full((2,), -1.0, dtype=F32, device=DEV)
    for nparts in (1025, 4096, -1):
        with pytest.raises(RuntimeError, match="nparts"):
            C.clip_finalize(ws, nparts, 1.0, 1.0, out)
    with pytest.raises(RuntimeError, match="fp32"):
        C.clip_finalize(torch.ones(1024, dtype=F64, device=DEV), 1024, 1.0, 1.0, out)
    wide = torch.full((8,), -1.0, dtype=F32, device=DEV)
    for bad in (wide[::2][:2], wide[:1], wide.to(F64)[:2]):
        with pytest.raises(RuntimeError, match="out"):
            C.clip_finalize(ws, 1024, 1.0, 1.0, bad)
    assert bool((out == -1).all()) and bool((wide == -1).all())
    C.clip_finalize(ws, 0, 1.0, 1.0, out)  # an empty sum is legal
    assert out.tolist() == [0.0, 1.0]


def test_sumsq_refuses_negative_slot():
    C = _C()
    nb = C.sumsq_blocks()
    big = torch.full((3 * nb,), -1.0, dtype=F32, device=DEV)
    x = torch.ones(16, dtype=F32, device=DEV)
    with pytest.raises(RuntimeError, match="slot"):
        C.sumsq(x, big[nb:], -1)  # slot -1 of this view is big[:nb]
    with pytest.raises(RuntimeError, match="ws"):
        C.sumsq(x, big[:2 * nb], 2)
    assert bool((big == -1).all())


def test_scale_refuses_bad_pointer():
    C = _C()
    x = torch.ones(16, dtype=BF16, device=DEV)
    big = torch.full((8,), 2.0, dtype=F32, device=DEV)
    for bad in (big[:0], big.to(F64)[:1], big.to(BF16)[:1]):
        with pytest.raises(RuntimeError, match="a_ptr"):
            C.scale_(x, 1.0, bad)
    assert bool((x == 1).all())


if __name__ == "__main__":
    if sys.argv[1:] != ["--child"]:
        sys.exit("usage: test_optim_kernels_gpu.py --child (started by test_ieee_variants_in_child)")
    run_variant_checks()
    print("variant checks passed")
