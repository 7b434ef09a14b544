"""RMSNorm / LayerNorm, GELU and scale+PE kernels on the paths the sibling tests in
test_kernels_gpu.py do not reach: the multi-row (grid-strided) norm backward, every LayerNorm
variant and width template, rows with a large mean, the weight gradient written into a gradient
slot, padded output rows, the width limit, the bindings' argument checks, empty inputs, and the
second grid-stride iteration of the elementwise kernels.

Every reference is float64 on the same, already rounded inputs. For the fused residual the
reference starts from h = x + residual rounded to the input dtype, as the kernel rounds it."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS = 1e-5
BF16, F32 = torch.bfloat16, torch.float32


def _id(v):
    return str(v).replace("torch.", "")


def _C():
    from gke_ray_train_amd import _native
    return _native.kernels()


def _vec(dtype):
    return 8 if dtype == BF16 else 4


def _max_d(dtype):  # 2048 sixteen-byte chunks: the widest row norm.hip's templates cover
    return 2048 * _vec(dtype)


def _close(a, b, atol, rtol, what=""):  # as in test_kernels_gpu.py
    a, b = a.float(), b.float()
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    bad = (err > tol)
    assert not torch.isnan(a).any(), f"{what}: NaN in kernel output"
    assert bad.float().mean().item() < 1e-3, f"{what}: max err {err.max().item():.4g} (mean {err.mean().item():.3g})"
    # no element may be far off: a wrong row / tile edge fails even if it is < 0.1 % of the tensor
    worst = (err / tol).max().item()
    assert worst <= 10.0, f"{what}: an element is {worst:.1f}x its tolerance (max err {err.max().item():.4g})"


# ----------------------------------------------------------------------------- norm helpers
def _norm_inputs(rows, d, dtype, seed, residual, bias):
    g = torch.Generator(device=DEV).manual_seed(seed)

    def rn(*shape):
        return torch.randn(*shape, device=DEV, dtype=torch.float32, generator=g)

    x = rn(rows, d).to(dtype)
    r = rn(rows, d).to(dtype) if residual else None
    w = (1 + 0.1 * rn(d)).to(dtype)
    b = (0.1 * rn(d)).to(dtype) if bias else None
    gy = rn(rows, d).to(dtype)
    gh = rn(rows, d).to(dtype)
    return x, r, w, b, gy, gh


def _norm_ref64(kind, x, r, w, b, gy, gh=None):
    """float64 norm of h = x (+ r, rounded to the input dtype like the kernel's h) and its gradients
    for upstream gy on y and gh on h."""
    h = (x if r is None else x + r).double().requires_grad_()
    wd = w.double().requires_grad_()
    bd = None if b is None else b.double().requires_grad_()
    if kind == "rms":
        y = h * torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + EPS) * wd
    else:
        y = F.layer_norm(h, (h.shape[-1],), wd, bd, EPS)
    loss = (y * gy.double()).sum()
    if gh is not None:
        loss = loss + (h * gh.double()).sum()
    loss.backward()
    return dict(y=y.detach(), h=h.detach(), dx=h.grad, dw=wd.grad, db=None if bd is None else bd.grad)


def _norm_run(kind, x, r, w, b, gy, gh=None):
    """The public op on the GPU; gh: a gradient into the h output of add_rms_norm (the RES backward)."""
    from gke_ray_train_amd import ops
    xs = x.clone().requires_grad_()
    rs = None if r is None else r.clone().requires_grad_()
    ws = w.clone().requires_grad_()
    bs = None if b is None else b.clone().requires_grad_()
    h = None
    if kind == "rms" and r is None:
        y = ops.rms_norm(xs, ws, EPS)
    elif kind == "rms":
        y, h = ops.add_rms_norm(xs, rs, ws, EPS)
    else:
        # with b=None autograd itself rejects a non-None gradient for the bias input, so a backward
        # that runs proves that layer_norm returned None for db
        y = ops.layer_norm(xs, ws, bs, EPS, residual=rs)
    if h is not None and gh is not None:
        torch.autograd.backward([y, h], [gy, gh])
    else:
        y.backward(gy)
    return dict(y=y.detach(), h=None if h is None else h.detach(), dx=xs.grad,
                dres=None if rs is None else rs.grad, dw=ws.grad, db=None if bs is None else bs.grad)


def _norm_compare(kind, out, ref, dtype, what):
    """The sibling tests' tolerances (test_rmsnorm / test_layernorm)."""
    tol = 2e-2 if dtype == BF16 else 1e-4
    kw = 20 if kind == "rms" else 30
    _close(out["y"], ref["y"], tol, tol, f"{what} y")
    if out["h"] is not None:
        _close(out["h"], ref["h"], tol, tol, f"{what} h")
    _close(out["dx"], ref["dx"], tol * 5, tol, f"{what} dx")
    if out["dres"] is not None:
        _close(out["dres"], ref["dx"], tol * 5, tol, f"{what} dres")
    _close(out["dw"], ref["dw"], tol * kw, tol * 2, f"{what} dw")
    assert (out["db"] is None) == (ref["db"] is None), f"{what}: db presence"
    if ref["db"] is not None:
        _close(out["db"], ref["db"], tol * 30, tol * 2, f"{what} db")


# ----------------------------------------------------------------------------- A: multi-row backward
# Above 512 rows a backward workgroup visits several rows, keeps dw / db partial sums across them
# and prefetches the row one grid stride ahead (clamped). 513: one workgroup takes two rows;
# 1025: one takes three; 1337: a mix of two and three. op: rms / add (fused residual, gradient
# into h) / ln / lnres. A Latin square of (rows, d) per op, plus the largest case for add and ln.
_A_PAIRS = {
    "rms": [(513, 64), (1025, 520), (1337, 2056)],
    "add": [(513, 520), (1025, 2056), (1337, 64), (1337, 2056)],
    "ln": [(513, 2056), (1025, 64), (1337, 520), (1337, 2056)],
    "lnres": [(513, 64), (1025, 520), (1337, 2056)],
}
_A_CASES = [(op, rows, d, dt) for op, pairs in _A_PAIRS.items() for rows, d in pairs for dt in (BF16, F32)]


@pytest.mark.parametrize("op,rows,d,dtype", _A_CASES, ids=_id)
def test_norm_multirow_backward(op, rows, d, dtype):
    kind = "rms" if op in ("rms", "add") else "ln"
    x, r, w, b, gy, gh = _norm_inputs(rows, d, dtype, seed=rows * 31 + d, residual=op in ("add", "lnres"),
                                      bias=kind == "ln")
    gh = gh if op == "add" else None
    out = _norm_run(kind, x, r, w, b, gy, gh)
    ref = _norm_ref64(kind, x, r, w, b, gy, gh)
    _norm_compare(kind, out, ref, dtype, f"{op} {rows}x{d}")


# ----------------------------------------------------------------------------- B: LayerNorm variants
# widths around the template edges (V = 16-byte vector): one chunk; below one wave of chunks (bf16);
# one chunk past a wave; one chunk in the backward's second per-thread slot; the maximum (FULL)
def _b_cases():
    cases = []
    for dt in (BF16, F32):
        for wi, d in enumerate((_vec(dt), 504, 520, 2056, _max_d(dt))):
            for vi, (res, bias) in enumerate(((False, False), (False, True), (True, False), (True, True))):
                cases.append((dt, d, (1, 3, 5, 70)[(wi + vi) % 4], res, bias))
    return cases


@pytest.mark.parametrize("dtype,d,rows,residual,bias", _b_cases(), ids=_id)
def test_layernorm_variants(dtype, d, rows, residual, bias):
    x, r, w, b, gy, _ = _norm_inputs(rows, d, dtype, seed=7 * d + rows, residual=residual, bias=bias)
    out = _norm_run("ln", x, r, w, b, gy)
    ref = _norm_ref64("ln", x, r, w, b, gy)
    _norm_compare("ln", out, ref, dtype, f"ln {rows}x{d} res={residual} bias={bias}")
    if not bias:
        yt = F.layer_norm((x if r is None else x + r).float(), (d,), w.float(), None, EPS)
        tol = 2e-2 if dtype == BF16 else 1e-4
        _close(out["y"], yt, tol, tol, "ln y vs F.layer_norm(bias=None)")


@pytest.mark.parametrize("dtype", [BF16, F32], ids=_id)
@pytest.mark.parametrize("wi", range(5), ids=["V", "504", "520", "2056", "max"])
def test_rmsnorm_template_widths(wi, dtype):
    """The same widths through RMSNorm, alternating plain and fused-residual (gradient into h)."""
    d = (_vec(dtype), 504, 520, 2056, _max_d(dtype))[wi]
    rows = (70, 5, 3, 1, 70)[wi]
    x, r, w, _, gy, gh = _norm_inputs(rows, d, dtype, seed=11 * d + rows, residual=wi % 2 == 0, bias=False)
    out = _norm_run("rms", x, r, w, None, gy, gh)
    ref = _norm_ref64("rms", x, r, w, None, gy, gh if r is not None else None)
    _norm_compare("rms", out, ref, dtype, f"rms {rows}x{d}")


# ----------------------------------------------------------------------------- C: large mean, zero row
@pytest.mark.parametrize("d", [1096, 2048])
def test_layernorm_rows_with_large_mean(d):
    """Rows whose mean is up to 1000 standard deviations away from zero, fp32 (in bf16 the output
    rounding hides the effect). A one-pass variance E[x^2] - mean^2 is off by 0.26 .. 0.44 here.
    Bound: 4 x the error of torch's own fp32 layer_norm against float64 on the same inputs (the
    margin covers the different summation order, wave butterfly against Welford).
    Seen on an MI355X, max error against float64, d = 1096 / 2048:
      torch fp32 (the yardstick)  y 1.41e-4 / 9.5e-5   dx 1.9e-5 / 1.3e-5
      the kernel                  y 1.44e-4 / 6.9e-5   dx 1.5e-5 / 5.1e-6"""
    rows = 70
    g = torch.Generator(device=DEV).manual_seed(0)
    x = torch.linspace(-1000, 1000, rows, device=DEV)[:, None] + torch.randn(rows, d, device=DEV, generator=g)
    w = 1 + 0.1 * torch.randn(d, device=DEV, generator=g)
    b = 0.1 * torch.randn(d, device=DEV, generator=g)
    gy = torch.randn(rows, d, device=DEV, generator=g)
    out = _norm_run("ln", x, None, w, b, gy)
    ref = _norm_ref64("ln", x, None, w, b, gy)
    xt, wt, bt = (t.clone().requires_grad_() for t in (x, w, b))
    yt = F.layer_norm(xt, (d,), wt, bt, EPS)
    yt.backward(gy)
    yard = dict(y=yt.detach(), dx=xt.grad, dw=wt.grad, db=bt.grad)
    for k in ("y", "dx", "dw", "db"):
        e_torch = (yard[k].double() - ref[k]).abs().max().item()
        e_kernel = (out[k].double() - ref[k]).abs().max().item()
        print(f"large-mean d={d} {k}: torch fp32 err {e_torch:.3g}, kernel err {e_kernel:.3g}")
        assert torch.isfinite(out[k]).all(), k
        if k in ("y", "dx"):
            assert e_kernel <= 4 * e_torch, f"{k}: kernel {e_kernel:.3g} > 4 x torch fp32 {e_torch:.3g}"
    # the column sums do not depend on the summation order of the mean: the usual tolerance
    _close(out["dw"], ref["dw"], 1e-4 * 30, 1e-4 * 2, "large-mean dw")
    _close(out["db"], ref["db"], 1e-4 * 30, 1e-4 * 2, "large-mean db")


@pytest.mark.parametrize("dtype", [BF16, F32], ids=_id)
@pytest.mark.parametrize("kind", ["rms", "ln"])
def test_norm_all_zero_row(kind, dtype):
    """A batch with an all-zero row: rstd = 1 / sqrt(eps) there; y is exactly b (LayerNorm) or 0
    (RMSNorm) and every gradient is finite and within the usual tolerance."""
    rows, d, z = 5, 520, 2
    x, _, w, b, gy, _ = _norm_inputs(rows, d, dtype, seed=5, residual=False, bias=kind == "ln")
    x[z] = 0
    out = _norm_run(kind, x, None, w, b, gy)
    ref = _norm_ref64(kind, x, None, w, b, gy)
    if kind == "ln":
        assert torch.equal(out["y"][z], b)
    else:
        assert (out["y"][z] == 0).all()
    for k in ("dx", "dw", "db"):
        assert out[k] is None or torch.isfinite(out[k]).all(), k
    _norm_compare(kind, out, ref, dtype, f"{kind} zero row")


# ----------------------------------------------------------------------------- D: dw into a slot
def _rms_bwd_inputs(rows, d, dtype, seed):
    x, _, w, _, gy, _ = _norm_inputs(rows, d, dtype, seed=seed, residual=False, bias=False)
    _, h, rstd = _C().rmsnorm_fwd(x, None, w, EPS, 0)
    hd = h.double()
    dw64 = (gy.double() * hd * torch.rsqrt(hd.pow(2).mean(-1, keepdim=True) + EPS)).sum(0)
    return h, w, rstd, gy, dw64


@pytest.mark.parametrize("dtype", [BF16, F32], ids=_id)
@pytest.mark.parametrize("d", [520, 4096])
def test_rmsnorm_bwd_weight_gradient_into_slot(dtype, d):
    """rmsnorm_bwd(..., dw_out, accumulate): the column-sum kernel writes the weight gradient in the
    parameter dtype (data-parallel gradient slot); accumulate adds to what the slot holds."""
    C = _C()
    rows = 600
    h, w, rstd, dy, dw64 = _rms_bwd_inputs(rows, d, dtype, seed=d + 1)
    tol = 2e-2 if dtype == BF16 else 1e-4
    dx0, dw0 = C.rmsnorm_bwd(dy, h, w, rstd, None, None, False)
    assert dw0.dtype == F32
    _close(dw0, dw64, tol * 20, tol * 2, "dw fp32")
    slot = torch.full((d,), float("nan"), device=DEV, dtype=dtype)
    dx1, ret = C.rmsnorm_bwd(dy, h, w, rstd, None, slot, False)
    assert ret.data_ptr() == slot.data_ptr()
    assert not torch.isnan(slot).any(), "accumulate=False must overwrite the slot"
    _close(slot, dw64, tol * 20, tol * 2, "dw into slot")
    assert torch.equal(dx1, dx0)
    prior = (25 + torch.randn(d, device=DEV, generator=torch.Generator(device=DEV).manual_seed(9))).to(dtype)
    slot = prior.clone()
    dx2, _ = C.rmsnorm_bwd(dy, h, w, rstd, None, slot, True)
    _close(slot, prior.double() + dw64, tol * 20, tol * 2, "dw accumulated into slot")
    assert torch.equal(dx2, dx0)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=_id)
def test_rmsnorm_public_path_writes_gradient_slot(dtype, monkeypatch):
    """ops.rms_norm with a gradient slot on the weight, two backward passes: the first write
    replaces what the slot held, the second adds, notify fires each time, w.grad stays empty."""
    from gke_ray_train_amd import ops
    from gke_ray_train_amd.ops import fused
    from gke_ray_train_amd.ops.linear import GradSlot
    monkeypatch.setattr(fused, "_NORM_DIRECT_GRAD", True)
    rows, d = 600, 520
    tol = 2e-2 if dtype == BF16 else 1e-4
    fired = []
    w = None
    total = torch.zeros(d, device=DEV, dtype=torch.float64)
    view = torch.full((d,), float("nan"), device=DEV, dtype=dtype)
    for step in range(2):
        x, _, w0, _, gy, _ = _norm_inputs(rows, d, dtype, seed=40 + step, residual=False, bias=False)
        if w is None:
            w = torch.nn.Parameter(w0)
            w._grt_slot = GradSlot(view, fired.append)
        xs = x.clone().requires_grad_()
        ops.rms_norm(xs, w, EPS).backward(gy)
        ref = _norm_ref64("rms", x, None, w.detach(), None, gy)
        total += ref["dw"]
        assert len(fired) == step + 1 and fired[-1] is w
        assert w.grad is None
        _close(xs.grad, ref["dx"], tol * 5, tol, f"dx step {step}")
        _close(view, total, tol * 20, tol * 2, f"slot after step {step}")


# ----------------------------------------------------------------------------- E: padded output rows
@pytest.mark.parametrize("dtype", [BF16, F32], ids=_id)
@pytest.mark.parametrize("d", [520, 4096])
@pytest.mark.parametrize("pad", [8, 64])
def test_rmsnorm_padded_output_rows(pad, d, dtype):
    """pad > 0: y is the [rows, d] view of a [rows, d + pad] buffer; values and the backward through
    the strided view are bit-identical to pad = 0."""
    from gke_ray_train_amd import ops
    rows = 5
    x, r, w, _, gy, gh = _norm_inputs(rows, d, dtype, seed=d + pad, residual=True, bias=False)
    res = {}
    for p in (0, pad):
        xs, rs, ws = (t.clone().requires_grad_() for t in (x, r, w))
        y = ops.rms_norm(xs, ws, EPS, pad=p)
        y.backward(gy)
        xa, ra, wa = (t.clone().requires_grad_() for t in (x, r, w))
        ya, ha = ops.add_rms_norm(xa, ra, wa, EPS, pad=p)
        torch.autograd.backward([ya, ha], [gy, gh])
        for t in (y, ya):
            assert t.shape == (rows, d) and t.stride() == (d + p, 1)
        res[p] = [t.detach().clone() for t in (y, xs.grad, ws.grad, ya, ha, xa.grad, ra.grad, wa.grad)]
    for a, b_ in zip(res[0], res[pad]):
        assert torch.equal(a, b_)


# ----------------------------------------------------------------------------- F: width limit
@pytest.mark.parametrize("dtype", [BF16, F32], ids=_id)
@pytest.mark.parametrize("over", ["2x", "one chunk"])
def test_norm_width_limit_raises(dtype, over):
    """Rows wider than 2048 sixteen-byte chunks are refused by all five bindings (the widest
    templates would leave the tail out of the sums and its outputs unwritten)."""
    from gke_ray_train_amd import ops
    C = _C()
    d = 2 * _max_d(dtype) if over == "2x" else _max_d(dtype) + _vec(dtype)
    x = torch.randn(4, d, device=DEV, dtype=dtype)
    w = torch.ones(d, device=DEV, dtype=dtype)
    stat = torch.ones(4, device=DEV)
    with pytest.raises(RuntimeError, match="2048"):
        ops.rms_norm(x, w, EPS)
    with pytest.raises(RuntimeError, match="2048"):
        ops.add_rms_norm(x, x, w, EPS)
    with pytest.raises(RuntimeError, match="2048"):
        ops.layer_norm(x, w, w, EPS)
    with pytest.raises(RuntimeError, match="2048"):
        C.rmsnorm_bwd(x, x, w, stat, None, None, False)
    with pytest.raises(RuntimeError, match="2048"):
        C.rmsnorm_bwd_dx(x, x, w, stat, None)
    with pytest.raises(RuntimeError, match="2048"):
        C.layernorm_bwd(x, x, w, stat, stat, None)
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- G: argument checks
@pytest.mark.parametrize("dtype", [BF16, F32], ids=_id)
def test_norm_argument_checks(dtype):
    """Every operand the kernels dereference is checked against the row tensor before a launch."""
    from gke_ray_train_amd import ops
    C = _C()
    other = F32 if dtype == BF16 else BF16
    rows, d = 6, 64
    x = torch.randn(rows, d, device=DEV, dtype=dtype)
    w = torch.ones(d, device=DEV, dtype=dtype)
    b = torch.zeros(d, device=DEV, dtype=dtype)
    stat = torch.ones(rows, device=DEV)
    w_strided = torch.ones(2 * d, device=DEV, dtype=dtype)[::2]
    bad_forward = {
        "ln residual dtype": lambda: ops.layer_norm(x, w, b, EPS, residual=x.to(other)),
        "ln residual dtype (binding)": lambda: C.layernorm_fwd(x, x.to(other), w, b, EPS),
        "ln residual shape": lambda: C.layernorm_fwd(x, x[:-1].contiguous(), w, b, EPS),
        "rms residual dtype": lambda: C.rmsnorm_fwd(x, x.to(other), w, EPS, 0),
        "ln b length": lambda: ops.layer_norm(x, w, b[:-_vec(dtype)], EPS),
        "ln b dtype": lambda: ops.layer_norm(x, w, b.to(other), EPS),
        "ln b on the CPU": lambda: ops.layer_norm(x, w, b.cpu(), EPS),
        "ln w length": lambda: ops.layer_norm(x, w[:-_vec(dtype)], b, EPS),
        "ln w dtype": lambda: ops.layer_norm(x, w.to(other), b, EPS),
        "ln w strided": lambda: C.layernorm_fwd(x, None, w_strided, b, EPS),
        "rms w strided": lambda: C.rmsnorm_fwd(x, None, w_strided, EPS, 0),
        "rms w length": lambda: ops.rms_norm(x, w[:-_vec(dtype)], EPS),
        "rms d % V": lambda: ops.rms_norm(x[:, :d - 2].contiguous(), w[:d - 2].contiguous(), EPS),
        "ln d % V": lambda: ops.layer_norm(x[:, :d - 2].contiguous(), w[:d - 2].contiguous(), None, EPS),
    }
    for name, call in bad_forward.items():
        with pytest.raises(RuntimeError):
            call()
            pytest.fail(f"{name}: accepted")
    odd = x[:, :d - 2].contiguous()
    backwards = {
        "rmsnorm_bwd": lambda dy, h, w_, mean, rstd: C.rmsnorm_bwd(dy, h, w_, rstd, None, None, False),
        "rmsnorm_bwd_dx": lambda dy, h, w_, mean, rstd: C.rmsnorm_bwd_dx(dy, h, w_, rstd, None),
        "layernorm_bwd": lambda dy, h, w_, mean, rstd: C.layernorm_bwd(dy, h, w_, mean, rstd, None),
    }
    for op, call in backwards.items():
        call(x, x, w, stat, stat)  # the well-formed call is accepted
        bad = {
            "dy shape": (x[:-1].contiguous(), x, w, stat, stat),
            "dy dtype": (x.to(other), x, w, stat, stat),
            "dy on the CPU": (x.cpu(), x, w, stat, stat),
            "w length": (x, x, w[:-_vec(dtype)], stat, stat),
            "w dtype": (x, x, w.to(other), stat, stat),
            "w strided": (x, x, w_strided, stat, stat),
            "rstd length": (x, x, w, stat, stat[:-1]),
            "rstd dtype": (x, x, w, stat, stat.to(BF16)),
            "d % V": (odd, odd, w[:d - 2].contiguous(), stat, stat),
        }
        if op == "layernorm_bwd":
            bad["mean length"] = (x, x, w, stat[:-1], stat)
            bad["mean dtype"] = (x, x, w, stat.double(), stat)
        for name, args in bad.items():
            with pytest.raises(RuntimeError):
                call(*args)
                pytest.fail(f"{op} {name}: accepted")
    with pytest.raises(RuntimeError):
        C.rmsnorm_bwd(x, x, w, stat, x.to(other), None, False)  # dres dtype
    with pytest.raises(RuntimeError):
        C.layernorm_bwd(x, x, w, stat, stat, x[:-1].contiguous())  # dres shape
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- H: empty input
@pytest.mark.parametrize("dtype", [BF16, F32], ids=_id)
def test_norm_empty_input(dtype):
    """rows == 0: correctly shaped empty outputs and dx, zero dw / db, nothing launched."""
    d = 520
    x = torch.empty(0, d, device=DEV, dtype=dtype)
    _, _, w, b, _, _ = _norm_inputs(1, d, dtype, seed=3, residual=False, bias=True)
    for kind, r, bias in (("rms", None, None), ("rms", x, None), ("ln", None, b), ("ln", x, b)):
        out = _norm_run(kind, x, r, w, bias, torch.empty_like(x), torch.empty_like(x))
        assert out["y"].shape == (0, d) and out["y"].dtype == dtype
        assert out["dx"].shape == (0, d)
        if r is not None:
            assert out["dres"].shape == (0, d)
            if kind == "rms":
                assert out["h"].shape == (0, d)
        assert out["dw"].shape == (d,) and not out["dw"].any()
        if bias is not None:
            assert out["db"].shape == (d,) and not out["db"].any()
    C = _C()
    stat = torch.empty(0, device=DEV)
    slot = torch.full((d,), 3.0, device=DEV, dtype=dtype)
    C.rmsnorm_bwd(x, x, w, stat, None, slot, True)
    assert (slot == 3).all(), "accumulating nothing leaves the slot as it is"
    C.rmsnorm_bwd(x, x, w, stat, None, slot, False)
    assert not slot.any()
    assert C.rmsnorm_bwd_dx(x, x, w, stat, None).shape == (0, d)
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- I: reproducibility
@pytest.mark.parametrize("dtype", [BF16, F32], ids=_id)
def test_norm_backward_bitwise_reproducible(dtype):
    """norm.hip promises a bitwise reproducible backward (per-workgroup slabs and a column-sum
    kernel, no float atomics): two runs over rows that share workgroups give the same bits."""
    C = _C()
    rows, d = 1337, 2056
    x, _, w, b, dy, _ = _norm_inputs(rows, d, dtype, seed=17, residual=False, bias=True)
    _, h, mean, rstd = C.layernorm_fwd(x, None, w, b, EPS)
    ln = [C.layernorm_bwd(dy, h, w, mean, rstd, None) for _ in range(2)]
    _, h, rstd = C.rmsnorm_fwd(x, None, w, EPS, 0)
    rms = [C.rmsnorm_bwd(dy, h, w, rstd, None, None, False) for _ in range(2)]
    for first, second in (ln, rms):
        for a, b_ in zip(first, second):
            assert torch.equal(a, b_)


# ----------------------------------------------------------------------------- GELU
# 2001 points over [-12, 12], then the edge block; |x| >= 40 is saturated: exp(-x^2 / 2) is below
# the smallest fp32 denormal, so the derivative is exactly the CDF, 1 or 0
_GELU_EDGES = [0.0, -0.0, 0.75, -0.75, 5.0, -5.0, 10.0, -10.0, 40.0, -40.0, 1e4, -1e4, 1e30, -1e30]


def _gelu_stream(numel, dtype):
    s = torch.cat([torch.linspace(-12, 12, 2001), torch.tensor(_GELU_EDGES)]).to(dtype)
    s = s.repeat(-(-numel // s.numel()))[:numel]
    return s.to(DEV).reshape(-1, _vec(dtype))


@pytest.mark.parametrize("dtype", [BF16, F32], ids=_id)
@pytest.mark.parametrize("size", ["V", "2048+V", "524288V+3V"])
def test_gelu_sizes_and_saturation(dtype, size):
    """numel = V, 2048 + V and 524288 V + 3 V (the grid is capped at 2048 x 256 threads, so the last
    size runs a second grid-stride iteration) against float64 erf-GELU and its derivative."""
    from gke_ray_train_amd import ops
    V = _vec(dtype)
    numel = {"V": V, "2048+V": 2048 + V, "524288V+3V": 524288 * V + 3 * V}[size]
    x = _gelu_stream(numel, dtype).requires_grad_()
    dy = torch.randn(x.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(numel)).to(dtype)
    y = ops.gelu(x)
    y.backward(dy)
    xr = x.detach().double().requires_grad_()
    yr = F.gelu(xr, approximate="none")
    yr.backward(dy.double())
    tol = 2e-2 if dtype == BF16 else 1e-5
    _close(y, yr, tol, tol, "gelu")
    _close(x.grad, xr.grad, tol, tol, "gelu bwd")
    assert not torch.isnan(x.grad).any()
    xd = x.detach()
    hi, lo = xd >= 40, xd <= -40
    if numel > 2015:
        assert hi.any() and lo.any()
    assert torch.equal(x.grad[hi], dy[hi]), "saturated x > 0: dx is dy exactly"
    assert (x.grad[lo] == 0).all(), "saturated x < 0: dx is +-0"
    assert torch.equal(y.detach()[hi], xd[hi]) and (y.detach()[lo] == 0).all()


@pytest.mark.parametrize("dtype", [BF16, F32], ids=_id)
def test_gelu_unvectorisable_gpu_tensor_takes_reference_path(dtype):
    """numel % V != 0 on a GPU tensor: the torch fallback, forward and gradient."""
    from gke_ray_train_amd import ops
    x = _gelu_stream(2048 + _vec(dtype), dtype).flatten()[2001 - 1:2001 + 14].reshape(3, 5).clone().requires_grad_()
    dy = torch.randn(3, 5, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1)).to(dtype)
    y = ops.gelu(x)
    assert y.dtype == dtype and y.shape == (3, 5)
    y.backward(dy)
    xr = x.detach().double().requires_grad_()
    yr = F.gelu(xr, approximate="none")
    yr.backward(dy.double())
    tol = 2e-2 if dtype == BF16 else 1e-5
    _close(y, yr, tol, tol, "gelu fallback")
    _close(x.grad, xr.grad, tol, tol, "gelu fallback bwd")


# ----------------------------------------------------------------------------- scale + PE
def _ulp_close(a, ref64, rtol, atol, what):
    err = (a.double() - ref64).abs()
    tol = atol + rtol * ref64.abs()
    worst = (err / tol.clamp_min(1e-300)).max().item() if err.numel() else 0.0
    assert not torch.isnan(a).any() and worst <= 1.0, f"{what}: an element is {worst:.2f}x its tolerance"


def _pe_case(B, S, d, dtype, max_len, seed):
    from gke_ray_train_amd.models import basic_llm
    C = _C()
    # one output ulp in bf16; two in fp32 (fused against separate multiply-add); the same factor of
    # max|pe| absolute, for cancellation of emb * scale against pe near zero
    rt = 2.0 ** -8 if dtype == BF16 else 2.0 ** -22
    scale = math.sqrt(d)
    pe = basic_llm.sinusoidal_pe(max_len, d).to(DEV)[0, :S]  # as the model slices it
    g = torch.Generator(device=DEV).manual_seed(seed)
    emb = torch.randn(B * S, d, device=DEV, generator=g).to(dtype)
    gout = torch.randn(B * S, d, device=DEV, generator=g).to(dtype)
    t = torch.arange(B * S, device=DEV)
    ref = emb.double() * scale + pe.double()[t % S]
    what = f"B={B} S={S} d={d}"
    _ulp_close(C.scale_add_pe(emb, pe, S, scale), ref, rt, rt * pe.abs().max().item(), f"scale_add_pe {what}")
    _ulp_close(C.scale_add_pe(emb, None, S, scale), emb.double() * scale, rt, 0.0, f"scale only {what}")
    es = emb.clone().requires_grad_()
    ps = pe.clone().requires_grad_()
    out = basic_llm._scale_add_pe(es, ps, S, scale)
    _ulp_close(out.detach(), ref, rt, rt * pe.abs().max().item(), f"_scale_add_pe {what}")
    out.backward(gout)
    assert ps.grad is None, "no gradient reaches pe"
    _ulp_close(es.grad, gout.double() * scale, 2.0 ** -8 if dtype == BF16 else 2.0 ** -23, 0.0, f"emb.grad {what}")


@pytest.mark.parametrize("dtype", [BF16, F32], ids=_id)
@pytest.mark.parametrize("d", [8, 520, 768])
def test_scale_add_pe(d, dtype):
    """out[t] = emb[t] * sqrt(d) + pe[t % S]: every position has its own pe row (max_len > S), so a
    wrong wrap over the batch shows at B > 1; pe = None is pure scaling."""
    for B in (1, 3):
        for S in (1, 7, 33):
            _pe_case(B, S, d, dtype, max_len=64, seed=B * 100 + S)


def test_scale_add_pe_second_grid_stride_iteration():
    """T d / V = 589824 vectors > 2048 x 256 threads: the kernel loops."""
    _pe_case(6, 1024, 768, BF16, max_len=1100, seed=6)
