"""Cross-entropy, RoPE, SwiGLU and embedding kernels on the paths the sibling tests in
test_kernels_gpu.py do not reach: the cross-entropy vector loop followed by its scalar tail (a
row-strided view of a padded-vocabulary buffer), a misaligned base, rows narrower than a vector or
than the workgroup, -inf logits, ignore_index other than -100, labels outside [0, V), an all-ignored
batch and the bias gradient of the fused LM head; the generic RoPE kernel at every head width, in
fp32, with per-token positions, on row-strided buffers and through its second grid-stride trip;
the embedding kernels' grid-stride and lane-loop trips; saturated SwiGLU gates; the bindings'
argument checks and empty inputs.

Every reference is float64 on the same, already rounded inputs, and every element is compared with a
bound of its own (no norm, no fraction left out). The bounds are derived from the arithmetic:
  bf16 output   the kernels compute in fp32 and round once: one bf16 ulp of the reference,
                2^-8 |ref|, on top of the op's fp32 term
  fp32 floor    2^-126 times the operands' magnitude: a result or factor below the smallest normal
                fp32 may be flushed to zero
  __expf        one ulp on the scaled argument: exp(x) carries (|x| + 2) 2^-23 relative
The fp32 terms were checked against the same formulas in float32 with plain torch ops (which stay
inside them with room to spare), not against what the kernels give."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
U24, U23 = 2.0 ** -24, 2.0 ** -23  # half an fp32 ulp (one rounding), one fp32 ulp
BF16_ULP = 2.0 ** -8               # one bf16 ulp, relative
FTZ = 2.0 ** -126                  # smallest normal fp32


def _id(v):
    return str(v).replace("torch.", "")


def _C():
    from gke_ray_train_amd import _native
    return _native.kernels()


def _vec(dtype):
    return 8 if dtype == BF16 else 4


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def _randn(g, *shape):
    """fp32 normal values drawn on the host (the same on every machine), moved to the GPU."""
    return torch.randn(*shape, generator=g, dtype=torch.float32).to(DEV)


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and bool((_bits(a) == _bits(b)).all())


def _nan_buffer(rows, cols, dtype):
    return torch.full((rows, cols), float("nan"), device=DEV, dtype=dtype)


def _out_tol(ref, fp32_tol, dtype):
    """fp32 term, the flush-to-zero floor, and for a bf16 output one bf16 ulp of the reference."""
    tol = fp32_tol + FTZ
    return tol + BF16_ULP * ref.abs() if dtype == BF16 else tol


def _check(out, ref, tol, what):
    """Every element of out within its own bound tol of the float64 ref; NaN / inf always fails."""
    assert out.shape == ref.shape, f"{what}: shape {tuple(out.shape)} != {tuple(ref.shape)}"
    if out.numel() == 0:
        return
    o = out.double()
    assert bool(torch.isfinite(o).all()), f"{what}: NaN or inf in the kernel output"
    err = (o - ref).abs()
    ratio = err / tol.clamp_min(1e-300)
    worst = ratio.max().item()
    if worst > 1.0:
        i = int(ratio.flatten().argmax())
        pytest.fail(f"{what}: element {i} is {worst:.3g}x its bound (got {o.flatten()[i].item():.9g}, "
                    f"ref {ref.flatten()[i].item():.9g}, bound {tol.flatten()[i].item():.3g})")


# ============================================================================= cross-entropy
_CE_KINDS = ["V3", "V200", "vector", "scalar", "view", "misaligned"]
_CE_N = 8


def _ce_shape(kind, dtype):
    """(V, ld, column offset of the view inside its buffer, vec_ok as cross_entropy.hip decides it)."""
    ve = _vec(dtype)
    if kind == "V3":
        return 3, 3, 0, False                      # below one vector; ld % VE != 0: scalar loop
    if kind == "V200":
        return 200, 200, 0, True                   # 25 / 50 vectors: most threads keep (-inf, 0)
    if kind == "vector":
        return 256 * ve, 256 * ve, 0, True         # one vector per thread, no tail
    if kind == "scalar":
        return 2 * 256 * ve + 1, 2 * 256 * ve + 1, 0, False  # ld % VE != 0: 2 VE + 1 scalar trips
    V = 256 * ve + ve + 3
    if kind == "view":                             # buf[:, :V]: second vector trip for thread 0 + 3-element tail
        return V, -(-V // ve) * ve + ve, 0, True
    return V, V + 1 + ve, 1, False                 # buf[:, 1:1 + V]: base off the 16-byte grid


def _ce_trips(V, vec_ok, dtype):
    """Loop trips of the busiest thread of ce_fwd_kernel."""
    ve = _vec(dtype)
    nvec = V // ve if vec_ok else 0
    return -(-nvec // 256) + -(-(V - nvec * ve) // 256)


def _ce_labels(V, dtype, ignore_index):
    ve = _vec(dtype)
    # 0, V - 1, one in the vector region, one in the tail (the last but one column), the ignored
    # value, two outside [0, V) (V itself and a negative that is not ignore_index), the middle
    lab = [0, V - 1, min(3 * ve + 1, V - 1), max(V - 2, 0), ignore_index, V, -7, V // 2]
    return torch.tensor(lab, device=DEV, dtype=torch.int64)


def _ce_logits(kind, dtype, ninf, labels, seed):
    """The [N, V] logits as a view of a NaN-filled buffer, rounded to dtype. Rows: 3 randn; shifted by
    +200 with a spread of about 60 (running-max rescale, most terms underflow); one dominant logit."""
    V, ld, off, _ = _ce_shape(kind, dtype)
    ve = _vec(dtype)
    g = _gen(seed)
    x = 3 * _randn(g, _CE_N, V)
    x[2] = 200 + 10 * _randn(g, V)
    x[3] = 200 + 10 * _randn(g, V)
    x[4] = _randn(g, V)
    x[4, V // 3] = 50.0
    if ninf:
        lab = labels.tolist()
        # thread 5's columns: its vectors in the vector loop, its elements in the scalar loop
        vec_ok = _ce_shape(kind, dtype)[3]
        nvec = V // ve if vec_ok else 0
        stride = [i * ve + k for i in range(5, nvec, 256) for k in range(ve)]
        stride += [j for j in range(nvec * ve + 5, V, 256)]
        sets = {"head": list(range(min(ve, V - 1))), "tail": [V - 1], "stride": stride}
        plan = {"head": (1, 5, 3), "tail": (0, 6, 3), "stride": (4, 7, 3)}
        for name, rows in plan.items():
            cols = sets[name]
            for r in rows:
                if lab[r] in cols or not cols:  # the label's logit stays finite (else the loss is +inf)
                    continue
                x[r, cols] = float("-inf")
        assert bool(torch.isfinite(x).any(1).all()), "every row keeps a finite logit"
        assert bool(torch.isinf(x).any()), "the case has -inf logits"
    buf = _nan_buffer(_CE_N, ld, dtype)
    buf[:, off:off + V] = x.to(dtype)
    return buf, buf[:, off:off + V]


def _ce_ref(x, labels, ignore_index, gscale, dtype, vec_ok):
    """float64 loss_rows / lse / dlogits of the rounded logits x, each with its per-element bound."""
    V = x.shape[1]
    xd = x.double()
    lse = torch.logsumexp(xd, 1)
    counted = (labels != ignore_index) & (labels >= 0) & (labels < V)
    xl = xd.gather(1, labels.clamp(0, V - 1)[:, None])[:, 0]
    loss = torch.where(counted, lse - xl, torch.zeros_like(lse))
    finite = torch.isfinite(xd)
    mx = xd.max(1).values
    mn = torch.where(finite, xd, mx[:, None]).min(1).values
    # each exp argument is x - running max >= min - max of the row: (R + 2) 2^-23 relative per __expf
    e_exp = ((mx - mn) + 2) * U23
    trips = _ce_trips(V, vec_ok, dtype)
    # a term passes through its own exp, a rescale in every later trip of its thread and the merge's
    # rescale; the sum adds once per trip plus the wave and workgroup reduction (16 more at most)
    e_sum = (trips + 1) * e_exp + (trips + 16) * U24
    # lse = gm + __logf(gs): d log(gs) = d gs / gs; __logf is a hardware log2 times a constant, one
    # ulp each on log(gs) >= 0; the final add rounds once
    lse_tol = e_sum + 2 * U23 * (lse - mx).abs() + U24 * lse.abs()
    loss_tol = torch.where(counted, lse_tol + U24 * loss.abs(), torch.zeros_like(lse))  # one subtraction
    p = torch.exp(xd - lse[:, None])
    onehot = torch.zeros_like(p)
    rows = torch.nonzero(counted)[:, 0]
    onehot[rows, labels[rows]] = 1.0
    gs = torch.where(counted, gscale.double(), torch.zeros_like(lse))[:, None]
    d = (p - onehot) * gs
    arg = torch.where(finite, (xd - lse[:, None]).abs(), torch.zeros_like(xd))
    # p = __expf(x - lse): the argument carries lse's error and one rounding of its own, the exp
    # (|arg| + 2) 2^-23; then one subtraction and one product
    p_tol = p * (lse_tol[:, None] + U24 * arg + (arg + 2) * U23)
    d_tol = gs.abs() * (p_tol + U23 * (p - onehot).abs())
    return dict(lse=lse, lse_tol=lse_tol, loss=loss, loss_tol=loss_tol, d=d,
                d_tol=_out_tol(d, d_tol, dtype) + FTZ * gs.abs(), counted=counted, finite=finite)


_CE_GSCALE = [1.0, 0.0, -2.5, 0.125, 3.0, 1.0, 1.0, -1.0]


@pytest.mark.parametrize("ignore_index", [-100, 0])
@pytest.mark.parametrize("ninf", [False, True], ids=["finite", "ninf"])
@pytest.mark.parametrize("dtype", [BF16, F32], ids=_id)
@pytest.mark.parametrize("kind", _CE_KINDS)
def test_ce_kernels(kind, dtype, ninf, ignore_index):
    """ce_fwd / ce_bwd called directly: per-row loss, lse and dlogits with a per-row gscale (0 and
    negative values included), out of place and in place; what surrounds a view stays as it was."""
    C = _C()
    V, ld, off, vec_ok = _ce_shape(kind, dtype)
    labels = _ce_labels(V, dtype, ignore_index)
    buf, x = _ce_logits(kind, dtype, ninf, labels, seed=V + 7 * ninf)
    before = buf.clone()
    gscale = torch.tensor(_CE_GSCALE, device=DEV)
    ref = _ce_ref(x, labels, ignore_index, gscale, dtype, vec_ok)
    assert bool(torch.isfinite(ref["lse"]).all()) and bool(torch.isfinite(ref["d"]).all())
    what = f"{kind} {_id(dtype)} V={V} ld={ld}"

    loss_rows, lse = C.ce_fwd(x, labels, ignore_index)
    assert loss_rows.dtype == F32 and lse.dtype == F32
    _check(lse, ref["lse"], ref["lse_tol"] + FTZ, f"{what} lse")
    _check(loss_rows, ref["loss"], ref["loss_tol"] + FTZ, f"{what} loss_rows")
    assert bool((loss_rows[~ref["counted"]] == 0).all()), "ignored / out-of-range rows: loss exactly 0"
    assert _same_bits(buf, before), "the forward writes nothing into the logits buffer"

    # the backward reads the kernel's own lse, as the autograd functions hand it over
    d = C.ce_bwd(x, labels, lse, gscale, ignore_index, False)
    assert d.shape == x.shape and d.dtype == dtype and d.is_contiguous()
    _check(d, ref["d"], ref["d_tol"], f"{what} dlogits")
    assert bool((d[~ref["counted"]] == 0).all()), "ignored / out-of-range rows: gradient exactly 0"
    assert bool((d[~ref["finite"]] == 0).all()), "-inf logits: gradient exactly 0"
    assert _same_bits(buf, before)

    r = C.ce_bwd(x, labels, lse, gscale, ignore_index, True)
    assert r.data_ptr() == x.data_ptr()
    _check(x, ref["d"], ref["d_tol"], f"{what} dlogits in place")
    assert _same_bits(x, d), "in place and out of place give the same bits"
    pad = torch.ones(ld, dtype=torch.bool, device=DEV)
    pad[off:off + V] = False
    assert _same_bits(buf[:, pad], before[:, pad]), "columns outside the view are left alone"


@pytest.mark.parametrize("inplace", [False, True], ids=["outofplace", "inplace"])
@pytest.mark.parametrize("ignore_index", [-100, 0])
@pytest.mark.parametrize("dtype", [BF16, F32], ids=_id)
@pytest.mark.parametrize("kind", ["V3", "V200", "view", "misaligned"])
def test_cross_entropy_op_mean_and_gradient(kind, dtype, ignore_index, inplace):
    """ops.cross_entropy: the mean runs over exactly the rows the kernel counts (not ignore_index,
    inside [0, V)); the gradient reaches the padded buffer through the view, zero outside it."""
    from gke_ray_train_amd import ops
    V, ld, off, vec_ok = _ce_shape(kind, dtype)
    labels = _ce_labels(V, dtype, ignore_index)
    buf, x = _ce_logits(kind, dtype, True, labels, seed=V + 3)
    buf = torch.where(torch.isnan(buf), torch.full_like(buf, 7.0), buf)  # a leaf autograd may sum over
    before = buf.clone()
    leaf = buf.requires_grad_()
    view = leaf[:, off:off + V]
    loss = ops.cross_entropy(view, labels, ignore_index, inplace_backward=inplace)
    nvalid = int(((labels != ignore_index) & (labels >= 0) & (labels < V)).sum())
    assert nvalid in (4, 5)
    up = 1.75
    (loss * up).backward()
    gscale = torch.full((_CE_N,), up / nvalid, device=DEV, dtype=torch.float64)
    ref = _ce_ref(before[:, off:off + V], labels, ignore_index, gscale, dtype, vec_ok)
    mean = ref["loss"].sum() / nvalid
    # the rows' bounds, one rounding per addition of the fp32 sum, one for the division
    mean_tol = (ref["loss_tol"].sum() + (_CE_N + 1) * U24 * ref["loss"].abs().sum()) / nvalid
    _check(loss.detach().reshape(1), mean.reshape(1), mean_tol.reshape(1), f"{kind} mean loss")
    grad = leaf.grad
    # gscale = up / nvalid is formed in fp32: two more roundings on every element
    _check(grad[:, off:off + V], ref["d"], ref["d_tol"] + U23 * ref["d"].abs(), f"{kind} gradient")
    pad = torch.ones(ld, dtype=torch.bool, device=DEV)
    pad[off:off + V] = False
    assert bool((grad[:, pad] == 0).all()), "no gradient outside the view"
    assert _same_bits(leaf.detach()[:, pad], before[:, pad]), "columns outside the view are left alone"
    if not inplace:
        assert _same_bits(leaf.detach(), before)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=_id)
@pytest.mark.parametrize("ignore_index", [-100, 0])
def test_cross_entropy_all_rows_ignored(dtype, ignore_index):
    """Every label ignored or out of range: the loss is exactly 0 and every gradient element is
    exactly 0 (not NaN), through both autograd functions."""
    from gke_ray_train_amd import ops
    V, N, d = 283, 7, 64
    g = _gen(11)
    labels = torch.tensor([ignore_index] * 5 + [V, -7], device=DEV)
    x = (3 * _randn(g, N, V)).to(dtype).requires_grad_()
    loss = ops.cross_entropy(x, labels, ignore_index)
    loss.backward()
    assert loss.item() == 0.0
    assert bool((x.grad == 0).all())
    h = _randn(g, N, d).to(dtype).requires_grad_()
    w = (0.05 * _randn(g, V, d)).to(dtype).requires_grad_()
    b = (0.1 * _randn(g, V)).to(dtype).requires_grad_()
    loss = ops.lm_head_cross_entropy(h, w, labels, bias=b, ignore_index=ignore_index)
    loss.backward()
    assert loss.item() == 0.0
    for t in (h, w, b):
        assert bool((t.grad == 0).all())


@pytest.mark.parametrize("row_weights", [False, True], ids=["mean", "weighted"])
@pytest.mark.parametrize("dtype", [BF16, F32], ids=_id)
def test_lm_head_cross_entropy_bias(dtype, row_weights):
    """lm_head_cross_entropy(bias=...): loss, dh, dW and db = dlogits.sum(0) against float64 taken
    from the logits as the GEMM rounds them; labels as in the kernel cases (ignored, out of range)."""
    from gke_ray_train_amd import ops
    N, d, V = 40, 64, 283
    g = _gen(21)
    h = _randn(g, N, d).to(dtype)
    w = (0.05 * _randn(g, V, d)).to(dtype)
    b = (0.5 * _randn(g, V)).to(dtype)
    labels = torch.randint(0, V, (N,), generator=g).to(DEV)
    labels[:8] = _ce_labels(V, dtype, -100)
    rw = (torch.rand(N, generator=g) / 8).to(DEV) if row_weights else None
    hs, ws, bs = (t.clone().requires_grad_() for t in (h, w, b))
    loss = ops.lm_head_cross_entropy(hs, ws, labels, bias=bs, row_weights=rw)
    loss.backward()
    logits = (h.double() @ w.double().t() + b.double()).to(dtype)  # float64 GEMM, rounded like the op's
    counted = (labels != -100) & (labels >= 0) & (labels < V)
    gscale = (rw.double() if row_weights else torch.full((N,), 1.0 / int(counted.sum()), device=DEV).double())
    ref = _ce_ref(logits, labels, -100, gscale, dtype, vec_ok=False)
    loss_ref = (ref["loss"] * gscale).sum()
    dl = ref["d"]
    # the GEMM tolerance of test_lm_head_ce (2e-2 on the loss; 2e-3 + 5e-2 |ref| on the gradients),
    # here on every element
    assert abs(loss.item() - loss_ref.item()) < 2e-2
    for name, got, want in (("dh", hs.grad, dl @ w.double()), ("dW", ws.grad, dl.t() @ h.double()),
                            ("db", bs.grad, dl.sum(0))):
        assert got.dtype == dtype
        _check(got, want, 2e-3 + 5e-2 * want.abs(), f"lm head {name}")


# ============================================================================= RoPE
_LLAMA3 = dict(type="llama3", factor=8.0, low_freq_factor=1.0, high_freq_factor=4.0,
               original_max_position_embeddings=64)


def _rope_ref(x, cos, sin, idx, sign, dtype):
    """float64 rotation of x [T, H, D] by the fp32 table rows idx (sign = -1: the backward).
    Bound: 4 x 2^-24 (|x1 c| + |x2 s|), two products and a sum, contracted or not."""
    half = x.shape[-1] // 2
    xd = x.double()
    x1, x2 = xd[..., :half], xd[..., half:]
    c = cos.double()[idx][:, None, :]
    s = sign * sin.double()[idx][:, None, :]
    ref = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1)
    mag = torch.cat([(x1 * c).abs() + (x2 * s).abs(), (x2 * c).abs() + (x1 * s).abs()], -1)
    return ref, _out_tol(ref, 4 * U24 * mag, dtype)


def _rope_case(C, dtype, D, hq, hkv, T, S, with_pos, scaling, seed, pad=64):
    """rope_fwd and rope_bwd on row-strided, NaN-surrounded buffers against float64; the adjoint."""
    from gke_ray_train_amd.ops import _ref
    g = _gen(seed)
    width, qw, kw = (hq + 2 * hkv) * D, hq * D, hkv * D
    ld = width + pad
    cos, sin = _ref.rope_tables(S, D, 10000.0, device=DEV, scaling=scaling)
    if with_pos:  # shuffled, with repeats, all inside [0, S)
        pos = torch.cat([torch.randperm(S, generator=g), torch.randint(0, S, (T,), generator=g)])[:T]
        pos = pos[torch.randperm(T, generator=g)].int().to(DEV)
        idx = pos.long()
    else:
        pos, idx = None, torch.arange(T, device=DEV) % S
    buf = _nan_buffer(T, ld, dtype)
    qkv = buf[:, :width]
    qkv.copy_(_randn(g, T, width).to(dtype))
    before = buf.clone()
    xq = qkv[:, :qw].reshape(T, hq, D)
    xk = qkv[:, qw:qw + kw].reshape(T, hkv, D)
    what = f"D={D} {_id(dtype)} hq={hq} hkv={hkv} T={T} pos={with_pos} scaling={scaling is not None}"

    q, k = C.rope_fwd(qkv, cos, sin, pos, hq, hkv, D, S)
    assert q.shape == (T, hq, D) and k.shape == (T, hkv, D) and q.dtype == dtype
    q_ref, q_tol = _rope_ref(xq, cos, sin, idx, 1.0, dtype)
    k_ref, k_tol = _rope_ref(xk, cos, sin, idx, 1.0, dtype)
    _check(q, q_ref, q_tol, f"rope_fwd q {what}")
    _check(k, k_ref, k_tol, f"rope_fwd k {what}")
    assert _same_bits(buf, before), "the forward writes nothing into qkv"

    dq = _randn(g, T, hq, D).to(dtype)
    dk = _randn(g, T, hkv, D).to(dtype)
    dbuf = _nan_buffer(T, ld, dtype)
    C.rope_bwd(dq, dk, dbuf[:, :width], cos, sin, pos, hq, hkv, D, S)
    dq_ref, dq_tol = _rope_ref(dq, cos, sin, idx, -1.0, dtype)
    dk_ref, dk_tol = _rope_ref(dk, cos, sin, idx, -1.0, dtype)
    gq = dbuf[:, :qw].reshape(T, hq, D)
    gk = dbuf[:, qw:qw + kw].reshape(T, hkv, D)
    _check(gq, dq_ref, dq_tol, f"rope_bwd dq columns {what}")
    _check(gk, dk_ref, dk_tol, f"rope_bwd dk columns {what}")
    assert _same_bits(dbuf[:, qw + kw:], _nan_buffer(T, ld - qw - kw, dtype)), \
        f"rope_bwd leaves the V columns and the row padding alone {what}"

    # <rope_fwd(x), g> = <x, rope_bwd(g)>, to the sum of the elements' bounds weighted by the other factor
    lhs = (q.double() * dq.double()).sum() + (k.double() * dk.double()).sum()
    rhs = (xq.double() * gq.double()).sum() + (xk.double() * gk.double()).sum()
    bound = ((q_tol * dq.double().abs()).sum() + (k_tol * dk.double().abs()).sum()
             + (dq_tol * xq.double().abs()).sum() + (dk_tol * xk.double().abs()).sum())
    assert abs(lhs.item() - rhs.item()) <= bound.item(), f"adjoint {what}: {lhs.item()} vs {rhs.item()}"
    return q, k, gq, gk, (q_ref, q_tol, k_ref, k_tol, dq_ref, dq_tol, dk_ref, dk_tol)


# (hq, hkv, per-token positions, llama3 scaling)
_ROPE_CONFIGS = [(4, 2, False, False), (3, 1, True, True), (1, 1, True, False), (4, 2, False, True)]


@pytest.mark.parametrize("dtype", [BF16, F32], ids=_id)
@pytest.mark.parametrize("D", [16, 48, 64, 128, 256])
def test_rope_against_float64(D, dtype):
    """Both RoPE kernels (ew_set_fast 1: rope128_kernel at D = 128; 0: the generic rope_kernel, which
    is also all there is at every other D) at T = 37, S = 16, so that t % S wraps."""
    C = _C()
    try:
        for fast in (1, 0):
            C.ew_set_fast(fast)
            for i, (hq, hkv, with_pos, scaled) in enumerate(_ROPE_CONFIGS):
                _rope_case(C, dtype, D, hq, hkv, T=37, S=16, with_pos=with_pos,
                           scaling=_LLAMA3 if scaled else None, seed=100 * D + 10 * i + fast)
            torch.cuda.synchronize()
    finally:
        C.ew_set_fast(1)


def test_rope_generic_kernel_second_grid_stride_trip():
    """D = 64, T = 4100, hq = 32, hkv = 1: 541,200 work items against 2048 x 256 = 524,288 per trip
    of rope_kernel. Every element is compared; the last token's rows (all of them in the second
    trip) once more by themselves."""
    C = _C()
    T, hq, hkv, D = 4100, 32, 1, 64
    assert T * (hq + hkv) * (D // 16) > 2048 * 256
    q, k, gq, gk, r = _rope_case(C, BF16, D, hq, hkv, T=T, S=96, with_pos=False, scaling=None, seed=5)
    q_ref, q_tol, k_ref, k_tol, dq_ref, dq_tol, dk_ref, dk_tol = r
    for name, got, ref, tol in (("q", q, q_ref, q_tol), ("k", k, k_ref, k_tol), ("dq", gq, dq_ref, dq_tol),
                                ("dk", gk, dk_ref, dk_tol)):
        _check(got[-1], ref[-1], tol[-1], f"last token {name}")
        assert bool((got[-1] != 0).any())


# ============================================================================= embedding
def _emb_tol(k, mag, ref, dtype):
    """A row hit k times: k x 2^-24 x sum |rows added| (whatever order the sort produced)."""
    return _out_tol(ref, k[:, None] * U24 * mag, dtype)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=_id)
@pytest.mark.parametrize("d", [8, 264, 520])
def test_embedding_forward_grid_stride(d, dtype):
    """n = 16384 + 5 two-dimensional ids: rows_grid caps the grid at 4096 workgroups of 4 rows, so the
    last 5 rows come from the grid-stride step; d = 264 (fp32) / 520 (bf16): second lane-loop trip."""
    C = _C()
    V = 1000
    g = _gen(d)
    w = _randn(g, V, d).to(dtype)
    ids = torch.randint(0, V, (3, 5463), generator=g).to(DEV)
    ids[0, 0], ids[-1, -1], ids[-1, -2] = 0, V - 1, 0
    assert ids.numel() == 16384 + 5
    out = C.embedding_fwd(ids, w)
    assert out.shape == (ids.numel(), d) and out.dtype == dtype
    assert _same_bits(out, w[ids.reshape(-1)]), "the gather is bit-exact"


def _emb_bwd_case(C, V, n, d, dtype, ids, seed):
    g = _gen(seed)
    dy = _randn(g, n, d).to(dtype)
    count = torch.bincount(ids, minlength=V).double()
    hit = count > 0
    assert bool((ids >= 0).all()) and bool((ids < V).all())
    total = torch.zeros(V, d, device=DEV, dtype=torch.float64).index_add_(0, ids, dy.double())
    mag = torch.zeros(V, d, device=DEV, dtype=torch.float64).index_add_(0, ids, dy.double().abs())
    what = f"V={V} n={n} d={d} {_id(dtype)}"

    dw = _nan_buffer(V, d, dtype)  # overwrite mode: every row is written
    C.embedding_bwd(dy, ids, dw, False)
    _check(dw, total, _emb_tol(count, mag, total, dtype), f"embedding_bwd overwrite {what}")
    assert bool((dw[~hit] == 0).all()), "rows no token hit come out exactly 0"

    prior = _randn(g, V, d).to(dtype)  # accumulate mode: dw += sum, unhit rows untouched
    dw = prior.clone()
    C.embedding_bwd(dy, ids, dw, True)
    want = prior.double() + total
    _check(dw, want, _emb_tol(count + 1, mag + prior.double().abs(), want, dtype), f"embedding_bwd accumulate {what}")
    assert _same_bits(dw[~hit], prior[~hit]), "accumulate mode leaves unhit rows bit-identical"
    return hit


@pytest.mark.parametrize("dtype", [BF16, F32], ids=_id)
@pytest.mark.parametrize("d", [8, 264, 520])
def test_embedding_backward_grid_stride(d, dtype):
    """V = 16384 + 3 rows of dW: the last 3 come from the grid-stride step, V - 1 among the hit ones.
    One id is hit 3000 times, ids 0 and V - 1 are hit, most rows are not."""
    C = _C()
    V, n = 16384 + 3, 5000
    g = _gen(3 * d)
    ids = torch.randint(0, V, (n,), generator=g)
    ids[0], ids[1], ids[2], ids[3] = 0, V - 1, V - 1, V - 2
    ids[4:][torch.randperm(n - 4, generator=g)[:3000]] = 7777
    ids = ids.to(DEV)
    hit = _emb_bwd_case(C, V, n, d, dtype, ids, seed=d + 1)
    assert int(torch.bincount(ids, minlength=V)[7777]) >= 3000
    assert bool(hit[0]) and bool(hit[V - 1]) and int(hit.sum()) < V // 4


@pytest.mark.parametrize("dtype", [BF16, F32], ids=_id)
def test_embedding_narrowest_row_small_vocabulary(dtype):
    """d = 8 (one 16-byte chunk in bf16, two in fp32; most lanes idle) at V = 10: one workgroup."""
    C = _C()
    V, n, d = 10, 50, 8
    g = _gen(8)
    ids = torch.randint(0, V - 3, (n,), generator=g)  # rows 7, 8 stay unhit
    ids[0], ids[1] = 0, V - 1
    ids = ids.to(DEV)
    w = _randn(g, V, d).to(dtype)
    assert _same_bits(C.embedding_fwd(ids, w), w[ids])
    _emb_bwd_case(C, V, n, d, dtype, ids, seed=9)


# ============================================================================= SwiGLU
# +-1.278: the zero of silu'; +-20: sigmoid rounds to 1 / 2e-9; +-88: __expf(88) is the last finite
# value; +-100: __expf(100) overflows to inf inside sigmoidf_
_GATES = [0.0, -0.0, 1e-30, -1e-30, 1.278, -1.278, 20.0, -20.0, 88.0, -88.0, 100.0, -100.0]


def _swiglu_inputs(rows, f, dtype, seed):
    g = _gen(seed)
    gate = 3 * _randn(g, rows, f)
    special = torch.tensor(_GATES, device=DEV).repeat(-(-rows * f // (2 * len(_GATES))))
    flat = gate.view(-1)
    flat[::2] = special[:flat[::2].numel()]  # every other gate is one of the edge values
    gu = torch.cat([gate, _randn(g, rows, f)], 1).to(dtype).contiguous()
    dout = _randn(g, rows, f).to(dtype)
    return gu, dout


def _swiglu_ref(gu, dout, dtype):
    """float64 silu(g) u and its gradients. sigma = 1 / (1 + __expf(-g)): the exp carries
    (|g| + 2) 2^-23, the add and the division three more half-ulps, each product one."""
    g, u = gu.double().chunk(2, -1)
    d = dout.double()
    sg = torch.sigmoid(g)
    e_exp = (g.abs() + 2) * U23
    out = g * sg * u
    out_tol = out.abs() * (e_exp + 4 * U24) + FTZ * (g * u).abs()
    du = d * g * sg
    du_tol = du.abs() * (e_exp + 4 * U24) + FTZ * (d * g).abs()
    dg = d * u * sg * (1 + g * (1 - sg))
    # 1 + g (1 - sigma) cancels: bound by the terms d u sigma (1 + |g|), not by the result; eight
    # half-ulps along the way (sigma 3, 1 - sigma, its product with g, the sum, two more factors)
    dg_tol = (d * u).abs() * sg * (1 + g.abs()) * (e_exp + 8 * U24) + FTZ * (d * u).abs() * (1 + g.abs())
    return dict(out=out, out_tol=_out_tol(out, out_tol, dtype), dgu=torch.cat([dg, du], -1),
                dgu_tol=_out_tol(torch.cat([dg, du], -1), torch.cat([dg_tol, du_tol], -1), dtype))


@pytest.mark.parametrize("dtype", [BF16, F32], ids=_id)
def test_swiglu_saturated_gates(dtype):
    """swiglu_fwd (pad 0 and 8) and swiglu_bwd through the single-pass and the grid-stride kernels at
    5 x 296 with gates at the edges of sigmoidf_: no NaN or inf, every element within its bound."""
    C = _C()
    rows, f = 5, 8 * 37
    gu, dout = _swiglu_inputs(rows, f, dtype, seed=37)
    ref = _swiglu_ref(gu, dout, dtype)
    try:
        for fast in (1, 0):
            C.ew_set_fast(fast)
            for pad in (0, 8):
                y = C.swiglu_fwd(gu, pad)
                assert y.shape == (rows, f) and y.stride() == (f + pad, 1)
                _check(y, ref["out"], ref["out_tol"], f"swiglu_fwd pad={pad} fast={fast}")
            dgu = C.swiglu_bwd(gu, dout)
            assert dgu.shape == gu.shape
            _check(dgu, ref["dgu"], ref["dgu_tol"], f"swiglu_bwd fast={fast}")
            torch.cuda.synchronize()
    finally:
        C.ew_set_fast(1)


def test_swiglu_transposing_kernels_against_float64():
    """swiglu_fwd_t / swiglu_bwd_t at 64 x 128 (one workgroup) with the same gates: both layouts of
    both results against float64."""
    C = _C()
    rows, f = 64, 128
    gu, dout = _swiglu_inputs(rows, f, BF16, seed=64)
    ref = _swiglu_ref(gu, dout, BF16)
    for pad in (0, 8):
        o, ot = C.swiglu_fwd_t(gu, pad)
        assert o.shape == (rows, f) and ot.shape == (f, rows)
        _check(o, ref["out"], ref["out_tol"], f"swiglu_fwd_t pad={pad}")
        _check(ot, ref["out"].t(), ref["out_tol"].t(), f"swiglu_fwd_t transposed pad={pad}")
    dgu, dgut = C.swiglu_bwd_t(gu, dout)
    assert dgu.shape == (rows, 2 * f) and dgut.shape == (2 * f, rows)
    _check(dgu, ref["dgu"], ref["dgu_tol"], "swiglu_bwd_t")
    _check(dgut, ref["dgu"].t(), ref["dgu_tol"].t(), "swiglu_bwd_t transposed")


# ============================================================================= argument checks
def _all_raise(bad):
    for name, call in bad.items():
        with pytest.raises(RuntimeError):
            call()
            pytest.fail(f"{name}: accepted")
    torch.cuda.synchronize()  # nothing was launched that could have faulted


def _misaligned(rows, cols, dtype):
    """A contiguous [rows, cols] tensor whose base is one element past a 16-byte boundary."""
    flat = torch.zeros(rows * cols + 8, device=DEV, dtype=dtype)
    t = flat[1:1 + rows * cols].view(rows, cols)
    assert t.data_ptr() % 16 != 0 and t.is_contiguous()
    return t


@pytest.mark.parametrize("dtype", [BF16, F32], ids=_id)
def test_ce_argument_checks(dtype):
    C = _C()
    N, V = 6, 64
    x = torch.randn(N, V, device=DEV).to(dtype)
    labels = torch.arange(N, device=DEV)
    gscale = torch.ones(N, device=DEV)
    _, lse = C.ce_fwd(x, labels, -100)
    C.ce_bwd(x, labels, lse, gscale, -100, False)  # the well-formed call is accepted
    strided = torch.arange(2 * N, device=DEV)[::2]
    _all_raise({
        "ce_bwd int32 labels": lambda: C.ce_bwd(x, labels.int(), lse, gscale, -100, False),
        "ce_bwd labels length": lambda: C.ce_bwd(x, labels[:-1], lse, gscale, -100, False),
        "ce_bwd labels strided": lambda: C.ce_bwd(x, strided, lse, gscale, -100, False),
        "ce_bwd labels on the CPU": lambda: C.ce_bwd(x, labels.cpu(), lse, gscale, -100, False),
        "ce_bwd lse bf16": lambda: C.ce_bwd(x, labels, lse.to(BF16), gscale, -100, False),
        "ce_bwd lse length": lambda: C.ce_bwd(x, labels, lse[:-1], gscale, -100, False),
        "ce_fwd labels on the CPU": lambda: C.ce_fwd(x, labels.cpu(), -100),
    })


@pytest.mark.parametrize("dtype", [BF16, F32], ids=_id)
def test_rope_bwd_argument_checks(dtype):
    from gke_ray_train_amd.ops import _ref
    C = _C()
    other = F32 if dtype == BF16 else BF16
    T, S, hq, hkv, D = 6, 6, 2, 1, 16
    width = (hq + 2 * hkv) * D
    cos, sin = _ref.rope_tables(S, D, 10000.0, device=DEV)
    dq = torch.randn(T, hq, D, device=DEV).to(dtype)
    dk = torch.randn(T, hkv, D, device=DEV).to(dtype)

    def run(dq_, dk_, dqkv):
        return lambda: C.rope_bwd(dq_, dk_, dqkv, cos, sin, None, hq, hkv, D, S)

    run(dq, dk, torch.zeros(T, width, device=DEV, dtype=dtype))()  # the well-formed call is accepted
    _all_raise({
        "dqkv narrower than (hq + hkv) D": run(dq, dk, torch.zeros(T, width, device=DEV, dtype=dtype)[:, :(hq + hkv) * D - 8]),
        "dqkv ld % 8": run(dq, dk, torch.zeros(T, width + 4, device=DEV, dtype=dtype)[:, :width]),
        "dqkv misaligned base": run(dq, dk, _misaligned(T, width, dtype)),
        "dqkv dtype": run(dq, dk, torch.zeros(T, width, device=DEV, dtype=other)),
        "dk dtype": run(dq, dk.to(other), torch.zeros(T, width, device=DEV, dtype=dtype)),
        "dqkv on the CPU": run(dq, dk, torch.zeros(T, width, dtype=dtype)),
    })


def test_swiglu_bwd_argument_checks():
    C = _C()
    gu = torch.randn(4, 2 * 16, device=DEV).to(BF16)
    dout = torch.randn(4, 16, device=DEV).to(BF16)
    C.swiglu_bwd(gu, dout)  # the well-formed call is accepted
    bad = _misaligned(4, 2 * 16, BF16)
    _all_raise({
        "f = 12 in bf16": lambda: C.swiglu_bwd(gu[:, :24].contiguous(), dout[:, :12].contiguous()),
        "f = 6 in fp32": lambda: C.swiglu_bwd(gu[:, :12].float().contiguous(), dout[:, :6].float().contiguous()),
        "dout dtype": lambda: C.swiglu_bwd(gu, dout.float()),
        "gu misaligned": lambda: C.swiglu_bwd(bad, dout),
        "dout misaligned": lambda: C.swiglu_bwd(gu, _misaligned(4, 16, BF16)),
    })


@pytest.mark.parametrize("dtype", [BF16, F32], ids=_id)
def test_embedding_bwd_argument_checks(dtype):
    C = _C()
    V, n, d = 10, 6, 16
    dy = torch.randn(n, d, device=DEV).to(dtype)
    dw = torch.zeros(V, d, device=DEV, dtype=dtype)
    ids = torch.arange(n, device=DEV)
    C.embedding_bwd(dy, ids, dw, False)  # the well-formed call is accepted
    _all_raise({
        "d = 12": lambda: C.embedding_bwd(dy[:, :12].contiguous(), ids, dw[:, :12].contiguous(), False),
        "ids on the CPU": lambda: C.embedding_bwd(dy, ids.cpu(), dw, False),
        "ids strided": lambda: C.embedding_bwd(dy, torch.arange(2 * n, device=DEV)[::2], dw, False),
        "dw on the CPU": lambda: C.embedding_bwd(dy, ids, dw.cpu(), False),
    })


@pytest.mark.parametrize("dtype", [BF16, F32], ids=_id)
def test_empty_inputs(dtype):
    """N = 0 rows of cross-entropy, T = 0 tokens of RoPE (both kernels), n = 0 ids: correctly shaped
    empty results, no error, nothing launched."""
    from gke_ray_train_amd import ops
    from gke_ray_train_amd.ops import _ref
    C = _C()
    V = 64
    x = torch.empty(0, V, device=DEV, dtype=dtype)
    labels = torch.empty(0, device=DEV, dtype=torch.int64)
    loss_rows, lse = C.ce_fwd(x, labels, -100)
    assert loss_rows.shape == (0,) and lse.shape == (0,)
    assert C.ce_bwd(x, labels, lse, torch.empty(0, device=DEV), -100, False).shape == (0, V)
    xs = x.clone().requires_grad_()
    loss = ops.cross_entropy(xs, labels)
    loss.backward()
    assert loss.item() == 0.0 and xs.grad.shape == (0, V)

    hq, hkv, S = 2, 1, 8
    try:
        for fast in (1, 0):
            C.ew_set_fast(fast)
            for D in (64, 128):
                cos, sin = _ref.rope_tables(S, D, 10000.0, device=DEV)
                width = (hq + 2 * hkv) * D
                q, k = C.rope_fwd(torch.empty(0, width, device=DEV, dtype=dtype), cos, sin, None, hq, hkv, D, S)
                assert q.shape == (0, hq, D) and k.shape == (0, hkv, D)
                C.rope_bwd(q, k, torch.empty(0, width, device=DEV, dtype=dtype), cos, sin, None, hq, hkv, D, S)
    finally:
        C.ew_set_fast(1)

    d = 16
    w = torch.randn(5, d, device=DEV).to(dtype)
    assert C.embedding_fwd(labels, w).shape == (0, d)
    dw = torch.full((5, d), 3.0, device=DEV, dtype=dtype)
    C.embedding_bwd(torch.empty(0, d, device=DEV, dtype=dtype), labels, dw, True)
    assert bool((dw == 3).all()), "accumulating nothing leaves dw as it is"
    C.embedding_bwd(torch.empty(0, d, device=DEV, dtype=dtype), labels, dw, False)
    assert not dw.any()
    torch.cuda.synchronize()
