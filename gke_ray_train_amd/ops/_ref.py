"""Pure-PyTorch reference implementations of every native op.

Used (a) on CPU hosts (gloo plumbing runs, unit tests) and (b) as the fp32 numerics oracle of
the HIP kernels in the GPU tests. Semantics mirror the HF / torch modules the reference scripts
run (Llama RMSNorm rounding, erf GELU, rotate-half RoPE, CE with ignore_index=-100).
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F


def rmsnorm(x, w, eps, residual=None):
    h = x if residual is None else (x + residual)
    hf = h.float()
    rstd = torch.rsqrt(hf.pow(2).mean(-1, keepdim=True) + eps)
    y = (hf * rstd * w.float()).to(x.dtype)
    return y, h


def layernorm(x, w, b, eps, residual=None):
    h = x if residual is None else (x + residual)
    y = F.layer_norm(h.float(), (h.shape[-1],), w.float(), None if b is None else b.float(), eps).to(x.dtype)
    return y, h


def swiglu(gu):
    g, u = gu.float().chunk(2, dim=-1)
    return (F.silu(g) * u).to(gu.dtype)


def gelu(x):
    return F.gelu(x.float(), approximate="none").to(x.dtype)


def rope_tables(seq_len, head_dim, theta=10000.0, device=None, scaling=None):
    """cos/sin tables [S, D/2] fp32 for the rotate-half convention.

    ``scaling`` = dict(type="llama3", factor, low_freq_factor, high_freq_factor,
    original_max_position_embeddings) reproduces Llama-3.1's frequency scaling.
    """
    inv = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.float64) / head_dim))
    if scaling and scaling.get("type", scaling.get("rope_type")) == "llama3":
        factor = scaling["factor"]
        lf, hf = scaling["low_freq_factor"], scaling["high_freq_factor"]
        old = scaling["original_max_position_embeddings"]
        low_wl, high_wl = old / lf, old / hf
        wl = 2 * math.pi / inv
        scaled = torch.where(wl > low_wl, inv / factor, inv)
        smooth = (old / wl - lf) / (hf - lf)
        mid = (1 - smooth) * scaled / factor + smooth * scaled
        is_mid = (wl >= high_wl) & (wl <= low_wl)
        inv = torch.where(is_mid, mid, scaled)
    t = torch.arange(seq_len, dtype=torch.float64)
    fr = torch.outer(t, inv)
    return fr.cos().float().to(device), fr.sin().float().to(device)


def apply_rope(x, cos, sin, pos=None):
    """x: [T, H, D]; cos/sin [S, D/2]; position of row t = pos[t] or t % S."""
    T = x.shape[0]
    S = cos.shape[0]
    idx = pos.long() if pos is not None else torch.arange(T, device=x.device) % S
    c = cos[idx].unsqueeze(1)
    s = sin[idx].unsqueeze(1)
    xf = x.float()
    x1, x2 = xf.chunk(2, dim=-1)
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1).to(x.dtype)


_M32 = 0xFFFFFFFF


def _fmix32(h):
    h = h ^ (h >> 16)
    h = (h * 0x85EBCA6B) & _M32
    h = h ^ (h >> 13)
    h = (h * 0xC2B2AE35) & _M32
    return h ^ (h >> 16)


def attn_dropout_keep(seed: int, B: int, H: int, Sq: int, Sk: int, p: float, device=None) -> torch.Tensor:
    """[B, H, Sq, Sk] bool keep-mask of the attention-probability dropout, bit-identical to the
    counter hash of csrc/include/grt_attn_dropout.h (element (b*H + h, q, k))."""
    thresh = min(_M32, math.ceil(p * 2 ** 32))
    bh = torch.arange(B * H, device=device, dtype=torch.int64).view(B, H, 1, 1)
    q = torch.arange(Sq, device=device, dtype=torch.int64).view(1, 1, Sq, 1)
    k = torch.arange(Sk, device=device, dtype=torch.int64).view(1, 1, 1, Sk)
    h = (seed & _M32) ^ ((bh * 0x9E3779B1) & _M32)
    h = _fmix32(h ^ ((q * 0x85EBCA77) & _M32))
    h = _fmix32(h ^ ((k * 0xC2B2AE3D) & _M32))
    return h >= thresh


def _splitmix64(x):
    """numpy uint64 splitmix64 finaliser (wrapping arithmetic), as hash_u64 in elementwise.hip."""
    import numpy as np
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def dropout_keep_mask(seed: int, offset: int, n: int, p: float) -> torch.Tensor:
    """[n] bool keep-mask of the element dropout kernels (elementwise.hip ``drop_keep``),
    recomputed independently on the host: element i keeps iff 16 bits of
    splitmix64(splitmix64(seed) ^ ((offset + i) / 4)), selected by (offset + i) % 4, are
    >= round(p * 65536)."""
    import numpy as np
    key = _splitmix64(np.array([seed & 0xFFFFFFFFFFFFFFFF], dtype=np.uint64))[0]
    idx = np.arange(offset, offset + n, dtype=np.uint64)
    h = _splitmix64(key ^ (idx >> np.uint64(2)))
    bits = (h >> (np.uint64(16) * (idx & np.uint64(3)))) & np.uint64(0xFFFF)
    thr = int(np.float32(p) * np.float32(65536.0) + np.float32(0.5))
    return torch.from_numpy(bits >= np.uint64(thr))


_M64 = (1 << 64) - 1


def _s64(x: int) -> int:
    """Python int -> the int64 with the same low 64 bits (torch has no uint64 arithmetic)."""
    x &= _M64
    return x - (1 << 64) if x >> 63 else x


def _lsr(x, s: int):
    return (x >> s) & ((1 << (64 - s)) - 1)  # logical shift of an int64 tensor / a masked python int


def _splitmix64_any(x):
    """hash_u64 (grt_common.h) on a python int (masked to 64 bits) or on an int64 tensor, whose
    wrapping two's-complement arithmetic gives the same bits as the kernel's uint64."""
    if isinstance(x, int):
        x = (x + 0x9E3779B97F4A7C15) & _M64
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
        return x ^ (x >> 31)
    x = x + _s64(0x9E3779B97F4A7C15)
    x = (x ^ _lsr(x, 30)) * _s64(0xBF58476D1CE4E5B9)
    x = (x ^ _lsr(x, 27)) * _s64(0x94D049BB133111EB)
    return x ^ _lsr(x, 31)


def sample_noise(seed: int, counter: int, B: int, V: int, device=None) -> torch.Tensor:
    """[B, V] float64 Gumbel noise of the sampler (csrc/kernels/sample.hip), the same bits:
        key = splitmix64(splitmix64(seed) + counter)            (64-bit wrapping add)
        h_i = splitmix64(key ^ ((row << 32) | i))               (i < 2^31)
        n_i = h_i >> 41 (the top 23 bits), u_i = (n_i + 0.5) * 2^-23, g_i = -log(-log(u_i))
    u_i is exact in fp32; the kernel takes the two logs in fp32, this takes them in float64."""
    key = _splitmix64_any((_splitmix64_any(seed & _M64) + counter) & _M64)
    row = torch.arange(B, device=device, dtype=torch.int64)[:, None] << 32
    idx = row | torch.arange(V, device=device, dtype=torch.int64)[None, :]
    n = _lsr(_splitmix64_any(idx ^ _s64(key)), 41)
    u = (n.double() + 0.5) * 2.0 ** -23
    return -torch.log(-torch.log(u))


def sample_filter(logits, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0):
    """The sampler's kept set, in float64 on z = fp32(logits) * fp32(1 / temperature) (the one
    fp32 multiply the kernel does; NaN counts as -inf). Returns (z [B, V] float64, keep [B, V] bool,
    frac [B, V] float64 = M_>(i) / Z, the top-p coordinate of every top-k survivor, inf elsewhere).
    top-k (0 or >= V: off) keeps i iff #{j : z_j > z_i} < k; top-p (1.0: off) keeps a survivor iff
    M_>(i) < top_p * Z, with e_j = exp(z_j - z_max), Z the survivors' sum and M_>(i) their sum over
    z_j > z_i. Ties stay or go together, the maximum always stays, -inf never does."""
    B, V = logits.shape
    inv_t = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(temperature), dtype=torch.float32)
    z = (logits.float() * inv_t.to(logits.device)).double()
    z = torch.where(torch.isnan(z), torch.full_like(z, -math.inf), z)
    asc, order = z.sort(-1)
    n_le = torch.searchsorted(asc, z, right=True)  # #{j : z_j <= z_i}
    keep = z > -math.inf
    if 0 < top_k < V:
        keep &= (V - n_le) < top_k
    zmax = asc[:, -1:]
    finite_max = torch.where(torch.isfinite(zmax), zmax, torch.zeros_like(zmax))
    e = torch.where(keep, torch.exp(z - finite_max), torch.zeros_like(z))
    e = torch.where(keep & (z == zmax), torch.ones_like(e), e)  # +inf rows: the maxima carry the mass
    Z = e.sum(-1, keepdim=True)
    # mass of the survivors with z_j <= z_i: a prefix sum in ascending order, read at n_le - 1
    e_asc = torch.gather(e, -1, order)
    m_le = torch.gather(e_asc.cumsum(-1), -1, (n_le - 1).clamp_(min=0))
    frac = torch.where(keep, ((Z - m_le) / Z).clamp_(min=0.0), torch.full_like(z, math.inf))
    frac = torch.where(keep & (z == zmax), torch.zeros_like(frac), frac)  # exactly 0 for the maximum
    if top_p < 1.0:
        keep = keep & (frac < top_p)
    return z, keep, frac


def sample_tokens(logits, seed: int = 0, counter: int = 0, temperature: float = 1.0, top_k: int = 0,
                  top_p: float = 1.0, do_sample: bool = True) -> torch.Tensor:
    """Host implementation (and oracle) of the device sampler: one token per row of logits [B, V],
    int64 [B] on the logits' device. Greedy: argmax of the raw logits. Sampling: Gumbel-max,
    argmax over the kept set (``sample_filter``) of z_i + g_i with ``sample_noise(seed, counter)``.
    Lowest index on ties; index 0 when nothing is kept. The same (seed, counter) and the same
    logits give the same tokens as the kernel (up to fp32-vs-float64 near-ties)."""
    B, V = logits.shape
    if do_sample:
        z, keep, _ = sample_filter(logits, temperature, top_k or 0, 1.0 if top_p is None else top_p)
        score = torch.where(keep, z + sample_noise(seed, counter, B, V, logits.device), torch.full_like(z, -math.inf))
    else:
        score = logits.double()
        score = torch.where(torch.isnan(score), torch.full_like(score, -math.inf), score)
    best = score.max(-1, keepdim=True).values
    idx = torch.arange(V, device=logits.device).expand(B, V)
    tok = torch.where(score == best, idx, torch.full_like(idx, V)).min(-1).values
    return torch.where(best.squeeze(-1) == -math.inf, torch.zeros_like(tok), tok)


def attention(q, k, v, causal=True, scale=None, seqlens_k=None, dropout_p=0.0, seed=0):
    """q [B,Sq,Hq,D], k/v [B,Sk,Hkv,D] -> o [B,Sq,Hq,D]; math in fp32 (explicit matmul/softmax —
    no SDPA backend dispatch). ``dropout_p`` drops attention probabilities with the kernel's mask."""
    B, Sq, Hq, D = q.shape
    Sk, Hkv = k.shape[1], k.shape[2]
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    rep = Hq // Hkv
    qf = q.float().transpose(1, 2)
    kf = k.float().transpose(1, 2).repeat_interleave(rep, dim=1)
    vf = v.float().transpose(1, 2).repeat_interleave(rep, dim=1)
    s = torch.matmul(qf, kf.transpose(-1, -2)) * scale
    mask = torch.zeros(Sq, Sk, dtype=torch.bool, device=q.device)
    if causal:
        off = Sk - Sq
        mask = torch.arange(Sk, device=q.device)[None, :] > (torch.arange(Sq, device=q.device)[:, None] + off)
    mask = mask[None, None].expand(B, 1, Sq, Sk)
    if seqlens_k is not None:
        kv = torch.arange(Sk, device=q.device)[None, :] >= seqlens_k.to(q.device).long()[:, None]
        mask = mask | kv[:, None, None, :]
    s = s.masked_fill(mask, float("-inf"))
    p = torch.softmax(s, dim=-1)
    p = torch.nan_to_num(p, nan=0.0)
    if dropout_p > 0.0:
        keep = attn_dropout_keep(seed, B, Hq, Sq, Sk, dropout_p, device=q.device)
        p = p * keep.to(p.dtype) / (1.0 - dropout_p)
    o = torch.matmul(p, vf).transpose(1, 2)
    return o.to(q.dtype)


def cross_entropy(logits, labels, ignore_index=-100):
    """torch's mean cross-entropy, except that a batch with every row ignored gives 0 (and zero
    gradients) like the GPU path's clamp_min(1) denominator, where torch's mean is 0 / 0 = NaN."""
    if not bool((labels != ignore_index).any()):
        return F.cross_entropy(logits.float(), labels, ignore_index=ignore_index, reduction="sum")
    return F.cross_entropy(logits.float(), labels, ignore_index=ignore_index)


def adamw_(p, g, m, v, step, lr, beta1, beta2, eps, wd, grad_scale=1.0, master=None):
    """In-place torch.optim.AdamW semantics (decoupled decay) on fp32 state."""
    pf = master if master is not None else p.float()
    gf = g.float() * grad_scale
    m.mul_(beta1).add_(gf, alpha=1 - beta1)
    v.mul_(beta2).addcmul_(gf, gf, value=1 - beta2)
    bc1 = 1 - beta1 ** step
    bc2 = 1 - beta2 ** step
    pf.mul_(1 - lr * wd)
    denom = (v.sqrt() / math.sqrt(bc2)).add_(eps)
    pf.addcdiv_(m, denom, value=-lr / bc1)
    if master is not None:
        p.copy_(pf)
    else:
        p.copy_(pf.to(p.dtype))


NF4_CODE = torch.tensor([
    -1.0, -0.6961928009986877, -0.5250730514526367, -0.39491748809814453,
    -0.28444138169288635, -0.18477343022823334, -0.09105003625154495, 0.0,
    0.07958029955625534, 0.16093020141124725, 0.24611230194568634, 0.33791524171829224,
    0.44070982933044434, 0.5626170039176941, 0.7229568362236023, 1.0])


def nf4_quantize(w, blocksize=64):
    flat = w.reshape(-1).float()
    blocks = flat.view(-1, blocksize)
    absmax = blocks.abs().amax(dim=1)
    normed = blocks / absmax.clamp_min(1e-30)[:, None]
    code = NF4_CODE.to(w.device)
    mids = (code[1:] + code[:-1]) / 2
    idx = (normed.unsqueeze(-1) > mids).sum(-1).to(torch.uint8).view(-1)
    packed = (idx[0::2] << 4) | idx[1::2]
    return packed, absmax


def nf4_dequantize(packed, absmax, n, blocksize=64, dtype=torch.bfloat16):
    code = NF4_CODE.to(packed.device)
    hi = (packed >> 4).long()
    lo = (packed & 15).long()
    idx = torch.stack([hi, lo], dim=1).view(-1)
    vals = code[idx].view(-1, blocksize) * absmax[:, None]
    return vals.view(-1)[:n].to(dtype)


def nf4_gemv(x, packed, absmax, N, K, h=None, lora_b=None, lora_off=None, scaling=1.0):
    """x [M, K] times the exact NF4 weight (fp32 level * fp32 absmax, blocksize 64), plus
    scaling * h[:, i r:(i + 1) r] lora_b[i]^T on rows lora_off[i] ...; float64 sums, rounded once."""
    w = nf4_dequantize(packed, absmax, N * K, 64, torch.float32).view(N, K)
    y = x.double() @ w.double().t()
    if lora_b:
        r = lora_b[0].shape[1]
        for i, (b, off) in enumerate(zip(lora_b, lora_off)):
            y[:, off:off + b.shape[0]] += scaling * (h[:, i * r:(i + 1) * r].double() @ b.double().t())
    return y.to(x.dtype)


# ----------------------------------------------------------------------------- 8-bit block-quantised moments
# The "dynamic" 8-bit type of the 8-bit-optimizers paper (Dettmers et al., 2021): decades 10^-6 ..
# 10^0, a linear fraction inside each decade (bin centres of [0.1, 1]), and twice as many fraction
# steps in every higher decade. A state tensor is cut into blocks of 256 consecutive elements, each
# with one fp32 absmax; an element is the uint8 code of the table entry nearest to x / absmax. The
# tables here are this project's own (the kernels in adamw8.hip build the same ones from the same
# formula); they are not bitsandbytes' tables.
Q8_BLOCK = 256
_Q8_DECADES = (1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1, 1.0)


def _q8_magnitudes(first_steps):
    """first_steps fraction steps in the decade of 10^-6, doubling per decade; float64, increasing."""
    out = []
    for i, d in enumerate(_Q8_DECADES):
        k = first_steps << i
        out.extend(d * (0.1 + 0.9 * (j + 0.5) / k) for j in range(k))
    return out


def _q8_tables():
    mag = _q8_magnitudes(1)  # 127 magnitudes; mirrored, with 0 and +-1, they would make 257 entries:
    # the smallest negative magnitude (-5.5e-7) is the one left out, so all 256 codes are in use
    signed = [-1.0] + [-x for x in reversed(mag[1:])] + [0.0] + mag + [1.0]
    unsigned = [0.0] + _q8_magnitudes(2) + [1.0]  # 254 magnitudes
    out = []
    for t in (signed, unsigned):
        assert len(t) == 256
        t32 = torch.tensor(t, dtype=torch.float64).to(torch.float32)
        mids = ((t32[1:].double() + t32[:-1].double()) / 2).to(torch.float32)
        out.append((t32, mids))
    return out


(Q8_SIGNED, _Q8_SIGNED_MIDS), (Q8_UNSIGNED, _Q8_UNSIGNED_MIDS) = _q8_tables()
Q8_ZERO_CODE = {True: int((Q8_SIGNED == 0).nonzero()), False: int((Q8_UNSIGNED == 0).nonzero())}  # 127, 0


def q8_table(signed: bool) -> torch.Tensor:
    """The 256 fp32 entries, increasing: signed for exp_avg, unsigned for exp_avg_sq."""
    return Q8_SIGNED if signed else Q8_UNSIGNED


def q8_blocks(n: int) -> int:
    return (n + Q8_BLOCK - 1) // Q8_BLOCK


def quantize_blockwise8(x, signed: bool):
    """x (any shape, read flat) -> (uint8 codes [n], fp32 absmax [ceil(n / 256)]). The code is the
    number of table midpoints below fp32(x / absmax), i.e. the nearest entry (the lower one at a
    tie); a block with absmax == 0 stores the code of 0.0. A non-finite element makes its block's
    absmax non-finite."""
    flat = x.detach().reshape(-1).to(torch.float32)
    n = flat.numel()
    nb = q8_blocks(n)
    blocks = torch.zeros(nb * Q8_BLOCK, dtype=torch.float32, device=flat.device)
    blocks[:n] = flat
    blocks = blocks.view(nb, Q8_BLOCK)
    absmax = blocks.abs().amax(dim=1)  # NaN propagates
    normed = torch.where(absmax[:, None] == 0, torch.zeros_like(blocks), blocks / absmax[:, None])
    mids = (_Q8_SIGNED_MIDS if signed else _Q8_UNSIGNED_MIDS).to(flat.device)
    codes = torch.bucketize(normed, mids, right=False)  # mids[c - 1] < x <= mids[c]
    codes = torch.where(normed.isnan(), torch.zeros_like(codes), codes)  # no midpoint is below NaN
    return codes.view(-1)[:n].to(torch.uint8), absmax


def dequantize_blockwise8(codes, absmax, signed: bool):
    """fp32(table[code] * absmax of the element's block), flat [n]."""
    n = codes.numel()
    table = q8_table(signed).to(codes.device)
    scale = absmax.to(torch.float32).repeat_interleave(Q8_BLOCK)[:n]
    return table[codes.reshape(-1).long()] * scale


def adamw8_(p, g, codes_m, absmax_m, codes_v, absmax_v, step, lr, beta1, beta2, eps, wd, grad_scale=1.0,
            master=None):
    """adamw_ on the dequantised moments: the parameter is computed from the fp32 new moments, which
    are quantised and stored (in place) only afterwards."""
    m = dequantize_blockwise8(codes_m, absmax_m, True).view(p.shape)
    v = dequantize_blockwise8(codes_v, absmax_v, False).view(p.shape)
    adamw_(p, g, m, v, step, lr, beta1, beta2, eps, wd, grad_scale=grad_scale, master=master)
    for x, codes, absmax, signed in ((m, codes_m, absmax_m, True), (v, codes_v, absmax_v, False)):
        c, a = quantize_blockwise8(x, signed)
        codes.copy_(c)
        absmax.copy_(a)


# ----------------------------------------------------------------------------- prompt-lookup speculative decoding
# Host implementations (and oracles) of the draft and accept steps of csrc/kernels/spec.hip. All
# of it is integer work, so the kernels give the same values bit for bit.
def prompt_lookup_draft(hist, n_hist: int, K: int, N: int):
    """K draft tokens for the sequence ``hist[:n_hist]`` (prompt + tokens emitted so far; any
    sequence of ints or a 1-D tensor). For n = min(N, n_hist - 1) down to 1, the last n tokens are
    searched among the earlier positions: an occurrence starting at s counts when its continuation
    holds at least one token (s + n < n_hist; it may overlap the suffix), and the latest one wins.
    The draft is hist[s + n : s + n + K], cut at the end of the history; unfilled slots, and every
    slot when no n matches, are -1, which equals no token."""
    h = hist.tolist() if hasattr(hist, "tolist") else list(hist)
    for n in range(min(N, n_hist - 1), 0, -1):
        tail = h[n_hist - n:n_hist]
        for s in range(n_hist - n - 1, -1, -1):
            if h[s:s + n] == tail:
                d = h[s + n:min(s + n + K, n_hist)]
                return d + [-1] * (K - len(d))
    return [-1] * K


def spec_accept(drafts, cand, n: int, max_new_tokens: int, eos_ids=(), finished: bool = False):
    """The accept step of one verify pass. ``cand[t]`` is the token the sampler draws from logits
    row t (token number n + t), ``drafts[i]`` the draft that was fed as input i + 1, ``n`` the
    number of tokens emitted so far. The accepted count a is the largest j with drafts[i] ==
    cand[i] for all i < j; cand[0 .. a] are emitted, cut after the first EOS among them and at
    ``max_new_tokens``. Returns (emitted, finished, finish_step): ``finish_step`` is the token
    number of the EOS when this step finished the row, else -1. A row that is finished or full
    (n >= max_new_tokens) is inert: nothing is emitted."""
    if finished or n >= max_new_tokens:
        return [], bool(finished), -1
    a = 0
    while a < len(drafts) and int(drafts[a]) == int(cand[a]):
        a += 1
    out = []
    for i in range(a + 1):
        if n + len(out) >= max_new_tokens:
            break
        out.append(int(cand[i]))
        if out[-1] in eos_ids:
            return out, True, n + len(out) - 1
    return out, False, -1


# ----------------------------------------------------------------------------- fp8 KV cache
# The format of the fp8 KV cache (csrc/kernels/kv_fp8.hip, decode_attention.hip): OCP e4m3fn codes
# with one fp32 scale per head vector (one (token, kv head) of K or V). This is the definition; the
# device quantiser reproduces it bit for bit on bf16 inputs.
KV_FP8_MAX = 448.0  # the largest finite e4m3fn value (code 126)


def kv_fp8_table() -> torch.Tensor:
    """The 256 fp32 values of the OCP e4m3fn codes (0x7F / 0xFF are NaN)."""
    return torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float()


def kv_fp8_quantize(x):
    """x [..., D] -> (uint8 codes [..., D], fp32 scale [...]): scale = max|x| / 448 over the last
    dim (1.0 for an all-zero vector), code = x / scale clamped to +-448 and rounded to nearest-even
    e4m3fn. The vector's largest element gets code 126, no NaN code is produced for finite x, and
    |dequant - x| <= max(|x| 2^-4, scale 2^-10) (half an ulp of 3 mantissa bits, or half the
    subnormal step)."""
    xf = x.float()
    amax = xf.abs().amax(-1)
    scale = torch.where(amax == 0, torch.ones_like(amax), amax / KV_FP8_MAX)
    y = (xf / scale.unsqueeze(-1)).clamp(-KV_FP8_MAX, KV_FP8_MAX)
    return y.to(torch.float8_e4m3fn).view(torch.uint8), scale


def kv_fp8_dequantize(codes, scale, dtype=torch.float32):
    """table[code] * scale (fp32 product), rounded to ``dtype``."""
    table = kv_fp8_table().to(codes.device)
    return (table[codes.long()] * scale.float().unsqueeze(-1)).to(dtype)
