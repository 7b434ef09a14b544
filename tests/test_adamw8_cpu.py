"""8-bit block-quantised AdamW on the host: the quantisation scheme of ops/_ref.py (tables, blocks
of 256, nearest entry), _ref.adamw8_ against a float64 AdamW, the AdamW8bit optimizer on CPU
parameters (state dicts in the torch.optim.AdamW layout, both ways between the 32-bit and the 8-bit
optimizer), make_optimizer's refusals, and the portable optimizer state of the data-parallel engine
(world 1 bit for bit; a ZeRO shard layout of world 2 resumed at world 1 to one quantisation step).

Bounds. The quantiser picks the table entry nearest to fp32(x / absmax); that one rounding can move
a value across a midpoint by at most 2^-24 |x|, so |table[code] absmax - x| <= (half the larger gap
to a neighbouring entry) absmax + 2^-24 |x| with the product taken in float64. _ref.adamw8_ is
_ref.adamw_ on the dequantised moments by definition (compared bitwise), and that in turn is held to
4 units of 2^-23 times the magnitude of the terms summed, the units of tests/test_optim_kernels_gpu.py:
the update is a chain of about six fp32 operations of half an ulp each.
"""
import math
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from gke_ray_train_amd.ops import _ref

F32, F64 = torch.float32, torch.float64
N = 4381  # 17 full blocks and one of 29 elements


def _half_gap(signed):
    """Per code: half the larger distance to a neighbouring entry (float64)."""
    t = _ref.q8_table(signed).double()
    gap = t[1:] - t[:-1]
    return torch.maximum(torch.cat([gap[:1], gap]), torch.cat([gap, gap[-1:]])) / 2


def _block_of(n):
    return torch.arange(n) // _ref.Q8_BLOCK


# ----------------------------------------------------------------------------- the tables
@pytest.mark.parametrize("signed", [True, False], ids=["signed", "unsigned"])
def test_table_properties(signed):
    t = _ref.q8_table(signed)
    assert t.dtype == F32 and t.numel() <= 256
    # every code is in use here: the signed table drops one of the 257 candidates (127 magnitudes
    # mirrored, 0, +-1), the smallest negative magnitude, instead of leaving a code unused
    assert t.numel() == 256
    assert bool((t[1:] > t[:-1]).all()), "entries must increase strictly"
    assert bool((t == 0).any()) and bool((t == 1).any())
    assert bool((t == -1).any()) == signed
    assert float(t[t > 0].min()) <= 1e-6
    assert float(t.abs().max()) == 1.0
    assert float(t[_ref.Q8_ZERO_CODE[signed]]) == 0.0
    # decades 10^-6 .. 10^0, more fraction steps in the higher ones
    pos = t[t > 0].double()
    counts = [int(((pos > 10.0 ** (d - 1)) & (pos <= 10.0 ** d)).sum()) for d in range(-5, 1)]
    assert counts == sorted(counts) and counts[-1] > counts[0], counts
    # the quantiser emits every code, and only for its own entry
    codes, absmax = _ref.quantize_blockwise8(t, signed)
    assert torch.equal(codes, torch.arange(256, dtype=torch.uint8)) and absmax.tolist() == [1.0]
    assert torch.equal(_ref.dequantize_blockwise8(codes, absmax, signed), t)


def _random_state(signed, seed, n=N):
    gen = torch.Generator().manual_seed(seed)
    # magnitudes over eight decades, as moments have
    x = torch.randn(n, generator=gen) * torch.exp(4 * torch.randn(n, generator=gen))
    if not signed:
        return x.abs()
    x[256:512] = -x[256:512].abs()  # a block whose largest element is negative ...
    x[300] = -3 * x[256:512].abs().max()
    return x


@pytest.mark.parametrize("signed", [True, False], ids=["signed", "unsigned"])
def test_requantisation_is_the_identity(signed):
    for seed in range(50):
        x = _random_state(signed, seed)
        codes, absmax = _ref.quantize_blockwise8(x, signed)
        if signed:
            assert codes[300] == 0 and absmax[1] == x[300].abs()  # ... is coded -1
        assert codes.dtype == torch.uint8 and codes.numel() == N and absmax.numel() == _ref.q8_blocks(N) == 18
        deq = _ref.dequantize_blockwise8(codes, absmax, signed)
        codes2, absmax2 = _ref.quantize_blockwise8(deq, signed)
        assert torch.equal(codes, codes2) and torch.equal(absmax, absmax2), seed


@pytest.mark.parametrize("signed", [True, False], ids=["signed", "unsigned"])
def test_host_quantiser_against_float64(signed):
    half = _half_gap(signed)
    table = _ref.q8_table(signed).double()
    worst = 0.0
    for seed in range(10):
        x = _random_state(signed, 100 + seed)
        codes, absmax = _ref.quantize_blockwise8(x, signed)
        assert torch.equal(absmax, torch.stack([b.abs().max() for b in x.split(_ref.Q8_BLOCK)]))
        a = absmax.double()[_block_of(N)]
        err = (table[codes.long()] * a - x.double()).abs()
        bound = half[codes.long()] * a + 2.0 ** -24 * x.double().abs()
        worst = max(worst, float((err / bound).max()))
        assert bool((err <= bound).all()), (seed, float((err / bound).max()))
        # fp32 and float64 normalisation pick the same entry except within one rounding of a midpoint
        c64 = torch.bucketize(x.double() / a, ((table[1:] + table[:-1]) / 2))
        assert int((c64 != codes.long()).sum()) <= 2
    print(f"worst error over bound: {worst:.4f}")


def test_zero_and_nonfinite_blocks():
    x = torch.zeros(600)
    x[256:512] = torch.randn(256)
    x[520] = float("nan")
    for signed in (True, False):
        xs = x if signed else x.abs()
        codes, absmax = _ref.quantize_blockwise8(xs, signed)
        assert absmax[0] == 0 and bool((codes[:256] == _ref.Q8_ZERO_CODE[signed]).all())
        assert math.isfinite(absmax[1]) and math.isnan(absmax[2])
        deq = _ref.dequantize_blockwise8(codes, absmax, signed)
        assert bool((deq[:256] == 0).all()) and bool(deq[:512].isfinite().all()) and bool(deq[512:].isnan().all())
    # fresh state: the zero code with absmax 0
    from gke_ray_train_amd.ops import AdamW8bit
    p = torch.nn.Parameter(torch.zeros(5000))
    st = AdamW8bit([p])._init_state(p)
    assert bool((st["exp_avg_q"] == 127).all()) and bool((st["exp_avg_sq_q"] == 0).all())
    assert not bool(st["exp_avg_absmax"].any()) and not bool(st["exp_avg_sq_absmax"].any())


# ----------------------------------------------------------------------------- _ref.adamw8_
def test_ref_adamw8_against_float64():
    gen = torch.Generator().manual_seed(5)
    lr, b1, b2, eps, wd, gs = 1e-2, 0.9, 0.999, 1e-8, 0.01, 0.37
    b1, b2 = (torch.tensor(b, dtype=F32).item() for b in (b1, b2))
    p = torch.randn(N, generator=gen)
    cm, am = _ref.quantize_blockwise8(0.01 * torch.randn(N, generator=gen), True)
    cv, av = _ref.quantize_blockwise8(0.01 * torch.rand(N, generator=gen), False)
    hm, hv = _half_gap(True), _half_gap(False)
    blk = _block_of(N)
    for step in (4, 5, 6):
        g = 3 * torch.randn(N, generator=gen)
        m0 = _ref.dequantize_blockwise8(cm, am, True)
        v0 = _ref.dequantize_blockwise8(cv, av, False)
        p0 = p.clone()
        _ref.adamw8_(p, g, cm, am, cv, av, step, lr, b1, b2, eps, wd, grad_scale=gs)
        # by definition: _ref.adamw_ on the dequantised moments, the parameter from the fp32 new moments
        pr, mr, vr = p0.clone(), m0.clone(), v0.clone()
        _ref.adamw_(pr, g, mr, vr, step, lr, b1, b2, eps, wd, grad_scale=gs)
        assert torch.equal(p, pr)
        assert torch.equal(cm, _ref.quantize_blockwise8(mr, True)[0]) and torch.equal(av, _ref.quantize_blockwise8(vr, False)[1])
        # float64 AdamW from the same dequantised state
        gf = g.double() * gs
        m64 = b1 * m0.double() + (1 - b1) * gf
        v64 = b2 * v0.double() + (1 - b2) * gf * gf
        upd = lr / (1 - b1 ** step) * m64 / (v64.sqrt() / math.sqrt(1 - b2 ** step) + eps)
        p64 = p0.double() * (1 - lr * wd) - upd
        u = 2.0 ** -23
        up, um, uv = u * ((p0.double() * (1 - lr * wd)).abs() + upd.abs()), u * ((b1 * m0.double()).abs() + ((1 - b1) * gf).abs()), u * v64
        assert bool(((p.double() - p64).abs() <= 4 * up).all())
        # the stored moments: nearest entry of the float64 value, to the fp32 error of the moment itself
        for codes, absmax, x64, unit, half, signed in ((cm, am, m64, um, hm, True), (cv, av, v64, uv, hv, False)):
            a = absmax.double()[blk]
            deq = _ref.q8_table(signed).double()[codes.long()] * a
            assert bool(((deq - x64).abs() <= half[codes.long()] * a + 4 * unit).all()), (step, signed)
            big = torch.stack([b.abs().max() for b in x64.split(_ref.Q8_BLOCK)])
            assert bool(((absmax.double() - big).abs() <= 4 * u * big).all())


# ----------------------------------------------------------------------------- AdamW8bit on CPU parameters
def _params(seed=0):
    gen = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(70, 70, generator=gen)),  # 4900 elements: 8-bit
            torch.nn.Parameter(torch.randn(70, generator=gen))]      # below min_8bit_size: fp32 moments


def _steps(opt, params, steps):
    for s in steps:
        gen = torch.Generator().manual_seed(1000 + s)
        for p in params:
            p.grad = torch.randn(p.shape, generator=gen)
        opt.step()


def test_min_8bit_size_and_state_layout():
    from gke_ray_train_amd.ops import AdamW8bit
    ps = _params()
    opt = AdamW8bit(ps, lr=1e-2)
    _steps(opt, ps, range(3))
    big, small = opt.state[ps[0]], opt.state[ps[1]]
    assert set(big) == {"step", "exp_avg_q", "exp_avg_absmax", "exp_avg_sq_q", "exp_avg_sq_absmax"}
    assert big["exp_avg_q"].dtype == torch.uint8 and big["exp_avg_q"].shape == (4900,)
    assert big["exp_avg_absmax"].dtype == F32 and big["exp_avg_sq_absmax"].shape == (20,)
    assert set(small) == {"step", "exp_avg", "exp_avg_sq"} and small["exp_avg"].dtype == F32
    assert opt.state_bytes() == 2 * 4900 + 8 * 20 + 8 * 70
    # with a lower threshold the small tensor is quantised too; with a higher one nothing is
    ps2 = _params()
    opt2 = AdamW8bit(ps2, lr=1e-2, min_8bit_size=64)
    _steps(opt2, ps2, range(1))
    assert "exp_avg_q" in opt2.state[ps2[1]]
    ps3 = _params()
    opt3 = AdamW8bit(ps3, lr=1e-2, min_8bit_size=5000)
    _steps(opt3, ps3, range(1))
    assert "exp_avg" in opt3.state[ps3[0]]
    with pytest.raises(RuntimeError, match="step"):
        opt.prepare_gpu_step()
    # the small tensor follows FusedAdamW exactly, the large one closely
    from gke_ray_train_amd.ops import FusedAdamW
    pf = _params()
    _steps(FusedAdamW(pf, lr=1e-2), pf, range(3))
    assert torch.equal(pf[1], ps[1])
    assert not torch.equal(pf[0], ps[0]) and float((pf[0] - ps[0]).detach().abs().max()) < 3e-3  # 3 steps of lr 1e-2


def test_state_dict_round_trip_continues_bit_for_bit():
    from gke_ray_train_amd.ops import AdamW8bit
    ps = _params()
    opt = AdamW8bit(ps, lr=1e-2)
    _steps(opt, ps, range(3))
    sd = opt.state_dict()
    # the torch.optim.AdamW layout: fp32 moments in the parameter's shape
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    assert sd["state"][0]["exp_avg"].shape == (70, 70) and sd["state"][0]["exp_avg_sq"].dtype == F32
    torch_opt = torch.optim.AdamW(_params(), lr=1e-2)
    torch_opt.load_state_dict(sd)  # loads into torch's own optimizer
    ps2 = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    opt2 = AdamW8bit(ps2, lr=1e-2)
    opt2.load_state_dict(sd)
    for k, v in opt.state[ps[0]].items():
        assert torch.equal(v, opt2.state[ps2[0]][k]), k
    _steps(opt, ps, range(3, 6))
    _steps(opt2, ps2, range(3, 6))
    for a, b in zip(ps, ps2):
        assert torch.equal(a, b)
    assert torch.equal(opt.state[ps[0]]["exp_avg_q"], opt2.state[ps2[0]]["exp_avg_q"])


def test_state_dicts_move_between_32_bit_and_8_bit():
    from gke_ray_train_amd.ops import AdamW8bit, FusedAdamW
    pf = _params()
    fused = FusedAdamW(pf, lr=1e-2)
    _steps(fused, pf, range(3))
    p8 = [torch.nn.Parameter(p.detach().clone()) for p in pf]
    opt8 = AdamW8bit(p8, lr=1e-2)
    opt8.load_state_dict(fused.state_dict())
    st = opt8.state[p8[0]]
    assert "exp_avg" not in st and float(st["step"]) == 3
    for key, signed in (("exp_avg", True), ("exp_avg_sq", False)):
        codes, absmax = _ref.quantize_blockwise8(fused.state[pf[0]][key], signed)
        assert torch.equal(st[key + "_q"], codes) and torch.equal(st[key + "_absmax"], absmax)
    assert torch.equal(opt8.state[p8[1]]["exp_avg"], fused.state[pf[1]]["exp_avg"])
    # and back: the 8-bit state dict in a 32-bit optimizer holds the dequantised moments
    pb = [torch.nn.Parameter(p.detach().clone()) for p in pf]
    back = FusedAdamW(pb, lr=1e-2)
    back.load_state_dict(opt8.state_dict())
    assert torch.equal(back.state[pb[0]]["exp_avg"].view(-1), _ref.dequantize_blockwise8(st["exp_avg_q"], st["exp_avg_absmax"], True))
    assert back.state[pb[0]]["exp_avg_sq"].shape == (70, 70)
    _steps(back, pb, range(3, 4))
    _steps(opt8, p8, range(3, 4))
    assert torch.equal(pb[0], p8[0])  # one step from the same dequantised moments: the same parameters


def test_make_optimizer_refuses_what_it_cannot_run():
    from gke_ray_train_amd.ops import make_optimizer
    for name in ("paged_adamw_8bit", "adamw_8bit", "adamw_bnb_8bit"):
        with pytest.raises(ValueError, match="8-bit"):
            make_optimizer(name, _params(), lr=1e-3, weight_decay=0.0)
        with pytest.raises(ValueError, match="8-bit"):
            make_optimizer(name, [{"params": _params(), "weight_decay": 0.0}], lr=1e-3, weight_decay=0.0)
        with pytest.raises(ValueError, match="8-bit.*offload"):
            make_optimizer(name, _params(), lr=1e-3, weight_decay=0.0, offload=True)


# ----------------------------------------------------------------------------- portable optimizer state
GLOBAL = 4
STEPS_A, STEPS_B = 2, 2


def _batch(step):
    return torch.randint(0, 512, (GLOBAL, 32), generator=torch.Generator().manual_seed(100 + step))


def _engine(world, cls=None, split_decay=True):
    from gke_ray_train_amd.models import build_llama
    from gke_ray_train_amd.ops import AdamW8bit
    from gke_ray_train_amd.parallel import DistributedDataParallel
    m = build_llama("llama-tiny", device="cpu", dtype=F32, seed=11)
    eng = DistributedDataParallel(m, bucket_cap_mb=0.07, shard_optimizer=world > 1, split_decay=split_decay)
    opt = (cls or AdamW8bit)(eng.optimizer_param_groups(0.05), lr=2e-3)
    return m, eng, opt


def _train(eng, opt, steps, rank, world):
    for s in steps:
        ids = _batch(s).view(world, GLOBAL // world, 32)[rank]
        eng(ids, labels=ids)["loss"].backward()
        eng.finish_gradient_sync()
        st = eng.clip_grad_norm_(0.5)
        opt.step(grad_scale=st)
        eng.after_optimizer_step()
        eng.zero_grad()
    eng.wait_params()


def test_portable_state_world_1_bit_for_bit():
    m, eng, opt = _engine(1)
    _train(eng, opt, range(STEPS_A), 0, 1)
    sd = eng.portable_optimizer_state_dict(opt)
    named = list(m.named_parameters())
    assert set(sd["state"]) == set(range(len(named)))
    for i, (_n, p) in enumerate(named):  # HF layout: fp32 moments per model parameter
        assert sd["state"][i]["exp_avg"].shape == p.shape and sd["state"][i]["exp_avg"].dtype == F32
    sd = {"state": {i: {k: v.clone() for k, v in st.items()} for i, st in sd["state"].items()},
          "param_groups": sd["param_groups"], "grt_param_names": sd["grt_param_names"]}
    params = {n: p.detach().clone() for n, p in named}
    _train(eng, opt, range(STEPS_A, STEPS_A + STEPS_B), 0, 1)
    m2, eng2, opt2 = _engine(1)
    with torch.no_grad():
        for n, p in m2.named_parameters():
            p.copy_(params[n])
    eng2.load_portable_optimizer_state_dict(opt2, sd)
    big = opt2.param_groups[0]["params"][0]
    assert opt2.state[big]["exp_avg_q"].dtype == torch.uint8 and "exp_avg" not in opt2.state[big]
    assert "exp_avg" in opt2.state[opt2.param_groups[1]["params"][0]]  # 1280 elements: fp32 moments
    _train(eng2, opt2, range(STEPS_A, STEPS_A + STEPS_B), 0, 1)
    for (n, a), (_n, b) in zip(m.named_parameters(), m2.named_parameters()):
        assert torch.equal(a, b), n


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _zero_writer(rank, world, port, q, path):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), OMP_NUM_THREADS="1",
                      GRT_GLOO_TENSOR_COLLECTIVES="1")
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        # one group for matrices and the 64-element norm weights: parameters start off the block grid
        _m, eng, opt = _engine(world, split_decay=False)
        _train(eng, opt, range(STEPS_A), rank, world)
        fp = opt.param_groups[0]["params"][0]
        assert eng.zero and opt.state[fp]["exp_avg_q"].numel() == fp.numel()  # the shard's own blocks
        sd = eng.portable_optimizer_state_dict(opt)
        if rank == 0:
            torch.save(sd, path)
        q.put((rank, None))
    except BaseException as e:
        q.put((rank, repr(e)))
        raise
    finally:
        dist.destroy_process_group()


def test_portable_state_zero_2_to_1_within_one_quantisation_step(tmp_path):
    from gke_ray_train_amd.ops import FusedAdamW
    path = str(tmp_path / "opt.pt")
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_zero_writer, args=(r, 2, port, q, path)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        for _ in procs:
            r, err = q.get(timeout=300)
            assert err is None, f"rank {r}: {err}"
    finally:
        for p in procs:
            p.join(timeout=60)
    sd = torch.load(path, weights_only=True)
    # the source moments as the world-1 flat state: through the 32-bit optimizer, which keeps them as they are
    _m, eng32, opt32 = _engine(1, FusedAdamW, split_decay=False)
    eng32.load_portable_optimizer_state_dict(opt32, sd)
    _m8, eng8, opt8 = _engine(1, split_decay=False)
    eng8.load_portable_optimizer_state_dict(opt8, sd)
    fp32, fp8 = opt32.param_groups[0]["params"][0], opt8.param_groups[0]["params"][0]
    st = opt8.state[fp8]
    assert float(st["step"]) == STEPS_A
    blk = _block_of(fp8.numel())
    for key, signed in (("exp_avg", True), ("exp_avg_sq", False)):
        src = opt32.state[fp32][key].double()
        assert float(src.abs().max()) > 0
        codes, absmax = st[key + "_q"], st[key + "_absmax"]
        got = opt8.flat_state_fp32(fp8, key).double()
        bound = 2 * _half_gap(signed)[codes.long()] * absmax.double()[blk]  # one table gap x absmax
        assert bool(((got - src).abs() <= bound).all()), key
        assert not torch.equal(got, src)  # the blocks moved: not exact
