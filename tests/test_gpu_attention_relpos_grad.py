"""-m gpu: vk_attention_relpos_grad against a float64 autograd restatement.

The restatement builds the bias from `lut` by indexing and lets torch differentiate the indexing; the attention itself is one
autograd function in float64 that rounds where the kernels round (csrc/attention_relpos_grad.hip): D from the 16-bit O the kernel is
given, P rounded for dV only, dS rounded for dQ / dK only, and the UNROUNDED dS, times the scale, as the gradient of the bias.
The rule is the project's standing one (tests/test_gpu_mixed_kernels.py `held`): the kernel's distance to that reference is at most
8 x torch's own in the storage type on the same inputs, with the type's epsilon (2^-7 for bf16) of the largest element as the floor.

Shapes: L = 1 (one token), 17 (one past a 16-row wave), 65 (one past a 64-wide tile), 80 (B = 3: a partial mask, every key masked,
no key masked).  Radii 4 / 3 against positions 0 .. L - 1 and coordinates 0 .. 11: both clamps are hit and an entry collects many terms."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from vltk_amd.layoutlmv3 import attention_relpos_grad      # noqa: E402

import finetune_util as U                                  # noqa: E402
import mixed_util as X                                     # noqa: E402

DTYPES = [torch.bfloat16, torch.float16]
MASKED = -2.0 ** 120         # below -1e30: it absorbs the score in fp32, and is a finite number of bf16
HEADS = 2


def bias_of(lut, rq, rk, r1, r2):
    """lut [heads, nlut], rq [B, Lq, 3] and rk [B, Lk, 3] int64 -> t1 + (tx + ty) [B, heads, Lq, Lk] by indexing."""
    n1, n2 = 2 * r1 + 1, 2 * r2 + 1
    dl = rk[:, None, :, :] - rq[:, :, None, :]
    t1, tx, ty = (lut[:, dl[..., c].clamp(-r, r) + r + off].transpose(0, 1) for c, r, off in ((0, r1, 0), (1, r2, n1), (2, r2, n1 + n2)))
    return t1 + (tx + ty)


class RelAttention16(torch.autograd.Function):
    """q, k, v [B, heads, L, d], bias [B, heads, Lq, Lk], mask [B, Lk] in float64 -> O; the backward with the kernels' roundings."""

    @staticmethod
    def forward(ctx, q, k, v, bias, mask, scale, dtype, keep, forward16=False):
        """forward16: O as vk_attention_relpos writes it, r(r(P) V) (the trainer's restatement); else the float64 O, which the kernel
        tests round themselves."""
        p = torch.softmax((q @ k.transpose(-1, -2) + bias) * scale + mask[:, None, None, :], -1)
        o = X._r(X._r(p, dtype) @ v, dtype) if forward16 else p @ v
        ctx.save_for_backward(q, k, v, p, X._r(o, dtype))
        ctx.cfg = (scale, dtype, keep)
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, p, og = ctx.saved_tensors
        scale, dtype, keep = ctx.cfg
        ds = p * (do @ v.transpose(-1, -2) - (do * og).sum(-1, keepdim=True))
        ds16 = X._r(ds, dtype)
        keep.update(p=p, ds=ds, og=og)
        return ds16 @ k * scale, ds16.transpose(-1, -2) @ q * scale, X._r(p, dtype).transpose(-1, -2) @ do, ds * scale, None, None, None, None, None


def grads(c, dtype, restated):
    """-> dict(dq, dk, dv, dlut, o, terms) float64 numpy in the head layout: the float64 restatement, or plain torch in `dtype`."""
    td = torch.float64 if restated else dtype
    q, k, v, lut = (torch.tensor(c[n], dtype=td, requires_grad=True) for n in ("q", "k", "v", "lut"))
    mask = torch.tensor(np.maximum(c["mask"], float(torch.finfo(td).min)), dtype=td)
    bias = bias_of(lut, c["rq"], c["rk"], *c["radii"])
    keep = {}
    if restated:
        o = RelAttention16.apply(q, k, v, bias, mask, c["scale"], dtype, keep)
    else:
        o = torch.softmax((q @ k.transpose(-1, -2) + bias) * c["scale"] + mask[:, None, None, :], -1) @ v
    o.backward(torch.tensor(c["dout"], dtype=td))
    return dict(dq=q.grad, dk=k.grad, dv=v.grad, dlut=lut.grad, o=o.detach(), terms=keep)


def run_kernel(c, dtype, o):
    """The kernel on the case's operands, in the trainer's layout (q | k | v and dq | dk | dv the column blocks of one buffer)
    -> dict(dq, dk, dv [B, heads, L, d], dlut) float32 on the CPU."""
    B, heads, Lx, d = c["q"].shape
    H = heads * d
    rows = lambda a, td: torch.as_tensor(a).transpose(1, 2).reshape(B * Lx, H).to(td)
    qkv = torch.cat([rows(c[n], dtype) for n in ("q", "k", "v")], 1).cuda()
    dqkv = torch.full((B * Lx, 3 * H), float("nan"), dtype=torch.float32, device="cuda")
    rq, rk = (c[n].to(torch.int32).cuda().contiguous() for n in ("rq", "rk"))
    out = attention_relpos_grad(qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], rows(o, dtype).cuda(), rows(c["dout"], dtype).cuda(), rq, rk,
                                torch.as_tensor(c["lut"], dtype=torch.float32).cuda(), *c["radii"], heads,
                                mask=torch.as_tensor(c["mask"], dtype=torch.float32).cuda(),
                                out=tuple(dqkv[:, i * H:(i + 1) * H] for i in range(3)))
    torch.cuda.synchronize()
    back = lambda t: t.cpu().reshape(B, Lx, heads, d).transpose(1, 2)
    return dict(dq=back(out[0]), dk=back(out[1]), dv=back(out[2]), dlut=out[3].cpu())


@functools.lru_cache(maxsize=None)
def bound_case(dtype, Lx, d, radii=(4, 3), triples="scattered"):
    r = np.random.Generator(np.random.PCG64([Lx, d, radii[0]]))
    B = 3 if Lx == 80 else 2
    q, k, v, dout = (X.round16(r.standard_normal((B, HEADS, Lx, d)), dtype) for _ in range(4))
    span = 1001 if radii[1] > 100 else 12
    rq = np.stack([np.broadcast_to(np.arange(Lx), (B, Lx)), r.integers(0, span, (B, Lx)), r.integers(0, span, (B, Lx))], -1)
    if triples == "shared y":                    # one text line: every pair meets at one entry of TY, the worst collision
        rq[..., 2] = 7
    mask = np.zeros((B, Lx))
    mask[0, r.choice(Lx, Lx // 3, replace=False)] = MASKED
    if B == 3:
        mask[1, :] = MASKED
    rq = torch.from_numpy(rq.copy())
    c = dict(q=q, k=k, v=v, dout=dout, mask=mask, rq=rq, rk=rq, radii=radii, scale=U.launcher_scale(d),
             lut=r.standard_normal((HEADS, (2 * radii[0] + 1) + 2 * (2 * radii[1] + 1))).astype(np.float32).astype(np.float64))
    return c, grads(c, dtype, True), grads(c, dtype, False)


def held(tag, c, got, ref, own, dtype):
    """One key: P = 1 and dS = dP - D is zero in the reference (O is v itself), so dQ, dK and dlut have no largest element to be
    relative to.  The kernel's dP and D are two fp32 sums of the same d exact products in different orders, at most (d + 2) 2^-24
    sum_c |dO_c v_c| apart: that, times the scale and the largest |q| or |k| it is multiplied with (1 for dlut), bounds them."""
    d = c["q"].shape[-1]
    noise = (d + 2) * 2.0 ** -24 * (np.abs(c["dout"]) * np.abs(c["v"])).sum(-1).max() * c["scale"] * max(1.0, np.abs(c["q"]).max(), np.abs(c["k"]).max())
    for name in ("dq", "dk", "dv", "dlut"):
        if not ref[name].any():
            assert c["q"].shape[2] == 1 and name != "dv" and got[name].abs().max() <= noise, (name, got[name].abs().max(), noise)
            continue
        d_cpu, d_gpu = U.maxnorm_rel(own[name].double(), ref[name]), U.maxnorm_rel(got[name].double(), ref[name])
        print(f"{tag} {name}: d_cpu {d_cpu:.2e} d_gpu {d_gpu:.2e} ratio {d_gpu / max(d_cpu, X.EPS16[dtype]):.4f}")
        assert torch.isfinite(got[name]).all() and d_gpu <= 8 * max(d_cpu, X.EPS16[dtype]), (name, d_cpu, d_gpu)


@pytest.mark.parametrize("Lx", [1, 17, 65, 80])
@pytest.mark.parametrize("d", [32, 64])
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_vs_float64(dtype, d, Lx):
    c, ref, own = bound_case(dtype, Lx, d)
    held(f"{dtype} d{d} L{Lx}", c, run_kernel(c, dtype, X._r(ref["o"], dtype)), ref, own, dtype)


@pytest.mark.parametrize("radii,triples", [((128, 256), "scattered"), ((4, 3), "shared y")], ids=["default radii", "shared y"])
def test_radii_and_collisions(radii, triples):
    dtype = torch.bfloat16
    c, ref, own = bound_case(dtype, 65, 64, radii, triples)
    held(f"{radii} {triples}", c, run_kernel(c, dtype, X._r(ref["o"], dtype)), ref, own, dtype)


def test_same_input_same_bits():
    c, ref, _ = bound_case(torch.bfloat16, 65, 64, (4, 3), "shared y")
    a, b = (run_kernel(c, torch.bfloat16, X._r(ref["o"], torch.bfloat16)) for _ in range(2))
    for name in a:
        assert a[name].numpy().tobytes() == b[name].numpy().tobytes(), name


def same_bits(got, want):
    """Equal values everywhere, equal bits wherever the reference is not zero (an exact 0 is +0 or -0 by the order of a sum)."""
    g, w = got.float().numpy(), want.float().numpy()
    return np.array_equal(g, w) and (g[w != 0].view(np.uint32) == w[w != 0].view(np.uint32)).all()


@pytest.mark.parametrize("d", [64, 32])
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_exact(dtype, d):
    """A zero table and K = 0, 64 keys: P = 1 / 64 everywhere; v in {-1, 0, 1} and one-hot +-1 rows of dout make O, P and every dS
    dyadic numbers of the 16-bit type (checked here), so the fixed-point sum, the fold and dQ / dK / dV have one right answer:
    dlut bit for bit, which pins the indices, both clamps, the quantum and the fold.  K = 0 makes dQ identically zero, so the
    dS -> dQ product has no exact case (a uniform P needs K = 0 under a zero table): the tolerance cases alone hold it.  Lq != Lk
    is not run either: every case is self-attention in the trainer's packed layout."""
    r = np.random.Generator(np.random.PCG64([d, 64]))
    B, Lq = 2, 64
    q = r.integers(-4, 5, (B, HEADS, Lq, d)).astype(np.float64)
    v = r.integers(-1, 2, (B, HEADS, Lq, d)).astype(np.float64)
    dout = np.zeros((B, HEADS, Lq, d))
    np.put_along_axis(dout, r.integers(0, d, (B, HEADS, Lq, 1)), r.choice([-1.0, 1.0], (B, HEADS, Lq, 1)), -1)
    rq = torch.from_numpy(np.stack([np.broadcast_to(np.arange(Lq), (B, Lq)), r.integers(0, 12, (B, Lq)), r.integers(0, 12, (B, Lq))], -1).copy())
    c = dict(q=q, k=np.zeros_like(q), v=v, dout=dout, mask=np.zeros((B, Lq)), rq=rq, rk=rq, radii=(4, 3), scale=U.launcher_scale(d),
             lut=np.zeros((HEADS, 9 + 2 * 7)))
    ref = grads(c, dtype, True)
    t = ref["terms"]
    assert all(X.is16(t[n].numpy(), dtype) for n in ("p", "ds", "og")) and X.is16(ref["o"].numpy(), dtype)
    assert ref["dlut"].count_nonzero() > 12      # sums of dyadic dS times the launcher's fp32 scale: exact in float64 either way round
    got = run_kernel(c, dtype, ref["o"])
    assert same_bits(got["dlut"], ref["dlut"])
    assert same_bits(got["dk"], ref["dk"]) and same_bits(got["dv"], ref["dv"]) and ref["dk"].any() and ref["dv"].any()
    assert not got["dq"].any() and not ref["dq"].any()


def test_nan_in_dout_poisons_its_head_only():
    c, ref, _ = bound_case(torch.bfloat16, 17, 32)
    c = dict(c, dout=c["dout"].copy())
    c["dout"][1, 1, 5, 3] = np.nan
    got = run_kernel(c, torch.bfloat16, X._r(ref["o"], torch.bfloat16))["dlut"]
    assert torch.isnan(got[1]).all() and torch.isfinite(got[0]).all() and got[0].any()


@pytest.mark.parametrize("accumulate", [False, True], ids=["write", "accumulate"])
def test_lut_grad_sums_by_bucket(accumulate):
    """vk_relpos_lut_grad at LayoutLMv3's sizes: each term of dlut summed by bucket in float64, ascending, one rounding."""
    from vltk_amd.layoutlmv3 import relpos_bucket_map, relpos_lut_grad
    r1, r2, heads = 128, 256, 3
    n1, n2 = 2 * r1 + 1, 2 * r2 + 1
    g = torch.Generator().manual_seed(5)
    bucket, dlut = relpos_bucket_map(32, 64, r1, r2), torch.randn((heads, n1 + 2 * n2), generator=g)
    for term, (bins, off, n) in enumerate(((32, 0, n1), (64, n1, n2), (64, n1 + n2, n2))):
        prior = torch.randn((heads, bins), generator=g)
        s = torch.zeros((heads, bins), dtype=torch.float64)
        for e in range(n):
            s[:, bucket[off + e]] += dlut[:, off + e].double()
        got = relpos_lut_grad(dlut.cuda(), bucket.cuda(), r1, r2, term, prior.cuda(), accumulate)
        assert torch.equal(got.cpu(), (prior.double() * accumulate + s).float()), term
