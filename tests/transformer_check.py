"""The per-element checker of the attention, LayerNorm and linear-epilogue op tests: float64 references
computed from the STORED (already rounded) operands, and for every output element a bound derived from the kernels' rounding
points.  Nothing here needs a GPU; tests/test_transformer_check_host.py and tests/test_linear_check_host.py prove on the CPU that
correct arithmetic fits the bounds and that wrong arithmetic (a dropped key, swapped V rows, a wrong divisor, a tanh-approximation
GELU, the activation before the residual) does not.

Why not max|a - b| / max|b|: one large reference element (a one-hot row returns a whole V element, about 4) sets the scale for
rows that average a hundred keys (about 0.1), so a bf16 kernel may be 0.03 off on an output of 0.1 and still pass.
"""
import numpy as np
import torch

# Unit roundoff (half the spacing of 1.0's neighbours) of the storage types.  bf16 keeps 8 significant bits: 2^-8.
U = {torch.float32: 2.0 ** -24, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
U32 = 2.0 ** -24
NAMES = {torch.float32: "fp32", torch.float16: "fp16", torch.bfloat16: "bf16"}
ROUNDS_P = {"mfma": True, "tiled": True, "lds": False, "stream": False}     # the matrix-core kernels round P to the storage type


def _heads(t, B, Lx, heads, d):
    return t.detach().cpu().double().reshape(B, Lx, heads, d).transpose(1, 2)          # [B, heads, Lx, d]


def attention_reference(q, k, v, add, B, heads, Lq, Lk, d):
    """float64 soft-max(q k^T / sqrt(d) + add) v from the stored q [B*Lq, H], k, v [B*Lk, H] and the additive mask [B, Lk] (or
    None), heads side by side in a row.  Returns a dict: ref and A = p |v| as [B*Lq, H], S = max_j sum_c |q_rc k_jc| / sqrt(d) as
    [B*Lq, H] (a row's value repeated over its head's columns), sumv = sum_j |v_jc| likewise, and the geometry."""
    qh, kh, vh = _heads(q, B, Lq, heads, d), _heads(k, B, Lk, heads, d), _heads(v, B, Lk, heads, d)
    s = qh @ kh.transpose(-1, -2) / np.sqrt(float(d))
    if add is not None:
        s = s + add.detach().cpu().double()[:, None, None, :]
    p = torch.softmax(s, -1)
    S = (qh.abs() @ kh.abs().transpose(-1, -2)).amax(-1, keepdim=True) / np.sqrt(float(d))      # [B, heads, Lq, 1]
    sumv = vh.abs().sum(2, keepdim=True)                                                         # [B, heads, 1, d]

    def rows(t):
        return t.expand(B, heads, Lq, d).permute(0, 2, 1, 3).reshape(B * Lq, heads * d)
    return dict(ref=rows(p @ vh), A=rows(p @ vh.abs()), S=rows(S), sumv=rows(sumv), Lk=Lk, d=d)


def attention_bound(r, td, route):
    """Per element, with u the storage type's unit roundoff and u_P = u where the kernel rounds P (mfma, tiled), else 0:

        (u_P + u) A  +  (2 (d + 2) 2^-24 S_r + (Lk + 8) 2^-24) A      [ + 2^-25 (1 + u_P / u sum_j |v_j|) for fp16 ]

    First term: every p_j carries one relative rounding u_P, so the weighted sum moves by at most u_P sum_j p_j |v_j| = u_P A;
    the output is rounded once, u |out| <= u A.  Second term, all fp32: a score is a d-term dot product times the scale (any
    summation order: at most (d + 1) 2^-24 of sum_c |q k| / sqrt(d) <= S_r), the exponent's argument is a difference of two
    scores, and its error passes into p_j as a relative one: 2 (d + 2) 2^-24 S_r (the + 2 also covers the product with log2 e in
    front of v_exp_f32, whose argument is at most 2 S_r).  The exponential, the Lk-term sum, the division and the Lk-term second
    product add (Lk + 8) 2^-24, again relative to A.  fp16 has a subnormal spacing of 2^-24 that the relative terms do not see:
    half of it on the output and on each rounded p_j (times |v_j|)."""
    u = U[td]
    up = u if ROUNDS_P[route] else 0.0
    bound = (up + u) * r["A"] + (2 * (r["d"] + 2) * U32 * r["S"] + (r["Lk"] + 8) * U32) * r["A"]
    if td == torch.float16:
        bound = bound + 2.0 ** -25 * (1 + up / u * r["sumv"])
    return bound


def layernorm_reference(x, gamma, beta, eps, scale, y_old=None):
    """float64 (x_hat gamma + beta) scale (+ y_old) over the rows of the stored x [M, C] (a tensor of any dtype, or float64 already),
    population variance and eps as the kernel.  Returns a dict: ref, x_hat, rstd = 1 / sqrt(var + eps) and max_row|x| as [M, 1]."""
    x = x.detach().cpu().double()
    g, b = gamma.detach().cpu().double(), beta.detach().cpu().double()
    mu = x.mean(1, keepdim=True)
    var = ((x - mu) ** 2).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = (x - mu) * rstd
    ref = (xh * g + b) * scale
    if y_old is not None:
        ref = ref + y_old.detach().cpu().double()
    return dict(ref=ref, xh=xh, rstd=rstd, xmax=x.abs().amax(1, keepdim=True), gamma=g, scale=scale, C=x.shape[1])


def layernorm_bound(r, td):
    """Per element, with K = C / 64 + 16:

        u |ref|  +  K 2^-24 (|gamma| (max_row|x| / sqrt(var + eps) + |x_hat|) |scale| + |ref|)

    The first term is the one rounding of the output.  The second is the fp32 arithmetic: a lane sums C / 64 terms, six shuffle
    steps join the lanes, so the mean is off by at most about (C / 64 + 6) 2^-24 max|x|, which moves x_hat by that over sigma;
    the variance's relative error moves x_hat by a multiple of |x_hat|; sqrt, division, the affine map, the scale and the
    accumulate are a few more roundings of the running value, bounded by |ref| and the terms before it."""
    K = r["C"] / 64.0 + 16
    return U[td] * r["ref"].abs() + K * U32 * (r["gamma"].abs() * (r["xmax"] * r["rstd"] + r["xh"].abs()) * abs(r["scale"]) + r["ref"].abs())


# The device math library's allowance, in ulps of the result, for erff and tanhf (the one figure of linear_bound that is not derived:
# no accuracy statement for them ships with the toolchain).  Measured on an MI355X with torch.erf / torch.tanh in fp32 on the device
# against float64 on the host, over z on the 2^-7 grid of [-10, 10] (erf at z / sqrt(2)); E = twice the worst error seen, rounded
# up to a whole number, and at least 2.  Measured (tests/test_gpu_linear.py::test_math_library_allowance prints them and holds
# the constants to the rule): erf 1.163 ulp worst, tanh 0.929 ulp worst.
E_ERF = 3                                                   # ceil(2 * 1.163)
E_TANH = 2                                                  # ceil(2 * 0.929)
GELU_SLOPE = 1.13                                           # sup |GELU'|: 1.1289, at z = sqrt 2
SQRT2 = float(np.sqrt(2.0))


def linear_reference(x, w, bias, res, act, exact):
    """float64 act(x . w^T + bias + res) from the stored operands: x [M, K], w [N, K] (any dtype), bias [N], res [M, N] or None.
    act: 0 none | 1 ReLU | 2 GELU (erf form) | 3 tanh.  Returns a dict: ref, z (the pre-activation) and err_z, the bound on the
    kernel's own error in z: 0 where the data makes z exact (`exact`), else (K + 2) 2^-24 (sum_k |x_k w_k| + |bias| + |res|), a
    K-term fp32 sum in any order and the two additions.  The products run on the caller's device (a float64 GEMM); the result is
    on the CPU."""
    xd, wd = x.double(), w.to(x.device).double()
    b = bias.to(x.device).double()
    z = xd @ wd.t() + b
    if res is not None:
        z = z + res.to(x.device).double()
    if exact:
        err_z = torch.zeros((), dtype=torch.float64).expand(z.shape)
    else:
        S = xd.abs() @ wd.abs().t() + b.abs()
        if res is not None:
            S = S + res.to(x.device).double().abs()
        err_z = ((x.shape[1] + 2) * U32 * S).cpu()
    z = z.cpu()
    ref = {0: lambda t: t, 1: lambda t: t.clamp_min(0.0), 2: lambda t: 0.5 * t * torch.erfc(-t / SQRT2), 3: torch.tanh}[act](z)
    return dict(ref=ref, z=z, err_z=err_z, act=act)


def linear_bound(r, out_td):
    """Per element, with t = z / sqrt 2, e = erf(t), phi = (2 / sqrt pi) exp(-t^2), E the math library's allowance in ulps:

        none, ReLU   err_z
        tanh         E 2^-23 |ref| + err_z
        GELU         1/2 |z| (E 2^-23 |e| + 2 2^-24 |t| phi + 2^-24 |1 + e|) + 2^-24 |ref| + 1.13 err_z
        16-bit out   + u |ref|     [fp16: + 2^-25]

    GELU in the kernel is 0.5f * z * (1.0f + erff(z * 0.70710678f)): erff returns e within E ulps (2^-23 |e| each); its argument
    carries the rounding of the product and of the constant, 2 2^-24 |t| in all, which erf' = phi turns into 2 2^-24 |t| phi; the
    sum 1 + e is rounded once, 2^-24 |1 + e| (where erf has saturated it cancels to zero and only E 2^-23 is left: the planted
    tails); the factor 1/2 |z| carries these to the result, whose last product rounds once more, 2^-24 |ref| (0.5f * z is exact).
    err_z reaches the result through the slope: at most 1 for ReLU and tanh, 1.13 = sup |GELU'|.  The output type rounds once,
    u |ref|; fp16's subnormal spacing 2^-24 is invisible to that term: half of it.  An fp32 output has no storage term: the last
    fp32 operation IS the output."""
    z, ref, err_z = r["z"], r["ref"], r["err_z"]
    if r["act"] in (0, 1):
        bound = err_z.clone()
    elif r["act"] == 3:
        bound = E_TANH * 2.0 ** -23 * ref.abs() + err_z
    else:
        t = z / SQRT2
        e = torch.erf(t)
        phi = 2.0 / np.sqrt(np.pi) * torch.exp(-t * t)
        one_plus_e = torch.erfc(-t)
        bound = 0.5 * z.abs() * (E_ERF * 2.0 ** -23 * e.abs() + 2 * U32 * t.abs() * phi + U32 * one_plus_e) + U32 * ref.abs() + GELU_SLOPE * err_z
    if out_td != torch.float32:
        bound = bound + U[out_td] * ref.abs()
        if out_td == torch.float16:
            bound = bound + 2.0 ** -25
    return bound


def ulp_error(got32, want64):
    """Worst |got - want| in ulps of the fp32 result (the spacing of fp32 numbers at |want|; at least the smallest normal's):
    how E_ERF and E_TANH are measured."""
    want64 = want64.double()
    spacing = 2.0 ** (torch.floor(torch.log2(want64.abs().clamp_min(2.0 ** -126))) - 23)
    return float(((got32.double() - want64).abs() / spacing).max())


def worst_ratio(out, ref, bound):
    """(max over EVERY element of |out - ref| / bound, its index).  An element off a zero bound, or not finite, counts as inf."""
    o = out.detach().cpu().double()
    assert o.shape == ref.shape == bound.shape, (o.shape, ref.shape, bound.shape)
    err = (o - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, np.inf), torch.zeros_like(err)))
    ratio = torch.where(torch.isfinite(o), ratio, torch.full_like(err, np.inf))
    i = int(ratio.argmax())
    return float(ratio.flatten()[i]), tuple(int(n) for n in np.unravel_index(i, ratio.shape))


def assert_within(out, ref, bound, label):
    """Every element of `out` within `bound` of `ref`; prints and returns the worst ratio."""
    w, at = worst_ratio(out, ref, bound)
    print(f"\n[{label}] worst |out - ref| / bound {w:.3f} at {at}", end="")
    o = out.detach().cpu().double()
    assert w <= 1.0, f"{label}: |out - ref| / bound = {w:.3g} at {at}: out {float(o[at])!r} ref {float(ref[at])!r} bound {float(bound[at]):.3g}"
    return w
