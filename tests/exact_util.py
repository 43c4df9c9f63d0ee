"""Exact-integer data for the convolution kernels (pure CPU; used by tests/test_conv_exact_host.py and, with the device
reference, by tests/test_gpu_conv_exact.py).

Activations are integers in [0, 15], weights integers in [-8, 8] (packed through the bias path: no BN scale), the bias an
integer per channel from widely spaced levels plus a jitter, the residual integers in [-64, 64].  Every product and every
partial sum in any order is then an integer below 2^24, exact in fp32 whichever MFMA, K order, tile shape or wave split a
kernel uses, so the one correct output is the float64 result rounded ONCE to the storage type (round to nearest even):
there is no tolerance.  The bias levels put each channel's outputs into a different f16 binade (ulp 1 ... 32), so the
rounding is exercised whatever K is.

`check_conditions` asserts, on the inputs and before anything is launched:
  (i)   max conv(|x|, |w|) + max |bias| + max |res| < 2^24;
  (ii)  f16 / bf16 storage: >= 20 % of the expected outputs differ from their float64 value and >= 3 % are exact ties
        (not asked of the three edge cases);
  (iii) no expected output is inf or NaN unless the case is the overflow case.
"""
import dataclasses
import zlib

import torch
import torch.nn.functional as F

F32, F16, BF16 = 0, 1, 4                                   # vk_dtype values (include/vltk_hip.h)
TORCH_DT = {F32: torch.float32, F16: torch.float16, BF16: torch.bfloat16}
LIMIT = float(1 << 24)
BIAS_LEVELS = (0, 1500, -1500, 3000, -3000, 6000, -6000, 12000, -12000, 24000, -24000, 40000, -40000)
EDGES = (None, "overflow", "subnormal", "spike")


@dataclasses.dataclass(frozen=True)
class Case:
    """One launch on integer data.  kind: conv (vk_conv2d) | dual (vk_conv1x1_dual: N = H = 1, W = M, cin | cin2) |
    mean (vk_conv1x1_meanpool: N images of 1 x W) | linear (vk_linear: N = H = 1, W = M, cin = K).  env: the A/B switches the
    launch runs under; route: the kernel it must then run on."""
    name: str
    route: str
    kind: str = "conv"
    N: int = 1
    H: int = 1
    W: int = 1
    cin: int = 64
    cout: int = 64
    k: int = 1
    stride: int = 1
    pad: int = 0
    dil: int = 1
    groups: int = 1
    cin2: int = 0
    res: bool = False
    relu: int = 0
    dt: int = F16
    out_dt: int = -1
    env: tuple = ()
    edge: str = None
    seed_name: str = ""                                     # cases that must share data share this

    @property
    def odt(self):
        return self.dt if self.out_dt < 0 else self.out_dt

    @property
    def out_hw(self):
        e = self.dil * (self.k - 1) + 1
        return (self.H + 2 * self.pad - e) // self.stride + 1, (self.W + 2 * self.pad - e) // self.stride + 1

    @property
    def M(self):
        ho, wo = self.out_hw
        return self.N * ho * wo

    def route_geometry(self):
        """Arguments of gpu_util.conv_route for this launch."""
        return dict(N=self.N, H=self.H, W=self.W, cin=self.cin, cout=self.cout, k=self.k, stride=self.stride, pad=self.pad,
                    dil=self.dil, groups=self.groups, relu=self.relu, dt=self.dt, out_dt=self.odt, cin2=self.cin2, res=self.res,
                    mean=self.kind == "mean")


def make_inputs(c: Case, device="cpu"):
    """x [N, cin (+ cin2), H, W], w [cout, (cin + cin2) / groups, k, k], bias [cout], res [N, cout, Ho, Wo] or None: float64
    tensors holding the integers (the edge cases: scaled / spiked as the module text says).  w and bias are drawn first, on
    the CPU: they depend on the layer alone, not on how many rows it is run on; x and res are drawn on `device`."""
    seed = zlib.crc32((c.seed_name or c.name).encode())
    g = torch.Generator().manual_seed(seed)
    gd = g if device == "cpu" else torch.Generator(device=device).manual_seed(seed)
    K = c.cin + c.cin2
    ri = lambda lo, hi, shape, gen=g, dev="cpu": torch.randint(lo, hi + 1, shape, generator=gen, device=dev,      # noqa: E731
                                                               dtype=torch.int16).double()
    ho, wo = c.out_hw
    w = ri(-8, 8, (c.cout, K // c.groups, c.k, c.k))
    lv = torch.tensor(BIAS_LEVELS, dtype=torch.float64)
    if c.relu:                                              # a ReLU would clamp the negative half to one value: mostly positive levels
        lv = torch.cat([lv[lv >= 0], lv[lv >= 0], lv])
    bias = lv[torch.randint(0, len(lv), (c.cout,), generator=g)] + ri(-40, 40, (c.cout,))
    x = ri(0, 3 if c.edge == "spike" else 15, (c.N, K, c.H, c.W), gd, device)
    res = ri(-64, 64, (c.N, c.cout, ho, wo), gd, device) if c.res else None
    if c.edge == "overflow":
        bias[1::16] = 70000.0
        bias[2::16] = -70000.0
    elif c.edge == "subnormal":                             # outputs are integers x 2^-24: many of them f16 subnormals
        x, w, bias, res = x * 2.0 ** -12, w * 2.0 ** -12, bias * 0.0, None if res is None else res * 0.0
    elif c.edge == "spike":                                 # one activation three orders above the rest
        x[c.N // 2, (c.cin // 2) % K, c.H // 2, c.W // 2] = 2047.0
    return x, w, bias, res


def host_subset(c: Case, rows=3000):
    """The same layer on at most about `rows` output rows (fewer images, or a shorter row list): what the CPU suite can hold;
    make_inputs gives it the full case's weights and bias."""
    ho, wo = c.out_hw
    if c.N * ho * wo <= rows:
        return c
    if c.N == 1 and c.H == 1 and c.k == 1:
        return dataclasses.replace(c, W=rows * c.stride, seed_name=c.seed_name or c.name)
    return dataclasses.replace(c, N=max(1, rows // (ho * wo)), seed_name=c.seed_name or c.name)


def conv64(x, w, c: Case):
    """The convolution in float64 (exact on this data) on x's device: a GEMM for 1x1, else F.conv2d on the CPU and GEMMs over
    im2col columns, a few images at a time, on a GPU."""
    w = w.to(x.device)
    if c.k == 1 and c.groups == 1:
        xs = x[:, :, ::c.stride, ::c.stride]
        n, k, h, ww = xs.shape
        return (xs.permute(0, 2, 3, 1).reshape(-1, k) @ w[:, :, 0, 0].t()).view(n, h, ww, -1).permute(0, 3, 1, 2)
    if x.device.type == "cpu":
        return F.conv2d(x, w, None, c.stride, c.pad, c.dil, c.groups)
    ho, wo = c.out_hw
    cg, og = x.shape[1] // c.groups, c.cout // c.groups
    step = max(1, (1 << 27) // (cg * c.k * c.k * ho * wo))
    out = torch.empty((x.shape[0], c.cout, ho * wo), dtype=torch.float64, device=x.device)
    for n0 in range(0, x.shape[0], step):
        for gi in range(c.groups):
            cols = F.unfold(x[n0:n0 + step, gi * cg:(gi + 1) * cg], c.k, c.dil, c.pad, c.stride)       # [n, cg*k*k, L]
            out[n0:n0 + step, gi * og:(gi + 1) * og] = torch.matmul(w[gi * og:(gi + 1) * og].reshape(og, -1), cols)
    return out.view(x.shape[0], c.cout, ho, wo)


def expected(c: Case, x, w, bias, res):
    """(float64 value, the same rounded once to the storage type) of the launch's output: [N, cout, Ho, Wo], for `mean` cases
    the float32 [N, cout] means of the f16-rounded outputs."""
    v = conv64(x, w, c) + bias.to(x.device).view(1, -1, 1, 1)
    if res is not None:
        v = v + res
    if c.relu:
        v = v.clamp_min_(0.0)
    y = v.to(TORCH_DT[c.odt])
    if c.kind == "mean":
        ho, wo = c.out_hw
        s = y.double().sum(dim=(2, 3))
        return v, (s / float(ho * wo)).float()
    return v, y


def rounding_stats(v, y):
    """Fractions of outputs that the storage type rounded, and of exact ties (the float64 value lies half way between the
    stored value and its neighbour on the other side)."""
    y64 = y.double()
    rounded = (y64 != v) & torch.isfinite(y64)
    if y.dtype == torch.float32:
        return float(rounded.float().mean()), 0.0
    bits = y.view(torch.int16).to(torch.int64) & 0xFFFF                     # sign-magnitude: the neighbours are bits +- 1
    mag, pos = bits & 0x7FFF, (bits >> 15) == 0
    up = torch.where(pos, bits + 1, torch.where(mag == 0, torch.ones_like(bits), bits - 1))
    dn = torch.where(pos & (mag > 0), bits - 1, torch.where(mag == 0, torch.full_like(bits, 0x8001), bits + 1))
    other = torch.where(v > y64, up, dn)
    other = ((other + 0x8000) % 0x10000 - 0x8000).to(torch.int16).view(y.dtype).double()
    tie = rounded & ((other - v).abs() == (y64 - v).abs())
    return float(rounded.float().mean()), float(tie.float().mean())


def check_conditions(c: Case, x, w, bias, res, v, y, bound=None):
    """Conditions (i) - (iii) of the module text; `bound`: max conv(|x|, |w|) when the caller computed it (else the cheap upper
    bound max|x| * sum over the longest weight row)."""
    scale = 2.0 ** 24 if c.edge == "subnormal" else 1.0                      # the scaled case: integers x 2^-24
    if bound is None:
        rowsum, top = float(w.abs().flatten(1).sum(dim=1).max()), float(x.abs().max())     # (grouped: a row is one group's taps)
        bound = top * rowsum
        if c.edge == "spike":                               # one large activation: it meets one weight per output
            assert int((x > 3).sum()) == 1
            bound = 3.0 * rowsum + top * float(w.abs().max())
    total = bound * scale + float(bias.abs().max()) + (float(res.abs().max()) if res is not None else 0.0)
    assert total < LIMIT, f"{c.name}: |x|.|w| + |bias| + |res| can reach {total:.3e} >= 2^24"
    ys = y if c.kind != "mean" else v.to(torch.float16)
    step = max(1, v.numel() >> 25)                          # the statistic on every step-th output of a very large tensor
    stats = rounding_stats(v.flatten()[::step], ys.flatten()[::step])
    if c.edge is None and c.odt != F32:
        assert stats[0] >= 0.20, f"{c.name}: only {stats[0]:.1%} of the expected outputs are rounded"
        assert stats[1] >= 0.03, f"{c.name}: only {stats[1]:.1%} of the expected outputs are ties"
    if c.edge != "overflow":
        assert bool(torch.isfinite(y.double()).all()), f"{c.name}: non-finite expected output"
    else:
        assert bool(torch.isinf(y.double()).any()), f"{c.name}: the overflow case does not overflow"
    assert not bool(torch.isnan(y.double()).any())
    return total, stats


# ---- vk_bottleneck64: three chained layers, a round to f16 after each ------------------------------------------------------
# The two intermediates must be rounded too, or the test says nothing about them: x in [0, 3]; w1 in [-1, 1] with bias levels
# {0, 0, 1000, 2500}; w2 / w3 in {-1, 0, 1} with 8 % non-zero and levels {0, 1500, 3000, -2000} / {0, +-1500, +-6000, 20000};
# projection weights in [-4, 4]; every bias + a jitter in [-20, 20].  The levels go round the channels in turn, so every case
# has the same share of each binade.
# The three edge cases, once: overflow (b3 +-70000 on a few channels: +inf, and 0 behind the ReLU); subnormal (x, w1 and the
# projection weights scaled by 2^-12, no bias: t1, t2 and the shortcut are integers x 2^-24, f16 subnormals that the next layer's
# MFMA reads as operands); spike (one x = 2047 in a block without biases).
def make_bneck(proj, N, H, W, seed=0, edge=None):
    g = torch.Generator().manual_seed(1000 + seed + int(proj))
    cin = 64 if proj else 256
    ri = lambda lo, hi, shape: torch.randint(lo, hi + 1, shape, generator=g).double()       # noqa: E731
    sparse = lambda shape: torch.where(torch.rand(shape, generator=g) < 0.08, ri(0, 1, shape) * 2 - 1, torch.zeros(shape).double())  # noqa: E731
    lev = lambda levels, n: torch.tensor(levels, dtype=torch.float64).repeat(n // len(levels) + 1)[:n] + ri(-20, 20, (n,))          # noqa: E731
    p = {"x": ri(0, 3, (N, cin, H, W)), "w1": ri(-1, 1, (64, cin, 1, 1)), "b1": lev((0, 0, 1000, 2500), 64),
         "w2": sparse((64, 64, 3, 3)), "b2": lev((0, 1500, 3000, -2000), 64),
         "w3": sparse((256, 64, 1, 1)), "b3": lev((0, 1500, -1500, 6000, -6000, 20000), 256)}
    if proj:
        p["wsc"] = ri(-4, 4, (256, cin, 1, 1))
    if edge == "overflow":
        p["b3"][1::16] = 70000.0
        p["b3"][2::16] = -70000.0
    elif edge == "subnormal":
        for k in ("x", "w1", "wsc"):
            if k in p:
                p[k] = p[k] * 2.0 ** -12
        for k in ("b1", "b2", "b3"):
            p[k] = p[k] * 0.0
    elif edge == "spike":                                   # (no bias: the rest of every map stays three orders below the spike's trace)
        p["x"][N // 2, cin // 2, H // 2, W // 2] = 2047.0
        for k in ("b1", "b2", "b3"):
            p[k] = p[k] * 0.0
    return p


def bneck_expected(p, proj):
    """[(float64 value, its f16 rounding)] of t1, t2 and y: each layer in float64 on the ROUNDED output of the one before, as
    include/vltk_hip.h documents for vk_bottleneck64; and the largest sum of magnitudes a layer can reach (condition (i))."""
    h = lambda t: t.to(torch.float16)                       # noqa: E731
    v1 = (F.conv2d(p["x"], p["w1"]) + p["b1"].view(1, -1, 1, 1)).clamp_min(0.0)
    t1 = h(v1)
    v2 = (F.conv2d(t1.double(), p["w2"], padding=1) + p["b2"].view(1, -1, 1, 1)).clamp_min(0.0)
    t2 = h(v2)
    v3 = F.conv2d(t2.double(), p["w3"]) + p["b3"].view(1, -1, 1, 1)
    v3 = v3 + (F.conv2d(p["x"], p["wsc"]) if proj else p["x"])
    v3 = v3.clamp_min(0.0)
    bounds = [float(F.conv2d(p["x"], p["w1"].abs()).max() + p["b1"].abs().max()),
              float(F.conv2d(t1.double(), p["w2"].abs(), padding=1).max() + p["b2"].abs().max()),
              float((F.conv2d(t2.double(), p["w3"].abs()) + (F.conv2d(p["x"], p["wsc"].abs()) if proj else p["x"])).max()
                    + p["b3"].abs().max())]
    return [(v1, t1), (v2, t2), (v3, h(v3))], bounds


def check_bneck_conditions(layers, bounds, edge=None):
    """(i) per layer on the actual rounded intermediates; (ii) on each of the three roundings, 10 % in place of 20 % (not asked of
    the edge cases); (iii).  The subnormal case must have subnormal values in both intermediates and in the output."""
    stats = []
    for i, ((v, y), b) in enumerate(zip(layers, bounds)):
        assert b * (2.0 ** 24 if edge == "subnormal" else 1.0) < LIMIT, b
        if edge == "overflow" and i == 2:
            assert bool(torch.isinf(y.double()).any()) and not bool(torch.isnan(y.double()).any())
        else:
            assert bool(torch.isfinite(y.double()).all())
        r, t = rounding_stats(v, y)
        if edge is None:
            assert r >= 0.10 and t >= 0.03, (r, t)
        if edge == "subnormal":
            a = y.double().abs()
            assert float(((a > 0) & (a < 2.0 ** -14)).float().mean()) >= 0.05, i
        stats.append((r, t))
    return stats


# ---- vk_stem: 7x7 stride-2 convolution + BN + ReLU + max-pool on integer pixels -------------------------------------------------
# pixels 0..255, weights in [-4, 4]; BN as gamma = 1, beta = an integer level, mean = 0, var = 1 - 1e-5: the fold scale
# 1 / sqrt(var + 1e-5) is 1 to within 1e-8, far inside half an ulp of a small integer, so the packed weights ARE the integers.
# The three edge cases, once: overflow (beta +-70000: +inf, and 0 behind the ReLU, through the pool); subnormal (pixels 0..15 and
# the weights scaled by 2^-12, beta 0: outputs are integers x 2^-24); spike (pixels 0..3 and one of 2047).  vk_stem takes the
# pixels as f32 and rounds them to f16 itself: every value here is exact in f16.
def make_stem(N, H, W, seed=0, edge=None):
    g = torch.Generator().manual_seed(2000 + seed)
    top = {None: 255, "overflow": 255, "subnormal": 15, "spike": 3}[edge]
    x = torch.randint(0, top + 1, (N, 3, H, W), generator=g).double()
    w = torch.randint(-4, 5, (64, 3, 7, 7), generator=g).double()
    beta = torch.tensor(BIAS_LEVELS[:9], dtype=torch.float64).repeat(8)[:64] + torch.randint(-40, 41, (64,), generator=g).double()
    if edge == "overflow":
        beta[1::16] = 70000.0
        beta[2::16] = -70000.0
    elif edge == "subnormal":
        x, w, beta = x * 2.0 ** -12, w * 2.0 ** -12, beta * 0.0
    elif edge == "spike":
        x[N // 2, 1, H // 2, W // 2] = 2047.0
    return x, w, beta


def stem_expected(x, w, beta, caffe):
    """(float64 conv + beta after the ReLU, its f16 rounding, the pooled f16 result): the max-pool of f16 values is exact."""
    v = (F.conv2d(x, w, None, 2, 3) + beta.view(1, -1, 1, 1)).clamp_min(0.0)
    y = v.to(torch.float16)
    pooled = F.max_pool2d(y.float(), 3, 2, 0, ceil_mode=True) if caffe else F.max_pool2d(y.float(), 3, 2, 1)
    return v, y, pooled.to(torch.float16)
