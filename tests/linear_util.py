"""The cases and the data of the vk_linear epilogue tests (pure CPU; used by tests/test_linear_check_host.py and, with the device,
by tests/test_gpu_linear.py).  The checker itself -- linear_reference / linear_bound -- is in tests/transformer_check.py
(DESIGN.md section 20a).

DYADIC data makes the pre-activation z = x . w^T + bias + residual ONE fp32 number whichever kernel, K order or tile computes it
(the tests/exact_util.py argument, scaled): x is a multiple of 2^-3 in [-1, 1], w a multiple of 2^-s with an integer numerator in
[-8, 8], bias (fp32) and residual multiples of 2^-(3+s), the residual with at most 8 significant bits (exact in bf16).  Every
product and every partial sum in any order is then a multiple of 2^-(3+s) below 2^24 of that unit: exact.  s follows K so that
std(x . w) is 2 to 3 (s = 3, 3, 4, 5, 6 at K = 32, 64, 128, 768, 3072): the activations are tested where they bend.  What is left
to the kernel is the activation in fp32 and ONE rounding to the output type; with act 0 / 1 nothing but the rounding is left and
the test asks for the bits.

Planted elements (every dyadic case): z = 0 exactly at one row of column 0 through a small shift of that column's bias; z far in
both tails (|z| >= 9.5: fp32 tanh is exactly +-1, erf has long saturated and 1 + erf cancels) through two rows x = +-sign(w[column 1]), or,
for a single row, through the bias of two columns.

`check_conditions` asserts on the inputs, before any launch: the 2^24 bound on sum |x| |w| + |bias| + |res|; every operand exact in
its storage type; >= 20 % of z in [-4, -0.25] and >= 20 % in [0.25, 4]; >= 1 % with |z| >= 6; some z == 0; for tanh some
|z| >= 9.5.

FINE data is dyadic data with w's numerator in [-128, 128] over 2^-(s+4): the same spread and the same argument (K * 8 * 128 units
stay below 2^24, 8 bits are exact in bf16), but z now has more bits than fp16 keeps wherever the activations bend, so fp16's
rounding -- and a second rounding where there should be one -- shows.  A few launches per type.

RANDOM data is what the encoders see: x ~ N(0, 1) and w ~ N(0, 1 / K) rounded to the storage type, bias 0.1 N(0, 1), residual
N(0, 1); the bound then carries the pre-activation's own error term.
"""
import dataclasses
import zlib

import numpy as np
import torch

F32, F16, BF16 = 0, 1, 4                                   # vk_dtype values (include/vltk_hip.h)
TORCH_DT = {F32: torch.float32, F16: torch.float16, BF16: torch.bfloat16}
DT_NAMES = {F32: "fp32", F16: "fp16", BF16: "bf16"}
ACT_NAMES = ("none", "relu", "gelu", "tanh")
LIMIT = float(1 << 24)
DTYPES = (F32, F16, BF16)


@dataclasses.dataclass(frozen=True)
class Case:
    """One vk_linear launch: y[M, N] = act(x[M, K] . w[N, K]^T + bias + res), on `data` ("dyadic" | "fine" | "random"); route: the kernel
    it must run on."""
    route: str
    M: int
    K: int
    N: int
    act: int
    res: bool
    dt: int
    out_dt: int = -1
    data: str = "dyadic"

    @property
    def odt(self):
        return self.dt if self.out_dt < 0 else self.out_dt

    @property
    def name(self):
        return (f"{self.data}-{DT_NAMES[self.dt]}{'-f32out' if self.odt != self.dt else ''}-M{self.M}-K{self.K}-N{self.N}-"
                f"{ACT_NAMES[self.act]}{'-res' if self.res else ''}")

    @property
    def seed_name(self):                                    # the data depends on the layer, not on the row count or the type
        return f"{self.data}-K{self.K}-N{self.N}-{self.act}-{int(self.res)}"

    def route_geometry(self):
        """Arguments of gpu_util.conv_route for this launch."""
        return dict(N=1, H=1, W=self.M, cin=self.K, cout=self.N, relu=self.act, res=self.res, dt=self.dt, out_dt=self.odt)


def ktile(dt):
    """Elements in one 128-byte K-tile of the generic kernel."""
    return 32 if dt == F32 else 64


# ---- the tables ---------------------------------------------------------------------------------------------------------------
GENERIC_N = (2, 5, 7, 64, 72, 128, 136, 384)                # narrow and 128-wide column tile, cout8 < tile, pads (2, 5, 7)
GENERIC_M = (127, 128, 129, 300)                            # the row tile is 128; M = 1 has its own rows below


def generic_cases(dt, act):
    """The designed table of one (dtype, activation): eight launches, one per N, and a single-row launch.  Over the eight, M walks
    {127, 128, 129, 300}, K alternates between one K-tile and 768, the residual is there in four and, in the 16-bit types, the
    output is fp32 in three or four (i + act a multiple of 3, or the single row of act 2 / 3).  Shifting the walk by `act` gives
    every value of M, N and K with every activation."""
    out = []
    for i, N in enumerate(GENERIC_N):
        M = GENERIC_M[(i + act) % 4]
        K = ktile(dt) if (i + act) % 2 == 0 else 768
        f32out = dt != F32 and (i + act) % 3 == 0
        out.append(Case("generic", M, K, N, act, (i // 2) % 2 == 1, dt, F32 if f32out else -1))
    out.append(Case("generic", 1, 768 if act % 2 else ktile(dt), 384, act, act >= 2, dt, F32 if dt != F32 and act >= 2 else -1))
    return out


# (M, K, N, act, res) of the two-per-CU kernel's launches: M over the 128-row tile (a whole number, one row more, one row less,
# 20.3 tiles), N one and three column tiles, K from the two-stage minimum to the FFN's 3072
DUO_BF16 = ((1024, 64, 256, 0, False), (1025, 128, 768, 1, False), (1151, 768, 256, 2, False), (2600, 3072, 768, 0, True),
            (1024, 768, 768, 1, True), (1025, 3072, 256, 2, True), (1151, 64, 768, 2, False), (2600, 128, 256, 2, True))
DUO_F16 = ((1024, 768, 256, 0, False), (1025, 3072, 768, 1, True), (1151, 768, 768, 0, True), (2600, 3072, 256, 1, False),
           (1151, 64, 768, 1, True), (2600, 128, 768, 0, False))     # f16, K <= 512, N = 256 is the weight-stationary kernel's
# the same geometry where the two-per-CU kernel has no epilogue for it: the generic kernel must take the launch, and be right
DUO_FALLBACK = (Case("generic", 1151, 768, 256, 2, True, F16), Case("generic", 1151, 768, 256, 3, True, BF16),
                Case("generic", 1151, 768, 256, 2, True, BF16, F32))


def duo_cases(dt):
    return [Case("duo", M, K, N, act, res, dt) for M, K, N, act, res in (DUO_BF16 if dt == BF16 else DUO_F16)]


def random_cases(dt):
    """Two generic and two two-per-CU launches on N(0, 1) data; the last two are the encoders' feed-forward pair at a benchmark
    batch's row count.  fp32 has no two-per-CU build: all four run on the generic kernel."""
    big = "generic" if dt == F32 else "duo"
    gelu = big if dt != F16 else "generic"                  # the GELU epilogue is in the bf16 build only
    return [Case("generic", 300, 768, 136, 2, True, dt, data="random"), Case("generic", 129, 768, 384, 3, False, dt, data="random"),
            Case(gelu, 2600, 768, 3072, 2, False, dt, data="random"), Case(big, 2600, 3072, 768, 0, True, dt, data="random")]


def fine_cases(dt):
    """Every activation on the generic kernel at K = 768 (z a multiple of 2^-12), and the two-per-CU kernel's epilogues."""
    out = [Case("generic", 300, 768, 136, act, act % 2 == 1, dt, data="fine") for act in range(4)]
    if dt == BF16:
        out += [Case("duo", 1151, 768, 256, 2, True, dt, data="fine"), Case("duo", 1151, 768, 256, 1, False, dt, data="fine")]
    if dt == F16:
        out += [Case("generic", 1151, 768, 256, 2, True, dt, data="fine"), Case("duo", 1151, 768, 256, 1, False, dt, data="fine")]
    return out


def all_cases():
    for dt in DTYPES:
        for act in range(4):
            yield from generic_cases(dt, act)
        if dt != F32:
            yield from duo_cases(dt)
        yield from fine_cases(dt)
        yield from random_cases(dt)
    yield from DUO_FALLBACK


# ---- data -----------------------------------------------------------------------------------------------------------------------
def scale_exp(K, data="dyadic"):
    """s: x . w has variance K * (3 / 8) * 24 * 4^-s = 9 K 4^-s; the nearest s to a variance of 6.  Fine data: four bits more."""
    return int(round(0.5 * np.log2(1.5 * K))) + (4 if data == "fine" else 0)


def make_inputs(c: Case, rows=None):
    """x [M, K], w [N, K], bias [N] (fp32), res [M, N] or None as CPU tensors in their storage types.  w and bias depend on the
    layer alone and are drawn first (column 0's bias is then shifted by the planted zero); `rows`: the same layer on at most that
    many rows, what the CPU suite can hold (tests/test_linear_check_host.py)."""
    M = c.M if rows is None else min(rows, c.M)
    td = TORCH_DT[c.dt]
    gen = np.random.Generator(np.random.PCG64(zlib.crc32(c.seed_name.encode())))
    if c.data == "random":
        w = torch.from_numpy((gen.standard_normal((c.N, c.K)) * (1.0 / c.K) ** 0.5).astype(np.float32)).to(td)
        bias = torch.from_numpy((gen.standard_normal(c.N) * 0.1).astype(np.float32))
        x = torch.from_numpy(gen.standard_normal((M, c.K)).astype(np.float32)).to(td)
        res = torch.from_numpy(gen.standard_normal((M, c.N)).astype(np.float32)).to(td) if c.res else None
        return x, w, bias, res
    s = scale_exp(c.K, c.data)
    unit = 2.0 ** -(3 + s)
    top = 128 if c.data == "fine" else 8
    w = gen.integers(-top, top + 1, (c.N, c.K)).astype(np.float64) * 2.0 ** -s
    if c.N >= 64:
        bias = gen.integers(-int(3 / unit), int(3 / unit) + 1, c.N).astype(np.float64) * unit
    else:                                                   # a few columns: +-2.5 in turn (0 for the odd one out) and a jitter, so that
        level = np.where(np.arange(c.N) % 2 == 0, 2.5, -2.5) * (np.arange(c.N) < c.N // 2 * 2)      # both bends and both tails are met
        bias = level + gen.integers(-int(0.5 / unit), int(0.5 / unit) + 1, c.N).astype(np.float64) * unit
    x = gen.integers(-8, 9, (M, c.K)).astype(np.float64) * 0.125
    # the residual: an 8-bit numerator times a power of two that is a multiple of the unit, within about +-2
    res = gen.integers(-255, 256, (M, c.N)).astype(np.float64) * max(unit, 2.0 ** -7) if c.res else None
    r0 = (lambda m, n: res[m, n] if c.res else 0.0)
    c1 = 1 % c.N
    if M >= 3:                                              # both tails through two rows: x = +-sign(w[c1]) gives +-sum |w[c1]|
        x[1] = np.sign(w[c1])
        x[2] = -x[1]
        if c.res:
            res[1, c1], res[2, c1] = 0.5, -0.5
    else:                                                   # a single row: through the bias of columns 1 and 2
        assert c.N >= 3
        bias[1] = 10.0 - (x[0] @ w[1] + r0(0, 1))
        bias[2] = -10.0 - (x[0] @ w[2] + r0(0, 2))
    # z = 0 exactly in column 0, at the row (of the first hundred, past the planted ones) where it is nearest already: the shift
    # of that column's bias is small
    rows0 = np.arange(3, min(M, 100)) if M >= 3 else np.arange(1)
    z0 = x[rows0] @ w[0] + bias[0] + (res[rows0, 0] if c.res else 0.0)
    bias[0] -= z0[np.argmin(np.abs(z0))]
    t = lambda a, d: torch.from_numpy(a.astype(np.float32)).to(d)              # noqa: E731
    return t(x, td), t(w, td), t(bias, torch.float32), (t(res, td) if c.res else None)


def check_conditions(c: Case, x, w, bias, res, z=None):
    """The conditions of the module text on a dyadic case's stored operands (z: their float64 pre-activation, when the caller
    has it).  Returns the fractions (negative bend, positive bend, saturated)."""
    assert c.data in ("dyadic", "fine")
    s = scale_exp(c.K, c.data)
    unit = 2.0 ** -(3 + s)
    top = 128 if c.data == "fine" else 8
    xd, wd, bd = x.double(), w.double(), bias.double()
    rd = res.double() if res is not None else torch.zeros((), dtype=torch.float64)
    # exactly representable: the stored operands are the designed multiples, in range
    assert bool((xd * 8 == (xd * 8).round()).all()) and float(xd.abs().max()) <= 1.0, c.name
    assert bool((wd * 2.0 ** s == (wd * 2.0 ** s).round()).all()) and float(wd.abs().max()) <= top * 2.0 ** -s, c.name
    assert bool((bd / unit == (bd / unit).round()).all()), c.name
    assert bias.dtype == torch.float32 and x.dtype == w.dtype == TORCH_DT[c.dt]
    if res is not None:
        assert res.dtype == TORCH_DT[c.dt] and bool((rd / unit == (rd / unit).round()).all()), c.name
        assert bool((rd.to(torch.bfloat16).double() == rd).all()), f"{c.name}: a residual with more than 8 significant bits"
    total = float((xd.abs() @ wd.abs().t() + bd.abs() + rd.abs()).max())
    assert total / unit < LIMIT, f"{c.name}: sum |x||w| + |bias| + |res| reaches {total / unit:.3e} units >= 2^24"
    if z is None:
        z = xd @ wd.t() + bd + rd
    z = z.detach().cpu().double()
    assert bool((z / unit == (z / unit).round()).all())
    assert bool((z.float().double() == z).all()), f"{c.name}: z is not an fp32 number"
    neg = float(((z >= -4) & (z <= -0.25)).double().mean())
    pos = float(((z >= 0.25) & (z <= 4)).double().mean())
    sat = float((z.abs() >= 6).double().mean())
    assert neg >= 0.20, f"{c.name}: only {neg:.1%} of z in [-4, -0.25]"
    assert pos >= 0.20, f"{c.name}: only {pos:.1%} of z in [0.25, 4]"
    assert sat >= 0.01, f"{c.name}: only {sat:.2%} of z with |z| >= 6"
    assert bool((z == 0).any()), f"{c.name}: no z == 0"
    if c.act == 3:
        assert bool((z.abs() >= 9.5).any()), f"{c.name}: no |z| >= 9.5"
    assert bool((z >= 6).any()) and bool((z <= -6).any()), f"{c.name}: a tail is missing"
    return neg, pos, sat


# ---- the kernels' arithmetic restated in torch fp32 (what the bound is derived for), and its mutants --------------------------
def gelu_erf32(z):
    return 0.5 * z * (1.0 + torch.erf(z * np.float32(0.70710678118654752)))


def gelu_tanh32(z):
    return 0.5 * z * (1.0 + torch.tanh(np.float32(0.7978845608028654) * (z + np.float32(0.044715) * z * z * z)))


def restate(c: Case, x, w, bias, res, mutant=None):
    """fp32 sum of the stored operands, + bias + residual, the activation in fp32, one rounding to the output type.  mutant:
    None | "gelu_tanh" | "act_before_res" | "round_z" | "neighbour_bias" | "erf_no_sqrt2"."""
    td, od = TORCH_DT[c.dt], TORCH_DT[c.odt]
    b = bias.roll(1) if mutant == "neighbour_bias" else bias
    z = x.float() @ w.float().t() + b
    r = res.float() if res is not None else None
    if r is not None and mutant != "act_before_res":
        z = z + r
    if mutant == "round_z":
        z = z.to(td).float()
    if c.act == 1:
        z = z.clamp_min(0.0)
    elif c.act == 2:
        if mutant == "gelu_tanh":
            z = gelu_tanh32(z)
        elif mutant == "erf_no_sqrt2":
            z = 0.5 * z * (1.0 + torch.erf(z))
        else:
            z = gelu_erf32(z)
    elif c.act == 3:
        z = torch.tanh(z)
    if r is not None and mutant == "act_before_res":
        z = z + r
    return z.to(od)
