"""TEST INFRASTRUCTURE ONLY -- the case tables of the training kernels' tests at the trainer's extents (test_gpu_train_extents.py,
test_gpu_nan_surroundings.py, test_gpu_ce_infinite.py) and their CPU halves, so that tests/test_train_extents_host.py can assert
every table's exactness preconditions without a GPU.  Nothing here touches a GPU, and nothing here is the code under test.

GEMM data are integers in [-8, 8]: every product is an integer of at most 64, so a sum of K of them (and a bias and an old C of at
most 8 each) is an integer below 64 K + 16 <= 262 352 < 2^24 and exact in fp32 in any order; the float64 BLAS product is exact
for the same reason and is the reference."""
import functools

import numpy as np
import torch

import lxmert_pretrain_util as P
import train_util as U

# ---- A. GEMM extents -----------------------------------------------------------------------------------------------------------------
FORMS32 = {"NT": (0, 1), "NN": (0, 0), "TN": (1, 0), "TT": (1, 1)}
LONG_K = [(65, 130, 4099), (33, 65, 2051)]                # K is no multiple of 16, 32 or 64; 65 and 129 K steps
LARGE_LONG_K = (1400, 1500, 2051)                         # 11 x 12 tiles of 128: the large tile on any device of up to 264 CUs
# the trainer's calls at BERT-base width, B Lx = 896 rows, dense leading dimensions: (form, (M, N, K), bias)
TRAINER_CALLS = ([("NT", s, True) for s in ((896, 2304, 768), (896, 3072, 768), (896, 768, 3072))] +
                 [("NN", s, False) for s in ((896, 768, 2304), (896, 768, 3072), (896, 3072, 768))] +
                 [("TN", s, False) for s in ((2304, 768, 896), (3072, 768, 896), (768, 3072, 896))])
COL_SUMS = [(4099, 768), (4099, 3072)]                    # 17 slices of 256 rows


def large_tile_rule(M, N, cus):
    """The launchers' rule (csrc/train.hip, csrc/gemm16.hip): the 128 x 128 tile where such tiles fill at least half the CUs."""
    return 2 * (-(-M // 128)) * (-(-N // 128)) >= cus


@functools.lru_cache(maxsize=4)
def gemm_case(M, N, K, seed, one_hot=False):
    """-> op(A) [M, K], op(B) [K, N], bias [N], C0 [M, N] (integers in [-8, 8] as float64; one_hot: one +-1 per row of op(A), so
    that the product is a row of op(B), a number of either 16-bit type) and the exact product op(A) op(B) by float64 BLAS."""
    r = np.random.Generator(np.random.PCG64([M, N, K, seed]))
    b = r.integers(-8, 9, (K, N)).astype(np.float64)
    if one_hot:
        a = np.zeros((M, K))
        a[np.arange(M), r.integers(0, K, M)] = r.choice([-1.0, 1.0], M)
    else:
        a = r.integers(-8, 9, (M, K)).astype(np.float64)
    bias, c0 = r.integers(-8, 9, N).astype(np.float64), r.integers(-8, 9, (M, N)).astype(np.float64)
    out = (a, b, bias, c0, a @ b)
    for t in out:                                          # shared between the tests of a size
        t.flags.writeable = False
    return out


def gemm_sums_exact(a, b):
    """sum_k |a_k| |b_k| + 16 < 2^24 for every element, from max_i sum_k |a_ik| times max |b| (no second product needed)."""
    return float(np.abs(a).sum(1).max() * np.abs(b).max()) + 16 < 2 ** 24


# ---- B. attention backward at 12 heads of d = 64 ------------------------------------------------------------------------------------
# (kind as in test_gpu_mixed_kernels.exact_data, (B, heads, Lq, Lk, d, packed[, keys left]))
ATT16_EXACT = [("d", (1, 12, 257, 515, 64, False, 128)), ("d", (2, 12, 130, 130, 64, True, 64)), ("c", (1, 12, 515, 257, 64, False)),
               ("a", (1, 12, 515, 128, 64, False)), ("b", (1, 12, 515, 128, 64, False))]
ATT32_EXACT = ATT16_EXACT                                 # the same lengths through test_gpu_attention_grad's own kinds
ATT_BOUND = (12, 164, 164, 64, True)                      # (heads, Lq, Lk, d, packed), B = 3 as every BOUND case


# ---- E. cross-entropy rows with infinite logits ---------------------------------------------------------------------------------------
CE_SHAPES = [(2, 8, "scalar"), (100, 104, "scalar"), (128, 128, "vec"), (128, 131, "scalar"), (3129, 3136, "vec"), (3129, 3131, "scalar")]


def ce_rows(C, td):
    """-> (logits [M, C] of torch dtype `td`, labels int64 [M], kinds [M]).  kind "finite": -inf at columns that are not the
    label (column 0; the whole first 16-byte chunk; the tail behind the last whole chunk; scattered; everywhere but two columns);
    "label": the label's own logit is -inf; "nan": every logit -inf, a +inf beside the label, a +inf at the label, and NaN
    logits, which must stay NaN although fmaxf drops them from the running maximum: a NaN at column 0 in front of finite logits
    (of C = 2 too), the whole first 16-byte chunk NaN, a NaN in the last column behind nothing but -inf."""
    r = np.random.Generator(np.random.PCG64([C, 51]))
    draw = lambda: r.standard_normal(C) * 2
    rows, labels, kinds = [], [], []

    def add(x, label, kind):
        rows.append(x), labels.append(label), kinds.append(kind)
    for _ in range(3 if C == 2 else 1):
        x = draw()
        x[0] = -np.inf
        add(x, C - 1, "finite")
    if C >= 100:
        x = draw()
        x[:8] = -np.inf
        add(x, C // 2, "finite")
        x = draw()
        x[(C // 8 * 8 if C % 8 else C - 8):] = -np.inf
        add(x, 1, "finite")
        x = draw()
        x[r.uniform(size=C) < 0.3] = -np.inf
        x[0], x[C // 2] = -np.inf, 0.75
        add(x, C // 2, "finite")
        x = np.full(C, -np.inf)
        x[C // 3], x[C - 2] = 1.5, -0.25
        add(x, C // 3, "finite")
    x = draw()
    x[C - 1] = -np.inf
    add(x, C - 1, "label")
    add(np.full(C, -np.inf), 0, "nan")
    x = draw()
    x[C - 1] = np.inf
    add(x, 0, "nan")
    x = draw()
    x[0] = np.inf
    add(x, 0, "nan")
    x = draw()
    x[0] = np.nan
    add(x, C - 1, "nan")
    if C >= 100:
        x = draw()
        x[:8] = np.nan
        add(x, C // 2, "nan")
    x = np.full(C, -np.inf)
    x[C - 1] = np.nan
    add(x, 0, "nan")
    return torch.from_numpy(np.array(rows, np.float32)).to(td), np.array(labels, np.int64), kinds


def ce_loss_reference(x, labels, form, td):
    """float64 per-row loss as torch defines it, and `ce_bound` of the row's finite columns (a -inf logit adds exactly 0 to the
    sum, so the row's arithmetic is that of its finite columns; the step counts are the full row's)."""
    x = x.double().numpy()
    ref, bound = np.zeros(len(x)), np.zeros(len(x))
    for i, (row, lab) in enumerate(zip(x, labels)):
        fin = np.isfinite(row)
        if np.isnan(row).any() or np.isposinf(row).any() or not fin.any():
            ref[i] = np.nan
        elif not fin[lab]:
            ref[i] = np.inf
        else:
            r = P.ce_reference(row[fin][None], np.array([int(fin[:lab].sum())]))
            r["C"] = len(row)
            ref[i], bound[i] = r["ref"][0], P.ce_bound(r, form, td)[0]
    return ref, bound


def ce_grad_reference(x, labels, scale):
    """float64 dlogits = (softmax - onehot) scale and its per-element bound by `train_util.ce_grad_reference` on each row's finite
    columns; exactly 0 with a zero bound at a -inf column.  A label whose logit is -inf is exactly -scale; the other columns of
    such a row are train_util's for the finite columns with the label moved to an appended column so far below the maximum that
    its exponential is 0 in float64 (p = 0 and no weight in the bound's mean, as the -inf label itself).  NaN rows as
    `ce_loss_reference`."""
    x = np.asarray(x, np.float64)
    ref, bound = np.zeros(x.shape), np.zeros(x.shape)
    for i, (row, lab) in enumerate(zip(x, labels)):
        fin = np.isfinite(row)
        if np.isnan(row).any() or np.isposinf(row).any() or not fin.any():
            ref[i] = np.nan
        elif fin[lab]:
            r, b = U.ce_grad_reference(row[fin][None], np.array([int(fin[:lab].sum())]), scale)
            ref[i, fin], bound[i, fin] = r[0], b[0]
        else:
            sub = np.append(row[fin], row[fin].max() - 1e4)
            assert np.exp(sub[-1] - sub.max()) == 0.0
            r, b = U.ce_grad_reference(sub[None], np.array([len(sub) - 1]), scale)
            ref[i, fin], bound[i, fin], ref[i, lab] = r[0, :-1], b[0, :-1], -scale
    return ref, bound
