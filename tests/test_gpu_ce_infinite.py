"""GPU (-m gpu): `vk_cross_entropy` (both forms, three storage types) and `vk_cross_entropy_grad` on rows that hold infinite
or NaN logits, against what torch computes for them (tests/extents_util.py: `ce_rows` and the float64 references over a row's finite
columns, which is the same softmax: a -inf logit has probability 0).

  -inf at non-label columns    a finite loss within the existing `ce_bound`; gradient exactly 0 at the -inf columns, the existing
                               bound elsewhere, the row sum as test_gpu_train_kernels asserts it
  the label's logit is -inf    loss +inf; gradient -scale at the label, the softmax of the rest elsewhere (torch: p - onehot)
  every logit -inf, or a +inf  NaN, as torch (loss and the whole gradient row)
  a NaN logit                  NaN, as torch: at column 0 in front of finite logits (of C = 2 too), a whole first 16-byte chunk,
                               the last column behind nothing but -inf

The running (max, sum) of csrc/losses.hip starts at (-inf, 0): before the fix an element met while the maximum was still -inf
computed exp(-inf - -inf) = NaN, and the first kind of row came out NaN.  The NaN rows hold the fix to the element: fmaxf drops a
NaN from the running maximum, so a select on "the maximum is still -inf" would add 0 for a NaN logit and return a finite loss."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from vltk_amd import _lib as L             # noqa: E402
from vltk_amd import train as T            # noqa: E402

import extents_util as E                   # noqa: E402
import gpu_util as G                       # noqa: E402
import lxmert_pretrain_util as P           # noqa: E402

DTS = [L.VK_F32, L.VK_F16, L.VK_BF16]
IDS = ["fp32", "fp16", "bf16"]
FORMS = {"vec": L.VK_CE_FORM_VEC, "scalar": L.VK_CE_FORM_SCALAR}


@pytest.mark.parametrize("C,ld,form", E.CE_SHAPES, ids=[f"{c}-{ld}-{f}" for c, ld, f in E.CE_SHAPES])
@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_cross_entropy_with_infinite_logits(dt, C, ld, form):
    td = G.TDT[dt]
    x, labels, kinds = E.ce_rows(C, td)
    M = len(labels)
    stored = torch.full((M, ld), 200.0, dtype=td)                                      # padding that would swamp the sum if read
    stored[:, :C] = x
    xd, lab = stored.to(G.DEV), torch.from_numpy(labels).to(G.DEV)
    assert L.load().vk_cross_entropy_form(C, ld, dt, int(xd.data_ptr() % 16 == 0)) == FORMS[form] == FORMS[P.ce_form(C, ld, td)]
    rows = torch.full((M + 1,), 77.0, dtype=torch.float32, device=G.DEV)
    L.call("vk_cross_entropy", G.P(xd), ld, M, C, G.P(lab), -100, G.P(rows), dt, G.stream())
    torch.cuda.synchronize()
    assert float(rows[M]) == 77.0, "the launch wrote behind its last row"
    got = rows[:M].cpu().numpy().astype(np.float64)
    ref, bound = E.ce_loss_reference(x, labels, form, td)
    finite = np.array([k == "finite" for k in kinds])
    assert finite.sum() >= 3 and np.isfinite(ref[finite]).all()
    err = np.abs(got[finite] - ref[finite])
    print(f"\n[ce -inf {IDS[DTS.index(dt)]} C={C} ({form})] rows {got}; worst |out - ref| / bound {(err / bound[finite]).max():.3f}", end="")
    assert np.isfinite(got[finite]).all(), "a -inf logit beside the label made a finite row's loss non-finite"
    assert (err <= bound[finite]).all(), (got, ref)
    for i, k in enumerate(kinds):
        if k == "label":
            assert got[i] == np.inf and ref[i] == np.inf, (i, got[i])
        if k == "nan":
            assert np.isnan(got[i]) and np.isnan(ref[i]), (i, got[i])


@pytest.mark.parametrize("C,ld", [(2, 2), (100, 104), (128, 128), (3129, 3131)])
def test_cross_entropy_grad_with_infinite_logits(C, ld):
    x, labels, kinds = E.ce_rows(C, torch.float32)
    x = x.numpy()
    M = len(labels)
    scale = np.float32(1.0 / M)
    xb = torch.full((M, ld), 200.0, dtype=torch.float32)
    xb[:, :C] = torch.from_numpy(x)
    xv = xb.to(G.DEV)[:, :C]
    obuf = torch.full((M * (C + 1) + C + 1,), 1e30, dtype=torch.float32, device=G.DEV)  # a padding column, a guard row behind
    ov = obuf[:M * (C + 1)].view(M, C + 1)[:, :C]
    T.cross_entropy_grad(xv, torch.from_numpy(labels).to(G.DEV), scale, out=ov)
    torch.cuda.synchronize()
    host = obuf.cpu().numpy()
    assert (host[:M * (C + 1)].reshape(M, C + 1)[:, C] == np.float32(1e30)).all() and (host[M * (C + 1):] == np.float32(1e30)).all()
    got = host[:M * (C + 1)].reshape(M, C + 1)[:, :C].astype(np.float64)
    ref, bound = E.ce_grad_reference(x, labels, float(scale))
    worst = 0.0
    for i, k in enumerate(kinds):
        if k == "nan":
            assert np.isnan(got[i]).all() and np.isnan(ref[i]).all(), i
            continue
        ninf = np.isneginf(x[i])
        ninf[labels[i]] = False
        assert (got[i][ninf] == 0).all(), (i, "a -inf column's gradient is not exactly 0")
        assert (np.abs(got[i] - ref[i]) <= bound[i]).all(), (i, k)
        assert abs(got[i].sum()) <= bound[i].sum(), (i, k)
        worst = max(worst, (np.abs(got[i] - ref[i])[bound[i] > 0] / bound[i][bound[i] > 0]).max())
        if k == "label":
            assert got[i][labels[i]] == -np.float64(scale)
    print(f"ce_grad -inf C={C}: worst |err| / bound = {worst:.3e}")
