"""CPU: what vk_attention_relpos_grad_check refuses (host only: no pointer is read), the workspace size, and the entry -> bucket map
the table gradient is summed through, against relpos_lut's own fold."""
import pytest
import torch

from vltk_amd import _lib as L
from vltk_amd.layoutlmv3 import relative_position_bucket, relpos_bucket_map, relpos_lut

P = 0x1000          # a 16-byte aligned address that is never read


def check(**kw):
    a = dict(q=P, k=P, v=P, mask=None, rel_q=P, rel_k=P, lut=P, r1=128, r2=256, o=P, dout=P, dq=P, dk=P, dv=P, dlut=P, ld=768, B=2, heads=12,
             Lq=709, Lk=709, d=64, dt=L.VK_BF16, ws=P, ws_bytes=None)
    a.update(kw)
    if a["ws_bytes"] is None:
        a["ws_bytes"] = L.load().vk_attention_relpos_grad_workspace_bytes(a["B"], a["heads"], a["Lq"], a["r1"], a["r2"])
    ld = a["ld"]
    return L.load().vk_attention_relpos_grad_check(a["q"], ld, a["k"], ld, a["v"], ld, a["mask"], a["rel_q"], a["rel_k"], a["lut"], a["r1"], a["r2"],
                                                   a["o"], ld, a["dout"], ld, a["dq"], ld, a["dk"], ld, a["dv"], ld, a["dlut"], a["B"], a["heads"],
                                                   a["Lq"], a["Lk"], a["d"], a["dt"], a["ws"], a["ws_bytes"])


REFUSED = [dict(dlut=None), dict(rel_k=None), dict(lut=P + 2), dict(o=None), dict(dq=P + 8), dict(dt=L.VK_F32), dict(d=48), dict(ld=760),
           dict(ld=772), dict(r1=0), dict(r1=1024, r2=1024), dict(ws=P + 4), dict(ws_bytes=3 * 2 * 12 * 709 * 4), dict(Lk=0),
           dict(B=4096, Lq=1024, Lk=1024, ws_bytes=1 << 40), dict(B=2, heads=1, ld=64, Lq=46341, Lk=46341, ws_bytes=1 << 40)]


def test_check_accepts_the_flagship_shape_and_the_largest_size():
    assert check() == L.VK_OK and check(B=32) == L.VK_OK and check(mask=P) == L.VK_OK
    assert check(B=4095, Lq=1024, Lk=1024, ws_bytes=1 << 40) == L.VK_OK          # B Lq Lk < 2^32: 30 bits remain


@pytest.mark.parametrize("kw", REFUSED, ids=str)
def test_check_refuses(kw):
    assert check(**kw) == L.VK_EINVAL and L.load().vk_last_error()


def test_workspace_bytes():
    f = L.load().vk_attention_relpos_grad_workspace_bytes
    nlut = 257 + 2 * 513
    # the statistics of vk_attention_grad_16, 8-byte aligned, the int64 histogram, two maxima and a flag word per head
    assert f(2, 12, 709, 128, 256) == 3 * 2 * 12 * 709 * 4 + 8 * (12 * nlut + 18)
    assert f(1, 1, 1, 4, 3) == 16 + 8 * (23 + 2)
    assert f(0, 12, 709, 128, 256) == 0 and f(2, 12, 709, 0, 256) == 0


@pytest.mark.parametrize("bins,r", [(32, 128), (64, 256)])
def test_bucket_map_is_the_folds(bins, r):
    bucket = relpos_bucket_map(bins, bins, r, r)
    n = 2 * r + 1
    assert bucket.dtype == torch.int32 and bucket.shape == (3 * n,) and int(bucket.min()) == 0 and int(bucket.max()) == bins - 1
    assert torch.equal(bucket[:n].long(), relative_position_bucket(torch.arange(-r, r + 1), bins, r))
    assert torch.equal(bucket[:n], bucket[n:2 * n]) and torch.equal(bucket[:n], bucket[2 * n:])
    w = torch.arange(3 * 2 * bins, dtype=torch.float32).reshape(3, 2, bins)      # every weight distinct: the table names its bucket
    lut, _, _ = relpos_lut(w[0], w[1], w[2], r, r)
    for t in range(3):
        assert torch.equal(lut[:, t * n:(t + 1) * n], w[t][:, bucket[t * n:(t + 1) * n].long()])
