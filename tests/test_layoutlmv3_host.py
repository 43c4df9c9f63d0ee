"""CPU (-m "not gpu"): the host side of vk_attention_relpos: the table fold against transformers' stored
buckets and bias tensor, the rule that names the kernel form, and what the check refuses (it reads through no pointer, so made-up
addresses do)."""
import os

import numpy as np
import pytest
import torch

from vltk_amd import _lib as L
from vltk_amd.layoutlmv3 import attention_relpos_form, relative_position_bucket, relpos_lut, relpos_triples


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "layoutlmv3_relpos.npz"))


@pytest.mark.parametrize("bins,maxd", [(32, 128), (64, 256)])
def test_buckets_are_transformers_and_saturate(g, bins, maxd):
    """Every delta in [-max_distance - 2, max_distance + 2]; beyond max_distance the bucket is the one at max_distance, which is
    what lets the kernel clamp the difference."""
    delta = torch.arange(-maxd - 2, maxd + 3)
    got = relative_position_bucket(delta, bins, maxd)
    assert got.tolist() == g[f"bucket/{bins}_{maxd}"].tolist()
    assert got[:3].unique().tolist() == [bins // 2 - 1] and got[-3:].unique().tolist() == [bins - 1]
    far = relative_position_bucket(torch.tensor([-10 ** 6, -2000, 2000, 10 ** 6]), bins, maxd)
    assert far.tolist() == [bins // 2 - 1, bins // 2 - 1, bins - 1, bins - 1]


def test_table_lookup_is_transformers_bias(g):
    """T1[c(pk - pq)] + (TX[c(xk - xq)] + TY[c(yk - yq)]) from the folded table and the triples, in the kernel's order of additions,
    equals transformers' rel_pos + rel_2d_pos bit for bit."""
    lut, r1, r2 = relpos_lut(g["w1"], g["wx"], g["wy"])
    assert (r1, r2) == (128, 256) and lut.shape == (4, 257 + 2 * 513) and lut.dtype == torch.float32
    rel = relpos_triples(torch.from_numpy(g["position_ids"]), torch.from_numpy(g["bbox"])).long()
    d = rel[:, None, :, :] - rel[:, :, None, :]                                 # [B, query, key, 3]: key minus query
    hd = torch.arange(4)[None, :, None, None]
    t1 = lut[hd, d[..., 0].clamp(-r1, r1)[:, None] + r1]
    tx = lut[hd, d[..., 1].clamp(-r2, r2)[:, None] + r2 + 257]
    ty = lut[hd, d[..., 2].clamp(-r2, r2)[:, None] + r2 + 257 + 513]
    assert torch.equal(t1 + (tx + ty), torch.from_numpy(g["bias"]))


@pytest.mark.parametrize("Lq,queries", [(1, 16), (16, 16), (17, 32), (27, 32), (33, 64), (77, 96), (97, 128), (709, 128)])
def test_matrix_core_form_sizes_its_workgroup_from_lq(Lq, queries, monkeypatch):
    monkeypatch.delenv("VK_ATTENTION_MFMA", raising=False)
    for td, d in ((torch.bfloat16, 64), (torch.float16, 32)):
        assert attention_relpos_form(Lq, Lq, d, td, 3 * 4 * d, 3 * 4 * d, 3 * 4 * d) == ("mfma", queries)


def test_strict_form_takes_the_rest(monkeypatch):
    monkeypatch.delenv("VK_ATTENTION_MFMA", raising=False)
    assert attention_relpos_form(77, 77, 64, torch.float32, 768, 768, 768) == ("strict", 16)
    assert attention_relpos_form(77, 77, 48, torch.bfloat16, 768, 768, 768) == ("strict", 16)              # head dim
    assert attention_relpos_form(77, 77, 64, torch.bfloat16, 772, 768, 768) == ("strict", 16)              # a row off the 16-byte grid
    assert attention_relpos_form(77, 77, 64, torch.float16, 768, 768, 768, aligned16=False) == ("strict", 16)
    assert attention_relpos_form(77, 77, 256, torch.float16, 768, 768, 768) == ("strict", 16)
    monkeypatch.setenv("VK_ATTENTION_MFMA", "0")
    assert attention_relpos_form(77, 77, 64, torch.bfloat16, 768, 768, 768) == ("strict", 16)
    with pytest.raises(ValueError, match="head dim 257"):
        attention_relpos_form(77, 77, 257, torch.float32, 768, 768, 768)
    with pytest.raises(ValueError, match="bad geometry"):
        attention_relpos_form(0, 77, 64, torch.float32, 768, 768, 768)


GOOD = dict(q=0x1000, ldq=768, k=0x2000, ldk=768, v=0x3000, ldv=768, mask=None, rel_q=0x4000, rel_k=0x4000, lut=0x5000, r1=128, r2=256,
            out=0x6000, ldo=768, B=2, heads=12, Lq=709, Lk=709, d=64, dt=L.VK_BF16)
REFUSALS = [(dict(q=None), "null"), (dict(rel_k=None), "null"), (dict(lut=None), "null"), (dict(out=None), "null"),
            (dict(B=0), "positive"), (dict(Lk=0), "positive"), (dict(d=0), "positive"),
            (dict(r1=0), "radii"), (dict(r2=-1), "radii"), (dict(r1=512, r2=512), "LDS budget"), (dict(r1=2 ** 30, r2=2 ** 30), "LDS budget"),
            (dict(ldk=767), "leading dimension"), (dict(ldo=700), "leading dimension"),
            (dict(v=0x3001), "aligned to their element"), (dict(lut=0x5002), "4-byte"), (dict(mask=0x7001), "4-byte"),
            (dict(dt=L.VK_I32), "dtype"), (dict(d=300, heads=2, dt=L.VK_F32), "head dim 300")]


def test_check_accepts_and_refuses():
    lib = L.load()
    assert lib.vk_attention_relpos_check(*GOOD.values()) == L.VK_OK
    assert lib.vk_attention_relpos_check(*(GOOD | dict(mask=0x7000, v=0x3002, ldq=770, dt=L.VK_F16)).values()) == L.VK_OK    # the strict form's
    for change, text in REFUSALS:
        with pytest.raises(ValueError, match=text):
            L.call("vk_attention_relpos_check", *(GOOD | change).values())
