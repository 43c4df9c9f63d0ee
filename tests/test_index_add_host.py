"""CPU (-m "not gpu"): what `vk_index_add_rows_check` refuses, one bad argument each (host only: the pointers are made-up addresses
that nothing reads through), and the workspace size function."""
import pytest

from vltk_amd import _lib as L

P = 0x10000                                  # an aligned, non-null "pointer"
GOOD = dict(src=P, ld_src=8, M=40, idx=P, src_row=None, n=40, dst=P, ld_dst=8, R=10, C=8, padding_idx=-1, workspace=P, bytes=None)


def check(**kw):
    a = dict(GOOD, **kw)
    if a["bytes"] is None:
        a["bytes"] = L.load().vk_index_add_rows_workspace_bytes(max(a["n"], 1), max(a["R"], 1), max(a["C"], 1)) or 1 << 20
    L.call("vk_index_add_rows_check", *a.values())


@pytest.mark.parametrize("bad", [dict(src=None), dict(idx=None), dict(dst=None), dict(workspace=None), dict(n=0), dict(R=0), dict(C=0),
                                 dict(M=0), dict(ld_src=7), dict(ld_dst=7), dict(n=2 ** 31), dict(R=2 ** 31), dict(padding_idx=10),
                                 dict(padding_idx=-2), dict(bytes=GOOD["n"] * 16), dict(src=P + 2), dict(workspace=P + 4)],
                         ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_refuses(bad):
    with pytest.raises(ValueError, match="index_add_rows"):
        check(**bad)


def test_good_call_and_workspace_size():
    check()
    check(src_row=P, padding_idx=9)
    size = L.load().vk_index_add_rows_workspace_bytes
    for n0, n1 in ((1, 2), (31, 32), (32, 33), (1024, 1025), (2 ** 20, 2 ** 20 + 1)):
        assert 0 < size(n0, 100, 8) <= size(n1, 100, 8)
    for c0, c1 in ((1, 2), (3, 4), (768, 769)):
        assert 0 < size(100, 100, c0) <= size(100, 100, c1)
    assert size(2 ** 31, 100, 8) == 0 and size(100, 0, 8) == 0
