"""CPU only: `bert_ops.check_text_inputs`, the host check LXMERT and VisualBERT run on their ids before any launch or capture (the
embedding kernels index their tables with them unchecked)."""
import pytest
import torch

from vltk_amd.bert_ops import check_ids, check_text_inputs

CFG = dict(vocab_size=300, type_vocab_size=2, max_position_embeddings=16)


def ids(B=2, Lt=7, fill=5):
    return torch.full((B, Lt), fill, dtype=torch.int64)


def test_valid_inputs_pass():
    check_text_inputs(ids(), None, CFG)
    x = ids()
    x[0, 0], x[1, -1] = 0, CFG["vocab_size"] - 1
    tt = ids(fill=0)
    tt[1, 3] = CFG["type_vocab_size"] - 1
    check_text_inputs(x, tt, CFG)
    check_text_inputs(ids(Lt=CFG["max_position_embeddings"]), None, CFG)
    check_text_inputs(x.to(torch.int32), tt.to(torch.int32), CFG)


@pytest.mark.parametrize("bad", [-1, 300, 301, 2 ** 40, -2 ** 40])
def test_input_id_outside_the_vocabulary(bad):
    x = ids()
    x[1, 2] = bad
    with pytest.raises(IndexError, match="input_ids"):
        check_text_inputs(x, None, CFG)


@pytest.mark.parametrize("bad", [-1, 2, 7])
def test_token_type_outside_its_table(bad):
    tt = ids(fill=0)
    tt[0, 6] = bad
    with pytest.raises(IndexError, match="token_type_ids"):
        check_text_inputs(ids(), tt, CFG)


def test_more_tokens_than_positions():
    with pytest.raises(ValueError, match="max_position_embeddings"):
        check_text_inputs(ids(Lt=CFG["max_position_embeddings"] + 1), None, CFG)


def test_wrong_shapes():
    with pytest.raises(ValueError, match="input_ids"):
        check_text_inputs(torch.zeros((14,), dtype=torch.int64), None, CFG)
    with pytest.raises(ValueError, match="input_ids"):
        check_text_inputs(torch.zeros((2, 7, 1), dtype=torch.int64), None, CFG)
    for shape in ((2, 6), (7, 2), (14,), (1, 7)):
        with pytest.raises(ValueError, match="token_type_ids"):
            check_text_inputs(ids(), torch.zeros(shape, dtype=torch.int64), CFG)


def test_shape_is_checked_before_the_values():
    """A wrong shape with a bad value in it is reported as the shape: the value check reads min / max of the right tensor."""
    tt = torch.full((2, 6), 9, dtype=torch.int64)
    with pytest.raises(ValueError):
        check_text_inputs(ids(), tt, CFG)


def test_check_ids_alone():
    check_ids("visual_token_type_ids", None, (2, 3), 2)
    check_ids("visual_token_type_ids", torch.ones((2, 3), dtype=torch.int64), (2, 3), 2)
    with pytest.raises(IndexError, match=r"\[0, 2\)"):
        check_ids("visual_token_type_ids", torch.full((2, 3), 2), (2, 3), 2)
    with pytest.raises(ValueError):
        check_ids("visual_token_type_ids", torch.ones((3, 2), dtype=torch.int64), (2, 3), 2)
