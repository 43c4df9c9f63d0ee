"""-m gpu: LXMERT refuses ids outside its tables, a token type outside its table, more tokens than positions and a wrong shape
on the host, before any launch or capture; a refused call leaves the model as it was (the next valid forward equals the one
before, bit for bit)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from vltk_amd.bert_ops import check_text_inputs                                                    # noqa: E402
from vltk_amd.lxmert import LxmertEncoder, LxmertForQuestionAnswering, lxmert_config, make_lxmert_qa_state_dict     # noqa: E402


def test_bad_ids_are_refused_before_any_launch():
    cfg = lxmert_config(vocab_size=300, hidden_size=128, num_attention_heads=4, intermediate_size=256, l_layers=1, x_layers=1, r_layers=1,
                        max_position_embeddings=16, visual_feat_dim=128)
    nqa, B, Lq, V = 10, 2, 7, 12
    sd = make_lxmert_qa_state_dict(cfg, nqa, 3)
    qa = LxmertForQuestionAnswering(cfg, nqa, precision="bf16").load_state_dict(sd)
    enc = LxmertEncoder(cfg, precision="bf16").load_state_dict({k[len("lxmert."):]: v for k, v in sd.items() if k.startswith("lxmert.")})
    gen = np.random.Generator(np.random.PCG64(5))
    ids = torch.from_numpy(gen.integers(1, 300, (B, Lq)))
    tts = torch.from_numpy(gen.integers(0, 2, (B, Lq)))
    feats = torch.from_numpy(np.maximum(gen.standard_normal((B, V, 128)), 0).astype(np.float32))
    pos = torch.from_numpy(gen.uniform(0, 1, (B, V, 4)).astype(np.float32))

    def with_id(i, j, val, base=ids):
        t = base.clone()
        t[i, j] = val
        return t
    long_ids = torch.from_numpy(gen.integers(1, 300, (B, 17)))
    bad = [(IndexError, with_id(0, 3, -1), tts), (IndexError, with_id(1, 6, 300), tts), (IndexError, ids, with_id(1, 0, 2, tts)),
           (ValueError, long_ids, None), (ValueError, ids, tts[:, :6]), (ValueError, ids.view(-1), None)]
    # the host function first, with nothing launched: the calls below rely on it
    for exc, i, t in bad:
        with pytest.raises(exc):
            check_text_inputs(i, t, cfg)

    before = [o.clone() for o in enc(ids, feats, pos, token_type_ids=tts)]
    score = qa(ids, feats, pos, token_type_ids=tts).clone()
    replay = enc.capture(ids, feats, pos, token_type_ids=tts)
    for exc, i, t in bad:
        with pytest.raises(exc):
            enc(i, feats, pos, token_type_ids=t)
        with pytest.raises(exc):
            qa(i, feats, pos, token_type_ids=t)
        with pytest.raises(exc):
            enc.capture(i, feats, pos, token_type_ids=t)
        with pytest.raises(exc):
            replay(i, feats, pos, token_type_ids=t)
    after = enc(ids, feats, pos, token_type_ids=tts)
    for a, b in zip(after, before):
        assert torch.equal(a, b)
    assert torch.equal(qa(ids, feats, pos, token_type_ids=tts), score)
    got = replay(ids, feats, pos, token_type_ids=tts)
    torch.cuda.synchronize()
    for a, b in zip(got, before):
        assert torch.equal(a, b)
