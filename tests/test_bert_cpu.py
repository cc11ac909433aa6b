"""The frozen BERT text tower (`--text_encoder bert`) without a GPU: the restatement's layer against `transformers`' own
`BertLayer` (through tests/golden/bert_layer_small.npz, written by tools/gen_bert_golden.py) and its whole model against a
random-weight `BertModel` where the package is installed, the library's parameter table and workspace plan (spec-only
towers, bind=False), and the Python layer: state-dict matching, mask checks, packing and splitting, the tokenising path
of the cache writer."""
import os

import numpy as np
import pytest
import torch

from bert_ref import Bert, BertLayer, named_shapes, randomize_like_trained, state_for_tower
from conftest import GOLDEN, rel_err


def _fixture_layer():
    z = np.load(os.path.join(GOLDEN, "bert_layer_small.npz"))
    names = [str(n) for n in z["names"]]
    blk = BertLayer(64, int(z["heads"]), 256).double()
    own = dict(blk.named_parameters())
    assert list(own) == names                       # the registration order of transformers' layer
    with torch.no_grad():
        for n in names:
            own[n].copy_(torch.from_numpy(z["param." + n]).double())
    return z, blk


def test_layer_matches_the_transformers_layer(report):
    """tests/bert_ref.BertLayer in float64 on the fixture's input and parameters against what transformers' BertLayer
    computed in fp32 under its additive key mask: the valid rows of every sequence within 1e-5 relative (L2), the bound
    tests/test_clip_text_cpu.py uses.  Measured with exactly these shapes: 2.1e-7, 2.3e-7, 2.5e-7 -- the package's own
    fp32 rounding."""
    z, blk = _fixture_layer()
    x, want = torch.from_numpy(z["x"]).double(), torch.from_numpy(z["y"])
    lens = z["lens"].tolist()
    assert x.shape == (3, 33, 64) and lens == [33, 20, 1]
    keep = torch.arange(33)[None, :] < torch.tensor(lens)[:, None]
    key_mask = torch.zeros(3, 33, dtype=torch.float64).masked_fill_(~keep, float("-inf"))
    with torch.no_grad():
        y, plain = blk(x, key_mask), blk(x)
        packed = blk.forward_packed(torch.cat([x[r, :l] for r, l in enumerate(lens)]), lens)
    errs = [rel_err(y[r, :l], want[r, :l]) for r, l in enumerate(lens)]
    report("bert layer vs transformers' BertLayer(64, 2 heads, 256), lengths %s: valid rows %s"
           % (lens, " ".join("%.1e" % e for e in errs)))
    assert max(errs) < 1e-5, errs
    # the mask matters on this fixture: without it the padded sequences are far away (sequence 0 has no padding), and so
    # are sequences 0 and 1 taken together
    assert rel_err(plain[1, :20], want[1, :20]) > 1e-2 and rel_err(plain[2, :1], want[2, :1]) > 1e-2
    both = lambda t: torch.cat([t[0, :33].reshape(-1), t[1, :20].reshape(-1)])
    assert rel_err(both(plain), both(want)) > 1e-2
    # packed rows are the valid rows of the padded run
    valid = torch.cat([y[r, :l] for r, l in enumerate(lens)])
    assert rel_err(packed, valid) < 1e-14


def test_model_matches_a_random_weight_bertmodel(report):
    """A whole BertModel(BertConfig(nano sizes)) with random weights, loaded BY NAME into the restatement: float64 against
    the package's fp32 last_hidden_state[:, 0] within 1e-5; the restatement's padded-with-mask and packed forwards agree to
    float64 rounding."""
    tr = pytest.importorskip("transformers")
    torch.manual_seed(50)
    cfg = tr.BertConfig(vocab_size=64, max_position_embeddings=40, hidden_size=64, num_attention_heads=1,
                        num_hidden_layers=2, intermediate_size=256, hidden_dropout_prob=0.0,
                        attention_probs_dropout_prob=0.0)
    hf = tr.BertModel(cfg).float().eval()
    g = torch.Generator().manual_seed(51)
    with torch.no_grad():
        for name, p in hf.named_parameters():                 # a spread the init does not have: see randomize_like_trained
            if ".query." in name or ".key." in name:
                if p.dim() == 2:
                    p.mul_(1.0 / (0.02 * 8.0))
            if name.endswith("bias"):
                p.add_(0.02 * torch.randn(p.shape, generator=g))
    own = Bert("bert_nano").double()
    sd = {k: v for k, v in hf.state_dict().items() if not k.startswith("pooler.") and k in dict(own.named_parameters())}
    assert set(sd) == set(dict(own.named_parameters()))       # every parameter but the pooler, under the same names
    with torch.no_grad():
        for n, p in own.named_parameters():
            assert tuple(p.shape) == tuple(sd[n].shape), n
            p.copy_(sd[n].double())
    lens = [9, 5, 1]
    ids = torch.zeros(3, 9, dtype=torch.long)
    for r, l in enumerate(lens):
        ids[r, :l] = torch.randint(1, 64, (l,), generator=g)
    am = (torch.arange(9)[None, :] < torch.tensor(lens)[:, None]).long()
    with torch.no_grad():
        want = hf(input_ids=ids, attention_mask=am).last_hidden_state[:, 0]
        padded = own(ids, am)
        packed = own.forward_packed(torch.cat([ids[r, :l] for r, l in enumerate(lens)]), lens)
    e = rel_err(padded, want)
    report(f"bert restatement (float64) vs transformers BertModel (fp32, random weights, nano sizes): [CLS] {e:.1e}; "
           f"padded vs packed {rel_err(packed, padded):.1e}")
    assert e < 1e-5, e
    assert rel_err(packed, padded) < 1e-14


# ---------------------------------------------------------------------------------------------- the library's tables
@pytest.mark.parametrize("variant", ["bert_micro", "bert_nano"])
def test_spec_only_tower_reports_the_bert_table(variant):
    from multimodal_dataset_distillation_amd.text_tower import TextTower
    tw = TextTower(variant, max_batch=4, compute_dtype="bf16", bind=False)
    ref = Bert(variant)
    tab = tw.param_table()
    assert {(n, tuple(s)) for n, s, _ in tab} == set(named_shapes(ref)) and len(tab) == len(named_shapes(ref))
    sizes = [int(np.prod(s)) for _, s, _ in tab]
    assert [o for _, _, o in tab] == np.concatenate([[0], np.cumsum(sizes)[:-1]]).tolist()
    assert tw.param_numel == sum(sizes) == sum(p.numel() for p in ref.parameters())
    cfg = ref.cfg
    assert (tw.feature_dim, tw.context, tw.vocab) == (cfg.width, cfg.positions, cfg.vocab)
    # query, key and value of a layer lie next to each other: one [3 D, D] linear
    off = {n: o for n, _, o in tab}
    d = cfg.width
    for l in range(cfg.layers):
        pre = "encoder.layer.%d.attention.self." % l
        assert off[pre + "key.weight"] == off[pre + "query.weight"] + d * d
        assert off[pre + "value.weight"] == off[pre + "key.weight"] + d * d
        assert off[pre + "key.bias"] == off[pre + "query.bias"] + d and off[pre + "value.bias"] == off[pre + "key.bias"] + d
    assert not any(n.startswith("pooler.") for n in off)
    tw.close()


def test_bert_base_uncased_sizes_and_workspace_plan():
    from multimodal_dataset_distillation_amd.text_tower import TextTower
    full = TextTower("bert_base_uncased", max_batch=1000, compute_dtype="bf16", bind=False)
    tab = full.param_table()
    # 109,482,240 (BertModel of bert-base-uncased) - 590,592 (pooler.dense: 768 x 768 + 768)
    assert full.param_numel == 108_891_648 == 109_482_240 - 590_592
    layers = 1 + max(int(n.split(".")[2]) for n, _, _ in tab if n.startswith("encoder.layer."))
    shapes = {n: tuple(s) for n, s, _ in tab}
    assert layers == 12 and full.feature_dim == 768 and full.context == 512 and full.vocab == 30522
    assert shapes["embeddings.word_embeddings.weight"] == (30522, 768)
    assert shapes["embeddings.position_embeddings.weight"] == (512, 768)
    assert shapes["embeddings.token_type_embeddings.weight"] == (2, 768)
    assert shapes["encoder.layer.11.intermediate.dense.weight"] == (3072, 768)
    # the workspace is planned from max_tokens rows, not from max_batch * 512
    packed = TextTower("bert_base_uncased", max_batch=1000, compute_dtype="bf16", bind=False, max_tokens=4096)
    assert full.max_tokens == 1000 * 512 and packed.max_tokens == 4096
    assert packed.workspace_bytes < full.workspace_bytes // 20
    # at full length the activations are 12 width-768 bf16 columns per row (x, x1, the sum, attention out, the linear's
    # output: 5; qkv: 3; the GELU output: 4)
    assert full.workspace_bytes > 1000 * 512 * 12 * 768 * 2
    with pytest.raises(RuntimeError, match="invalid argument"):
        TextTower("bert_base_uncased", max_batch=4, bind=False, max_tokens=1 << 20)       # 2^20 * 4 * 768 >= 2^31
    full.close()
    packed.close()


# the workspace sizes of the CLIP variants at max_batch = 4, as the commit before the BERT tower planned them
CLIP_WORKSPACE = {("clip_text_b32", "bf16"): 253_730_304, ("clip_text_b32", "f32"): 404_725_248,
                  ("clip_text_micro", "bf16"): 2_065_152, ("clip_text_micro", "f32"): 3_797_760,
                  ("clip_text_nano", "bf16"): 435_712, ("clip_text_nano", "f32"): 835_072}


@pytest.mark.parametrize("variant,dtype", sorted(CLIP_WORKSPACE))
def test_clip_workspace_is_what_it_was(variant, dtype):
    from multimodal_dataset_distillation_amd.text_tower import TextTower
    tw = TextTower(variant, max_batch=4, compute_dtype=dtype, bind=False)
    assert tw.workspace_bytes == CLIP_WORKSPACE[(variant, dtype)]
    # max_tokens is BERT's: a CLIP tower computes whole contexts whatever it says
    other = TextTower(variant, max_batch=4, compute_dtype=dtype, bind=False, max_tokens=7)
    assert other.workspace_bytes == tw.workspace_bytes and other.max_tokens == 4 * tw.context
    tw.close()
    other.close()


# ---------------------------------------------------------------------------------------------- the Python layer
def test_state_dict_is_matched_by_name(tmp_path):
    from multimodal_dataset_distillation_amd.text_tower import TextTower
    tw = TextTower("bert_nano", max_batch=4, compute_dtype="f32", bind=False)
    torch.manual_seed(4)
    ref = Bert("bert_nano")
    randomize_like_trained(ref, 5)
    sd = state_for_tower(ref)
    flat = tw.flat_from_state_dict(sd)
    for name, shape, off in tw.param_table():
        assert torch.equal(flat[off:off + int(np.prod(shape))].reshape(shape), sd[name]), name
    # any order, fp16, the `bert.` prefix, and what BertForPreTraining / BertModel carry beside the tower
    mixed = {"cls.predictions.bias": torch.zeros(64), "bert.pooler.dense.weight": torch.zeros(64, 64),
             "pooler.dense.bias": torch.zeros(64), "bert.embeddings.position_ids": torch.arange(40)[None],
             "embeddings.token_type_ids": torch.zeros(1, 40, dtype=torch.long)}
    for k in reversed(list(sd)):
        mixed["bert." + k] = sd[k].half()
    got = tw.flat_from_state_dict(mixed)
    assert got.dtype == torch.float32 and torch.equal(got, flat.half().float())
    lacking = dict(sd); del lacking["embeddings.LayerNorm.bias"]
    with pytest.raises(ValueError, match="lacks 'embeddings.LayerNorm.bias'"):
        tw.flat_from_state_dict(lacking)
    wrong = dict(sd); wrong["encoder.layer.1.intermediate.dense.weight"] = sd["encoder.layer.1.intermediate.dense.weight"].t().contiguous()
    with pytest.raises(ValueError, match="intermediate.dense.weight.*shape"):
        tw.flat_from_state_dict(wrong)
    path = str(tmp_path / "state.pt")                       # the same two through a file, before any GPU is asked for
    torch.save(lacking, path)
    with pytest.raises(ValueError, match="lacks"):
        tw.load_state_dict_file(path)
    torch.save(wrong, path)
    with pytest.raises(ValueError, match="shape"):
        tw.load_state_dict_file(path)
    tw.close()


def test_masks_and_ids_are_checked_before_anything_runs():
    from multimodal_dataset_distillation_amd.text_tower import TextTower
    tw = TextTower("bert_nano", max_batch=4, compute_dtype="f32", bind=False, max_tokens=16)
    ids = torch.tensor([[5, 6, 7, 0], [8, 9, 0, 0]])
    packed, lens = tw.pack(ids)                               # no mask: ids != 0
    assert packed.dtype == torch.int32 and packed.tolist() == [5, 6, 7, 8, 9] and lens == [3, 2]
    packed, lens = tw.pack(ids.numpy(), np.array([[1, 1, 1, 1], [1, 0, 0, 0]]))      # the mask decides: id 0 may be valid
    assert packed.tolist() == [5, 6, 7, 0, 8] and lens == [4, 1]
    assert tw.pack(ids, torch.tensor([[True, True, False, False], [True, True, True, True]]))[1] == [2, 4]
    with pytest.raises(ValueError, match="ones followed by zeros"):
        tw.encode(ids, torch.tensor([[1, 0, 1, 0], [1, 1, 0, 0]]))                      # a hole
    with pytest.raises(ValueError, match="ones followed by zeros"):
        tw.encode(torch.tensor([[5, 0, 7, 0], [8, 9, 0, 0]]))                           # a [PAD] inside, no mask given
    with pytest.raises(ValueError, match="row 1 is empty"):
        tw.encode(ids, torch.tensor([[1, 1, 0, 0], [0, 0, 0, 0]]))
    with pytest.raises(ValueError, match="zeros and ones"):
        tw.encode(ids, torch.tensor([[2, 1, 0, 0], [1, 0, 0, 0]]))
    with pytest.raises(ValueError, match="shape"):
        tw.encode(ids, torch.ones(2, 3, dtype=torch.long))
    for bad in (-1, tw.vocab, tw.vocab + 5):
        other = ids.clone(); other[1, 1] = bad
        with pytest.raises(ValueError, match=r"\[0, 64\)"):
            tw.encode(other, torch.tensor([[1, 1, 1, 0], [1, 1, 0, 0]]))
    other = ids.clone(); other[1, 3] = tw.vocab + 5            # outside the table, but padding: never read
    assert tw.pack(other, torch.tensor([[1, 1, 1, 0], [1, 1, 0, 0]]))[0].tolist() == [5, 6, 7, 8, 9]
    with pytest.raises(ValueError, match="40 positions"):
        tw.encode(torch.ones(2, tw.context + 1, dtype=torch.long))
    with pytest.raises(ValueError, match="integers"):
        tw.encode(ids.float())
    with pytest.raises(ValueError, match="more than max_tokens = 16"):
        tw.encode(torch.ones(2, 17, dtype=torch.long))
    with pytest.raises(RuntimeError, match="no CPU path"):    # everything above was refused before this
        tw.encode(ids)
    tw.close()
    clip = TextTower("clip_text_nano", max_batch=4, compute_dtype="f32", bind=False)
    with pytest.raises(ValueError, match="attention_mask"):
        clip.encode(torch.zeros(2, clip.context, dtype=torch.long), torch.ones(2, clip.context, dtype=torch.long))
    clip.close()


def test_packing_splits_in_order_by_sequences_and_rows():
    from multimodal_dataset_distillation_amd.text_tower import plan_calls
    lens = [1, 33, 7, 40, 32, 3, 3, 3]
    # (first sequence, sequences, rows): two sequences at the most, 48 rows at the most
    assert plan_calls(lens, 2, 48) == [(0, 2, 34), (2, 2, 47), (4, 2, 35), (6, 2, 6)]
    assert plan_calls(lens, 3, 48) == [(0, 3, 41), (3, 1, 40), (4, 3, 38), (7, 1, 3)]     # the row limit cuts a call short
    assert plan_calls(lens, 100, 40) == [(0, 2, 34), (2, 1, 7), (3, 1, 40), (4, 3, 38), (7, 1, 3)]
    assert plan_calls(lens, 100, 1000) == [(0, 8, 122)]
    assert plan_calls([5], 1, 5) == [(0, 1, 5)]
    for calls in (plan_calls(lens, 2, 48), plan_calls(lens, 100, 40)):
        assert [c[0] for c in calls] == np.concatenate([[0], np.cumsum([c[1] for c in calls])[:-1]]).tolist()
        assert sum(c[2] for c in calls) == sum(lens)
    with pytest.raises(ValueError, match="more than max_tokens"):
        plan_calls(lens, 2, 39)
    with pytest.raises(ValueError, match="empty"):
        plan_calls([3, 0, 2], 2, 48)


def test_captions_are_tokenised_with_the_users_vocabulary(tmp_path):
    """embed_text's --captions/--vocab path: transformers.BertTokenizer on a ten-word vocabulary file, padding=True."""
    pytest.importorskip("transformers")
    from multimodal_dataset_distillation_amd import embed_text
    vocab = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]", "a", "dog", "runs", "fast", "##er"]
    vpath, cpath = str(tmp_path / "vocab.txt"), str(tmp_path / "captions.txt")
    with open(vpath, "w") as f:
        f.write("\n".join(vocab) + "\n")
    with open(cpath, "w") as f:
        f.write("A dog runs faster\nDog\na zebra runs\n")
    ids, mask = embed_text._tokenize_bert(cpath, vpath)
    assert ids.tolist() == [[2, 5, 6, 7, 8, 9, 3], [2, 6, 3, 0, 0, 0, 0], [2, 5, 1, 7, 3, 0, 0]]     # lower-cased, [UNK], word pieces
    assert mask.tolist() == [[1] * 7, [1, 1, 1, 0, 0, 0, 0], [1, 1, 1, 1, 1, 0, 0]]
    from multimodal_dataset_distillation_amd.text_tower import TextTower
    tw = TextTower("bert_nano", max_batch=4, bind=False)
    assert tw.pack(ids, mask)[1] == [7, 3, 5] and tw.pack(ids)[1] == [7, 3, 5]
    tw.close()
    with pytest.raises(SystemExit, match="--vocab"):
        embed_text._tokenize_bert(cpath, None)


def test_embed_text_parser_keeps_clip_and_adds_bert():
    from multimodal_dataset_distillation_amd import embed_text
    ap = embed_text.build_parser()
    a = ap.parse_args(["--dataset", "flickr", "--file_type", "text", "--tokens", "t.npz", "--text_encoder", "bert",
                       "--bert_weights", "s.pt"])
    assert a.text_encoder == "bert" and a.variant is None and embed_text.DEFAULT_VARIANT["bert"] == "bert_base_uncased"
    c = ap.parse_args(["--dataset", "flickr", "--file_type", "text", "--tokens", "t.npy", "--clip_weights", "s.pt"])
    assert c.text_encoder == "clip" and embed_text.DEFAULT_VARIANT["clip"] == "clip_text_b32"
    with pytest.raises(SystemExit, match="--clip_weights"):          # still required for clip, before any GPU is asked for
        embed_text.main(ap.parse_args(["--dataset", "flickr", "--file_type", "text", "--tokens", "t.npy"]))
    with pytest.raises(SystemExit, match="--bert_weights"):
        embed_text.main(ap.parse_args(["--dataset", "flickr", "--file_type", "text", "--tokens", "t.npy", "--text_encoder", "bert"]))
    with pytest.raises(SystemExit, match="no bert tower"):
        embed_text.main(ap.parse_args(["--dataset", "flickr", "--file_type", "text", "--tokens", "t.npy", "--text_encoder",
                                       "bert", "--bert_weights", "s.pt", "--variant", "clip_text_nano"]))
