"""Host side of the pretraining forward, without a GPU: the shim, the reference's key names, shapes and weight tying at full
size, the state_dict round trip, the unchanged C ABI, the fp64 restatements against the golden recorded from the reference's
forward (and, where the reference is importable, against its modules), the single-frame filter's text side and tie rule, the
refusals, and the seeds the GPU tests draw with."""
import inspect
import json
import os

import numpy as np
import pytest
import torch

import pretrain_cases as pc
from common import GOLDEN
from oracle import ref_shim

IDS = [c.name for c in pc.CASES]


def _full(cls, **kw):
    from vidil_amd.tokenizer import SyntheticBertTokenizer

    with torch.device("meta"):                               # names and shapes only: nothing is allocated or initialised
        return cls(tokenizer=SyntheticBertTokenizer(), **kw)


def _keys():
    with open(os.path.join(GOLDEN, pc.KEYS)) as f:
        return json.load(f)


def test_the_shim_imports_and_the_signatures_are_the_references():
    from models.blip_pretrain import (BLIP_Pretrain, BLIP_Pretrain_Video, blip_pretrain, blip_pretrain_from_pretrained,  # noqa: F401
                                      blip_video_pretrain)
    from vidil_amd import blip_pretrain as bp
    from vidil_amd.blip_retrieval import BLIP_Retrieval

    assert blip_video_pretrain is bp.blip_video_pretrain and issubclass(BLIP_Pretrain_Video, BLIP_Pretrain)
    assert issubclass(BLIP_Pretrain, BLIP_Retrieval)         # the momentum state, the EMA, the ITC direction, the draw: inherited
    for name in ("_momentum_update", "_itc_direction", "_draw_from_weights", "_enqueue_features", "ensure_momentum_state"):
        assert getattr(BLIP_Pretrain, name) is getattr(BLIP_Retrieval, name)
    init = inspect.signature(BLIP_Pretrain.__init__).parameters
    assert list(init)[1:] == ["med_config", "image_size", "vit", "vit_grad_ckpt", "vit_ckpt_layer", "embed_dim", "queue_size",
                              "momentum", "tokenizer"]
    assert (init["med_config"].default, init["image_size"].default, init["queue_size"].default, init["momentum"].default) == \
        ("configs/bert_config.json", 224, 57600, 0.995)
    assert inspect.signature(BLIP_Pretrain_Video.__init__) == inspect.signature(BLIP_Pretrain.__init__)
    for cls, first in ((BLIP_Pretrain, "image"), (BLIP_Pretrain_Video, "video")):
        ps = inspect.signature(cls.forward).parameters
        assert list(ps)[:4] == ["self", first, "caption", "alpha"]
        for name in ("negatives", "seed", "details"):
            assert ps[name].kind == inspect.Parameter.KEYWORD_ONLY and ps[name].default is None
    for f in (blip_pretrain_from_pretrained, blip_video_pretrain):
        assert inspect.signature(f).parameters["pretrained"].default is None


@pytest.mark.parametrize("video", [False, True], ids=["image", "video"])
def test_full_size_names_shapes_and_tying_equal_the_references(video):
    from vidil_amd.blip_pretrain import BLIP_Pretrain, BLIP_Pretrain_Video

    ref = _keys()
    m = _full(BLIP_Pretrain_Video if video else BLIP_Pretrain)
    sd = m.state_dict(keep_vars=True)
    own = {k: list(v.shape) for k, v in sd.items() if "position_ids" not in k}
    assert own == {k: v for k, v in ref["state_dict"].items() if "position_ids" not in k}
    assert m.image_queue.shape == m.text_queue.shape == (256, 57600) and m.queue_ptr.dtype == torch.long and m.queue_ptr.shape == (1,)
    assert "idx_queue" not in sd and "ptr_queue" not in sd
    assert m.text_encoder.config.vocab_size == m.text_decoder.config.vocab_size == 30524
    # tied names are one Parameter object: exactly the fixture's groups and no others
    groups = {}
    for k, v in sd.items():
        groups.setdefault(id(v), []).append(k)
    shared = sorted(sorted(g) for g in groups.values() if len(g) > 1)
    assert shared == ref["shared"]
    tied = [g for g in shared if any(k.startswith("text_encoder.") for k in g)]
    assert tied and all(sorted(k.split(".", 1)[0] for k in g) == ["text_decoder", "text_encoder"] for g in tied)
    assert not [g for g in tied if any(".attention." in k for k in g)]                 # the self-attention blocks stay apart
    for g in tied:
        assert g[0].replace("text_decoder.bert.", "text_encoder.") == g[1]
    assert len(list(m.parameters())) == ref["n_parameters"]
    # the momentum text encoder shares nothing with the online one (nor with the decoder)
    online = {id(p) for p in m.text_encoder.parameters()} | {id(p) for p in m.text_decoder.parameters()}
    assert not online & {id(p) for p in m.text_encoder_m.parameters()}
    assert len(list(m.text_encoder_m.parameters())) == len(list(m.text_encoder.parameters()))
    assert [[type(a).__name__, type(b).__name__] for a, b in m.model_pairs] == [["VisionTransformer"] * 2, ["Linear"] * 2,
                                                                               ["BertModel"] * 2, ["Linear"] * 2]
    assert all(not p.requires_grad for _, mm in m.model_pairs for p in mm.parameters())


def test_a_vocabulary_of_bert_base_is_resized_to_the_tokenizers(tmp_path):
    """The reference's configs/bert_config.json has 30,522 entries and the constructor resizes to the tokenizer's 30,524."""
    from vidil_amd.blip import _DEFAULT_MED_CONFIG
    from vidil_amd.blip_pretrain import BLIP_Pretrain

    with open(_DEFAULT_MED_CONFIG) as f:
        cfg = json.load(f)
    cfg["vocab_size"] = 30522
    path = tmp_path / "bert_config.json"
    path.write_text(json.dumps(cfg))
    m = _full(BLIP_Pretrain, med_config=str(path))
    assert m.text_encoder.embeddings.word_embeddings.weight.shape[0] == 30524
    assert m.text_encoder.embeddings.word_embeddings.weight is m.text_decoder.bert.embeddings.word_embeddings.weight
    assert m.text_decoder.cls.predictions.decoder.weight.shape[0] == 30524 and m.text_encoder_m.config.vocab_size == 30524


def test_state_dict_round_trip_is_strict_and_keeps_the_tying():
    c = pc.case("video")
    a, b = pc.small_model(c, seed=1), pc.small_model(c, seed=2)
    msg = b.load_state_dict({k: v.clone() for k, v in a.state_dict().items()}, strict=True)
    assert not msg.missing_keys and not msg.unexpected_keys
    assert all(torch.equal(v, b.state_dict()[k]) for k, v in a.state_dict().items())
    assert b.text_encoder.encoder.layer[1].crossattention.self.key.weight is b.text_decoder.bert.encoder.layer[1].crossattention.self.key.weight
    assert b.text_encoder.encoder.layer[1].attention.self.key.weight is not b.text_decoder.bert.encoder.layer[1].attention.self.key.weight
    assert b.image_queue.data_ptr() == b._key_store("image_queue")[-c.queue_size:].data_ptr()      # in place: the store follows


def test_the_c_abi_is_unchanged():
    from vidil_amd import _lib

    lib = _lib.load()
    assert lib.vidil_num_entry_points() == 28 and lib.vidil_abi_version() == 13 and len(_lib.SIGNATURES) == 28


def test_the_ema_reads_the_shared_tensors_and_the_enqueue_moves_queue_ptr():
    c = pc.case("image")
    m = pc.small_model(c)
    shared = m.text_decoder.bert.encoder.layer[0].intermediate.dense.weight
    assert shared is m.text_encoder.encoder.layer[0].intermediate.dense.weight
    mom = m.text_encoder_m.encoder.layer[0].intermediate.dense.weight
    old = mom.clone()
    m._momentum_update()
    assert torch.equal(mom, old * pc.MOMENTUM + shared * (1. - pc.MOMENTUM))
    f = torch.arange(c.B * pc.EMBED, dtype=torch.float32).view(c.B, pc.EMBED)
    m._dequeue_and_enqueue(f, -f)
    assert torch.equal(m.image_queue[:, :c.B], f.t()) and torch.equal(m.text_queue[:, :c.B], -f.t()) and int(m.queue_ptr) == c.B
    m._dequeue_and_enqueue(f, -f)
    assert int(m.queue_ptr) == 0                                                        # queue of 12: wrapped


@pytest.mark.parametrize("c", pc.CASES, ids=IDS)
def test_the_restatements_reproduce_the_golden_and_the_chosen_seeds_exclude_no_draw(c):
    g = pc.golden()
    m = pc.small_model(c)
    image_queue, text_queue = m.image_queue.clone(), m.text_queue.clone()
    ptr = 0
    ids, mask = pc.token_ids(c, 0)
    assert mask.sum(1).tolist() == pc.lens(c)
    for call in range(pc.CALLS):
        k = f"{c.name}/{call}/"
        t = lambda n: torch.from_numpy(g[k + n])
        temp = float(g[k + "temp"])
        assert temp == pytest.approx(min(0.5, c.temp0))
        # the momentum features of the call are the columns the call enqueued
        assert torch.equal(t("image_queue")[:, ptr:ptr + c.B].T, t("image_feat_m")) and torch.equal(t("text_queue")[:, ptr:ptr + c.B].T, t("text_feat_m"))
        ita = pc.loss_ita64(t("image_feat"), t("text_feat"), t("image_feat_m"), t("text_feat_m"), image_queue, text_queue, temp, c.alpha[call])
        assert abs(ita - float(g[k + "loss_ita"])) <= 1e-5, (ita, g[k + "loss_ita"])
        assert abs(pc.loss_itm64(t("itm_logits")) - float(g[k + "loss_itm"])) <= 1e-5
        assert abs(pc.loss_lm64(t("lm_lp_label"), t("lm_lp_mean")) - float(g[k + "loss_lm"])) <= 1e-5 * float(g[k + "loss_lm"])
        assert g[k + "lm_lp_label"].shape == (sum(pc.lens(c)) - c.B,)                    # every real token but the first
        assert torch.allclose(t("sim_i2t"), t("image_feat") @ t("text_feat_m").T / temp, atol=1e-5)
        assert torch.allclose(t("sim_t2i"), t("text_feat") @ t("image_feat_m").T / temp, atol=1e-5)
        assert not torch.allclose(t("sim_i2t"), t("sim_t2i").T, atol=1e-3)               # (not transposes of each other)
        image_queue, text_queue = t("image_queue"), t("text_queue")
        ptr = (ptr + c.B) % c.queue_size
        assert int(g[k + "queue_ptr"][0]) == ptr
        own = np.arange(c.B)
        for name in ("neg_image_of_text", "neg_text_of_image"):                          # the reference never draws a row's own index
            assert (g[k + name] != own).all()
        for stream, s in ((0, t("sim_t2i")), (1, t("sim_i2t"))):
            d, close = pc.draws(s, pc.DRAW_SEEDS[c.name] + call, stream)
            assert not close.any() and (d.numpy() != own).all()
            w = pc.draw_weights(s)
            assert (w.diagonal() == 0).all() and (w + torch.eye(c.B) >= 1e-4).all()
    assert ptr == (pc.CALLS * c.B) % c.queue_size and (c.name != "image" or ptr == 0)


@pytest.fixture
def reference(monkeypatch):
    """(make_pretrain_golden, the reference's vit / med / blip_pretrain modules).  Loading the reference aliases models.med,
    models.vit and models.blip in sys.modules to ITS files: they are put back afterwards, so that later tests import the shims."""
    import sys

    names = ("models.med", "models.vit", "models.blip")
    saved = {n: sys.modules.get(n) for n in names}
    monkeypatch.syspath_prepend(GOLDEN)
    import make_pretrain_golden as mp

    try:
        yield (mp,) + tuple(mp.load_reference())
    finally:
        for n, mod in saved.items():
            if mod is None:
                sys.modules.pop(n, None)
            else:
                sys.modules[n] = mod


@pytest.mark.skipif(not ref_shim.available(), reason="needs the reference tree")
def test_the_lm_and_itm_restatements_reproduce_the_reference_modules(reference):
    import nlvr_cases as nc

    mp, vit_mod, med, rp = reference
    c = pc.case("image")
    ours = pc.small_model(c)
    o = mp.ref_object(rp.BLIP_Pretrain, rp, vit_mod, med, image_size=c.image_size, hidden=nc.HIDDEN, depth=2, heads=nc.HEADS,
                      cfg=mp.mr.ref_config(med, nc.HIDDEN, pc.rc.cfg_fields()), embed_dim=pc.EMBED, queue_size=c.queue_size,
                      momentum=pc.MOMENTUM, tokenizer=pc.vq.VqaTokenizer())
    mp.mr.load_strict(o, ours)
    ids, mask = pc.token_ids(c, 0)
    dec = ids.clone()
    dec[:, 0] = pc.vq.DEC
    with torch.no_grad():
        enc = o.visual_encoder(pc.pixels(c, 0))
        res = o.text_decoder(dec, attention_mask=mask, encoder_hidden_states=enc, encoder_attention_mask=torch.ones(enc.shape[:-1], dtype=torch.long),
                             labels=dec.masked_fill(dec == 0, -100), return_dict=True)
        lm, _, _ = pc.loss_lm_of_logits64(res.logits, ids, mask)
        assert abs(lm - float(res.loss)) <= 1e-5 * float(res.loss)
        logits = torch.randn(3 * c.B, 2, generator=torch.Generator().manual_seed(5)) * 3
        labels = torch.cat([torch.ones(c.B, dtype=torch.long), torch.zeros(2 * c.B, dtype=torch.long)])
        assert abs(pc.loss_itm64(logits) - float(torch.nn.functional.cross_entropy(logits, labels))) <= 1e-6


def test_sentence_tokenization_against_the_references_strings():
    from vidil_amd.pretrain import sentence_tokenization

    g = pc.golden()
    n = len([k for k in g if k.startswith("sentences/") and k.endswith("/in")])
    assert n >= 5
    for i in range(n):
        text, want = str(g[f"sentences/{i}/in"]), [str(s) for s in np.atleast_1d(g[f"sentences/{i}/out"])]
        assert sentence_tokenization(text, pc.NaiveNlp()) == want == sentence_tokenization(text, "naive"), text
    assert [str(s) for s in np.atleast_1d(g["sentences/2/out"])] == ["ok"]               # nothing longer than 3: the original
    assert sentence_tokenization("A:B c d", "naive") == ["b c d"]                       # lower-cased, ':' is a boundary, 'a' dropped


def test_sentence_tokenization_uses_capfilts_splitter_by_default(monkeypatch):
    from vidil_amd import capfilt
    from vidil_amd.pretrain import sentence_tokenization

    monkeypatch.setitem(capfilt.split_sentences.__dict__, "_nlp", pc.NaiveNlp())
    assert sentence_tokenization("First one here\nSecond one") == ["first one here", "second one"]


class _StubFilterer:
    """Stands in for BLIP_ITM: hands out given logits of class 1 and records the pairs it was asked for."""

    def __init__(self, scores_sn):
        self.scores, self.calls = scores_sn, []
        outer = self

        class _ViT:
            def forward_both(self, x):
                return None, torch.zeros(x.shape[0] * 2, 4, device=x.device)

        self.visual_encoder = _ViT()

    def tokenize(self, texts):
        return torch.zeros(len(texts), 35, dtype=torch.int32), torch.ones(len(texts), dtype=torch.int32)

    def itm_pairs(self, y16, n_images, ids, lens, group_start=None, max_group=0, pair_text=None):
        self.calls.append((n_images, ids.shape[0], group_start.tolist(), max_group, pair_text.tolist()))
        S, N = self.scores.shape
        one = self.scores.t().reshape(-1)                                               # pair (frame n, sentence s) at n * S + s
        return torch.stack([torch.zeros_like(one), one], 1)


def test_select_frame_takes_the_first_maximum_in_the_references_flat_order(monkeypatch):
    from vidil_amd import pretrain

    monkeypatch.setattr(pretrain, "require_cuda", lambda *a: None)
    # 3 sentences x 2 frames; the maximum 2.0 occurs at (sentence 1, frame 1) = flat 3 and (sentence 2, frame 0) = flat 4
    scores = torch.tensor([[0.0, 1.0], [0.5, 2.0], [2.0, -1.0]])
    f = _StubFilterer(scores)
    frame, sentence, got = pretrain.select_frame(f, torch.zeros(2, 3, 8, 8), "aaaa. bbbb. aaaa", "naive")
    # the second sentence repeats the first's text: two distinct texts, three sentences
    assert f.calls == [(2, 2, [0, 3, 6], 3, [0, 1, 0, 0, 1, 0])]
    assert (frame, sentence) == (1, "bbbb") and got.shape == (3, 2)
    assert torch.allclose(got, torch.softmax(torch.stack([torch.zeros(3, 2), scores], -1), -1)[..., 1])
    many = pretrain.select_frames(f, torch.zeros(2, 2, 3, 8, 8), ["aaaa. bbbb. aaaa"] * 2, "naive")
    assert [(a, b) for a, b, _ in many] == [(1, "bbbb")] * 2


def test_refusals_on_host_tensors_change_no_state():
    from vidil_amd import kernels as K

    c = pc.case("image")
    m = pc.small_model(c)
    x, caps = pc.pixels(c, 0), pc.captions(c, 0)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    with pytest.raises(K.VidilHipError, match="BLIP_Pretrain.forward: input is on cpu"):
        m(x, caps, 0.4)
    v = pc.small_model(pc.case("video"))
    with pytest.raises(K.VidilHipError, match="BLIP_Pretrain_Video.forward: input is on cpu"):
        v(pc.pixels(pc.case("video"), 0), pc.captions(pc.case("video"), 0), alpha=0.4)
    with pytest.raises(TypeError, match="call forward"):
        m.loss_forward(x, caps, 0.4, torch.arange(c.B))
    assert all(torch.equal(v_, m.state_dict()[k]) for k, v_ in before.items())


def test_the_select_frame_seeds_separate_the_oracles_best_pair():
    """The top-2 margin of the CPU oracle's scores is at least 10 x PRED_REL for every select_frame case, so the GPU's argmax
    (scores within 2 x PRED_REL x max(1, max|logit|) of the existing per-sentence calls) is the oracle's."""
    from vidil_amd.pretrain import sentence_tokenization

    f = pc.small_filterer()
    for seed, text in pc.SELECT_CASES:
        sents = sentence_tokenization(text, pc.NaiveNlp())
        assert len(sents) in (2, 3)
        top = torch.sort(pc.select_oracle(f, pc.select_pixels(seed), sents).flatten(), descending=True).values
        assert float(top[0] - top[1]) >= 10 * pc.PRED_REL, (seed, top[:3])
