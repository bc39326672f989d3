"""The reference's call surface over the text stack on the GPU: BertModel.forward / BertLMHeadModel.forward with the HF
signature, BLIP_Base, BLIP_Embedding — against the reference's own outputs (tests/golden/forward_small.npz, written by
tests/golden/make_forward_golden.py from the reference's models/med.py) on the committed small weights (hidden 256, 4 heads,
2 layers, vocabulary 512; B = 4, T = 12, Te = 26), and against the library's own entry points bit for bit.

Tolerances are the ones the existing small-model tests apply to the same weights:
  hidden states   max|d| < 6e-3                                   tests/test_models_gpu.py:170 (encode vs med_itm_small.npz)
  decoder logits  max|d| <= 1.25e-3 x max(1, max|ref|), mean|d| <= 0.4 x that        tests/test_models_gpu.py:33,42-51
  loss sums       a sequence of n targets within 2 n g, the mean within 2 g, g the logit gate
                                                                  tests/test_caption_scoring_gpu.py:190-193 (|d lse| <= max|d logit|)
  ViT tokens      max|d| < 5e-3, mean|d| < 5e-4                   tests/test_models_gpu.py:79
  retrieval       a candidate's score within 2e-2 of the fp32 oracle      tests/test_video_retrieval_gpu.py:62
"""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import video_retrieval_cases as VC
import vqa_cases as vq
from common import load_golden, load_into

pytestmark = pytest.mark.gpu
DEV = "cuda"
HIDDEN_TOL = 6e-3
PLAIN_F16_REL = 1.25e-3
B, T, TE, C, V = 4, 12, 26, 256, 512
LENS, ENC_LENS = [12, 7, 3, 1], [26, 20, 5, 26]


def _small_cfg():
    from vidil_amd.med import BertConfig

    return BertConfig(hidden_size=256, num_attention_heads=4, intermediate_size=512, num_hidden_layers=2, vocab_size=512,
                      max_position_embeddings=64, encoder_width=256)


@pytest.fixture(scope="module")
def gold():
    _, g = load_golden("forward_small.npz")
    return g


@pytest.fixture(scope="module")
def encoder():
    from vidil_amd.med import BertModel

    sd, _ = load_golden("med_itm_small.npz")
    return load_into(BertModel(_small_cfg()), sd, "text_encoder.").to(DEV).eval()


@pytest.fixture(scope="module")
def decoder():
    from vidil_amd.med import BertLMHeadModel

    sd, _ = load_golden("med_decoder_small.npz")
    return load_into(BertLMHeadModel(_small_cfg()), sd, "text_decoder.").to(DEV).eval()


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def enc_states(gold):
    return dev(gold["enc"]).float()                           # f16-representable values: the 16-bit cast inside is exact


def worst(got, ref, mask=None):
    """max|got - ref| over all positions, or over those whose mask is 1."""
    d = (got.detach().float().cpu() - torch.from_numpy(np.asarray(ref))).abs()
    if mask is not None:
        d = d[torch.from_numpy(np.asarray(mask)).bool()]
    return d.max().item(), d.mean().item()


# ------------------------------------------------------------------------------------------------ 1. it no longer raises
def test_text_encoder_call_of_the_reference_no_longer_raises(encoder, gold):
    """eval_retrieval_video.py:46 — NotImplementedError("use BertModel.encode ...") before this feature."""
    out = encoder(dev(gold["ids_right"]), attention_mask=dev(gold["mask_right"]), mode="text")
    h = out.last_hidden_state
    assert tuple(h.shape) == (B, T, C) and h.dtype == torch.float32 and h.is_cuda and bool(torch.isfinite(h).all())
    assert out.pooler_output is None and out.hidden_states is None and out[0] is h
    assert tuple(out.last_hidden_state[:, 0, :].shape) == (B, C)


# ------------------------------------------------------------------------------------------------ 2. bit identity, prefix masks
def test_prefix_masks_give_the_bits_of_encode(encoder, gold):
    ids, mask = dev(gold["ids_right"]), dev(gold["mask_right"])
    ids32, lens = ids.to(torch.int32).contiguous(), torch.tensor(LENS, dtype=torch.int32, device=DEV)
    enc = enc_states(gold)
    enc16 = enc.half().reshape(B * TE, C).contiguous()
    # mode='text'
    want, _ = encoder.encode(ids32, lens, None)
    got = encoder(ids, attention_mask=mask, mode="text").last_hidden_state
    assert torch.equal(got, want.view(B, T, C))
    # int32 ids, f16 encoder states, no encoder_attention_mask
    want, _ = encoder.encode(ids32, lens, encoder.project_cross_kv(enc16, B, TE))
    got = encoder(ids32, attention_mask=mask, encoder_hidden_states=enc16.view(B, TE, C), return_dict=True).last_hidden_state
    assert torch.equal(got, want.view(B, T, C))
    assert torch.equal(encoder(ids, attention_mask=mask, encoder_hidden_states=enc)[0], got)       # f32 states, int64 ids
    # a prefix encoder_attention_mask = cross kv_len
    ckl = torch.tensor(ENC_LENS, dtype=torch.int32, device=DEV)
    want, _ = encoder.encode(ids32, lens, encoder.project_cross_kv(enc16, B, TE, kv_len=ckl), cross_kv_len=ckl)
    got = encoder(ids, attention_mask=mask, encoder_hidden_states=enc, encoder_attention_mask=dev(gold["encmask_prefix"]),
                  return_dict=False)
    assert isinstance(got, tuple) and len(got) == 2 and got[1] is None
    assert torch.equal(got[0], want.view(B, T, C))


def test_decoder_loss_gives_the_bits_of_score(decoder, gold):
    """reduction='none' on right-padded captions = BertLMHeadModel.score's loss_sum (what caption_nll returns at
    label_smoothing=0.1), with and without a prefix encoder_attention_mask."""
    ids, mask, labels = dev(gold["dec_right_ids"]), dev(gold["mask_right"]), dev(gold["dec_right_labels"])
    enc = enc_states(gold)
    enc16 = enc.half().reshape(B * TE, C).contiguous()
    for em, ckl in ((dev(gold["encmask_prefix"]), ENC_LENS), (None, None)):
        res = decoder.score(enc16, B, ids.cpu(), LENS, label_smoothing=0.1, prompt_length=1, cross_kv_len=ckl)
        out = decoder(ids, attention_mask=mask, encoder_hidden_states=enc, encoder_attention_mask=em, labels=labels,
                      return_dict=True, reduction="none")
        assert res.count.cpu().tolist() == [n - 1 for n in LENS]
        assert out.loss.dtype == torch.float32 and tuple(out.loss.shape) == (B,)
        assert torch.equal(out.loss, res.loss_sum), (out.loss, res.loss_sum)


# ------------------------------------------------------------------------------------------------ 3. the reference's outputs
ENCODER_CASES = [(mode, name) for mode in ("text", "mm") for name in ("ones", "right", "left", "holes")]


@pytest.mark.parametrize("mode,name", ENCODER_CASES)
def test_encoder_vs_reference(encoder, gold, mode, name):
    mask = gold[f"mask_{name}"]
    kw = dict(mode="text") if mode == "text" else dict(encoder_hidden_states=enc_states(gold))
    got = encoder(dev(gold[f"ids_{name}"]), attention_mask=dev(mask), return_dict=True, **kw).last_hidden_state
    mx, mean = worst(got, gold[f"{mode}_{name}"], None if name in ("ones", "right") else mask)
    print(f"\n{mode} {name}: max|d| = {mx:.3e}, mean|d| = {mean:.3e}")
    assert mx < HIDDEN_TOL
    if name == "ones":                                          # attention_mask=None is all ones
        none = encoder(dev(gold["ids_ones"]), return_dict=True, **kw).last_hidden_state
        assert worst(none, gold[f"{mode}_ones"])[0] < HIDDEN_TOL


@pytest.mark.parametrize("name", ["prefix", "holes"])
def test_encoder_attention_mask_vs_reference(encoder, gold, name):
    got = encoder(dev(gold["ids_right"]), attention_mask=dev(gold["mask_right"]), encoder_hidden_states=enc_states(gold),
                  encoder_attention_mask=dev(gold[f"encmask_{name}"]), return_dict=True).last_hidden_state
    mx, mean = worst(got, gold[f"mm_right_enc{name}"])
    print(f"\nencoder_attention_mask {name}: max|d| = {mx:.3e}, mean|d| = {mean:.3e}")
    assert mx < HIDDEN_TOL


def test_an_explicit_all_ones_encoder_attention_mask_vs_reference(encoder, gold):
    """The reference's callers pass image_atts = ones: the mask route (compaction, cross kv_len = Te, the row clearing of
    project_cross_kv) with nothing to mask, against the same golden as the default None."""
    kw = dict(attention_mask=dev(gold["mask_right"]), encoder_hidden_states=enc_states(gold))
    ones = torch.ones((B, TE), dtype=torch.long, device=DEV)
    got = encoder(dev(gold["ids_right"]), encoder_attention_mask=ones, return_dict=True, **kw).last_hidden_state
    none = encoder(dev(gold["ids_right"]), return_dict=True, **kw).last_hidden_state
    mx, mean = worst(got, gold["mm_right"])
    print(f"\nencoder_attention_mask ones: max|d| = {mx:.3e}, mean|d| = {mean:.3e}; |ones - None| = {(got - none).abs().max().item():.3e}")
    assert mx < HIDDEN_TOL


def test_output_hidden_states_vs_reference(encoder, gold):
    out = encoder(dev(gold["ids_right"]), attention_mask=dev(gold["mask_right"]), encoder_hidden_states=enc_states(gold),
                  output_hidden_states=True, return_dict=True)
    hs = out.hidden_states
    assert isinstance(hs, tuple) and len(hs) == 3 and all(h.dtype == torch.float32 and tuple(h.shape) == (B, T, C) for h in hs)
    figures = [worst(hs[0], gold["mm_right_hidden0"])[0], worst(hs[1], gold["mm_right_hidden1"])[0], worst(hs[2], gold["mm_right"])[0]]
    print(f"\nhidden states: max|d| = {figures}")
    assert max(figures) < HIDDEN_TOL
    assert torch.equal(hs[2], out.last_hidden_state)
    plain = encoder(dev(gold["ids_right"]), attention_mask=dev(gold["mask_right"]), encoder_hidden_states=enc_states(gold))
    assert torch.equal(plain.last_hidden_state, out.last_hidden_state)          # asking for them changes nothing
    tup = encoder(dev(gold["ids_right"]), attention_mask=dev(gold["mask_right"]), encoder_hidden_states=enc_states(gold),
                  output_hidden_states=True, return_dict=False)
    assert len(tup) == 3 and tup[1] is None and len(tup[2]) == 3


@pytest.mark.parametrize("name", ["right", "left"])
def test_decoder_vs_reference(decoder, gold, name):
    """Causal x padding mask: logits, both reductions of the label-smoothed loss, return_logits, the tuple form.  Labels: -100
    on the padding; left-padded also on the first real token, which the reference predicts from a padded position."""
    ids, mask_np, labels = dev(gold[f"dec_{name}_ids"]), gold[f"mask_{name}"], dev(gold[f"dec_{name}_labels"])
    kw = dict(attention_mask=dev(mask_np), encoder_hidden_states=enc_states(gold), labels=labels)
    if name == "right":
        kw["encoder_attention_mask"] = dev(gold["encmask_prefix"])
    ref = torch.from_numpy(gold[f"dec_{name}_logits"])
    sel = None if name == "right" else torch.from_numpy(mask_np).bool()
    scale = max(1.0, ref.abs().max().item())
    g = PLAIN_F16_REL * scale
    o_none = decoder(ids, reduction="none", return_dict=True, **kw)
    o_mean = decoder(ids, return_dict=True, **kw)
    assert tuple(o_none.logits.shape) == (B, T, V) and o_none.logits.dtype == torch.float32
    d = (o_none.logits.cpu() - ref).abs()
    d = d if sel is None else d[sel]
    n_tgt = torch.tensor([n - 1 for n in LENS], dtype=torch.float32)
    assert (gold[f"dec_{name}_labels"][:, 1:] >= 0).sum(1).tolist() == n_tgt.long().tolist()
    d_none = (o_none.loss.cpu() - torch.from_numpy(gold[f"dec_{name}_loss_none"])).abs()
    d_mean = abs(o_mean.loss.item() - float(gold[f"dec_{name}_loss_mean"]))
    print(f"\ndecoder {name}: logits max|d| = {d.max().item():.3e} mean|d| = {d.mean().item():.3e} (gate {g:.3e}); "
          f"|d loss| none {d_none.tolist()} (bounds {(2 * n_tgt * g).tolist()}), mean {d_mean:.3e} (bound {2 * g:.3e})")
    assert d.max().item() <= g and d.mean().item() <= 0.4 * g
    assert bool((d_none <= 2.0 * n_tgt * g).all())
    assert o_mean.loss.dim() == 0 and o_mean.loss.dtype == torch.float32 and d_mean <= 2.0 * g
    assert torch.equal(o_mean.logits, o_none.logits)
    lg = decoder(ids, return_logits=True, **kw)
    assert torch.is_tensor(lg) and tuple(lg.shape) == (B, T - 1, V) and torch.equal(lg, o_none.logits[:, :-1])
    tup = decoder(ids, reduction="none", return_dict=False, **kw)
    assert len(tup) == 2 and torch.equal(tup[0], o_none.loss) and torch.equal(tup[1], o_none.logits)
    del kw["labels"]
    no_labels = decoder(ids, return_dict=True, **kw)
    assert no_labels.loss is None and torch.equal(no_labels.logits, o_none.logits)
    assert len(decoder(ids, return_dict=False, **kw)) == 1


def test_lm_head_in_several_row_blocks_gives_the_bits_of_one_block(decoder, gold, monkeypatch):
    """The 48 rows of the batch through the LM head in blocks of 32 rows of scratch (32 + 16; each block's buffer is rounded up to
    one 512-row vocabulary launch) against the one-block call: same logits, same losses."""
    from vidil_amd import med

    ids, labels = dev(gold["dec_right_ids"]), dev(gold["dec_right_labels"])
    kw = dict(attention_mask=dev(gold["mask_right"]), encoder_hidden_states=enc_states(gold), labels=labels, reduction="none")
    one = decoder(ids, **kw)
    monkeypatch.setattr(med, "LOGITS_BLOCK_BYTES", 32 * 4 * V)
    two = decoder(ids, **kw)
    assert torch.equal(two.logits, one.logits) and torch.equal(two.loss, one.loss)
    assert torch.equal(decoder(ids, return_logits=True, **kw), one.logits[:, :-1])


# ------------------------------------------------------------------------------------------------ 4. padding independence
@pytest.mark.parametrize("causal", [False, True])
def test_kept_rows_do_not_depend_on_where_the_padding_is(encoder, gold, causal):
    """BertModel.masked_pass on the SAME embedded rows (same ids, same positions) laid out right-padded and left-padded: the
    rows with mask 1 hold the same bits.  (Through forward() itself the two layouts differ in their position indices, so
    there the left-padded form is compared with the reference only: test_encoder_vs_reference.)"""
    Tp = 33 if causal else T
    ids = torch.zeros((B, Tp), dtype=torch.int32, device=DEV)
    ids[:, :T] = dev(gold["ids_right"], torch.int32)
    lens = torch.tensor(LENS, device=DEV)
    t = torch.arange(Tp, device=DEV)
    keep_r = t[None, :] < lens[:, None]
    keep_l = t[None, :] >= (Tp - lens)[:, None]
    src = (t[None, :] - (Tp - lens)[:, None]) % Tp              # left layout: position t holds the right layout's row t - (Tp - n)
    rows = (torch.arange(B, device=DEV)[:, None] * Tp + src).reshape(-1)
    enc16 = enc_states(gold).half().reshape(B * TE, C).contiguous()
    cross = encoder.project_cross_kv(enc16, B, TE, v_rowmajor=Tp > 32)
    h32, h16 = encoder.embed(ids.reshape(-1), Tp, 0)
    r32, _ = encoder.masked_pass(h32, h16, B, Tp, keep_r, causal=causal, cross=cross)
    l32, _ = encoder.masked_pass(h32.index_select(0, rows), h16.index_select(0, rows), B, Tp, keep_l, causal=causal, cross=cross)
    assert torch.equal(l32.view(B, Tp, C)[keep_l], r32.view(B, Tp, C)[keep_r])
    assert bool(torch.isfinite(r32.view(B, Tp, C)[keep_r]).all())


def test_a_served_call_reads_nothing_back(encoder, decoder, gold):
    """No host synchronisation per call (the reference's loops make thousands): under torch's sync debug mode a masked
    multimodal encoder call and a decoder call with labels complete."""
    ids, enc = dev(gold["ids_holes"]), enc_states(gold)
    kw = dict(attention_mask=dev(gold["mask_holes"]), encoder_hidden_states=enc, encoder_attention_mask=dev(gold["encmask_holes"]))
    d_ids, d_kw = dev(gold["dec_left_ids"]), dict(attention_mask=dev(gold["mask_left"]), encoder_hidden_states=enc,
                                                  labels=dev(gold["dec_left_labels"]))
    encoder(ids, **kw), decoder(d_ids, **d_kw)                   # (weights packed, library loaded)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        a = encoder(ids, **kw).last_hidden_state
        b = decoder(d_ids, **d_kw).loss
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b))


# ------------------------------------------------------------------------------------------------ 5. BLIP_Base
@pytest.fixture(scope="module")
def small_med_json(tmp_path_factory):
    c = _small_cfg()
    path = tmp_path_factory.mktemp("cfg") / "med_small.json"
    path.write_text(json.dumps({k: getattr(c, k) for k in ("hidden_size", "num_attention_heads", "intermediate_size",
                                                           "num_hidden_layers", "vocab_size", "max_position_embeddings")}))
    return str(path)


def test_blip_base_three_modes_vs_reference(small_med_json, gold):
    """Three captions of 12 / 5 / 9 tokens in ONE batch (padded to 12 and masked) against the reference run on each caption
    alone; the image tokens are this library's small ViT's (vit_small.npz weights), the reference's its own."""
    from vidil_amd.blip import BLIP_Base
    from vidil_amd.vit import VisionTransformer

    sd_v, g_v = load_golden("vit_small.npz")
    sd_e, _ = load_golden("med_itm_small.npz")
    m = BLIP_Base(med_config=small_med_json, image_size=64, vit="base", tokenizer=vq.VqaTokenizer())
    m.visual_encoder = load_into(VisionTransformer(img_size=64, patch_size=16, embed_dim=256, depth=2, num_heads=4), sd_v, "visual_encoder.")
    m.text_encoder.config.encoder_width = 256
    m.text_encoder = load_into(type(m.text_encoder)(m.text_encoder.config), sd_e, "text_encoder.")
    m = m.to(DEV).eval()
    lens = gold["base_lens"].tolist()
    captions = [vq.words(row[1:n - 1]) for row, n in zip(gold["base_ids"], lens)]
    keep = np.arange(max(lens))[None, :] < np.asarray(lens)[:, None]
    x = dev(g_v["x"])
    img = m(x, captions, mode="image")
    mx, mean = worst(img, g_v["y"])
    assert tuple(img.shape) == (3, 17, 256) and mx < 5e-3 and mean < 5e-4
    txt = m(x, captions, "text")
    mm = m(x, captions, "multimodal")
    assert tuple(txt.shape) == tuple(mm.shape) == (3, max(lens), 256)
    e_txt, e_mm = worst(txt, gold["base_text"], keep)[0], worst(mm, gold["base_mm"], keep)[0]
    print(f"\nBLIP_Base: image max|d| = {mx:.3e}, text {e_txt:.3e}, multimodal {e_mm:.3e}")
    assert e_txt < HIDDEN_TOL and e_mm < HIDDEN_TOL
    # one caption alone (the reference's own call shape) gives its rows of the batch up to the token count of the launch
    one = m(x[1:2], captions[1], "multimodal")
    assert tuple(one.shape) == (1, lens[1], 256) and worst(one[0], gold["base_mm"][1, :lens[1]])[0] < HIDDEN_TOL
    with pytest.raises(AssertionError):
        m(x, captions, "fusion")


# ------------------------------------------------------------------------------------------------ 6. BLIP_Embedding
def _small_matcher(cls, small_med_json):
    """cls (BLIP_ITM or a subclass) at the small geometry: 64 x 64 images (17 tokens), embed 64, vocabulary 512."""
    from vidil_amd.med import BertModel
    from vidil_amd.vit import VisionTransformer

    m = cls(med_config=small_med_json, image_size=64, vit="base", embed_dim=64, tokenizer=vq.VqaTokenizer())
    m.visual_encoder = VisionTransformer(img_size=64, patch_size=16, embed_dim=256, depth=2, num_heads=4)
    m.vision_proj = torch.nn.Linear(256, 64)
    m.text_encoder.config.encoder_width = 256
    m.text_encoder = BertModel(config=m.text_encoder.config, add_pooling_layer=False)
    return m.eval()


def test_blip_embedding_heads(small_med_json):
    from common import perturb_
    from vidil_amd.blip_embedding import BLIP_Embedding
    from vidil_amd.blip_itm import BLIP_ITM

    torch.manual_seed(5)
    emb = _small_matcher(BLIP_Embedding, small_med_json)
    perturb_(emb, 31)
    with torch.no_grad():                                       # spread the similarities and the ITM logits
        emb.vision_proj.weight.mul_(8); emb.text_proj.weight.mul_(8); emb.itm_head.weight.mul_(20)
    itm = _small_matcher(BLIP_ITM, small_med_json)
    itm.load_state_dict(emb.state_dict(), strict=True)
    emb, itm = emb.to(DEV), itm.to(DEV)
    x = torch.from_numpy(np.random.default_rng(3).standard_normal((3, 3, 64, 64), dtype=np.float32)).to(DEV)
    texts = ["w200", "w137 w201 w300", "w174 w202 w303 w120 w130 w140 w150", "w333 w334", "w148 w204"]
    got = emb(x, texts[:3], match_head="itm")
    assert tuple(got.shape) == (3, 2) and got.dtype == torch.float32 and torch.equal(got, itm(x, texts[:3], match_head="itm"))
    assert got.std().item() > 0
    image_feat, text_feat, sim = emb(x, texts)                  # the reference's default head: 'itc'
    assert tuple(image_feat.shape) == (3, 64) and tuple(text_feat.shape) == (5, 64) and tuple(sim.shape) == (3, 5)
    assert torch.allclose(image_feat.norm(dim=-1).cpu(), torch.ones(3), atol=1e-6)          # (tests/test_models_gpu.py:237)
    assert torch.allclose(text_feat.norm(dim=-1).cpu(), torch.ones(5), atol=1e-6)
    exact = image_feat.double().cpu() @ text_feat.double().cpu().t()
    # f32 rounding of a 64-term dot product of unit vectors: sum|a_i b_i| <= 1, so |fl(dot) - dot| <= 64 u, plus u for the result
    assert (sim.double().cpu() - exact).abs().max().item() <= 65 * 2.0 ** -24
    assert torch.equal(sim, itm(x, texts, match_head="itc"))
    one_feat, one_text, one_sim = emb(x[:1], texts[1])          # a bare string is ONE caption (the reference's tokenizer call)
    assert tuple(one_text.shape) == (1, 64) and tuple(one_sim.shape) == (1, 1)
    assert tuple(emb(x[:1], texts[1], match_head="itm").shape) == (1, 2)
    with pytest.raises(ValueError):
        emb(x, texts[:3], match_head="both")


# ------------------------------------------------------------------------------------------------ 7. limits
def test_unserved_shapes_raise_before_any_launch_and_the_next_call_works(encoder, decoder, gold):
    from vidil_amd import kernels as K

    ids, mask = dev(gold["ids_right"]), dev(gold["mask_right"])
    before = encoder(ids, attention_mask=mask, mode="text").last_hidden_state.clone()
    with pytest.raises(K.VidilHipError, match="769"):            # causal attention past 768 keys
        decoder(torch.zeros((1, 769), dtype=torch.long, device=DEV), mode="text")
    with pytest.raises(K.VidilHipError, match="769"):
        encoder(torch.zeros((1, 769), dtype=torch.long, device=DEV), is_decoder=True, mode="text")
    with pytest.raises(K.VidilHipError, match="16385"):          # more than 16,384 encoder states
        encoder(ids[:1], encoder_hidden_states=torch.zeros((1, 16385, C), dtype=torch.float16, device=DEV))
    with pytest.raises(ValueError, match="max_position_embeddings"):
        encoder(torch.zeros((1, 65), dtype=torch.long, device=DEV), mode="text")
    torch.cuda.synchronize()
    assert torch.equal(encoder(ids, attention_mask=mask, mode="text").last_hidden_state, before)


def test_more_than_768_encoder_states_take_the_key_split_and_the_long_key_forms(encoder, gold):
    """8 query rows over 800 encoder states with a mask with holes on both sides: fragment tiles and the key-split form of
    vidil_attention (at most 32 query rows per unit).  The same sequences padded to 40 tokens: plain rows and the long-key
    form (more than 32).  Each against the fp32 oracle (oracle/med_ref.py's layers under both masks: vqa_cases.stack) at the
    positions whose mask is 1, under HIDDEN_TOL."""
    rng = np.random.default_rng(17)
    Tq, Tl, Te = 8, 40, 800
    enc_np = rng.standard_normal((B, Te, C)).astype(np.float16)
    emask = (rng.random((B, Te)) < 0.7).astype(np.int64)
    emask[:, 5] = 1
    ids = np.zeros((B, Tl), dtype=np.int64)
    ids[:, :Tq] = gold["ids_holes"][:, :Tq]
    mask = np.zeros((B, Tl), dtype=np.int64)
    mask[:, :Tq] = gold["mask_holes"][:, :Tq]
    mask[:, 0] = 1
    sd, _ = load_golden("med_itm_small.npz")
    with torch.no_grad():
        ref = vq.stack(sd, "text_encoder.", torch.from_numpy(ids[:, :Tq]), torch.from_numpy(mask[:, :Tq]),
                       torch.from_numpy(enc_np).float(), torch.from_numpy(emask), False)
    kw = dict(encoder_hidden_states=dev(enc_np), encoder_attention_mask=dev(emask))
    short = encoder(dev(ids[:, :Tq]), attention_mask=dev(mask[:, :Tq]), **kw).last_hidden_state
    long_ = encoder(dev(ids), attention_mask=dev(mask), **kw).last_hidden_state
    e_short, e_long = worst(short, ref, mask[:, :Tq])[0], worst(long_[:, :Tq], ref, mask[:, :Tq])[0]
    print(f"\n800 encoder states: key-split form max|d| = {e_short:.3e}, long-key form max|d| = {e_long:.3e}")
    assert e_short < HIDDEN_TOL and e_long < HIDDEN_TOL


# ------------------------------------------------------------------------------------------------ the reference's evaluation()
@torch.no_grad()
def _reference_evaluation(model, texts, video_batches, tokenizer, device, config):
    """The body of the reference's evaluation() (eval_retrieval_video.py:37-118) as a call sequence on our objects: world size
    1, the progress logger and the .cpu() staging of the video features left out, nothing else changed."""
    num_text = len(texts)
    text_bs = 256
    text_ids = []
    text_embeds = []
    text_atts = []
    for i in range(0, num_text, text_bs):
        text = texts[i: min(num_text, i + text_bs)]
        text_input = tokenizer(text, padding='max_length', truncation=True, max_length=35, return_tensors="pt").to(device)
        text_output = model.text_encoder(text_input.input_ids, attention_mask=text_input.attention_mask, mode='text')
        text_embed = F.normalize(model.text_proj(text_output.last_hidden_state[:, 0, :]))
        text_embeds.append(text_embed)
        text_ids.append(text_input.input_ids)
        text_atts.append(text_input.attention_mask)

    text_embeds = torch.cat(text_embeds, dim=0)
    text_ids = torch.cat(text_ids, dim=0)
    text_atts = torch.cat(text_atts, dim=0)
    text_ids[:, 0] = tokenizer.additional_special_tokens_ids[0]

    video_feats = []
    video_embeds = []
    for video in video_batches:
        B_, N, C_, W, H = video.size()
        video = video.view(-1, C_, W, H)
        video = video.to(device, non_blocking=True)
        video_feat = model.visual_encoder(video)
        video_embed = model.vision_proj(video_feat[:, 0, :])
        video_embed = video_embed.view(B_, N, -1).mean(dim=1)
        video_embed = F.normalize(video_embed, dim=-1)

        video_feat = video_feat.view(B_, -1, video_feat.shape[-1])
        video_feats.append(video_feat)
        video_embeds.append(video_embed)

    video_feats = torch.cat(video_feats, dim=0)
    video_embeds = torch.cat(video_embeds, dim=0)

    sims_matrix = video_embeds @ text_embeds.t()
    score_matrix_v2t = torch.full((len(texts), len(texts)), -100.0).to(device)

    for i, sims in enumerate(sims_matrix):
        topk_sim, topk_idx = sims.topk(k=config['k_test'], dim=0)

        encoder_output = video_feats[i].repeat(config['k_test'], 1, 1).to(device, non_blocking=True)
        encoder_att = torch.ones(encoder_output.size()[:-1], dtype=torch.long).to(device, non_blocking=True)
        output = model.text_encoder(text_ids[topk_idx],
                                    attention_mask=text_atts[topk_idx],
                                    encoder_hidden_states=encoder_output,
                                    encoder_attention_mask=encoder_att,
                                    return_dict=True,
                                    )
        score = model.itm_head(output.last_hidden_state[:, 0, :])[:, 1]
        score_matrix_v2t[i, topk_idx] = score + topk_sim

    sims_matrix = sims_matrix.t()
    score_matrix_t2v = torch.full((len(texts), len(texts)), -100.0).to(device)

    for i, sims in enumerate(sims_matrix):
        topk_sim, topk_idx = sims.topk(k=config['k_test'], dim=0)
        encoder_output = video_feats[topk_idx].to(device, non_blocking=True)
        encoder_att = torch.ones(encoder_output.size()[:-1], dtype=torch.long).to(device, non_blocking=True)
        output = model.text_encoder(text_ids[i].repeat(config['k_test'], 1),
                                    attention_mask=text_atts[i].repeat(config['k_test'], 1),
                                    encoder_hidden_states=encoder_output,
                                    encoder_attention_mask=encoder_att,
                                    return_dict=True,
                                    )
        score = model.itm_head(output.last_hidden_state[:, 0, :])[:, 1]
        score_matrix_t2v[i, topk_idx] = score + topk_sim

    return score_matrix_v2t.cpu().numpy(), score_matrix_t2v.cpu().numpy()


def test_the_reference_evaluation_loop_runs_unmodified(tmp_path):
    """4 videos x 2 frames, 6 texts, k_test = 3 on the small BLIP_Retrieval: the reference's loop through
    model.text_encoder(...) / visual_encoder / vision_proj / text_proj / itm_head against video_retrieval.evaluation on the
    same model and inputs, and both against the fp32 oracle of every pair.  The bound tests/test_video_retrieval_gpu.py:62
    applies to this model's candidate scores, 2e-2, holds for either path against the oracle and for the two paths against
    each other (measured: loop 1.7e-3 and evaluation 7.3e-3 from the oracle, 6.9e-3 between them — the loop runs every token
    through the last layer in f32 heads, evaluation the [CLS] rows through 16-bit heads)."""
    from oracle import clip_ref, med_ref, retrieval_ref
    from vidil_amd import video_retrieval as VR

    NV, NF, K_TEST = 4, 2, 3
    texts = VC.TEXTS[:6]
    m = VC.small_video_retrieval(tmp_path)
    u8 = VC.frames(NF)[:NV]
    # ---- fp32 oracle of every (video, text) pair (video_retrieval_cases.oracle for these texts)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    tokens, vid_emb, _ = VC.video_embeds_ref(sd, u8)
    ids, lens = m.tokenize(texts)
    ids = ids.long()
    mask = (torch.arange(ids.shape[1])[None] < lens[:, None]).long()
    with torch.no_grad():
        txt_emb = retrieval_ref.text_features(sd, ids, mask, layers=VC.LAYERS, H=VC.HEADS)
        ids[:, 0] = m.tokenizer.enc_token_id
        itm = torch.empty(NV, len(texts))
        for v in range(NV):
            h, _ = med_ref.bert_model(sd, "text_encoder.", ids, mask, layers=VC.LAYERS, H=VC.HEADS,
                                      enc=tokens[v].repeat(len(texts), 1, 1), is_decoder=False)
            itm[v] = F.linear(h[:, 0, :], sd["itm_head.weight"], sd["itm_head.bias"])[:, 1]
    ref = (itm + vid_emb @ txt_emb.t()).numpy()                  # [4, 6]
    # ---- the two device paths
    m = m.to(DEV)
    x = clip_ref.preprocess_u8(u8.reshape(NV * NF, VC.SIZE, VC.SIZE, 3)).view(NV, NF, 3, VC.SIZE, VC.SIZE)
    v2t, t2v = _reference_evaluation(m, texts, [x[:3], x[3:]], m.tokenizer, DEV, dict(k_test=K_TEST))
    assert v2t.shape == (6, 6) and t2v.shape == (6, 6)
    assert (v2t[NV:] == -100.0).all()                           # (the reference sizes both matrices by the texts)
    v2t = v2t[:NV]
    t2v = t2v[:, :NV]
    own_v2t, own_t2v = VR.evaluation(m, [u8[:3], u8[3:]], texts, K_TEST)
    for name, loop, own, want in (("v2t", v2t, own_v2t, ref), ("t2v", t2v, own_t2v, ref.T)):
        cand = own != -100.0
        assert np.array_equal(loop != -100.0, cand) and int(cand.sum()) == own.shape[0] * K_TEST
        e_loop, e_own = np.abs(loop[cand] - want[cand]).max(), np.abs(own[cand] - want[cand]).max()
        between = np.abs(loop[cand] - own[cand]).max()
        print(f"\n{name}: |loop - oracle| = {e_loop:.3e}, |evaluation - oracle| = {e_own:.3e}, |loop - evaluation| = {between:.3e}")
        assert e_loop < 2e-2 and e_own < 2e-2 and between < 2e-2
