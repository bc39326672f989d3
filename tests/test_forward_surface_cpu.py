"""The reference's call surface over the text stack, without a GPU: the signatures of BertModel.forward / BertLMHeadModel.forward
against the reference's own (tests/golden/forward_signatures.json, written by tests/golden/make_forward_golden.py), the refusals,
and the two factories BLIP_Base / BLIP_Embedding (state-dict names against the reference's, shims, checkpoint rule)."""
import inspect
import json
import os

import pytest
import torch

from common import GOLDEN


def _small_cfg():
    from vidil_amd.med import BertConfig

    return BertConfig(hidden_size=256, num_attention_heads=4, intermediate_size=512, num_hidden_layers=2, vocab_size=512,
                      max_position_embeddings=64, encoder_width=256)


@pytest.mark.parametrize("cls", ["BertModel", "BertLMHeadModel"])
def test_forward_signature_equals_the_reference(cls):
    from vidil_amd import med

    with open(os.path.join(GOLDEN, "forward_signatures.json")) as f:
        want = [tuple(p) for p in json.load(f)[f"{cls}.forward"]]
    sig = inspect.signature(getattr(med, cls).forward)
    got = [(n, None if p.default is inspect.Parameter.empty else p.default) for n, p in sig.parameters.items() if n != "self"]
    assert got == want
    assert all(p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for p in sig.parameters.values())


IDS = torch.zeros((2, 3), dtype=torch.long)
REFUSED = dict(position_ids=IDS, head_mask=torch.ones(2, 4), inputs_embeds=torch.zeros(2, 3, 256), past_key_values=((IDS,),),
               use_cache=True, output_attentions=True)


@pytest.mark.parametrize("arg", sorted(REFUSED) + ["encoder_embeds"])
def test_bert_model_refuses_by_name_before_the_device_is_required(arg):
    """On a CPU model: the NotImplementedError that names the argument comes before the VidilHipError about the device."""
    from vidil_amd.med import BertModel

    m = BertModel(_small_cfg())
    value = torch.zeros(2, 3, 256) if arg == "encoder_embeds" else REFUSED[arg]
    with pytest.raises(NotImplementedError, match=arg):
        m(IDS, **{arg: value})


@pytest.mark.parametrize("arg", sorted(REFUSED))
def test_lm_head_model_refuses_by_name_before_the_device_is_required(arg):
    from vidil_amd.med import BertLMHeadModel

    m = BertLMHeadModel(_small_cfg())
    with pytest.raises(NotImplementedError, match=arg):
        m(IDS, **{arg: REFUSED[arg]})


def test_a_list_of_encoder_states_an_unknown_mode_and_the_parity_mode_are_refused_and_served_calls_need_the_device():
    from vidil_amd import kernels as K
    from vidil_amd.med import BertLMHeadModel, BertModel
    from vidil_amd.packing import set_parity_mode

    m = BertModel(_small_cfg())
    enc = torch.zeros(2, 5, 256)
    with pytest.raises(NotImplementedError, match="list as encoder_hidden_states"):
        m(IDS, encoder_hidden_states=[enc, enc])
    with pytest.raises(NotImplementedError, match="mode"):
        m(IDS, mode="fusion")
    for model in (m, BertLMHeadModel(_small_cfg())):                 # served arguments: the product path has no CPU fallback
        with pytest.raises(K.VidilHipError, match="cpu"):
            model(IDS, attention_mask=torch.ones_like(IDS), use_cache=False, output_attentions=False, return_dict=True, mode="text")
    with pytest.raises(ValueError, match="reduction"):
        BertLMHeadModel(_small_cfg())(IDS, reduction="sum")
    set_parity_mode(True, m)
    with pytest.raises(NotImplementedError, match="parity"):
        m(IDS, mode="text")


def test_model_output_is_read_by_attribute_name_and_position():
    from vidil_amd.med import ModelOutput

    a, b = torch.zeros(1), torch.ones(1)
    o = ModelOutput(loss=None, logits=a, past_key_values=None, hidden_states=(b,))
    assert o.logits is a and o["logits"] is a and o[0] is a and o[1] == (b,) and o.loss is None
    assert o.to_tuple() == (a, (b,))


@pytest.mark.parametrize("name,keys,size", [("BLIP_Base", "blip_base_keys.json", 224), ("BLIP_Embedding", "blip_embedding_keys.json", 384)])
def test_factories_construct_with_the_reference_names(name, keys, size):
    import vidil_amd.blip as blip
    import vidil_amd.blip_embedding as emb
    from vidil_amd.tokenizer import SyntheticBertTokenizer

    factory = dict(BLIP_Base=blip.blip_feature_extractor, BLIP_Embedding=emb.blip_embedding)[name]
    m = factory(tokenizer=SyntheticBertTokenizer())
    assert type(m).__name__ == name
    with open(os.path.join(GOLDEN, keys)) as f:
        ref_keys = set(json.load(f))
    mine = set(m.state_dict().keys())
    assert mine == ref_keys, sorted(mine ^ ref_keys)[:10]
    assert m.visual_encoder.patch_embed.num_patches == (size // 16) ** 2        # the reference's default image_size
    assert m.text_encoder.config.encoder_width == 768
    assert list(inspect.signature(type(m).forward).parameters)[1:3] == ["image", "caption"]


def test_constructor_arguments_and_forward_defaults_are_the_reference_ones():
    from vidil_amd.blip import BLIP_Base
    from vidil_amd.blip_embedding import BLIP_Embedding

    def params(f):
        return [(n, p.default) for n, p in inspect.signature(f).parameters.items() if n != "self"]

    common = [("med_config", "configs/med_config.json"), ("image_size", None), ("vit", "base"), ("vit_grad_ckpt", False),
              ("vit_ckpt_layer", 0)]
    base = [(n, 224 if n == "image_size" else d) for n, d in common]
    emb = [(n, 384 if n == "image_size" else d) for n, d in common] + [("embed_dim", 256)]
    assert params(BLIP_Base.__init__) == base + [("tokenizer", None)]           # (tokenizer=: this library's one addition)
    assert params(BLIP_Embedding.__init__) == emb + [("tokenizer", None)]
    assert params(BLIP_Base.forward)[2] == ("mode", inspect.Parameter.empty)
    assert params(BLIP_Embedding.forward)[2] == ("match_head", "itc")


def test_shims_import_and_point_at_the_library():
    import vidil_amd.blip as blip
    import vidil_amd.blip_embedding as emb
    from models.blip import BLIP_Base, blip_feature_extractor
    from models.blip_embedding import BLIP_Embedding, blip_embedding

    assert BLIP_Base is blip.BLIP_Base and blip_feature_extractor is blip.blip_feature_extractor
    assert BLIP_Embedding is emb.BLIP_Embedding and blip_embedding is emb.blip_embedding
    assert issubclass(BLIP_Embedding, __import__("vidil_amd.blip_itm", fromlist=["BLIP_ITM"]).BLIP_ITM)


@pytest.mark.parametrize("which", ["blip_feature_extractor", "blip_embedding"])
def test_factories_refuse_the_synthetic_tokenizer_with_a_checkpoint(which):
    """As blip_decoder does: the same RuntimeError, before the checkpoint is touched."""
    import vidil_amd.blip as blip
    import vidil_amd.blip_embedding as emb
    from vidil_amd.tokenizer import SyntheticBertTokenizer

    factory = dict(blip_feature_extractor=blip.blip_feature_extractor, blip_embedding=emb.blip_embedding)[which]
    with pytest.raises(RuntimeError, match="real bert-base-uncased tokenizer"):
        factory(pretrained="/nonexistent/checkpoint.pth", tokenizer=SyntheticBertTokenizer())
