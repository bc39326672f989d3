"""BLIP_NLVR, the parts that need no GPU: state-dict names and shapes and the forward signatures against the reference's
(tests/golden/blip_nlvr_keys.json, written by tests/golden/make_nlvr_golden.py), load_checkpoint's duplication semantics, the
refusals (by name, before the device is required), the shims, the pair-major schedule, and the pack-time fold in float64."""
import inspect
import json
import os

import numpy as np
import pytest
import torch

import nlvr_cases as nc
import vqa_cases as vq
from common import GOLDEN


@pytest.fixture(scope="module")
def ref():
    with open(os.path.join(GOLDEN, "blip_nlvr_keys.json")) as f:
        return json.load(f)


def test_state_dict_names_and_shapes_equal_the_reference(ref):
    from vidil_amd.blip_nlvr import BLIP_NLVR
    from vidil_amd.tokenizer import SyntheticBertTokenizer

    m = BLIP_NLVR(tokenizer=SyntheticBertTokenizer())                    # the reference's defaults: 480 x 480, ViT-B
    mine = {k: list(v.shape) for k, v in m.state_dict().items()}
    want = ref["state_dict"]
    assert {k for k in set(mine) ^ set(want) if "position_ids" not in k} == set()
    assert all(mine[k] == want[k] for k in want if k in mine)
    assert m.visual_encoder.pos_embed.shape[1] == 901 and m.text_encoder.config.encoder_width == 768
    merged = sorted({int(k.split(".")[3]) for k in mine if "merge_layer" in k})
    assert merged == [6, 7, 8, 9, 10, 11]
    assert mine["text_encoder.encoder.layer.6.crossattention.output.merge_layer.weight"] == [768, 1536]


def test_a_six_layer_stack_has_no_merge_layer():
    from vidil_amd.nlvr_encoder import BertModel

    keys = BertModel(nc.small_cfg(6)).state_dict().keys()
    assert not any("merge_layer" in k for k in keys) and any("layer.5.crossattention.self1.value.bias" in k for k in keys)
    assert sum("merge_layer.weight" in k for k in BertModel(nc.small_cfg(8)).state_dict()) == 2


def test_forward_signatures_equal_the_reference(ref):
    from vidil_amd.blip_nlvr import BLIP_NLVR
    from vidil_amd.nlvr_encoder import BertModel

    def params(f):
        return [(n, None if p.default is inspect.Parameter.empty else p.default) for n, p in inspect.signature(f).parameters.items()
                if n != "self"]

    sigs = ref["forward"]
    assert params(BertModel.forward) == [tuple(p) for p in sigs["BertModel.forward"]]
    assert params(BLIP_NLVR.forward) == [tuple(p) for p in sigs["BLIP_NLVR.forward"]]
    assert params(BLIP_NLVR.__init__) == [tuple(p) for p in sigs["BLIP_NLVR.__init__"]] + [("tokenizer", None)]
    assert dict(params(BLIP_NLVR.__init__))["image_size"] == 480


def test_the_shims_import():
    from models.blip_nlvr import BLIP_NLVR, blip_nlvr, load_checkpoint  # noqa: F401  (the reference's import paths)
    from models.nlvr_encoder import BertConfig, BertModel  # noqa: F401
    from vidil_amd import blip_nlvr as mine, nlvr_encoder

    assert BLIP_NLVR is mine.BLIP_NLVR and BertModel is nlvr_encoder.BertModel


# ------------------------------------------------------------------------------------------------ load_checkpoint
def _pretrain_checkpoint(model, grid):
    """A fabricated BLIP pre-training checkpoint for ``model``: single cross-attention names, a position grid of grid x grid."""
    g = torch.Generator().manual_seed(3)
    sd = {}
    for k, v in model.state_dict().items():
        if "position_ids" in k or "merge_layer" in k or ".self1." in k or ".dense1." in k or k.startswith("cls_head"):
            continue
        k = k.replace(".self0.", ".self.").replace(".dense0.", ".dense.")
        sd[k] = torch.randn(v.shape, generator=g)
    sd["visual_encoder.pos_embed"] = torch.randn(1, grid * grid + 1, sd["visual_encoder.pos_embed"].shape[-1], generator=g)
    return sd


def test_load_checkpoint_duplicates_pretraining_names_and_interpolates_the_position_grid(tmp_path, capsys):
    from vidil_amd.blip_nlvr import load_checkpoint
    from vidil_amd.vit import interpolate_pos_embed

    m = nc.small_model()
    sd = _pretrain_checkpoint(m, 24)
    path = str(tmp_path / "pretrain.pth")
    torch.save({"model": sd}, path)
    m, msg = load_checkpoint(m, path)                                  # a local path loads (the reference raises NameError)
    own = m.state_dict()
    for k, v in sd.items():
        if "crossattention.self." in k:
            assert torch.equal(own[k.replace("self", "self0")], v) and torch.equal(own[k.replace("self", "self1")], v)
        elif "crossattention.output.dense." in k:
            assert torch.equal(own[k.replace("dense", "dense0")], v) and torch.equal(own[k.replace("dense", "dense1")], v)
    assert tuple(own["visual_encoder.pos_embed"].shape) == (1, 901, 256)
    assert torch.equal(own["visual_encoder.pos_embed"], interpolate_pos_embed(sd["visual_encoder.pos_embed"], m.visual_encoder))
    missing = [k for k in msg.missing_keys if "position_ids" not in k]
    assert sorted(missing) == sorted([f"text_encoder.encoder.layer.{n}.crossattention.output.merge_layer.{p}" for n in (6, 7)
                                      for p in ("weight", "bias")] + [f"cls_head.{i}.{p}" for i in (0, 2) for p in ("weight", "bias")])
    assert all("crossattention.self." in k or "crossattention.output.dense." in k for k in msg.unexpected_keys)
    assert "reshape position embedding from 576 to 900" in capsys.readouterr().out


def test_load_checkpoint_loads_twin_names_untouched_and_the_factory_prints_the_missing_keys(tmp_path, capsys, monkeypatch):
    from vidil_amd import blip_nlvr as bn

    src = nc.small_model(seed=5)
    sd = {k: v.clone() for k, v in src.state_dict().items()}
    path = str(tmp_path / "nlvr.pth")
    torch.save({"model": sd}, path)
    m, msg = bn.load_checkpoint(nc.small_model(seed=6), path)
    assert not [k for k in msg.missing_keys if "position_ids" not in k] and not msg.unexpected_keys
    assert all(torch.equal(v, sd[k]) for k, v in m.state_dict().items())
    a = m.text_encoder.encoder.layer[0].crossattention
    assert not torch.equal(a.self0.key.weight, a.self1.key.weight) and not torch.equal(a.output.dense0.weight, a.output.dense1.weight)
    # blip_nlvr(pretrained): prints the missing keys as the reference does; a synthetic tokenizer with a checkpoint is refused
    fresh = nc.small_model(seed=7)
    monkeypatch.setattr(bn, "BLIP_NLVR", lambda **kw: fresh)
    monkeypatch.setattr(bn, "refuse_synthetic_with_checkpoint", lambda tok, pretrained: None)
    bn.blip_nlvr(pretrained=path)
    assert "missing keys:" in capsys.readouterr().out
    with pytest.raises(RuntimeError, match="invalid"):
        bn.load_checkpoint(m, str(tmp_path / "absent.pth"))


# ------------------------------------------------------------------------------------------------ refusals
IDS = torch.zeros((2, 3), dtype=torch.long)
ENC2 = [torch.zeros(2, 5, 256), torch.zeros(2, 5, 256)]
REFUSED = dict(position_ids=IDS, head_mask=torch.ones(2, 4), inputs_embeds=torch.zeros(2, 3, 256), encoder_embeds=torch.zeros(2, 3, 256),
               past_key_values=((IDS,),), use_cache=True, output_attentions=True, output_hidden_states=True, is_decoder=True)


@pytest.fixture(scope="module")
def twin():
    from vidil_amd.nlvr_encoder import BertModel

    return BertModel(nc.small_cfg())


@pytest.mark.parametrize("arg", sorted(REFUSED))
def test_the_twin_encoder_refuses_by_name_before_the_device_is_required(twin, arg):
    with pytest.raises(NotImplementedError, match=arg):
        twin(IDS, encoder_hidden_states=ENC2, **{arg: REFUSED[arg]})


def test_unserved_masks_modes_and_encoder_states_are_refused_by_name_and_a_served_call_needs_the_device(twin):
    from vidil_amd import kernels as K

    ones = torch.ones(2, 5)
    with pytest.raises(NotImplementedError, match="mode='text'"):
        twin(IDS, encoder_hidden_states=ENC2, mode="text")
    with pytest.raises(NotImplementedError, match="list of the two"):
        twin(IDS, encoder_hidden_states=ENC2[0])
    with pytest.raises(NotImplementedError, match="list of the two"):
        twin(IDS)
    with pytest.raises(NotImplementedError, match=r"encoder_attention_mask\[1\]"):
        twin(IDS, encoder_hidden_states=ENC2, encoder_attention_mask=[ones, torch.tensor([[1, 1, 1, 1, 0], [1, 1, 1, 1, 1]])])
    with pytest.raises(NotImplementedError, match="encoder_attention_mask"):
        twin(IDS, encoder_hidden_states=ENC2, encoder_attention_mask=ones)
    for mask in ([[0, 1, 1], [1, 1, 1]], [[1, 0, 1], [1, 1, 1]], [[0, 0, 0], [1, 1, 1]]):          # left padding, a hole, nothing
        with pytest.raises(NotImplementedError, match="attention_mask"):
            twin(IDS, attention_mask=torch.tensor(mask), encoder_hidden_states=ENC2)
    # served calls reach the device check (no CPU fallback)
    for kw in (dict(), dict(attention_mask=torch.tensor([[1, 1, 0], [1, 1, 1]]), encoder_attention_mask=[ones, None], return_dict=True)):
        with pytest.raises(K.VidilHipError, match="runs only on an AMD GPU"):
            twin(IDS, encoder_hidden_states=ENC2, **kw)
    with pytest.raises(K.VidilHipError, match="project_twin_kv"):
        twin.project_cross_kv(torch.zeros(10, 256), 2, 5)


def test_med_bert_model_still_refuses_a_list():
    from vidil_amd.med import BertModel

    with pytest.raises(NotImplementedError, match="a list as encoder_hidden_states"):
        BertModel(nc.small_cfg(2))(IDS, encoder_hidden_states=ENC2)


def test_parity_and_fp8_are_refused_and_the_process_defaults_leave_a_fresh_model_plain(monkeypatch):
    from vidil_amd import packing
    from vidil_amd.nlvr_encoder import BertModel

    monkeypatch.setattr(packing, "_parity_default", [True])              # what $VIDIL_PARITY=1 sets at import
    monkeypatch.setattr(packing, "_default", [packing.FP8])              # what $VIDIL_DTYPE=fp8 sets at import
    m = nc.small_model(image_size=32, init=False)
    assert not any(packing.parity_mode(s) for s in m.modules())
    assert all(packing.compute_dtype(s) == torch.float16 for s in m.modules())
    m._require_plain()
    with pytest.raises(ValueError, match="parity"):
        packing.set_parity_mode(True, m)
    with pytest.raises(ValueError, match="fp8"):
        packing.set_compute_dtype("fp8", m)
    with pytest.raises(ValueError, match="parity"):
        packing.set_parity_mode(True, m.text_encoder)
    m.text_encoder.__dict__["_parity"] = True                            # (switched on behind the model's back)
    with pytest.raises(ValueError, match="parity"):
        m._require_plain()
    with pytest.raises(NotImplementedError, match="parity"):
        m.text_encoder(IDS, encoder_hidden_states=ENC2)
    with pytest.raises(NotImplementedError, match="parity"):
        m.text_encoder.packed()
    m.text_encoder.__dict__["_parity"] = False
    packing.set_compute_dtype("bf16", m)
    m._require_plain()
    fresh = BertModel(nc.small_cfg())                                    # a bare twin encoder under the process defaults
    with pytest.raises(NotImplementedError, match="parity|fp8"):
        fresh(IDS, encoder_hidden_states=ENC2)


def test_tokenisation_follows_the_reference_and_longer_input_is_refused_by_name():
    """models/blip_nlvr.py:48-49 restated on the synthetic tokenizer: padding='longest', no truncation, first id := [ENC]."""
    m = nc.small_model(image_size=32, init=False)
    tok = m.tokenizer
    text = [vq.words(range(110, 150)), "w200"]                           # 42 and 3 tokens: nothing is cut
    want = tok(text, padding="longest", return_tensors="pt")
    want.input_ids[:, 0] = tok.enc_token_id
    ids, lens = m.tokenize(text)
    assert ids.dtype == torch.int32 and torch.equal(ids.long(), want.input_ids) and lens.tolist() == [42, 3]
    assert m.tokenize("w200")[0].tolist() == [[nc.ENC, 200, nc.SEP]]
    with pytest.raises(ValueError, match="65 tokens exceeds the text encoder's 64 positions"):
        m.tokenize([vq.words(range(110, 173))])
    # a missing target is refused by name too
    with pytest.raises(ValueError, match="needs targets"):
        m.forward(torch.zeros(2, 3, 32, 32), ["w200"], None, train=True)


# ------------------------------------------------------------------------------------------------ schedule
def test_pair_major_order_and_annotations(tmp_path):
    from vidil_amd import nlvr

    ex = [(2, 0, "a", 1), (0, 1, "b", 0), (2, 0, "c", 0), (1, 0, "d", 1), (0, 1, "e", 1), (2, 0, "f", 1)]
    s = nlvr.pair_major_order(ex, 3)
    assert s["pairs"].tolist() == [[0, 1], [1, 0], [2, 0]]                # ordered pairs: (0, 1) and (1, 0) are different units
    assert s["order"].tolist() == [1, 4, 3, 0, 2, 5] and s["group_start"].tolist() == [0, 2, 3, 6] and s["max_group"] == 3
    with pytest.raises(ValueError, match="outside"):
        nlvr.pair_major_order([(0, 3, "a", 1)], 3)
    path = tmp_path / "nlvr_dev.json"
    path.write_text(json.dumps([
        dict(images=["dev-1-img0.png", "dev-1-img1.png"], sentence="The LEFT image (shows) two dogs.", label="True"),
        dict(images=["dev-1-img0.png", "dev-2-img1.png"], sentence=" ".join(["word"] * 50), label="False")]))
    names, examples = nlvr.load_nlvr_annotations(str(path))
    assert names == ["dev-1-img0.png", "dev-1-img1.png", "dev-2-img1.png"]
    assert examples[0] == (0, 1, "the left image shows two dogs", 1)      # pre_caption; no left / right swap
    assert examples[1][:2] == (0, 2) and len(examples[1][2].split(" ")) == 40 and examples[1][3] == 0


# ------------------------------------------------------------------------------------------------ the fold
@pytest.mark.parametrize("merge", [False, True])
def test_the_fold_equals_the_literal_sequence_in_float64(merge):
    """[ctx0 | ctx1] · Wf^T + bf against (dense0(ctx0) + dense1(ctx1)) / 2 and merge_layer(cat[dense0(ctx0), dense1(ctx1)])."""
    from vidil_amd.nlvr_encoder import fold_twin_output

    rng = np.random.default_rng(11)
    C, M = 64, 37
    t = lambda *s: torch.from_numpy(rng.standard_normal(s))
    w0, b0, w1, b1, wm, bm = t(C, C), t(C), t(C, C), t(C), t(C, 2 * C), t(C)
    ctx0, ctx1 = t(M, C), t(M, C)
    d0, d1 = ctx0 @ w0.T + b0, ctx1 @ w1.T + b1
    literal = torch.cat([d0, d1], 1) @ wm.T + bm if merge else (d0 + d1) / 2
    wf, bf = fold_twin_output(w0, b0, w1, b1, *((wm, bm) if merge else ()))
    assert wf.dtype == torch.float64 and tuple(wf.shape) == (C, 2 * C)
    got = torch.cat([ctx0, ctx1], 1) @ wf.T + bf
    assert (got - literal).abs().max().item() <= 1e-12 * max(1.0, literal.abs().max().item())


def test_the_packed_fold_is_rounded_once_and_the_averaging_fold_is_exact():
    from vidil_amd.nlvr_encoder import BertModel, fold_twin_output

    m = nc.small_model(image_size=32).text_encoder
    p = m.packed()
    for n in (0, 7):
        o = m.encoder.layer[n].crossattention.output
        d = p["layers"][n]
        assert tuple(d["cf_w"].shape) == (256, 512) and d["cf_w"].dtype == torch.float16 and d["cf_b"].dtype == torch.float32
        merge = (o.merge_layer.weight, o.merge_layer.bias) if n >= 6 else ()
        wf, bf = fold_twin_output(o.dense0.weight, o.dense0.bias, o.dense1.weight, o.dense1.bias, *merge)
        assert torch.equal(d["cf_w"], wf.to(torch.float16)) and torch.equal(d["cf_b"], bf.float())
    # averaging: halving commutes with the rounding, but for f16 subnormals (spacing 2^-24: at most half of it is lost)
    o = m.encoder.layer[0].crossattention.output
    half = torch.cat([o.dense0.weight, o.dense1.weight], 1).detach().to(torch.float16).float() * 0.5
    assert (p["layers"][0]["cf_w"].float() - half).abs().max().item() <= 2.0 ** -25
    normal = half.abs() >= 2.0 ** -14
    assert torch.equal(p["layers"][0]["cf_w"].float()[normal], half[normal])
    assert isinstance(p["layers"][0]["cq_w"], list) and len(p["layers"][0]["ckv_w"]) == 2 and "co_w" not in p["layers"][0]


def test_fixture_is_what_the_issue_asks_for():
    g = nc.golden()
    assert g["S_mask"].sum(1).tolist() == [3, 9, 20] and g["La_mask"].sum(1).tolist() == [9, 40] and g["Lb_mask"].sum(1).tolist() == [5, 9]
    assert g["G901_hidden"].shape == (5, 12, 256) and g["Y_hidden"].shape == g["S_hidden"].shape == (3, 20, 256)
    preds = np.concatenate([g["G17_pred"], g["G901_pred"], g["E_pred"]], 0)
    bound = nc.PRED_REL * max(1.0, float(np.abs(preds).max()))
    assert preds.shape == (12, 2) and float(np.abs(preds[:, 1] - preds[:, 0]).min()) >= 10 * bound
    assert int(g["seed"]) == nc.SEED and os.path.getsize(os.path.join(GOLDEN, "nlvr_small.npz")) < 1 << 20
