"""Generate the fixtures that let the live-reference checks of tests/test_oracle_cpu.py and tests/test_abi_and_host.py run
without the reference tree:

  fullsize_ref.npz               the reference's models/vit.py (ViT-B/16 @ 224) and models/med.py (BertLMHeadModel) at full
                                 size, run on the captioner weights and frame of tests/common.fullsize_captioner_state (numpy
                                 seeds: the test rebuilds them bit for bit): the ViT output and the
                                 last-position logits of the prompt
  med_decoder_keys.json          the state-dict key names of the reference's BertLMHeadModel(configs/med_config.json)
  visual_token_ontology.json.xz  the ontology files the two loaders read (oracle/tokens_ref.py: vg, vg_tencent;
                                 vidil_amd/visual_tokenization.py: also youcook2), as {relative path: file text}

Run where the reference tree and `transformers` are present (oracle/ref_shim.py finds the tree):

    python tests/golden/make_fullsize_golden.py
"""
import json
import lzma
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

from common import FULLSIZE_PROMPT, fullsize_captioner_state  # noqa: E402
from oracle import ref_shim, tokens_ref  # noqa: E402


def strip(sd, prefix):
    return {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}


def main():
    vit_mod, med_mod = ref_shim.load()
    sd, x = fullsize_captioner_state()
    v = vit_mod.VisionTransformer(img_size=224, patch_size=16, embed_dim=768, depth=12, num_heads=12).eval()
    v.load_state_dict(strip(sd, "visual_encoder."), strict=True)
    dec = med_mod.BertLMHeadModel(ref_shim.med_config()).eval()
    msg = dec.load_state_dict(strip(sd, "text_decoder."), strict=False)
    assert not msg.unexpected_keys and all("position_ids" in k for k in msg.missing_keys), msg
    ids = torch.tensor(FULLSIZE_PROMPT)
    with torch.no_grad():
        y = v(x)
        out = dec(ids, attention_mask=torch.ones_like(ids), encoder_hidden_states=y,
                  encoder_attention_mask=torch.ones(1, y.shape[1], dtype=torch.long), return_dict=True, is_decoder=True)
    np.savez_compressed(os.path.join(HERE, "fullsize_ref.npz"), y=y.numpy(), logits=out.logits[:, -1].numpy())

    keys = sorted(med_mod.BertLMHeadModel(ref_shim.med_config()).state_dict().keys())
    with open(os.path.join(HERE, "med_decoder_keys.json"), "w") as f:
        json.dump(keys, f, indent=0)

    from vidil_amd.visual_tokenization import _ONTOLOGY_FILES

    onto = os.path.join(ref_shim.REFERENCE_ROOT, "visual_token_ontology")
    paths = {p for spec in tokens_ref.ONTOLOGY_FILES.values() for p in spec.values()}
    for spec in _ONTOLOGY_FILES.values():
        paths.update(p for s in spec for p in ((s,) if isinstance(s, str) else s))
    files = {}
    for p in sorted(paths):
        with open(os.path.join(onto, p), encoding="utf-8") as f:
            files[p] = f.read()
    with lzma.open(os.path.join(HERE, "visual_token_ontology.json.xz"), "wt", encoding="utf-8") as f:
        json.dump(files, f)
    for name in ("fullsize_ref.npz", "med_decoder_keys.json", "visual_token_ontology.json.xz"):
        print(f"{name}: {os.path.getsize(os.path.join(HERE, name)) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
