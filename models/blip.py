"""Shim for ``from models.blip import ...`` -> vidil_amd.blip (the HIP-backed BLIP captioner)."""
from vidil_amd.blip import (BLIP_Base, BLIP_Decoder, BLIP_Video_Decoder, blip_decoder, blip_decoder_video,  # noqa: F401
                            blip_feature_extractor, create_vit, init_tokenizer, is_url, load_checkpoint)
