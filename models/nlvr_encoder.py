"""Shim for ``from models.nlvr_encoder import ...`` -> vidil_amd.nlvr_encoder (the twin cross-attention text encoder)."""
from vidil_amd.nlvr_encoder import BertConfig, BertModel  # noqa: F401
