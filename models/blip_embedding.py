"""Shim for ``from models.blip_embedding import ...`` -> vidil_amd.blip_embedding (the HIP-backed embedding model)."""
from vidil_amd.blip_embedding import BLIP_Embedding, blip_embedding  # noqa: F401
