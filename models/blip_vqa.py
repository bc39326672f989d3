"""Shim for ``from models.blip_vqa import ...`` -> vidil_amd.blip_vqa (the HIP-backed question-answering head)."""
from vidil_amd.blip_vqa import BLIP_VQA, blip_vqa  # noqa: F401
