"""Shim for ``from models.blip_vqa import ...`` -> vidil_amd.blip_vqa (the HIP-backed question-answering heads)."""
from vidil_amd.blip_vqa import BLIP_VQA, BLIP_Video_VQA, blip_vqa, blip_vqa_video  # noqa: F401
