"""Shim for ``from models.blip_nlvr import ...`` -> vidil_amd.blip_nlvr (the HIP-backed two-image reasoning head)."""
from vidil_amd.blip_nlvr import BLIP_NLVR, blip_nlvr, load_checkpoint  # noqa: F401
