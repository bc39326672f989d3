"""Import shim: ``from models.blip_retrieval import blip_retrieval`` (run_visual_tokenization.py:18) and
``from models.blip_retrieval import blip_retrieval_video`` (train_retrieval_video.py)."""
from vidil_amd.blip_retrieval import (BLIP_Retrieval, BLIP_Retrieval_Video, blip_retrieval,  # noqa: F401
                                      blip_retrieval_video)
