"""Import shim: ``from models.blip_pretrain import blip_pretrain_from_pretrained, blip_video_pretrain`` (pretrain_video.py:21)."""
from vidil_amd.blip_pretrain import (BLIP_Pretrain, BLIP_Pretrain_Video, blip_pretrain,  # noqa: F401
                                     blip_pretrain_from_pretrained, blip_video_pretrain)
