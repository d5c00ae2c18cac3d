"""Stale `ldm.modules.encoders.modules.BERTEmbedder` target of configs/frido/layout2i/frido_f8f4_vg.yaml:80 -> BERTEmbedder; the CLIP
image tower under the same old import path."""
from frido_amd.models import BERTEmbedder, FrozenClipImageEmbedder  # noqa: F401
