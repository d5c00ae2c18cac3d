"""`frido.modules.encoders.modules` import path (cond_stage_config.target) -> the HIP-backed embedders: BERTEmbedder, the CLIP text tower
and the CLIP image tower."""
from frido_amd.models import BERTEmbedder, FrozenCLIPTextEmbedder, FrozenClipImageEmbedder  # noqa: F401
