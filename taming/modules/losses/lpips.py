"""`taming.modules.losses.lpips` import path -> the HIP-backed perceptual metric."""
from frido_amd.models import LPIPS  # noqa: F401
