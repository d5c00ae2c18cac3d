"""`taming.models.msvqgan` import path (first_stage_config.target / configs/msvqgan `model.target`) -> HIP-backed MS-VQGAN."""
from frido_amd.models import MSFPNVQModel, VQModelInterface  # noqa: F401
