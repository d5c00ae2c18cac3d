"""`taming.modules.discriminator.model` -> the forward-only HIP implementation."""
from frido_amd.models import ActNorm, NLayerDiscriminator, weights_init  # noqa: F401
