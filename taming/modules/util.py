"""`taming.modules.util`: ActNorm only (a parameter holder; the discriminator folds it into its affine kernel)."""
from frido_amd.models import ActNorm  # noqa: F401
