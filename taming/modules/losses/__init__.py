"""`taming.modules.losses.DummyLoss` (lossconfig.target of every shipped first-stage config) and the LPIPS perceptual metric."""
from frido_amd.models import DummyLoss, LPIPS  # noqa: F401
